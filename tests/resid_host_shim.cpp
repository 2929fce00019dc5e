// The residual layer's host-compilable text (csrc/resid.inc: quantiser, row coder and decoder, bit gather, header, table
// validation) behind a C ABI, compiled by a host C++ compiler into a temporary directory by tests/test_resid_host.py,
// which judges it against tests/resid_reference.py without a GPU.  TEST INFRASTRUCTURE.
//
// The only product text restated here is what the kernels of csrc/resid.hip do around that text: the walk over blocks
// and rows, the prefix sum of a block's row lengths, and the rectangle's clipping.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "resid.inc"

extern "C" {

// one row: u[n] -> its bits as bytes (MSB first, zero padded); returns the bit count, k and the 16 candidate costs
int resid_shim_encode_row(const uint32_t* u, int n, uint8_t* out, int cap, int32_t* k_out, uint32_t* costs)
{
    if (n < 1 || n > resid::BLOCK_COLS) return -1;
    resid::RowCost rc;
    rc.init();
    for (int j = 0; j < n; ++j) rc.add(u[j]);
    uint32_t bits;
    *k_out = rc.pick(&bits);
    for (int k = 0; k < 16; ++k) costs[k] = rc.c[k];
    uint32_t words[resid::ROW_WORDS + 1];
    memset(words, 0xA5, sizeof words);
    const uint32_t got = resid::encode_row(u, n, 1, words);
    if (got != bits || words[resid::ROW_WORDS] != 0xA5A5A5A5u) return -2;
    if ((int)((bits + 7) / 8) > cap) return -3;
    for (uint32_t t = 0; t < (bits + 7) / 8; ++t) out[t] = (uint8_t)(words[t >> 2] >> (24 - 8 * (t & 3)));
    return (int)bits;
}

// bits [start, start + len) of p[0 .. limit) -> u[n]; 1 = a valid row, 0 = damaged
int resid_shim_decode_row(const uint8_t* p, uint32_t limit, uint64_t start, uint32_t len, int n, uint32_t* u)
{
    return resid::decode_row(p, limit, start, len, n, u, 1) ? 1 : 0;
}

void resid_shim_quantise(const int32_t* orig, const int32_t* recon, int64_t n, int32_t tau, int32_t* q, uint32_t* u, int32_t* back,
                         int32_t* rec)
{
    for (int64_t i = 0; i < n; ++i) {
        q[i] = resid::quantise(orig[i], recon[i], tau);
        u[i] = resid::fold(q[i]);
        back[i] = resid::unfold(u[i]);
        rec[i] = resid::enhance(recon[i], q[i], tau);
    }
}

uint32_t resid_shim_max_symbol(int32_t tau) { return resid::max_symbol(tau); }

int64_t resid_shim_bound(int32_t C, int32_t H, int32_t W)
{
    resid::Geom g;
    return resid::make_geom(C, H, W, &g) ? (int64_t)resid::body_bound(g) : 0;
}

// the whole body on the host, the way k_resid_encode / k_resid_pack build it; returns its bytes (-1: cap too small)
int64_t resid_shim_encode_body(const uint16_t* orig, const uint16_t* recon, int32_t C, int32_t H, int32_t W, int32_t tau, uint8_t* out,
                               int64_t cap)
{
    resid::Geom g;
    if (!resid::make_geom(C, H, W, &g) || tau < 0 || tau > 65535) return -2;
    std::vector<uint8_t> body(resid::HEADER_BYTES + 4 * (size_t)g.nblocks);
    resid::write_header(body.data(), (uint32_t)tau, (uint32_t)C, (uint32_t)H, (uint32_t)W);
    std::vector<uint32_t> priv((size_t)resid::BLOCK_ROWS * resid::ROW_WORDS), u(resid::BLOCK_COLS);
    int64_t b = 0;
    for (int c = 0; c < C; ++c)
        for (int by = 0; by < g.nby; ++by)
            for (int bx = 0; bx < g.nbx; ++bx, ++b) {
                const int rows = resid::block_rows(g, by), cols = resid::block_cols(g, bx);
                uint32_t start[resid::BLOCK_ROWS + 1], pos = 0;
                for (int r = 0; r < rows; ++r) {
                    const size_t base = ((size_t)c * H + (size_t)by * resid::BLOCK_ROWS + r) * W + (size_t)bx * resid::BLOCK_COLS;
                    for (int j = 0; j < cols; ++j) u[j] = resid::fold(resid::quantise(orig[base + j], recon[base + j], tau));
                    start[r] = pos;
                    pos += resid::encode_row(u.data(), cols, 1, priv.data() + (size_t)r * resid::ROW_WORDS);
                }
                start[rows] = pos;
                const uint32_t n = 2u * rows + (pos + 7u) / 8u;
                for (int t = 0; t < 4; ++t) body[resid::HEADER_BYTES + 4 * b + t] = (uint8_t)(n >> (8 * t));
                for (int r = 0; r < rows; ++r) {
                    const uint32_t len = start[r + 1] - start[r];
                    body.push_back((uint8_t)len);
                    body.push_back((uint8_t)(len >> 8));
                }
                for (uint32_t t = 0; t < (pos + 7u) / 8u; ++t)
                    body.push_back((uint8_t)resid::gather_byte(start, rows, priv.data(), resid::ROW_WORDS, t));
            }
    if ((int64_t)body.size() > cap) return -1;
    memcpy(out, body.data(), body.size());
    return (int64_t)body.size();
}

// {C, H, W, tau}; 0, or -1 and a message
int resid_shim_info(const uint8_t* body, size_t n, int64_t out[4], char* msg, size_t cap)
{
    resid::Header h;
    char local[256] = "";
    const int rc = resid::check_body(body, n, &h, local, sizeof local);
    if (msg && cap) snprintf(msg, cap, "%s", local);
    if (rc) return rc;
    out[0] = h.C; out[1] = h.H; out[2] = h.W; out[3] = h.tau;
    return 0;
}

// The rectangle (x0, y0, w, h) of the tile, the way k_resid_decode walks it: recon [C][h][w] in place.  Returns the status
// (0 = every block touched was sound), -1 for arguments lbdrn_resid_decode refuses on the host.
int resid_shim_decode_body(const uint8_t* body, size_t n, int32_t C, int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t w, int32_t h,
                           uint16_t* recon)
{
    resid::Geom g;
    if (!resid::make_geom(C, H, W, &g) || w < 1 || h < 1 || x0 < 0 || y0 < 0 || x0 > W - w || y0 > H - h) return -1;
    if (n < (size_t)resid::HEADER_BYTES || (n - resid::HEADER_BYTES) / 4 < (size_t)g.nblocks) return -1;
    resid::Header hd;
    if (!resid::read_header(body, &hd) || hd.C != (uint32_t)C || hd.H != (uint32_t)H || hd.W != (uint32_t)W) return 1;
    const int tau = (int)hd.tau;
    const uint64_t data0 = (uint64_t)resid::HEADER_BYTES + 4u * (uint64_t)g.nblocks;
    std::vector<uint64_t> offsets((size_t)g.nblocks + 1, 0);
    for (int64_t b = 0; b < g.nblocks; ++b) offsets[b + 1] = offsets[b] + resid::le32(body + resid::HEADER_BYTES + 4 * b);
    int status = 0;
    std::vector<uint32_t> u(resid::BLOCK_COLS);
    for (int c = 0; c < C; ++c)
        for (int by = y0 / resid::BLOCK_ROWS; by <= (y0 + h - 1) / resid::BLOCK_ROWS; ++by)
            for (int bx = x0 / resid::BLOCK_COLS; bx <= (x0 + w - 1) / resid::BLOCK_COLS; ++bx) {
                const int64_t b = ((int64_t)c * g.nby + by) * g.nbx + bx;
                const int rows = resid::block_rows(g, by), cols = resid::block_cols(g, bx);
                const uint64_t off = offsets[b];
                const uint32_t blen = resid::le32(body + resid::HEADER_BYTES + 4 * b);
                uint32_t start[resid::BLOCK_ROWS + 1];
                if (off > n - data0 || blen > n - data0 - off || !resid::check_block(body + data0 + off, blen, rows, cols, start)) {
                    status = 1;
                    continue;
                }
                const uint8_t* blk = body + data0 + off;
                const int r0 = y0 - by * resid::BLOCK_ROWS > 0 ? y0 - by * resid::BLOCK_ROWS : 0;
                const int r1 = y0 + h - by * resid::BLOCK_ROWS < rows ? y0 + h - by * resid::BLOCK_ROWS : rows;
                const int j0 = x0 - bx * resid::BLOCK_COLS > 0 ? x0 - bx * resid::BLOCK_COLS : 0;
                const int j1 = x0 + w - bx * resid::BLOCK_COLS < cols ? x0 + w - bx * resid::BLOCK_COLS : cols;
                for (int r = r0; r < r1; ++r) {
                    if (!resid::decode_row(blk, blen, start[r], start[r + 1] - start[r], cols, u.data(), 1)) status = 1;
                    for (int j = j0; j < j1; ++j) {
                        uint32_t v = u[j];
                        if (v > resid::max_symbol(tau)) { status = 1; v = 0; }
                        const size_t idx = ((size_t)c * h + (size_t)(by * resid::BLOCK_ROWS + r - y0)) * w + (size_t)(bx * resid::BLOCK_COLS + j - x0);
                        recon[idx] = resid::enhance(recon[idx], resid::unfold(v), tau);
                    }
                }
            }
    return status;
}

}  // extern "C"
