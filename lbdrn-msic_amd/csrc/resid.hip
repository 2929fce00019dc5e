// liblbdrn_resid.so (include/lbdrn_resid.h): the residual layer "LBR1" -- the difference between the original and the
// codec's own reconstruction, quantised for a stated maximum error and Rice-coded per row, on the GPU.  The format's text
// (quantiser, row coder and decoder, bit gather, header) is csrc/resid.inc, shared with the host tests.
//
//   k_resid_encode   one wave per block of 64 rows x 256 columns, lane i owning row i.  The block passes through LDS in
//                    chunks of 64 columns (coalesced 128-byte row loads of orig and recon, u = fold(q) stored as
//                    tile[row][col] with a pitch of 65 words: the wave's writes of one row fall on consecutive banks, and
//                    lane i's read of tile[i][j] on bank (i + j) % 32 -- distinct within each half of the wave, which is
//                    the group ds_read_b32 / ds_write_b32 are banked over).  First walk: the 16 candidate bit counts of
//                    the lane's row; second walk: the row's bits into the lane's private words in the workspace.  The
//                    block's byte count is a wave sum of the 64 bit lengths.
//   (rocprim exclusive scan of the byte counts)
//   k_resid_pack     one workgroup per block: the header (block 0), the block's table entry, its row lengths, and every
//                    byte of its concatenated rows gathered from the private streams (resid::gather_byte) -- ordinary
//                    byte stores, so neither the body's address nor a block's offset needs an alignment.
//   k_resid_table    decoder: the table's entries of the blocks as aligned u32 for the scan
//   k_resid_decode   one wave per block that intersects the rectangle: the block's extent from the table and the scan,
//                    checked against the body; a wave scan of the 64 row lengths places each lane's row, checked against
//                    the block's bytes; the lanes whose rows the rectangle takes decode alone (RowReader never reads
//                    outside the block), chunk by chunk through the same LDS tile, and the wave applies
//                    recon' = clamp(recon + q (2 tau + 1)) to the rectangle's samples with coalesced row accesses.
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "common.hpp"
#include "error_buffer.inc"
#include "../../include/lbdrn_resid.h"
#include "resid.inc"

namespace lbdrn {

constexpr int RS_CHUNK = 64;               // columns staged at a time
constexpr int RS_PITCH = RS_CHUNK + 1;     // words per LDS row

struct ResidWs {
    uint32_t* counts;    // [nblocks]       block byte lengths
    uint64_t* offsets;   // [nblocks + 1]
    void* scan_tmp;
    uint16_t* rowbits;   // [nblocks][64]
    uint32_t* priv;      // [nblocks][64][ROW_WORDS]
    size_t scan_bytes, total;
};

static int carve_resid(const resid::Geom& g, void* ws, ResidWs* w, bool decoder = false)
{
    size_t scan_bytes = 0;
    uint32_t* in = nullptr;
    uint64_t* out = nullptr;
    if (rocprim::exclusive_scan(nullptr, scan_bytes, in, out, (uint64_t)0, (size_t)g.nblocks, rocprim::plus<uint64_t>()) != hipSuccess) {
        set_error("rocprim::exclusive_scan: cannot size its scratch");
        return LBDRN_E_DEVICE;
    }
    char* p = (char*)ws;
    w->counts = (uint32_t*)p; p += align_up((size_t)g.nblocks * 4, 256);
    w->offsets = (uint64_t*)p; p += align_up((size_t)(g.nblocks + 1) * 8, 256);
    w->scan_tmp = p; p += align_up(scan_bytes, 256);
    w->rowbits = nullptr;
    w->priv = nullptr;
    if (!decoder) {     // the decoder needs the table, its scan and nothing else
        w->rowbits = (uint16_t*)p; p += align_up((size_t)g.nblocks * resid::BLOCK_ROWS * 2, 256);
        w->priv = (uint32_t*)p; p += align_up((size_t)g.nblocks * resid::BLOCK_ROWS * resid::ROW_WORDS * 4, 256);
    }
    w->scan_bytes = scan_bytes;
    w->total = (size_t)(p - (char*)ws);
    return 0;
}

struct ResidHeader {
    uint8_t b[resid::HEADER_BYTES];
};

__device__ __forceinline__ uint32_t rs_wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------ encoder

__global__ void __launch_bounds__(64) k_resid_encode(const uint16_t* __restrict__ orig, const uint16_t* __restrict__ recon,
                                                      resid::Geom g, int tau, uint32_t* __restrict__ priv,
                                                      uint16_t* __restrict__ rowbits, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t tile[resid::BLOCK_ROWS][RS_PITCH];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int bx = (int)(b % g.nbx), by = (int)((b / g.nbx) % g.nby), c = (int)(b / ((int64_t)g.nbx * g.nby));
    const int rows = resid::block_rows(g, by), cols = resid::block_cols(g, bx);
    const size_t base = ((size_t)c * g.H + (size_t)by * resid::BLOCK_ROWS) * g.W + (size_t)bx * resid::BLOCK_COLS;
    uint32_t* words = priv + ((size_t)b * resid::BLOCK_ROWS + lane) * resid::ROW_WORDS;

    resid::RowCost cost;
    resid::RowWriter wr;
    cost.init();
    wr.init(words);
    uint32_t bits = 0;
    int k = 0;
    for (int walk = 0; walk < 2; ++walk) {
        if (walk == 1) {
            k = cost.pick(&bits);
            if (lane >= rows) bits = 0;
            if (bits) wr.put((uint32_t)k, resid::K_BITS);
        }
        for (int c0 = 0; c0 < cols; c0 += RS_CHUNK) {
            const int cw = min(RS_CHUNK, cols - c0);
            __syncthreads();
            if (lane < cw)
                for (int r = 0; r < rows; ++r) {
                    const size_t idx = base + (size_t)r * g.W + c0 + lane;
                    tile[r][lane] = resid::fold(resid::quantise(orig[idx], recon[idx], tau));
                }
            __syncthreads();
            if (lane < rows) {
                if (walk == 0)
                    for (int j = 0; j < cw; ++j) cost.add(tile[lane][j]);
                else if (bits)
                    for (int j = 0; j < cw; ++j) wr.symbol(tile[lane][j], k);
            }
        }
    }
    if (bits) wr.finish();
    rowbits[(size_t)b * resid::BLOCK_ROWS + lane] = (uint16_t)bits;
    const uint32_t total = rs_wave_sum(bits);
    if (lane == 0) counts[b] = 2u * (uint32_t)rows + (total + 7u) / 8u;
}

__global__ void __launch_bounds__(256) k_resid_pack(resid::Geom g, ResidHeader hdr, const uint32_t* __restrict__ priv,
                                                     const uint16_t* __restrict__ rowbits, const uint32_t* __restrict__ counts,
                                                     const uint64_t* __restrict__ offsets, uint8_t* __restrict__ body,
                                                     uint64_t* __restrict__ body_bytes)
{
    __shared__ uint32_t start[resid::BLOCK_ROWS + 1];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int by = (int)((b / g.nbx) % g.nby);
    const int rows = resid::block_rows(g, by);
    const uint16_t* lens = rowbits + (size_t)b * resid::BLOCK_ROWS;
    if (tid == 0) {
        uint32_t pos = 0;
        for (int r = 0; r < rows; ++r) { start[r] = pos; pos += lens[r]; }
        start[rows] = pos;
    }
    __syncthreads();
    const uint32_t n = counts[b];
    const uint64_t data0 = (uint64_t)resid::HEADER_BYTES + 4u * (uint64_t)g.nblocks;
    uint8_t* dst = body + data0 + offsets[b];
    if (b == 0 && tid < resid::HEADER_BYTES) body[tid] = hdr.b[tid];
    if (tid < 4) body[resid::HEADER_BYTES + 4 * b + tid] = (uint8_t)(n >> (8 * tid));
    const uint32_t* mine = priv + (size_t)b * resid::BLOCK_ROWS * resid::ROW_WORDS;
    for (uint32_t t = tid; t < n; t += 256) {
        if (t < 2u * (uint32_t)rows) {
            const uint32_t v = lens[t >> 1];
            dst[t] = (uint8_t)((t & 1u) ? v >> 8 : v);
        } else {
            dst[t] = (uint8_t)resid::gather_byte(start, rows, mine, resid::ROW_WORDS, t - 2u * (uint32_t)rows);
        }
    }
    if (b == g.nblocks - 1 && tid == 0) *body_bytes = data0 + offsets[b] + n;
}

// ------------------------------------------------------------------ decoder

__global__ void __launch_bounds__(256) k_resid_table(const uint8_t* __restrict__ body, int64_t nblocks, uint32_t* __restrict__ counts)
{
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b < nblocks) counts[b] = resid::le32(body + resid::HEADER_BYTES + 4 * b);
}

struct ResidRect {
    int x0, y0, w, h, bx0, by0;
};

__global__ void __launch_bounds__(64) k_resid_decode(const uint8_t* __restrict__ body, uint64_t n, resid::Geom g,
                                                      const uint32_t* __restrict__ counts, const uint64_t* __restrict__ offsets,
                                                      ResidRect rc, uint16_t* __restrict__ recon, int* __restrict__ status)
{
    __shared__ int32_t tile[resid::BLOCK_ROWS][RS_PITCH];
    const int lane = threadIdx.x;
    const int bx = rc.bx0 + (int)blockIdx.x, by = rc.by0 + (int)blockIdx.y, c = (int)blockIdx.z;
    const int64_t b = ((int64_t)c * g.nby + by) * g.nbx + bx;
    const int rows = resid::block_rows(g, by), cols = resid::block_cols(g, bx);
    resid::Header hd;
    if (!resid::read_header(body, &hd) || hd.C != (uint32_t)g.C || hd.H != (uint32_t)g.H || hd.W != (uint32_t)g.W) {
        if (lane == 0) atomicOr(status, 1);
        return;
    }
    const int tau = (int)hd.tau;
    const uint64_t data0 = (uint64_t)resid::HEADER_BYTES + 4u * (uint64_t)g.nblocks;    // (the host checked n >= data0)
    const uint64_t off = offsets[b];
    const uint32_t blen = counts[b];
    if (off > n - data0 || blen > n - data0 - off || blen < 2u * (uint32_t)rows || blen > resid::block_bound(rows, cols)) {
        if (lane == 0) atomicOr(status, 1);
        return;
    }
    const uint8_t* blk = body + data0 + off;
    // the lane's row: a wave scan of the 64 lengths
    const uint32_t len = lane < rows ? resid::le16(blk + 2 * lane) : 0u;
    uint32_t incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    const uint32_t total = 16u * (uint32_t)rows + __shfl(incl, 63, 64);
    if ((total + 7u) / 8u != blen) {
        if (lane == 0) atomicOr(status, 1);
        return;
    }
    const uint32_t start = 16u * (uint32_t)rows + incl - len;
    // what the rectangle takes of this block, in block coordinates
    const int r0 = max(rc.y0 - by * resid::BLOCK_ROWS, 0), r1 = min(rc.y0 + rc.h - by * resid::BLOCK_ROWS, rows);
    const int j0 = max(rc.x0 - bx * resid::BLOCK_COLS, 0), j1 = min(rc.x0 + rc.w - bx * resid::BLOCK_COLS, cols);
    const bool mine = lane >= r0 && lane < r1;
    const uint32_t umax = resid::max_symbol(tau);
    bool bad = len != 0 && len <= (uint32_t)resid::K_BITS;
    resid::RowReader rd;
    int k = 0;
    rd.init(blk, blen, start, mine ? len : 0u);
    if (mine && len) k = rd.parameter();
    int c0 = 0;
    for (; c0 < j1; c0 += RS_CHUNK) {
        const int cw = min(RS_CHUNK, cols - c0);
        __syncthreads();
        if (mine)
            for (int j = 0; j < cw; ++j) {
                uint32_t u = len ? rd.symbol(k) : 0u;
                if (u > umax) { bad = true; u = 0; }
                tile[lane][j] = resid::unfold(u);
            }
        __syncthreads();
        const int j = c0 + lane;
        if (lane < cw && j >= j0 && j < j1)
            for (int r = r0; r < r1; ++r) {
                const size_t idx = ((size_t)c * rc.h + (size_t)(by * resid::BLOCK_ROWS + r - rc.y0)) * rc.w +
                                   (size_t)(bx * resid::BLOCK_COLS + j - rc.x0);
                recon[idx] = resid::enhance(recon[idx], tile[r][lane], tau);
            }
    }
    if (mine && len && (rd.bad || (c0 >= cols && rd.left != 0))) bad = true;
    if (bad) atomicOr(status, 1);
}

// ------------------------------------------------------------------ host entry points

static int resid_encode(const uint16_t* orig, const uint16_t* recon, int C, int H, int W, int tau, void* body, size_t cap,
                        uint64_t* body_bytes, void* ws, size_t ws_bytes, hipStream_t s)
{
    LBDRN_REQUIRE(orig && recon && body && body_bytes, "lbdrn_resid_encode: null pointer");
    LBDRN_REQUIRE(((uintptr_t)orig & 1u) == 0, "lbdrn_resid_encode: orig is not 2-byte aligned");
    LBDRN_REQUIRE(((uintptr_t)recon & 1u) == 0, "lbdrn_resid_encode: recon is not 2-byte aligned");
    LBDRN_REQUIRE(((uintptr_t)body_bytes & 7u) == 0, "lbdrn_resid_encode: body_bytes is not 8-byte aligned");
    LBDRN_REQUIRE(((uintptr_t)ws & 255u) == 0, "lbdrn_resid_encode: workspace is not 256-byte aligned");   // (carve_resid: u32 / u64 regions at multiples of 256)
    LBDRN_REQUIRE(tau >= 0 && tau <= 65535, "lbdrn_resid_encode: tau = %d is outside 0..65535", tau);
    resid::Geom g;
    LBDRN_REQUIRE(resid::make_geom(C, H, W, &g), "lbdrn_resid_encode: geometry %d x %d x %d is out of range", C, H, W);
    ResidWs w;
    if (int rc = carve_resid(g, ws, &w)) return rc;
    if (!ws || ws_bytes < w.total) {
        set_error("residual codec workspace too small: %zu < %zu", ws_bytes, w.total);
        return LBDRN_E_WORKSPACE;
    }
    if (cap < resid::body_bound(g)) {
        set_error("residual body buffer too small: %zu < %zu", cap, resid::body_bound(g));
        return LBDRN_E_WORKSPACE;
    }
    ResidHeader hdr;
    resid::write_header(hdr.b, (uint32_t)tau, (uint32_t)C, (uint32_t)H, (uint32_t)W);
    k_resid_encode<<<(unsigned)g.nblocks, 64, 0, s>>>(orig, recon, g, tau, w.priv, w.rowbits, w.counts);
    LBDRN_LAUNCH_CHECK();
    LBDRN_HIP_TRY(rocprim::exclusive_scan(w.scan_tmp, w.scan_bytes, w.counts, w.offsets, (uint64_t)0, (size_t)g.nblocks,
                                          rocprim::plus<uint64_t>(), s));
    k_resid_pack<<<(unsigned)g.nblocks, 256, 0, s>>>(g, hdr, w.priv, w.rowbits, w.counts, w.offsets, (uint8_t*)body, body_bytes);
    LBDRN_LAUNCH_CHECK();
    return 0;
}

static int resid_decode(const void* body, size_t n, int C, int H, int W, int x0, int y0, int rw, int rh, uint16_t* recon,
                        int* status, void* ws, size_t ws_bytes, hipStream_t s)
{
    LBDRN_REQUIRE(body && recon && status, "lbdrn_resid_decode: null pointer");
    LBDRN_REQUIRE(((uintptr_t)recon & 1u) == 0, "lbdrn_resid_decode: recon_inout is not 2-byte aligned");
    LBDRN_REQUIRE(((uintptr_t)status & 3u) == 0, "lbdrn_resid_decode: status is not 4-byte aligned");
    LBDRN_REQUIRE(((uintptr_t)ws & 255u) == 0, "lbdrn_resid_decode: workspace is not 256-byte aligned");
    resid::Geom g;
    LBDRN_REQUIRE(resid::make_geom(C, H, W, &g), "lbdrn_resid_decode: geometry %d x %d x %d is out of range", C, H, W);
    LBDRN_REQUIRE(rw >= 1 && rh >= 1 && x0 >= 0 && y0 >= 0 && x0 <= W - rw && y0 <= H - rh,
                  "lbdrn_resid_decode: rectangle x0=%d y0=%d w=%d h=%d is not inside the %d x %d tile", x0, y0, rw, rh, W, H);
    LBDRN_REQUIRE(n >= (size_t)resid::HEADER_BYTES && (n - resid::HEADER_BYTES) / 4 >= (size_t)g.nblocks,
                  "lbdrn_resid_decode: a body of %zu bytes cannot hold the table of %lld blocks", n, (long long)g.nblocks);
    ResidWs w;
    if (int rc = carve_resid(g, ws, &w, true)) return rc;
    if (!ws || ws_bytes < w.total) {
        set_error("residual codec workspace too small: %zu < %zu", ws_bytes, w.total);
        return LBDRN_E_WORKSPACE;
    }
    ResidRect rc;
    rc.x0 = x0; rc.y0 = y0; rc.w = rw; rc.h = rh;
    rc.bx0 = x0 / resid::BLOCK_COLS; rc.by0 = y0 / resid::BLOCK_ROWS;
    const unsigned nbx = (unsigned)((x0 + rw - 1) / resid::BLOCK_COLS - rc.bx0 + 1);
    const unsigned nby = (unsigned)((y0 + rh - 1) / resid::BLOCK_ROWS - rc.by0 + 1);
    LBDRN_HIP_TRY(hipMemsetAsync(status, 0, sizeof(int), s));
    k_resid_table<<<(unsigned)((g.nblocks + 255) / 256), 256, 0, s>>>((const uint8_t*)body, g.nblocks, w.counts);
    LBDRN_LAUNCH_CHECK();
    LBDRN_HIP_TRY(rocprim::exclusive_scan(w.scan_tmp, w.scan_bytes, w.counts, w.offsets, (uint64_t)0, (size_t)g.nblocks,
                                          rocprim::plus<uint64_t>(), s));
    k_resid_decode<<<dim3(nbx, nby, (unsigned)C), 64, 0, s>>>((const uint8_t*)body, (uint64_t)n, g, w.counts, w.offsets, rc, recon, status);
    LBDRN_LAUNCH_CHECK();
    return 0;
}

}  // namespace lbdrn

extern "C" {

const char* lbdrn_resid_last_error(void) { return lbdrn::last_error(); }
int lbdrn_resid_abi_version(void) { return LBDRN_RESID_ABI_VERSION; }

size_t lbdrn_resid_bound(int32_t C, int32_t H, int32_t W)
{
    resid::Geom g;
    return resid::make_geom(C, H, W, &g) ? resid::body_bound(g) : 0;
}

size_t lbdrn_resid_workspace(int32_t C, int32_t H, int32_t W)
{
    resid::Geom g;
    lbdrn::ResidWs w;
    if (!resid::make_geom(C, H, W, &g) || lbdrn::carve_resid(g, nullptr, &w)) return 0;
    return w.total;
}

size_t lbdrn_resid_decode_workspace(int32_t C, int32_t H, int32_t W)
{
    resid::Geom g;
    lbdrn::ResidWs w;
    if (!resid::make_geom(C, H, W, &g) || lbdrn::carve_resid(g, nullptr, &w, true)) return 0;
    return w.total;
}

int lbdrn_resid_encode(const uint16_t* orig, const uint16_t* recon, int32_t C, int32_t H, int32_t W, int32_t tau, void* body,
                       size_t capacity, uint64_t* body_bytes, void* workspace, size_t workspace_bytes, void* stream)
{
    return lbdrn::resid_encode(orig, recon, C, H, W, tau, body, capacity, body_bytes, workspace, workspace_bytes, (hipStream_t)stream);
}

int lbdrn_resid_info(const void* body, size_t n, int32_t* C, int32_t* H, int32_t* W, int32_t* tau)
{
    LBDRN_REQUIRE(body && C && H && W && tau, "lbdrn_resid_info: null pointer");
    resid::Header h;
    char msg[256];
    if (resid::check_body((const uint8_t*)body, n, &h, msg, sizeof msg)) {
        lbdrn::set_error("lbdrn_resid_info: %s", msg);
        return LBDRN_E_ARG;
    }
    *C = (int32_t)h.C; *H = (int32_t)h.H; *W = (int32_t)h.W; *tau = (int32_t)h.tau;
    return 0;
}

int lbdrn_resid_decode(const void* body, size_t n, int32_t C, int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t w, int32_t h,
                       uint16_t* recon_inout, int32_t* status, void* workspace, size_t workspace_bytes, void* stream)
{
    return lbdrn::resid_decode(body, n, C, H, W, x0, y0, w, h, recon_inout, status, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
