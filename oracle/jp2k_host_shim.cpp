// The product's host-compilable JPEG 2000 text (csrc/jp2k_t1.inc: tier-1; csrc/jp2k_t2.inc: geometry, packet headers,
// file assembly) behind a C ABI, compiled by a host C++ compiler so that tests/test_jp2k_oracle.py can judge it against
// oracle/jp2k_oracle.c without a GPU.  TEST INFRASTRUCTURE; built by oracle/build.py into oracle/_build/.
//
// The only product text restated here is the staging of a block in k_jp2k_blocks (csrc/jp2k.hip): sign / magnitude,
// mag[((y >> 2) * 64 + x) * 4 + (y & 3)], numbps from the OR of the magnitudes, the zeroed flag words and the filled tables.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "jp2k_t1.inc"
#include "jp2k_t2.inc"

extern "C" {

// One block of w x h coefficients (rows `stride` apart) of a subband of orientation `orient`.  Returns the byte count the
// coder reports (bytes beyond `cap` are counted, not written); *passes, *numbps as the kernel stores them.
int jp2k_shim_code_block(const int32_t* coef, int stride, int w, int h, int orient, uint8_t* out, int cap, int32_t* passes,
                         int32_t* numbps)
{
    static thread_local uint32_t mag[16 * 64 * 4];
    static thread_local uint16_t st[jp2k::T1_NST * jp2k::T1_STW];
    uint32_t mqtab[jp2k::MQ_ENTRIES];
    uint8_t zc[256], cx[32];
    if (w < 1 || h < 1 || w > 64 || h > 64) return -1;
    memset(st, 0, sizeof st);
    jp2k::t1_fill_tables(mqtab, zc, orient, 0, 1);
    uint32_t top = 0;
    for (int y = 0; y < 64; ++y)
        for (int x = 0; x < 64; ++x) {
            uint32_t m = 0;
            if (y < h && x < w) {
                const int v = coef[(size_t)y * stride + x];
                m = v < 0 ? (0x80000000u | (uint32_t)(-v)) : (uint32_t)v;
            }
            mag[((y >> 2) * 64 + x) * 4 + (y & 3)] = m;
            top |= m & 0x7FFFFFFFu;
        }
    const int nb = top ? 32 - __builtin_clz(top) : 0;
    const jp2k::T1Result r = jp2k::t1_encode_block(mag, st, cx, mqtab, zc, w, h, nb, out, cap);
    *passes = r.passes;
    *numbps = r.numbps;
    return r.bytes;
}

// The block table of make_geometry, eight values per block: slab, x, y, w, h, orient, mb, cap.  Returns the number of
// blocks (-1: the geometry is refused); writes the first `cap` of them.
int64_t jp2k_shim_blocks(int C, int H, int W, int bits, int64_t* rec, int64_t cap)
{
    jp2k::Geometry g;
    if (!jp2k::make_geometry(C, H, W, bits, true, &g)) return -1;
    if ((int64_t)g.blocks.size() != g.nblocks) return -2;
    for (int64_t k = 0; k < g.nblocks && k < cap; ++k) {
        const jp2k::Block& b = g.blocks[(size_t)k];
        int64_t* q = rec + 8 * k;
        q[0] = b.slab; q[1] = b.x; q[2] = b.y; q[3] = b.w; q[4] = b.h; q[5] = b.orient; q[6] = b.mb; q[7] = b.cap;
    }
    return g.nblocks;
}

// put_packet_header for a packet of `nbands` bands of gw x gh blocks announcing mb bit-planes; rec: three values per
// block, band by band in raster order: passes, numbps, bytes.  Returns the header's length.
int64_t jp2k_shim_packet_header(int nbands, const int32_t* gw, const int32_t* gh, const int32_t* mb, const int32_t* rec, uint8_t* out,
                                size_t cap)
{
    jp2k::Packet pk;
    memset(&pk, 0, sizeof pk);
    pk.nbands = nbands;
    int64_t n = 0;
    for (int b = 0; b < nbands; ++b) {
        pk.band[b].orient = nbands == 1 ? 0 : b + 1;
        pk.band[b].gw = gw[b]; pk.band[b].gh = gh[b]; pk.band[b].mb = mb[b];
        pk.band[b].first = n;
        n += (int64_t)gw[b] * gh[b];
    }
    std::vector<jp2k::BlockOut> res((size_t)(n ? n : 1));
    for (int64_t k = 0; k < n; ++k) {
        res[(size_t)k].passes = (uint32_t)rec[3 * k];
        res[(size_t)k].numbps = (uint32_t)rec[3 * k + 1];
        res[(size_t)k].bytes = (uint32_t)rec[3 * k + 2];
        res[(size_t)k].pad = 0;
    }
    jp2k::Writer w = {out, cap, 0};
    jp2k::put_packet_header(w, pk, res.data());
    return (int64_t)w.n;
}

// assemble: res holds four values per block of the table (bytes, passes, numbps, 0), data the blocks' bytes back to back
int64_t jp2k_shim_assemble(int C, int H, int W, int bits, const uint32_t* res, const uint8_t* data, uint64_t total, uint8_t* out, size_t cap)
{
    jp2k::Geometry g;
    if (!jp2k::make_geometry(C, H, W, bits, true, &g)) return -1;
    static_assert(sizeof(jp2k::BlockOut) == 16, "four 32-bit values");
    return (int64_t)jp2k::assemble(g, (const jp2k::BlockOut*)res, data, total, out, cap);
}

}  // extern "C"
