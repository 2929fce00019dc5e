// The host build of the TIFF writer's format text: csrc/tiffw.inc compiled by a host compiler behind a few C functions for
// tests/test_tiff_write_host.py, tests/test_gpu_tiff_write.py (ctypes) and tests/tiff_write_main.cpp.  The 64 lanes of a
// step are a loop here, so a segment's bytes equal the device's.  TEST INFRASTRUCTURE.
#include <stdlib.h>
#include <string.h>

#include "tiffw.inc"

extern "C" {

uint64_t tiffw_shim_bound(uint64_t n) { return tiffw::bound((size_t)n); }
uint64_t tiffw_shim_cap(int compression) { return tiffw::segment_cap(compression); }
uint32_t tiffw_shim_block_tokens(void) { return (uint32_t)tiffw::TOKCAP; }
uint32_t tiffw_shim_adler32(const uint8_t* p, size_t n) { return tiff::adler32(p, n, 0, 1); }

// one segment: in[0 .. n) -> out[0 .. cap); returns the stream's size.  stats (may be null): blocks, tokens, kinds of
// block used (1 stored | 2 fixed | 4 dynamic), stored blocks.  The state is a heap allocation of exactly its size, filled
// with `fill` first.
uint64_t tiffw_shim_deflate(const uint8_t* in, size_t n, uint8_t* out, size_t cap, uint32_t* stats, int fill)
{
    tiffw::DeflateState* st = (tiffw::DeflateState*)malloc(sizeof(tiffw::DeflateState));
    memset(st, fill, sizeof *st);
    const size_t got = tiffw::deflate(in, n, out, cap, st, 0, 1);
    if (stats) memcpy(stats, st->stats, sizeof st->stats);
    free(st);
    return got;
}

// code lengths of freq[0 .. n) under `limit` bits
void tiffw_shim_lengths(const uint32_t* freq, int n, int limit, uint8_t* len)
{
    tiffw::DeflateState* st = (tiffw::DeflateState*)malloc(sizeof(tiffw::DeflateState));
    memset(st, 0xA5, sizeof *st);
    tiffw::build_lengths(freq, n, limit, len, st, 0, 1);
    free(st);
}

// the code-length stream of ll[0 .. nll) and d[0 .. nd): symbol | extra << 8 each; returns their number (at most nll + nd)
uint32_t tiffw_shim_rle(const uint8_t* ll, int nll, const uint8_t* d, int nd, uint16_t* syms)
{
    uint8_t len[tiffw::DOFF + 32];
    memset(len, 0, sizeof len);
    memcpy(len, ll, (size_t)nll);
    memcpy(len + tiffw::DOFF, d, (size_t)nd);
    return tiffw::rle_lengths(len, nll, nd, syms);
}

int64_t tiffw_shim_segment_count(const lbdrn_tiffw_layout* L)
{
    tiff::Geom g;
    return tiffw::make_geom(*L, &g) ? g.nseg : 0;
}

int64_t tiffw_shim_expected(const lbdrn_tiffw_layout* L, int64_t s)
{
    tiff::Geom g;
    return tiffw::make_geom(*L, &g) && s >= 0 && s < g.nseg ? tiff::seg_expected(g, s) : -1;
}

// segment s of planes[C][H][W] as the gather stage leaves it: seg[0 .. expected(s))
int tiffw_shim_gather(const lbdrn_tiffw_layout* L, const void* planes, int64_t s, uint8_t* seg)
{
    tiff::Geom g;
    if (!tiffw::make_geom(*L, &g) || s < 0 || s >= g.nseg) return -1;
    for (int r = 0; r < g.seg_h; ++r) {
        if (g.bps == 1) tiffw::gather_row<uint8_t>(g, (const uint8_t*)planes, s, r, seg, 0);
        else tiffw::gather_row<uint16_t>(g, (const uint16_t*)planes, s, r, seg, 0);
    }
    return 0;
}

}  // extern "C"
