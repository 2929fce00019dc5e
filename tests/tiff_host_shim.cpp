// The host build of the TIFF reader's format text: csrc/tiff.inc compiled by a host compiler, one lane of one, behind a
// few C functions for tests/test_tiff_host.py (ctypes) and tests/tiff_damage_main.cpp.  TEST INFRASTRUCTURE.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "tiff.inc"

extern "C" {

// the status of one segment decoded into out[0 .. expect); the tables are a heap allocation of exactly their size
int tiff_shim_decode(int compression, const uint8_t* in, size_t n, uint8_t* out, size_t expect)
{
    if (compression == tiff::COMP_DEFLATE) {
        tiff::InflateTables* t = (tiff::InflateTables*)malloc(sizeof(tiff::InflateTables));
        memset(t, 0xA5, sizeof *t);
        const int st = tiff::inflate(in, n, out, expect, t, 0, 1);
        free(t);
        return st;
    }
    if (compression == tiff::COMP_LZW) {
        tiff::LzwTables* t = (tiff::LzwTables*)malloc(sizeof(tiff::LzwTables));
        memset(t, 0xA5, sizeof *t);
        const int st = tiff::lzw(in, n, out, expect, t, 0, 1);
        free(t);
        return st;
    }
    if (compression == tiff::COMP_PACKBITS) {
        tiff::PackBitsTables* t = (tiff::PackBitsTables*)malloc(sizeof(tiff::PackBitsTables));
        memset(t, 0xA5, sizeof *t);
        const int st = tiff::packbits(in, n, out, expect, t, 0, 1);
        free(t);
        return st;
    }
    if (compression == tiff::COMP_NONE) {
        if (n < expect) return tiff::ST_TRUNCATED;
        memcpy(out, in, expect);
        return 0;
    }
    return -1;
}

int64_t tiff_shim_segment_count(const lbdrn_tiff_layout* L)
{
    tiff::Geom g;
    return tiff::make_geom(*L, &g) ? g.nseg : 0;
}

int64_t tiff_shim_expected(const lbdrn_tiff_layout* L, int64_t s)
{
    tiff::Geom g;
    return tiff::make_geom(*L, &g) && s >= 0 && s < g.nseg ? tiff::seg_expected(g, s) : -1;
}

uint64_t tiff_shim_cap(int compression) { return tiff::segment_cap(compression); }

uint32_t tiff_shim_adler32(const uint8_t* p, size_t n) { return tiff::adler32(p, n, 0, 1); }

}  // extern "C"
