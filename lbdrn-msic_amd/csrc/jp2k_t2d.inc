// JPEG 2000 on the host side of liblbdrn_jp2k_dec's decoder: everything that is not tier-1 or the wavelet.  Walks the JP2
// boxes (T.800 Annex I) to the codestream, reads the main header and the tile-part headers (Annex A), derives the
// geometry (B.5 - B.7, ceiling divisions of tile coordinates: any tile size) and parses the packet headers (B.10: tag
// trees, Table B.4, Lblock, bit un-stuffing) into a table of code blocks.  Plain C++ without any HIP, included by
// jp2k_dec.hip; Band is jp2k_t2.inc's.
//
// Accepted: unsigned components of one depth of 1..16 bits without sub-sampling, any tile size, reversible 5/3 with up to
// DEC_MAX_LEVELS decompositions, no component transform or the reversible one (RCT, on three components or more), one
// layer, LRCP, code blocks up to 64 x 64 of style 0, default precincts or a precinct partition (one size per resolution
// in COD, up to DEC_MAX_PRECINCTS precincts per resolution of a tile), no quantisation, SOP / EPH, several tile-parts
// per tile, COM / TLM / PLT / PLM / CRG skipped.  Everything else is DEC_UNSUPPORTED with the feature named.
//
// Precincts (B.6, B.7): the precinct grid of a resolution of a tile is anchored at 0 in the resolution's coordinates; in
// a band above the lowest resolution a precinct spans half its size; a code block never exceeds a precinct, so the
// block exponents of a resolution are min(COD's, PP - 1) (min(COD's, PP) at the lowest).  Precinct and block boundaries
// coincide, so a band's blocks are those of its own zero-anchored grid whatever the partition: it only decides which
// packet carries a block, and over which sub-grid that packet's tag trees are built.
//
// Every offset and length is checked against the buffer before it is used: all reads go through Bytes, which answers 0
// beyond the end and remembers that it was asked.  What the device gets is a table that satisfies, per block,
//   offset + length <= n,  1 <= w, h <= 64,  numbps <= mb <= 31,  1 <= passes <= 3 * numbps - 2   (or passes == 0)
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "jp2k_t2.inc"

namespace jp2k {

enum { DEC_OK = 0, DEC_BAD = -1, DEC_UNSUPPORTED = -3 };   // the values of LBDRN_E_ARG and LBDRN_E_UNSUPPORTED
constexpr int DEC_MAX_LEVELS = 16;
constexpr int64_t DEC_MAX_BLOCKS = (int64_t)1 << 24;
constexpr int64_t DEC_MAX_SAMPLES = (int64_t)1 << 33;
constexpr int64_t DEC_MAX_PRECINCTS = (int64_t)1 << 20;    // per resolution of a tile

struct DecError {
    int code;
    char msg[256];
    int fail(int c, const char* fmt, ...)
    {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof msg, fmt, ap);
        va_end(ap);
        code = c;
        return c;
    }
};

struct Bytes {         // bounded reads
    const uint8_t* p;
    size_t n;
    bool has(size_t at, size_t len) const { return at <= n && len <= n - at; }
    unsigned u8(size_t at) const { return at < n ? p[at] : 0u; }
    unsigned u16(size_t at) const { return has(at, 2) ? (unsigned)p[at] << 8 | p[at + 1] : 0u; }
    uint32_t u32(size_t at) const { return has(at, 4) ? (uint32_t)u16(at) << 16 | u16(at + 2) : 0u; }
};

struct DecParams {
    int C, H, W, bits;
    int XT, YT;            // tile size; image and tile grid start at (0, 0)
    int NL;                // decompositions
    int cbw, cbh;
    int mct;               // 1: the reversible component transform on components 0 - 2
    int ppx[DEC_MAX_LEVELS + 1], ppy[DEC_MAX_LEVELS + 1];   // precinct exponents per resolution, from the lowest (15: default)
    int guard;
    int eps[1 + 3 * 32];   // exponents: LL, then HL LH HH of each resolution from the lowest
    int sop, eph;
    int ntx, nty, tw, th;  // tiles across and down; the largest tile's size (the slab's)
};
struct DecSegment { size_t at, end; };    // the packets of one tile-part: behind SOD .. the tile-part's end
struct DecStream {
    DecParams p;
    std::vector<std::vector<DecSegment>> parts;   // per tile, in the order of the codestream
};

struct DecBlock {      // one code block, in the order the packets carry them: tile, resolution, component, precinct, band, raster
    int32_t tile, comp, res, band, gx, gy;      // gx, gy: in the band's block grid
    int32_t prec;                // its precinct, in raster order of the resolution's precinct grid
    int32_t numbps, passes;      // passes 0: the file does not include the block (its coefficients are zero)
    int64_t offset;              // of its bytes in the file; -1 when not included
    int32_t length, mb;
    int32_t x, y, w, h;          // in the tile-component's slab (Mallat layout)
    int32_t orient;
};

inline int64_t dec_cdiv(int64_t a, int64_t b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }
inline int64_t dec_fdiv(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

inline void dec_tile_rect(const DecParams& p, int t, int64_t* x0, int64_t* y0, int64_t* x1, int64_t* y1)
{
    const int tx = t % p.ntx, ty = t / p.ntx;
    *x0 = (int64_t)tx * p.XT; *y0 = (int64_t)ty * p.YT;
    *x1 = *x0 + p.XT < p.W ? *x0 + p.XT : p.W;
    *y1 = *y0 + p.YT < p.H ? *y0 + p.YT : p.H;
}

struct DecRes {        // one resolution of one tile: its bands, its code-block size and its precinct grid
    int nbands;        // 0: the resolution is empty and has no packet
    Band bd[3];        // gw, gh: the band's whole block grid
    int cbw, cbh;      // code blocks here: COD's, cut down to a precinct's span in the bands (B.7)
    int pbx, pby;      // exponents of a precinct's span in the bands' coordinates: PP - 1, PP at the lowest resolution
    int64_t px0, py0;  // the precinct grid's first column and row, counted from the origin
    int64_t npx, npy;  // precincts across and down (B-16)
};

// The bands of resolution r of tile t (B-14, B-15) and its precinct grid; returns the number of bands.
inline int dec_bands(const DecParams& p, int t, int r, DecRes* rs)
{
    Band* bd = rs->bd;
    rs->nbands = 0;
    rs->npx = rs->npy = 0;
    int64_t x0, y0, x1, y1;
    dec_tile_rect(p, t, &x0, &y0, &x1, &y1);
    const int64_t s = (int64_t)1 << (p.NL - r);
    const int64_t rx0 = dec_cdiv(x0, s), rx1 = dec_cdiv(x1, s), ry0 = dec_cdiv(y0, s), ry1 = dec_cdiv(y1, s);
    if (rx1 <= rx0 || ry1 <= ry0) return 0;
    const int ppx = p.ppx[r], ppy = p.ppy[r];
    rs->pbx = r == 0 ? ppx : ppx - 1; rs->pby = r == 0 ? ppy : ppy - 1;       // (dec_read_headers: PP >= 1 above r = 0)
    rs->cbw = p.cbw < (1 << rs->pbx) ? p.cbw : 1 << rs->pbx;
    rs->cbh = p.cbh < (1 << rs->pby) ? p.cbh : 1 << rs->pby;
    rs->px0 = rx0 >> ppx; rs->py0 = ry0 >> ppy;
    rs->npx = ((rx1 + ((int64_t)1 << ppx) - 1) >> ppx) - rs->px0;
    rs->npy = ((ry1 + ((int64_t)1 << ppy) - 1) >> ppy) - rs->py0;
    const int n = r == 0 ? 1 : 3;
    const int nb = r == 0 ? p.NL : p.NL - r + 1;
    const int64_t lx0 = dec_cdiv(rx0, 2), lx1 = dec_cdiv(rx1, 2), ly0 = dec_cdiv(ry0, 2), ly1 = dec_cdiv(ry1, 2);
    for (int b = 0; b < n; ++b) {
        Band& q = bd[b];
        q.orient = r == 0 ? 0 : b + 1;
        const int xo = q.orient & 1, yo = q.orient >> 1;
        const int64_t half = nb ? (int64_t)1 << (nb - 1) : 0, full = (int64_t)1 << nb;
        const int64_t bx0 = dec_cdiv(x0 - half * xo, full), bx1 = dec_cdiv(x1 - half * xo, full);
        const int64_t by0 = dec_cdiv(y0 - half * yo, full), by1 = dec_cdiv(y1 - half * yo, full);
        q.bx0 = (int)bx0; q.by0 = (int)by0;
        q.w = (int)(bx1 - bx0); q.h = (int)(by1 - by0);
        q.x = r == 0 ? 0 : (xo ? (int)(lx1 - lx0) : 0);
        q.y = r == 0 ? 0 : (yo ? (int)(ly1 - ly0) : 0);
        if (q.w <= 0 || q.h <= 0) q.gw = q.gh = 0;
        else {
            q.gw = (int)(dec_cdiv(bx1, rs->cbw) - dec_fdiv(bx0, rs->cbw));
            q.gh = (int)(dec_cdiv(by1, rs->cbh) - dec_fdiv(by0, rs->cbh));
        }
        q.mb = p.guard + p.eps[r == 0 ? 0 : 1 + 3 * (r - 1) + b] - 1;   // (E-2)
        q.first = 0;
    }
    rs->nbands = n;
    return n;
}

// The blocks of band b that lie in precinct (px, py) of the resolution's grid: a rectangle of the band's block grid, from
// (*gx0, *gy0), *gw x *gh blocks; 0 x 0 when the precinct holds nothing of the band.
inline void dec_precinct_blocks(const DecRes& rs, int b, int64_t px, int64_t py, int* gx0, int* gy0, int* gw, int* gh)
{
    const Band& q = rs.bd[b];
    *gx0 = *gy0 = *gw = *gh = 0;
    if (q.w <= 0 || q.h <= 0) return;
    const int64_t bx1 = (int64_t)q.bx0 + q.w, by1 = (int64_t)q.by0 + q.h;
    const int64_t cx0 = (rs.px0 + px) << rs.pbx, cx1 = (rs.px0 + px + 1) << rs.pbx;
    const int64_t cy0 = (rs.py0 + py) << rs.pby, cy1 = (rs.py0 + py + 1) << rs.pby;
    const int64_t ax0 = cx0 > q.bx0 ? cx0 : q.bx0, ax1 = cx1 < bx1 ? cx1 : bx1;
    const int64_t ay0 = cy0 > q.by0 ? cy0 : q.by0, ay1 = cy1 < by1 ? cy1 : by1;
    if (ax1 <= ax0 || ay1 <= ay0) return;
    *gx0 = (int)(dec_fdiv(ax0, rs.cbw) - dec_fdiv(q.bx0, rs.cbw));
    *gy0 = (int)(dec_fdiv(ay0, rs.cbh) - dec_fdiv(q.by0, rs.cbh));
    *gw = (int)(dec_cdiv(ax1, rs.cbw) - dec_fdiv(ax0, rs.cbw));
    *gh = (int)(dec_cdiv(ay1, rs.cbh) - dec_fdiv(ay0, rs.cbh));
}

inline void dec_block_rect(const DecRes& rs, const Band& q, int gx, int gy, int* x, int* y, int* w, int* h)
{
    const int64_t cx0 = (dec_fdiv(q.bx0, rs.cbw) + gx) * rs.cbw, cy0 = (dec_fdiv(q.by0, rs.cbh) + gy) * rs.cbh;
    const int64_t ax0 = cx0 > q.bx0 ? cx0 : q.bx0, ay0 = cy0 > q.by0 ? cy0 : q.by0;
    const int64_t ax1 = cx0 + rs.cbw < (int64_t)q.bx0 + q.w ? cx0 + rs.cbw : (int64_t)q.bx0 + q.w;
    const int64_t ay1 = cy0 + rs.cbh < (int64_t)q.by0 + q.h ? cy0 + rs.cbh : (int64_t)q.by0 + q.h;
    *x = q.x + (int)(ax0 - q.bx0); *y = q.y + (int)(ay0 - q.by0);
    *w = (int)(ax1 - ax0); *h = (int)(ay1 - ay0);
}

// the number of code blocks, or a negative code (more precincts in a resolution of a tile than DEC_MAX_PRECINCTS, more
// blocks than DEC_MAX_BLOCKS).  A band's blocks are counted from its own grid: the precincts partition it.
inline int64_t dec_count_blocks(const DecParams& p, DecError* e)
{
    int64_t n = 0;
    for (int t = 0; t < p.ntx * p.nty; ++t)
        for (int r = 0; r <= p.NL; ++r) {
            DecRes rs;
            const int nbands = dec_bands(p, t, r, &rs);
            if (rs.npx > DEC_MAX_PRECINCTS || rs.npy > DEC_MAX_PRECINCTS || rs.npx * rs.npy > DEC_MAX_PRECINCTS)
                return e->fail(DEC_UNSUPPORTED, "precinct partition: resolution %d of tile %d has %lld x %lld precincts (at most %lld)", r, t,
                               (long long)rs.npx, (long long)rs.npy, (long long)DEC_MAX_PRECINCTS);
            for (int b = 0; b < nbands; ++b) {
                const int64_t m = (int64_t)rs.bd[b].gw * rs.bd[b].gh;
                if (m <= DEC_MAX_BLOCKS) n += m * p.C;
                if (m > DEC_MAX_BLOCKS || n > DEC_MAX_BLOCKS) return e->fail(DEC_UNSUPPORTED, "more than %lld code blocks", (long long)DEC_MAX_BLOCKS);
            }
        }
    return n;
}

// ------------------------------------------------------------------ headers

inline int dec_read_headers(const uint8_t* f, size_t n, DecStream* s, DecError* e)
{
    if (!f) return e->fail(DEC_BAD, "null buffer");
    const Bytes in = {f, n};
    DecParams& p = s->p;
    memset(&p, 0, sizeof p);
    s->parts.clear();
    size_t at = 0, end = n;
    if (n >= 12 && in.u32(0) == 12 && !memcmp(f + 4, "jP  ", 4)) {       // JP2: walk the boxes to jp2c
        bool found = false;
        while (in.has(at, 8)) {
            uint64_t len = in.u32(at);
            size_t hdr = 8;
            if (len == 1) {
                if (!in.has(at, 16)) break;
                len = (uint64_t)in.u32(at + 8) << 32 | in.u32(at + 12);
                hdr = 16;
            } else if (len == 0) len = n - at;
            if (len < hdr || len > n - at) return e->fail(DEC_BAD, "box at %zu runs beyond the file", at);
            if (!memcmp(f + at + 4, "jp2c", 4)) { end = at + (size_t)len; at += hdr; found = true; break; }
            at += (size_t)len;
        }
        if (!found) return e->fail(DEC_BAD, "no jp2c box");
    }
    const Bytes cs = {f, end};      // nothing of the codestream lies behind its box
    if (!cs.has(at, 4) || cs.u16(at) != 0xFF4F) return e->fail(DEC_BAD, "no SOC marker");
    at += 2;
    bool have_siz = false, have_cod = false;
    int have_qcd = -1;
    while (cs.has(at, 4) && cs.u16(at) != 0xFF90) {
        const unsigned marker = cs.u16(at), len = cs.u16(at + 2);
        const size_t q = at + 4;
        if (len < 2 || !cs.has(at + 2, len)) return e->fail(DEC_BAD, "marker segment %04X runs beyond the stream", marker);
        if (marker == 0xFF51) {
            if (len < 41) return e->fail(DEC_BAD, "short SIZ");
            const uint32_t W = cs.u32(q + 2), H = cs.u32(q + 6), XT = cs.u32(q + 18), YT = cs.u32(q + 22);
            if (cs.u32(q + 10) || cs.u32(q + 14) || cs.u32(q + 26) || cs.u32(q + 30))
                return e->fail(DEC_UNSUPPORTED, "image or tile offsets are not supported");
            const unsigned C = cs.u16(q + 34);
            if (C < 1 || len != 38 + 3 * C) return e->fail(DEC_BAD, "bad SIZ");
            if (C > 16384) return e->fail(DEC_UNSUPPORTED, "%u components (at most 16384)", C);
            if (W < 1 || H < 1 || XT < 1 || YT < 1) return e->fail(DEC_BAD, "empty image or tile in SIZ");
            if (W > 0x7FFFFFFFu || H > 0x7FFFFFFFu || (int64_t)W * H > DEC_MAX_SAMPLES / C)
                return e->fail(DEC_UNSUPPORTED, "%u x %u x %u samples (at most 2^33)", C, H, W);
            for (unsigned c = 0; c < C; ++c) {
                if (cs.u8(q + 37 + 3 * c) != 1 || cs.u8(q + 38 + 3 * c) != 1) return e->fail(DEC_UNSUPPORTED, "sub-sampled components are not supported");
                if (cs.u8(q + 36 + 3 * c) & 0x80) return e->fail(DEC_UNSUPPORTED, "signed components are not supported");
                if (cs.u8(q + 36 + 3 * c) != cs.u8(q + 36)) return e->fail(DEC_UNSUPPORTED, "components of different depths are not supported");
            }
            p.bits = (int)cs.u8(q + 36) + 1;
            if (p.bits > 16) return e->fail(DEC_UNSUPPORTED, "components of %d bits (at most 16)", p.bits);
            p.C = (int)C; p.W = (int)W; p.H = (int)H;
            p.XT = (int)(XT < W ? XT : W); p.YT = (int)(YT < H ? YT : H);      // (a larger tile is the image)
            have_siz = true;
        } else if (marker == 0xFF52) {
            if (len < 12) return e->fail(DEC_BAD, "short COD");
            const unsigned scod = cs.u8(q);
            p.sop = (scod >> 1) & 1; p.eph = (scod >> 2) & 1;
            if (cs.u8(q + 1) != 0) return e->fail(DEC_UNSUPPORTED, "progression order %u is not supported (LRCP only)", cs.u8(q + 1));
            if (cs.u16(q + 2) != 1) return e->fail(DEC_UNSUPPORTED, "%u quality layers are not supported (one only)", cs.u16(q + 2));
            if (cs.u8(q + 4) > 1) return e->fail(DEC_UNSUPPORTED, "multiple component transform %u is not supported (0 or 1)", cs.u8(q + 4));
            p.mct = (int)cs.u8(q + 4);
            p.NL = (int)cs.u8(q + 5);
            if (p.NL > DEC_MAX_LEVELS) return e->fail(DEC_UNSUPPORTED, "%d decompositions (at most %d)", p.NL, DEC_MAX_LEVELS);
            if ((scod & 1) && len < 12u + (unsigned)p.NL + 1)
                return e->fail(DEC_UNSUPPORTED, "precinct partition: COD of %u bytes does not hold the %d precinct sizes it announces", len, p.NL + 1);
            for (int r = 0; r <= p.NL; ++r) {      // lowest resolution first; PPx in the low nibble
                p.ppx[r] = (scod & 1) ? (int)(cs.u8(q + 10 + r) & 15) : 15;
                p.ppy[r] = (scod & 1) ? (int)(cs.u8(q + 10 + r) >> 4) : 15;
                if (r > 0 && (p.ppx[r] == 0 || p.ppy[r] == 0)) return e->fail(DEC_BAD, "precinct exponent 0 at resolution %d", r);
            }
            if (cs.u8(q + 6) > 4 || cs.u8(q + 7) > 4) return e->fail(DEC_UNSUPPORTED, "code blocks larger than 64 x 64 are not supported");
            p.cbw = 1 << (cs.u8(q + 6) + 2); p.cbh = 1 << (cs.u8(q + 7) + 2);
            if (cs.u8(q + 8) != 0) return e->fail(DEC_UNSUPPORTED, "code-block style %u is not supported (0 only)", cs.u8(q + 8));
            if (cs.u8(q + 9) != 1) return e->fail(DEC_UNSUPPORTED, "the irreversible 9/7 transform is not supported");
            have_cod = true;
        } else if (marker == 0xFF5C) {
            if (len < 4) return e->fail(DEC_BAD, "short QCD");
            if ((cs.u8(q) & 31) != 0) return e->fail(DEC_UNSUPPORTED, "quantisation is not supported (reversible streams only)");
            p.guard = (int)(cs.u8(q) >> 5);
            for (unsigned k = 0; k + 3 < len && k < 97; ++k) p.eps[k] = (int)(cs.u8(q + 1 + k) >> 3);
            have_qcd = (int)len - 3;
        } else if (marker == 0xFF53 || marker == 0xFF5D || marker == 0xFF5E || marker == 0xFF5F) {
            return e->fail(DEC_UNSUPPORTED, "marker %04X (COC / QCC / RGN / POC) is not supported", marker);
        } else if (marker == 0xFF60) {
            return e->fail(DEC_UNSUPPORTED, "packed packet headers (PPM) are not supported");
        }   // COM, TLM, PLM, CRG and anything else with a length: skipped
        at += 2 + (size_t)len;
    }
    if (!have_siz || !have_cod || have_qcd < 0) return e->fail(DEC_BAD, "SIZ, COD or QCD missing");
    if (p.mct && p.C < 3) return e->fail(DEC_UNSUPPORTED, "the component transform on %d components is not supported (T.800 has it on three)", p.C);
    if (have_qcd < 1 + 3 * p.NL) return e->fail(DEC_BAD, "QCD has %d exponents for %d bands", have_qcd, 1 + 3 * p.NL);
    for (int k = 0; k < 1 + 3 * p.NL; ++k)
        if (p.guard + p.eps[k] - 1 > 31) return e->fail(DEC_UNSUPPORTED, "%d magnitude bit-planes (at most 31)", p.guard + p.eps[k] - 1);
    p.ntx = (int)dec_cdiv(p.W, p.XT); p.nty = (int)dec_cdiv(p.H, p.YT);
    p.tw = p.XT; p.th = p.YT;
    const int64_t ntiles = (int64_t)p.ntx * p.nty;
    if (ntiles > 65535) return e->fail(DEC_BAD, "%lld tiles (a codestream holds at most 65535)", (long long)ntiles);
    if ((uint64_t)ntiles * 14 > (uint64_t)(end - at) + 14) return e->fail(DEC_BAD, "%lld tiles in %zu bytes: tile-parts are missing", (long long)ntiles, end - at);
    s->parts.resize((size_t)ntiles);
    while (cs.has(at, 12) && cs.u16(at) == 0xFF90) {
        const unsigned isot = cs.u16(at + 4);
        const uint32_t psot = cs.u32(at + 6);
        if (cs.u16(at + 2) != 10) return e->fail(DEC_BAD, "bad SOT at %zu", at);
        if ((int64_t)isot >= ntiles) return e->fail(DEC_BAD, "tile-part of tile %u, the image has %lld", isot, (long long)ntiles);
        size_t part_end;
        if (psot == 0) {
            if (end - at < 14) return e->fail(DEC_BAD, "the last tile-part has no room for EOC");
            part_end = end - 2;
        } else {
            if (psot < 14 || !cs.has(at, psot)) return e->fail(DEC_BAD, "tile-part of tile %u runs beyond the stream", isot);
            part_end = at + psot;
        }
        if (cs.u8(at + 10) != s->parts[isot].size()) return e->fail(DEC_BAD, "tile %u: tile-part %u is out of order", isot, cs.u8(at + 10));
        const Bytes tp = {f, part_end};
        size_t q = at + 12;
        for (;;) {
            if (!tp.has(q, 2)) return e->fail(DEC_BAD, "no SOD in a tile-part of tile %u", isot);
            const unsigned marker = tp.u16(q);
            if (marker == 0xFF93) break;
            if (marker == 0xFF61) return e->fail(DEC_UNSUPPORTED, "packed packet headers (PPT) are not supported");
            if (marker == 0xFF52 || marker == 0xFF53 || marker == 0xFF5C || marker == 0xFF5D || marker == 0xFF5E || marker == 0xFF5F)
                return e->fail(DEC_UNSUPPORTED, "marker %04X in a tile-part header (parameters of one tile) is not supported", marker);
            if (marker != 0xFF64 && marker != 0xFF58) return e->fail(DEC_BAD, "marker %04X in a tile-part header", marker);
            const unsigned len = tp.u16(q + 2);
            if (len < 2 || !tp.has(q + 2, len)) return e->fail(DEC_BAD, "marker segment %04X runs beyond its tile-part", marker);
            q += 2 + (size_t)len;
        }
        s->parts[isot].push_back(DecSegment{q + 2, part_end});
        at = part_end;
    }
    if (!cs.has(at, 2) || cs.u16(at) != 0xFFD9) return e->fail(DEC_BAD, "no EOC where the tile-parts end (offset %zu)", at);
    for (int64_t t = 0; t < ntiles; ++t)
        if (s->parts[(size_t)t].empty()) return e->fail(DEC_BAD, "tile %lld is missing", (long long)t);
    return DEC_OK;
}

// ------------------------------------------------------------------ packet headers (B.10)

struct BitReader {     // after a byte of 0xFF the next byte carries seven bits
    const uint8_t* in;
    size_t n, pos;
    unsigned cur, prev;
    int used;
    bool bad;
    void begin(const uint8_t* in_, size_t n_) { in = in_; n = n_; pos = 0; cur = prev = 0; used = 0; bad = false; }
    int get()
    {
        if (used == 0) {
            prev = cur;
            if (pos >= n) { bad = true; return 0; }
            cur = in[pos++];
            used = prev == 0xFF ? 7 : 8;
        }
        return (int)((cur >> --used) & 1u);
    }
    uint32_t bits(int k)
    {
        uint32_t r = 0;
        for (; k > 0; --k) r = (r << 1) | (uint32_t)get();
        return r;
    }
    void end()
    {
        used = 0;
        if (cur == 0xFF) {          // the stuffed byte after a last 0xFF
            if (pos >= n) bad = true;
            else ++pos;
        }
    }
};

struct TagTreeReader {  // B.10.2, reading: a node's value is learnt once, as zeros up to it and a one
    struct Node { int parent, value, low, known; };
    std::vector<Node> nodes;
    void build(int w, int h)
    {
        nodes.clear();
        std::vector<int> lw, lh, first;
        int cw = w, ch = h, total = 0;
        for (;;) {
            lw.push_back(cw); lh.push_back(ch); first.push_back(total);
            total += cw * ch;
            if (cw * ch <= 1) break;
            cw = (cw + 1) / 2; ch = (ch + 1) / 2;
        }
        nodes.assign((size_t)total, Node{-1, 0x3FFFFFFF, 0, 0});
        for (size_t l = 0; l + 1 < lw.size(); ++l)
            for (int y = 0; y < lh[l]; ++y)
                for (int x = 0; x < lw[l]; ++x)
                    nodes[(size_t)(first[l] + y * lw[l] + x)].parent = first[l + 1] + (y / 2) * lw[l + 1] + x / 2;
    }
    // whether the leaf's value is known to lie below the threshold, reading what is needed to tell
    bool below(BitReader& br, int leaf, int threshold)
    {
        int stack[40], sp = 0, node = leaf;
        while (nodes[(size_t)node].parent >= 0 && sp < 40) { stack[sp++] = node; node = nodes[(size_t)node].parent; }
        int low = 0;
        for (;;) {
            Node& nd = nodes[(size_t)node];
            if (low < nd.low) low = nd.low;
            while (low < threshold && !nd.known && !br.bad) {
                if (br.get()) { nd.value = low; nd.known = 1; }
                else ++low;
            }
            if (nd.known && low < nd.value) low = nd.value;
            nd.low = low;
            if (!sp) break;
            node = stack[--sp];
        }
        const Node& lf = nodes[(size_t)leaf];
        return lf.known && lf.value < threshold;
    }
};


inline int dec_get_passes(BitReader& br)   // Table B.4
{
    if (!br.get()) return 1;
    if (!br.get()) return 2;
    uint32_t v = br.bits(2);
    if (v < 3) return 3 + (int)v;
    v = br.bits(5);
    if (v < 31) return 6 + (int)v;
    return 37 + (int)br.bits(7);
}

// One packet header of the only layer.  rec: three values per block of the packet (band by band, raster order):
// passes (0: not included), numbps, bytes.  Returns the header's length, or -1 when it runs beyond `n` or announces a
// length of more than 31 bits.
inline int64_t dec_packet_header(const uint8_t* in, size_t n, int nbands, const int32_t* gw, const int32_t* gh, const int32_t* mb, int32_t* rec)
{
    BitReader br;
    br.begin(in, n);
    int64_t total = 0;
    for (int k = 0; k < nbands; ++k) total += (int64_t)gw[k] * gh[k];
    for (int64_t k = 0; k < 3 * total; ++k) rec[k] = 0;
    if (!br.get()) {          // an empty packet
        br.end();
        return br.bad ? -1 : (int64_t)br.pos;
    }
    int32_t* r = rec;
    TagTreeReader ti, tz;
    for (int k = 0; k < nbands && !br.bad; ++k) {
        const int nblk = gw[k] * gh[k];
        if (!nblk) continue;
        ti.build(gw[k], gh[k]);
        tz.build(gw[k], gh[k]);
        for (int i = 0; i < nblk && !br.bad; ++i, r += 3) {
            if (!ti.below(br, i, 1)) continue;          // not in this (the only) layer
            int z = 1;
            while (!tz.below(br, i, z) && !br.bad && z < 64) ++z;
            --z;
            const int passes = dec_get_passes(br);
            int lblock = 3;
            while (br.get() && !br.bad) ++lblock;
            const int nbits = lblock + floor_log2((uint32_t)passes);
            if (nbits > 31) return -1;
            r[0] = passes;
            r[1] = mb[k] - z;
            r[2] = (int32_t)br.bits(nbits);
        }
    }
    br.end();
    return br.bad ? -1 : (int64_t)br.pos;
}

// ------------------------------------------------------------------ the block table

// Parses every packet of every tile.  out: one record per code block, validated (see the head of this file).
inline int dec_parse(const uint8_t* f, size_t n, const DecStream& s, std::vector<DecBlock>* out, DecError* e)
{
    const DecParams& p = s.p;
    const Bytes in = {f, n};
    const int64_t total = dec_count_blocks(p, e);
    if (total < 0) return (int)total;
    out->clear();
    std::vector<int32_t> r3;
    for (int t = 0; t < p.ntx * p.nty; ++t) {
        const std::vector<DecSegment>& segs = s.parts[(size_t)t];
        size_t seg = 0;
        size_t at = segs[0].at, end = segs[0].end;
        if (end > n || at > end) return e->fail(DEC_BAD, "tile %d: its tile-part lies beyond the buffer", t);
        for (int r = 0; r <= p.NL; ++r)
            for (int c = 0; c < p.C; ++c) {
                DecRes rs;
                const int nbands = dec_bands(p, t, r, &rs);
                if (nbands <= 0) continue;
                const Band* bd = rs.bd;
                for (int64_t pr = 0; pr < rs.npx * rs.npy; ++pr) {      // one packet per precinct, with or without blocks
                    while (at == end && seg + 1 < segs.size()) {      // the next tile-part of this tile
                        ++seg;
                        at = segs[seg].at; end = segs[seg].end;
                        if (end > n || at > end) return e->fail(DEC_BAD, "tile %d: its tile-part lies beyond the buffer", t);
                    }
                    int32_t gx0[3], gy0[3], gw[3], gh[3], mb[3];
                    int64_t nblk = 0;
                    for (int b = 0; b < nbands; ++b) {
                        dec_precinct_blocks(rs, b, pr % rs.npx, pr / rs.npx, &gx0[b], &gy0[b], &gw[b], &gh[b]);
                        mb[b] = bd[b].mb;
                        nblk += (int64_t)gw[b] * gh[b];
                    }
                    if (p.sop && end - at >= 6 && in.u16(at) == 0xFF91) at += 6;
                    r3.assign((size_t)(nblk ? nblk : 1) * 3, 0);
                    const int64_t used = dec_packet_header(f + at, end - at, nbands, gw, gh, mb, r3.data());
                    if (used < 0) return e->fail(DEC_BAD, "tile %d, resolution %d, component %d: the packet header runs beyond its tile-part", t, r, c);
                    at += (size_t)used;
                    if (at > end) return e->fail(DEC_BAD, "tile %d: a packet header runs beyond its tile-part", t);
                    if (p.eph) {
                        if (end - at < 2 || in.u16(at) != 0xFF92) return e->fail(DEC_BAD, "tile %d, resolution %d, component %d: EPH missing", t, r, c);
                        at += 2;
                    }
                    int64_t i = 0;
                    for (int b = 0; b < nbands; ++b)
                        for (int gy = gy0[b]; gy < gy0[b] + gh[b]; ++gy)
                            for (int gx = gx0[b]; gx < gx0[b] + gw[b]; ++gx, ++i) {
                                DecBlock k;
                                memset(&k, 0, sizeof k);
                                k.tile = t; k.comp = c; k.res = r; k.band = b; k.gx = gx; k.gy = gy; k.prec = (int32_t)pr;
                                k.mb = bd[b].mb; k.orient = bd[b].orient;
                                dec_block_rect(rs, bd[b], gx, gy, &k.x, &k.y, &k.w, &k.h);
                                k.passes = r3[(size_t)(3 * i)]; k.numbps = r3[(size_t)(3 * i + 1)]; k.length = r3[(size_t)(3 * i + 2)];
                                k.offset = -1;
                                if (k.w < 1 || k.h < 1 || k.w > 64 || k.h > 64 || k.x < 0 || k.y < 0 || k.x + k.w > p.tw || k.y + k.h > p.th)
                                    return e->fail(DEC_BAD, "tile %d: a code block of %d x %d at (%d, %d)", t, k.w, k.h, k.x, k.y);
                                if (k.passes) {
                                    if (k.mb < 0 || k.mb > 31 || k.numbps < 1 || k.numbps > k.mb || k.passes < 1 || k.passes > 3 * k.numbps - 2)
                                        return e->fail(DEC_BAD, "tile %d, resolution %d, component %d: a block of %d passes in %d of %d bit-planes",
                                                       t, r, c, k.passes, k.numbps, k.mb);
                                    if (k.length < 0 || (size_t)k.length > end - at)
                                        return e->fail(DEC_BAD, "tile %d: block data runs beyond the tile-part", t);
                                    k.offset = (int64_t)at;
                                    at += (size_t)k.length;
                                }
                                out->push_back(k);
                            }
                }
            }
        if (at != end || seg + 1 != segs.size())
            return e->fail(DEC_BAD, "tile %d: %zu bytes of its tile-parts are not accounted for", t, end - at);
    }
    if ((int64_t)out->size() != total) return e->fail(DEC_BAD, "%zu code blocks parsed, the geometry has %lld", out->size(), (long long)total);
    return DEC_OK;
}

}  // namespace jp2k
