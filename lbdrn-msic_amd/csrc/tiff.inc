// The TIFF reader's format text (include/lbdrn_tiff.h), written once for the device and the host: the segment geometry of
// a layout, and the three segment decoders -- Deflate (RFC 1950 / 1951), TIFF LZW and PackBits.  csrc/tiff.hip compiles it
// for the kernels, tests/tiff_host_shim.cpp and tests/tiff_damage_main.cpp compile the same text with a host compiler.
// No state, no allocation, no I/O.
//
// Every decoder is written for `nl` cooperating lanes that all run the same control flow on the same values (the device
// passes its lane and 64, the host 0 and 1): the bit decoding is done by every lane alike, the bulk work -- staging input,
// copying literal runs and matches, filling the fast Huffman table, the Adler-32 sums -- is shared out by lane.  Tables
// live in memory the caller hands in (LDS on the device).  Lanes of one wave see each other's LDS accesses in program
// order (the LDS serves a wave's instructions in order), so TIFF_WAVE_FENCE only has to keep the compiler from reordering;
// output bytes that other lanes wrote to global memory are read back once per segment, after TIFF_MEM_SYNC.
//
// Bounds: a decoder reads in[0 .. n) and writes out[0 .. expect), nothing else, whatever the stream holds; every loop
// iteration consumes at least one input bit or produces at least one output byte, or ends the segment with a status.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lbdrn_tiff.h"

#if defined(__HIPCC__)
#define TIFF_HD __host__ __device__ inline
#else
#define TIFF_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define TIFF_WAVE_FENCE() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront")
#define TIFF_MEM_SYNC() __syncthreads()
#else
#define TIFF_WAVE_FENCE() ((void)0)
#define TIFF_MEM_SYNC() ((void)0)
#endif

namespace tiff {

constexpr int COMP_NONE = 1, COMP_LZW = 5, COMP_DEFLATE = 8, COMP_PACKBITS = 32773;
constexpr int MAX_C = 65535, MAX_SIDE = 1 << 20;
constexpr int64_t MAX_SEGMENTS = (int64_t)1 << 30;

// status[s] of a damaged segment
constexpr int ST_OK = 0;
constexpr int ST_TRUNCATED = 1;      // the stream ends before the segment's expected size is produced
constexpr int ST_BAD_CODE = 2;       // an invalid Huffman code, block type, stored length, LZW code or PackBits run
constexpr int ST_BAD_DISTANCE = 3;   // a match distance points before the segment's start
constexpr int ST_BAD_HEADER = 4;     // the zlib header is not a Deflate stream's
constexpr int ST_BAD_CHECK = 5;      // the Adler-32 is wrong

// The segment cap: the largest uncompressed segment the device decodes, per codec, set so that one segment alone -- one
// wave, the unit of parallelism -- takes at most 0.25 s at the rate measured for a lone segment on an MI355X
// (profiles/tiff_read_timing.txt, scripts/tiff_read_timing.py):
//     Deflate    4.43 MB/s of output on literal-heavy streams (predicted 16-bit scene samples, dynamic or fixed blocks; stored
//                blocks 281 MB/s, a constant raster 180 MB/s)  ->  1.06 MiB in 0.25 s; the cap is 768 KiB (0.18 s)
//     LZW        1.81 MB/s on noise (2.73 MB/s on scene samples, 14.1 MB/s on a constant raster)  ->  0.43 MiB; the cap is 384 KiB
//     PackBits   183.0 MB/s (literal runs of scene samples; 209 MB/s noise)  ->  43.6 MiB; the cap is 40 MiB
// Uncompressed segments are only placed, by as many workgroups as they have rows: no cap beyond the layout's own limits.
constexpr size_t CAP_DEFLATE = (size_t)768 << 10;
constexpr size_t CAP_LZW = (size_t)384 << 10;
constexpr size_t CAP_PACKBITS = (size_t)40 << 20;
constexpr size_t CAP_NONE = (size_t)1 << 46;      // 2^20 x 2^20 x 65535 samples of 2 bytes stay below it

TIFF_HD size_t segment_cap(int compression)
{
    return compression == COMP_DEFLATE ? CAP_DEFLATE : compression == COMP_LZW ? CAP_LZW
         : compression == COMP_PACKBITS ? CAP_PACKBITS : compression == COMP_NONE ? CAP_NONE : 0;
}

// ---------------------------------------------------------------- geometry

struct Geom {
    int C, H, W;
    int bps;            // bytes per sample
    int spp;            // samples per pixel inside a segment: C chunky, 1 planar
    int seg_w, seg_h, segs_x, segs_y, tiled, big_endian, predictor, compression;
    int64_t per_plane;  // segments of one plane (all of them when chunky)
    int64_t nseg;
    int64_t row_bytes;  // bytes of one segment row
    int64_t seg_bytes;  // bytes of a full segment
    int64_t pitch;      // bytes between two segments' slots in the workspace
};

TIFF_HD bool make_geom(const lbdrn_tiff_layout& L, Geom* g)
{
    if (L.C < 1 || L.C > MAX_C || L.H < 1 || L.H > MAX_SIDE || L.W < 1 || L.W > MAX_SIDE) return false;
    if (L.bits != 8 && L.bits != 16) return false;
    if ((L.big_endian | 1) != 1 || (L.tiled | 1) != 1 || (L.planar != 1 && L.planar != 2)) return false;
    if (L.predictor != 1 && L.predictor != 2) return false;
    if (L.compression != COMP_NONE && L.compression != COMP_LZW && L.compression != COMP_DEFLATE && L.compression != COMP_PACKBITS) return false;
    if (L.seg_w < 1 || L.seg_w > MAX_SIDE || L.seg_h < 1 || L.seg_h > MAX_SIDE) return false;
    if (!L.tiled && (L.seg_w != L.W || L.seg_h > L.H)) return false;
    g->C = L.C; g->H = L.H; g->W = L.W;
    g->bps = L.bits / 8;
    g->spp = L.planar == 1 ? L.C : 1;
    g->seg_w = L.seg_w; g->seg_h = L.seg_h;
    g->segs_x = (L.W + L.seg_w - 1) / L.seg_w;
    g->segs_y = (L.H + L.seg_h - 1) / L.seg_h;
    g->tiled = L.tiled; g->big_endian = L.big_endian; g->predictor = L.predictor; g->compression = L.compression;
    g->per_plane = (int64_t)g->segs_x * g->segs_y;
    g->nseg = g->per_plane * (L.planar == 2 ? L.C : 1);
    g->row_bytes = (int64_t)L.seg_w * g->spp * g->bps;
    g->seg_bytes = g->row_bytes * L.seg_h;
    g->pitch = (g->seg_bytes + 15) / 16 * 16;
    return g->nseg <= MAX_SEGMENTS && g->nseg * (int64_t)L.seg_h < ((int64_t)1 << 31);
}
// rows of segment s that lie inside the image
TIFF_HD int seg_rows(const Geom& g, int64_t s)
{
    const int y0 = (int)((s % g.per_plane) / g.segs_x) * g.seg_h;
    return g.H - y0 < g.seg_h ? g.H - y0 : g.seg_h;
}
// bytes segment s holds once decompressed: a tile is always whole in the file, the last strip may be short
TIFF_HD int64_t seg_expected(const Geom& g, int64_t s) { return g.tiled ? g.seg_bytes : g.row_bytes * seg_rows(g, s); }

// ---------------------------------------------------------------- input staging

constexpr uint32_t STAGE = 512;      // bytes of the stream held in the table memory at a time

struct Input {
    const uint8_t* in;
    size_t n;
    uint8_t* stage;      // [STAGE]
    size_t base;         // stage holds in[base .. base + STAGE), as far as the stream reaches
    int lane, nl;
    TIFF_HD void init(const uint8_t* in_, size_t n_, uint8_t* stage_, int lane_, int nl_)
    {
        in = in_; n = n_; stage = stage_; lane = lane_; nl = nl_;
        base = ~(size_t)0 - STAGE;      // nothing staged
    }
    // the byte at i < n
    TIFF_HD uint32_t byte(size_t i)
    {
        if (i - base >= (size_t)STAGE) {
            TIFF_WAVE_FENCE();
            base = i >= 8 ? i - 8 : 0;      // a little behind: the LZW reader steps back by up to two bytes
            for (uint32_t k = (uint32_t)lane; k < STAGE; k += (uint32_t)nl)
                if (base + k < n) stage[k] = in[base + k];
            TIFF_WAVE_FENCE();
        }
        return stage[i - base];
    }
};

// ---------------------------------------------------------------- Adler-32 of out[0 .. n), the lanes sharing the bytes

TIFF_HD uint64_t lane_sum(uint64_t v, int nl)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);      // (each lane's share is below 2^56: no carry is lost in 64 bits)
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t other = ((uint64_t)(uint32_t)__shfl_xor((int)hi, o, 64) << 32) | (uint32_t)__shfl_xor((int)lo, o, 64);
        v += other;
        lo = (uint32_t)v; hi = (uint32_t)(v >> 32);
    }
#endif
    (void)nl;
    return v;
}

// s1 = 1 + sum b[j], s2 = n + sum (n - j) b[j], both modulo 65521
TIFF_HD uint32_t adler32(const uint8_t* out, size_t n, int lane, int nl)
{
    constexpr uint32_t M = 65521u;
    uint64_t a1 = 0, a2 = 0;
    if ((size_t)lane < n) {
        uint32_t w = (uint32_t)((n - (size_t)lane) % M);      // (n - j) mod M, stepped down by nl per byte
        for (size_t j = (size_t)lane; j < n; j += (size_t)nl) {
            const uint32_t b = out[j];
            a1 += b;
            a2 += (uint64_t)w * b;                              // < 2^24 a term, at most 2^32 terms
            w = w >= (uint32_t)nl ? w - (uint32_t)nl : w + M - (uint32_t)nl;
        }
    }
    a1 = lane_sum(a1, nl);
    a2 = lane_sum(a2 % M, nl);
    const uint32_t s1 = (uint32_t)((1u + a1) % M), s2 = (uint32_t)((n % M + a2) % M);
    return (s2 << 16) | s1;
}

// ---------------------------------------------------------------- Deflate

constexpr uint32_t WINDOW = 32768;     // the history a match may reach into, kept as a ring in the table memory
constexpr int LIT_FAST = 10, DIST_FAST = 9;      // bits looked up at once; longer codes walk the canonical counts
constexpr int MAXBITS = 15, MAXLCODES = 286, MAXDCODES = 30, FIXLCODES = 288;

struct Huffman {
    uint16_t count[MAXBITS + 1];     // codes of each length
    uint16_t start[MAXBITS + 1];     // index in symbol[] of the first code of each length
    uint16_t first[MAXBITS + 1];     // the canonical code of that symbol
    uint16_t next[MAXBITS + 1];      // fill positions while symbol[] is ordered
    uint16_t symbol[FIXLCODES];      // symbols ordered by code
};

struct InflateTables {
    uint8_t window[WINDOW];
    uint8_t stage[STAGE];
    uint8_t lens[FIXLCODES + 32];
    Huffman lit, dist;
    uint16_t lit_fast[1 << LIT_FAST];      // symbol | length << 12; 0: not a code of at most LIT_FAST bits
    uint16_t dist_fast[1 << DIST_FAST];
};

TIFF_HD uint32_t reverse_bits(uint32_t v, int n)
{
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0F0Fu) << 4) | ((v >> 4) & 0x0F0Fu);
    v = ((v & 0x00FFu) << 8) | ((v >> 8) & 0x00FFu);
    return v >> (16 - n);
}

// Canonical code of lens[0 .. n): > 0 incomplete, 0 complete, < 0 over-subscribed.  Lane 0 orders the symbols, the lanes
// share the fast table: entry [the next fast_bits of the stream] of every code that short.
TIFF_HD int build_huffman(Huffman* h, uint16_t* fast, int fast_bits, const uint8_t* lens, int n, int lane, int nl)
{
    TIFF_WAVE_FENCE();
    if (lane == 0) {
        _Pragma("unroll 1") for (int l = 0; l <= MAXBITS; ++l) h->count[l] = 0;
        _Pragma("unroll 1") for (int s = 0; s < n; ++s) h->count[lens[s] & 15]++;
    }
    _Pragma("unroll 1") for (int k = lane; k < (1 << fast_bits); k += nl) fast[k] = 0;
    TIFF_WAVE_FENCE();
    int left = 1;
    _Pragma("unroll 1") for (int l = 1; l <= MAXBITS; ++l) {
        left = left * 2 - (int)h->count[l];
        if (left < 0) return left;
    }
    if (lane == 0) {
        uint32_t at = 0, code = 0;
        _Pragma("unroll 1") for (int l = 1; l <= MAXBITS; ++l) {
            h->start[l] = h->next[l] = (uint16_t)at;
            h->first[l] = (uint16_t)code;
            at += h->count[l];
            code = (code + h->count[l]) << 1;
        }
        _Pragma("unroll 1") for (int s = 0; s < n; ++s) {
            const int l = lens[s] & 15;
            if (l) h->symbol[h->next[l]++] = (uint16_t)s;
        }
    }
    TIFF_WAVE_FENCE();
    const int coded = n - (int)h->count[0];
    _Pragma("unroll 1") for (int k = lane; k < coded; k += nl) {
        const uint32_t s = h->symbol[k];
        const int l = lens[s] & 15;
        if (l > fast_bits) continue;
        const uint32_t code = (uint32_t)h->first[l] + ((uint32_t)k - h->start[l]);
        _Pragma("unroll 1") for (uint32_t e = reverse_bits(code, l); e < (1u << fast_bits); e += 1u << l) fast[e] = (uint16_t)(s | ((uint32_t)l << 12));
    }
    TIFF_WAVE_FENCE();
    return left;
}

struct BitsLSB {      // RFC 1951: bits from the least significant end of each byte
    Input* src;
    size_t ip;
    uint64_t buf;
    int cnt;
    TIFF_HD void init(Input* s, size_t at) { src = s; ip = at; buf = 0; cnt = 0; }
    // at least 25 bits afterwards, or all the stream has left: four staged bytes at once (one wait for four LDS reads), byte
    // by byte at the edge of the stage and at the stream's end
    TIFF_HD void refill()
    {
        if (cnt <= 32 && ip + 4 <= src->n && ip - src->base <= (size_t)(STAGE - 4)) {
            const uint8_t* p = src->stage + (ip - src->base);
            const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
            buf |= (uint64_t)v << cnt;
            cnt += 32; ip += 4;
            return;
        }
        while (cnt <= 24 && ip < src->n) { buf |= (uint64_t)src->byte(ip++) << cnt; cnt += 8; }
    }
    // k <= 16 bits; false: the stream ends first
    TIFF_HD bool take(int k, uint32_t* v)
    {
        if (cnt < k) { refill(); if (cnt < k) return false; }
        *v = (uint32_t)buf & ((1u << k) - 1u);
        buf >>= k; cnt -= k;
        return true;
    }
    TIFF_HD void align() { const int r = cnt & 7; buf >>= r; cnt -= r; }
    // the byte position of the next unread bit, after align()
    TIFF_HD size_t position() const { return ip - (size_t)(cnt >> 3); }
};

// one symbol: >= 0, or -ST_TRUNCATED / -ST_BAD_CODE
TIFF_HD int huffman_symbol(BitsLSB* b, const Huffman* h, const uint16_t* fast, int fast_bits)
{
    if (b->cnt < MAXBITS) b->refill();
    const uint32_t e = fast[(uint32_t)b->buf & ((1u << fast_bits) - 1u)];
    if (e) {
        const int l = (int)(e >> 12);
        if (l > b->cnt) return -ST_TRUNCATED;
        b->buf >>= l; b->cnt -= l;
        return (int)(e & 0xFFFu);
    }
    int code = 0, first = 0, index = 0;
    uint64_t bits = b->buf;
    _Pragma("unroll 1") for (int l = 1; l <= MAXBITS; ++l) {
        if (l > b->cnt) return -ST_TRUNCATED;
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int count = h->count[l];
        if (code - count < first) {
            b->buf >>= l; b->cnt -= l;
            return h->symbol[index + (code - first)];
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return -ST_BAD_CODE;
}

// in[0 .. n): a zlib stream.  out[0 .. expect).  Returns the segment's status.
TIFF_HD int inflate(const uint8_t* in, size_t n, uint8_t* out, size_t expect, InflateTables* t, int lane, int nl)
{
    Input src;
    src.init(in, n, t->stage, lane, nl);
    if (n < 2) return ST_TRUNCATED;
    const uint32_t cmf = src.byte(0), flg = src.byte(1);
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) return ST_BAD_HEADER;
    BitsLSB b;
    b.init(&src, 2);
    size_t pos = 0;
    bool longer = false;      // the stream holds more than the segment: decoding stops at the expected size
    uint32_t last = 0;
    while (!last && !longer) {
        uint32_t type, v;
        if (!b.take(1, &last) || !b.take(2, &type)) return ST_TRUNCATED;
        if (type == 3) return ST_BAD_CODE;
        if (type == 0) {      // stored
            b.align();
            uint32_t len, nlen;
            if (!b.take(16, &len) || !b.take(16, &nlen)) return ST_TRUNCATED;
            if ((len ^ 0xFFFFu) != nlen) return ST_BAD_CODE;
            const size_t at = b.position();
            if (at + len > n) return ST_TRUNCATED;
            size_t take = len;
            if (take > expect - pos) { take = expect - pos; longer = true; }
            TIFF_WAVE_FENCE();
            for (size_t i = (size_t)lane; i < take; i += (size_t)nl) {
                const uint8_t c = in[at + i];
                out[pos + i] = c;
                if (i + WINDOW >= take) t->window[(pos + i) & (WINDOW - 1)] = c;
            }
            TIFF_WAVE_FENCE();
            pos += take;
            b.init(&src, at + len);
            continue;
        }
        if (type == 1) {      // fixed code
            if (lane == 0) {
                for (int s = 0; s < FIXLCODES; ++s) t->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
                for (int s = 0; s < MAXDCODES; ++s) t->lens[FIXLCODES + s] = 5;
            }
            build_huffman(&t->lit, t->lit_fast, LIT_FAST, t->lens, FIXLCODES, lane, nl);
            build_huffman(&t->dist, t->dist_fast, DIST_FAST, t->lens + FIXLCODES, MAXDCODES, lane, nl);
        } else {              // dynamic code
            uint32_t nlen, ndist, ncode;
            if (!b.take(5, &nlen) || !b.take(5, &ndist) || !b.take(4, &ncode)) return ST_TRUNCATED;
            nlen += 257; ndist += 1; ncode += 4;
            if (nlen > (uint32_t)MAXLCODES || ndist > (uint32_t)MAXDCODES) return ST_BAD_CODE;
            // the code length code's lengths, in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 (5 bits each)
            const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                                      10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
            const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
            TIFF_WAVE_FENCE();
            if (lane == 0)
                for (int s = 0; s < 19; ++s) t->lens[s] = 0;
            for (uint32_t i = 0; i < ncode; ++i) {
                if (!b.take(3, &v)) return ST_TRUNCATED;
                const uint32_t at = i < 12 ? (uint32_t)(order_lo >> (5 * i)) & 31u : (uint32_t)(order_hi >> (5 * (i - 12))) & 31u;
                if (lane == 0) t->lens[at] = (uint8_t)v;
            }
            if (build_huffman(&t->lit, t->lit_fast, LIT_FAST, t->lens, 19, lane, nl) != 0) return ST_BAD_CODE;
            // the literal/length and distance lengths.  t->lens is rewritten while t->lit decodes them: decoding reads
            // count[], symbol[] and the fast table, which are complete, and never lens[]
            uint8_t* cl = t->lens;
            uint32_t index = 0, prev = 0;
            while (index < nlen + ndist) {
                const int sym = huffman_symbol(&b, &t->lit, t->lit_fast, LIT_FAST);
                if (sym < 0) return -sym;
                uint32_t rep = 1, val = (uint32_t)sym;
                if (sym >= 16) {
                    if (sym == 16) {
                        if (index == 0) return ST_BAD_CODE;
                        if (!b.take(2, &v)) return ST_TRUNCATED;
                        val = prev; rep = 3 + v;
                    } else if (sym == 17) {
                        if (!b.take(3, &v)) return ST_TRUNCATED;
                        val = 0; rep = 3 + v;
                    } else {
                        if (!b.take(7, &v)) return ST_TRUNCATED;
                        val = 0; rep = 11 + v;
                    }
                    if (index + rep > nlen + ndist) return ST_BAD_CODE;
                }
                if (lane == 0)
                    for (uint32_t r = 0; r < rep; ++r) {
                        const uint32_t k = index + r;      // distance lengths start at a fixed place behind the literals'
                        cl[k < nlen ? k : FIXLCODES + (k - nlen)] = (uint8_t)val;
                    }
                index += rep;
                prev = val;
            }
            TIFF_WAVE_FENCE();
            if (t->lens[256] == 0) return ST_BAD_CODE;      // no end-of-block code
            int left = build_huffman(&t->lit, t->lit_fast, LIT_FAST, t->lens, (int)nlen, lane, nl);
            if (left < 0 || (left > 0 && (int)nlen != (int)t->lit.count[0] + (int)t->lit.count[1])) return ST_BAD_CODE;      // incomplete: one code of one bit at most
            left = build_huffman(&t->dist, t->dist_fast, DIST_FAST, t->lens + FIXLCODES, (int)ndist, lane, nl);
            if (left < 0 || (left > 0 && (int)ndist != (int)t->dist.count[0] + (int)t->dist.count[1])) return ST_BAD_CODE;
        }
        for (;;) {      // the block's symbols
            const int sym = huffman_symbol(&b, &t->lit, t->lit_fast, LIT_FAST);
            if (sym < 0) return -sym;
            if (sym == 256) break;
            if (pos >= expect) { longer = true; break; }
            if (sym < 256) {
                if (lane == 0) {
                    out[pos] = (uint8_t)sym;
                    t->window[pos & (WINDOW - 1)] = (uint8_t)sym;
                }
                ++pos;
                continue;
            }
            const uint32_t li = (uint32_t)sym - 257u;
            if (li >= 29u) return ST_BAD_CODE;
            uint32_t len, extra = 0;
            if (li < 8u) len = 3u + li;
            else if (li == 28u) len = 258u;
            else {
                const int eb = (int)(li >> 2) - 1;
                if (!b.take(eb, &extra)) return ST_TRUNCATED;
                len = 3u + ((4u + (li & 3u)) << eb) + extra;
            }
            const int ds = huffman_symbol(&b, &t->dist, t->dist_fast, DIST_FAST);
            if (ds < 0) return -ds;
            if (ds >= MAXDCODES) return ST_BAD_CODE;
            uint32_t dist;
            if (ds < 4) dist = 1u + (uint32_t)ds;
            else {
                const int eb = (ds >> 1) - 1;
                if (!b.take(eb, &extra)) return ST_TRUNCATED;
                dist = 1u + ((2u + ((uint32_t)ds & 1u)) << eb) + extra;
            }
            if ((size_t)dist > pos) return ST_BAD_DISTANCE;
            if ((size_t)len > expect - pos) { len = (uint32_t)(expect - pos); longer = true; }
            // every source byte lies before pos: byte i of the match is byte i mod dist of the dist bytes in front of it
            TIFF_WAVE_FENCE();
            const size_t from = pos - dist;
            for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)nl) {
                const uint32_t j = dist >= len ? i : i % dist;
                const uint8_t c = t->window[(from + j) & (WINDOW - 1)];
                t->window[(pos + i) & (WINDOW - 1)] = c;
                out[pos + i] = c;
            }
            TIFF_WAVE_FENCE();
            pos += len;
            if (longer) break;
        }
    }
    if (pos < expect) return ST_TRUNCATED;
    if (longer) return ST_OK;      // stopped at the expected size, in front of the stream's end: its check is not reached
    b.align();
    uint32_t want = 0, v;
    for (int k = 0; k < 4; ++k) {
        if (!b.take(8, &v)) return ST_TRUNCATED;
        want = (want << 8) | v;
    }
    TIFF_MEM_SYNC();      // the bytes the other lanes wrote
    return adler32(out, expect, lane, nl) == want ? ST_OK : ST_BAD_CHECK;
}

// ---------------------------------------------------------------- TIFF LZW

constexpr int LZW_CLEAR = 256, LZW_EOI = 257, LZW_FIRST = 258, LZW_CODES = 4096;

struct LzwTables {
    uint32_t entry[LZW_CODES];      // of codes >= 258: prefix code | last byte << 12 | length << 20 (a string is at most 3839 bytes)
    uint8_t stage[STAGE];
};

// MSB-first codes of 9 .. 12 bits, Clear = 256, EOI = 257, "early change": the width grows once the table holds 511,
// 1023, 2047 entries.  The string of a code is written back to front along its prefix chain; lane 0 stores.
TIFF_HD int lzw(const uint8_t* in, size_t n, uint8_t* out, size_t expect, LzwTables* t, int lane, int nl)
{
    Input src;
    src.init(in, n, t->stage, lane, nl);
    const uint64_t total_bits = (uint64_t)n * 8u;
    uint64_t bit = 0;
    size_t pos = 0;
    int width = 9;
    uint32_t next = LZW_FIRST;
    int prev = -1;               // the code before this one, -1 after a Clear
    uint32_t prev_first = 0;     // the first byte of its string
    while (pos < expect) {
        if (bit + (uint64_t)width > total_bits) return ST_TRUNCATED;
        const size_t at = (size_t)(bit >> 3);
        uint32_t v = src.byte(at) << 16;
        if (at + 1 < n) v |= src.byte(at + 1) << 8;
        if (at + 2 < n) v |= src.byte(at + 2);
        const uint32_t code = (v >> (24 - (int)(bit & 7u) - width)) & ((1u << width) - 1u);
        bit += (uint64_t)width;
        if (code == (uint32_t)LZW_EOI) return ST_TRUNCATED;
        if (code == (uint32_t)LZW_CLEAR) {
            width = 9; next = LZW_FIRST; prev = -1;
            continue;
        }
        if (prev < 0) {          // the first code after a Clear is a byte
            if (code > 255u) return ST_BAD_CODE;
            if (lane == 0) out[pos] = (uint8_t)code;
            ++pos;
            prev = (int)code; prev_first = code;
            continue;
        }
        if (code > next || (code == next && next >= (uint32_t)LZW_CODES)) return ST_BAD_CODE;
        // the string: that of `code`, or, where the code is the entry about to be made, prev's string and its first byte
        uint32_t c = code == next ? (uint32_t)prev : code;
        const uint32_t len = (c < 256u ? 1u : (t->entry[c] >> 20)) + (code == next ? 1u : 0u);
        size_t p = pos + len;
        if (code == next) {
            --p;
            if (p < expect && lane == 0) out[p] = (uint8_t)prev_first;
        }
        while (c >= (uint32_t)LZW_FIRST) {      // prefix codes fall strictly: an entry is made from a code already in the table
            const uint32_t e = t->entry[c];
            --p;
            if (p < expect && lane == 0) out[p] = (uint8_t)(e >> 12);
            c = e & 0xFFFu;
        }
        if (c > 255u) return ST_BAD_CODE;        // (a chain cannot end in Clear or EOI; kept as a guard)
        if (lane == 0) out[pos] = (uint8_t)c;   // p == pos + 1 here
        const uint32_t first = c;
        if (next < (uint32_t)LZW_CODES) {
            const uint32_t plen = (uint32_t)prev < 256u ? 1u : (t->entry[prev] >> 20);
            TIFF_WAVE_FENCE();
            if (lane == 0) t->entry[next] = (uint32_t)prev | (first << 12) | ((plen + 1u) << 20);
            TIFF_WAVE_FENCE();
            ++next;
            if (next == (1u << width) - 1u && width < 12) ++width;
        }
        pos = len > expect - pos ? expect : pos + len;
        prev = (int)code; prev_first = first;
    }
    return ST_OK;
}

// ---------------------------------------------------------------- PackBits

struct PackBitsTables {
    uint8_t stage[STAGE];
};

TIFF_HD int packbits(const uint8_t* in, size_t n, uint8_t* out, size_t expect, PackBitsTables* t, int lane, int nl)
{
    Input src;
    src.init(in, n, t->stage, lane, nl);
    size_t ip = 0, pos = 0;
    while (pos < expect) {
        if (ip >= n) return ST_TRUNCATED;
        const uint32_t c = src.byte(ip++);
        if (c == 128u) continue;                 // the no-op byte
        if (c < 128u) {                          // c + 1 literal bytes
            const size_t run = c + 1u;
            if (run > n - ip) return ST_TRUNCATED;
            if (run > expect - pos) return ST_BAD_CODE;
            for (size_t i = (size_t)lane; i < run; i += (size_t)nl) out[pos + i] = in[ip + i];
            ip += run; pos += run;
        } else {                                 // the next byte 257 - c times
            const size_t run = 257u - c;
            if (ip >= n) return ST_TRUNCATED;
            const uint8_t v = (uint8_t)src.byte(ip++);
            if (run > expect - pos) return ST_BAD_CODE;
            for (size_t i = (size_t)lane; i < run; i += (size_t)nl) out[pos + i] = v;
            pos += run;
        }
    }
    return ST_OK;
}

}  // namespace tiff
