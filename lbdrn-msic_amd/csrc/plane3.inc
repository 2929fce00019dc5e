// The LBB3 payload's format text (include/lbdrn_plane3.h), written once for the device and the host: geometry and bounds,
// the eight modes, the mode words, the header and the host-side validation of a body's table.  The spatial predictors,
// the fold and the lane coder in both directions are csrc/plane_lane.inc, the one text LBB2 (csrc/plane_codec.hip) is built
// from as well; their names are reachable as plane3:: too.  csrc/plane3.hip compiles this file for the kernels,
// tests/plane3_host_shim.cpp and tests/plane3_damage_main.cpp compile the same text with a host compiler.  No state, no
// allocation, no I/O.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "plane_lane.inc"

#define P3_HD PL_HD

namespace plane3 {

using plane_lane::T, plane_lane::NSPATIAL, plane_lane::QESC;
using plane_lane::inner, plane_lane::predict, plane_lane::fold, plane_lane::unfold;
using plane_lane::Lane, plane_lane::start_parameters, plane_lane::head_word, plane_lane::read_head_word;
using plane_lane::encode_symbol, plane_lane::leading_ones, plane_lane::decode_symbol;

constexpr int NMODES = 8;             // each of the four spatial predictors plain or differential
constexpr int MAX_C = 16;
constexpr int MAX_SIDE = 1 << 20;
constexpr int WRITER_S = 256;         // rows of a unit as lbdrn_plane3_encode cuts them
constexpr int HEADER_WORDS = 5;
constexpr int MODES_PER_WORD = 10;
constexpr uint32_t MAGIC = 0x3350424Cu;   // 'L' 'B' 'P' '3', little-endian

// ---------------------------------------------------------------- geometry

struct Geom {
    int C, H, W, S, TX, NU;
    int64_t nunits;
};

P3_HD bool make_geom(int64_t C, int64_t H, int64_t W, int64_t S, Geom* g)
{
    if (C < 1 || C > MAX_C || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE || S < T || S > MAX_SIDE || S % T) return false;
    g->C = (int)C; g->H = (int)H; g->W = (int)W; g->S = (int)S;
    g->TX = (int)((W + T - 1) / T);
    g->NU = (int)((H + S - 1) / S);
    g->nunits = (int64_t)g->TX * g->NU;
    return true;
}
struct Unit {
    int x0, y0, tw, uh;
};
P3_HD Unit unit_of(const Geom& g, int64_t u)
{
    Unit r;
    const int ux = (int)(u % g.TX), uy = (int)(u / g.TX);
    r.x0 = ux * T; r.y0 = uy * g.S;
    r.tw = g.W - r.x0 < T ? g.W - r.x0 : T;
    r.uh = g.H - r.y0 < g.S ? g.H - r.y0 : g.S;
    return r;
}
P3_HD int passes(int uh) { return (uh + T - 1) / T; }
P3_HD int mode_words(int C) { return (C + MODES_PER_WORD - 1) / MODES_PER_WORD; }
// head and mode words, and the one word lane 0 takes at the unit's first step
P3_HD uint32_t min_unit_words(int C, int uh) { return (uint32_t)(C + passes(uh) * mode_words(C) + 1); }
// a lane takes at most one word a symbol
P3_HD uint32_t max_unit_words(int C, int uh, int tw) { return (uint32_t)(C + passes(uh) * mode_words(C)) + (uint32_t)C * (uint32_t)uh * (uint32_t)tw; }
P3_HD size_t body_bound(const Geom& g)
{
    const size_t full = (size_t)(g.H / g.S), last = (size_t)(g.H % g.S);
    const size_t fixed = (size_t)g.TX * (full * (size_t)(g.C + passes(g.S) * mode_words(g.C)) + (last ? (size_t)(g.C + passes((int)last) * mode_words(g.C)) : 0));
    return 4 * ((size_t)HEADER_WORDS + (size_t)g.nunits + fixed + (size_t)g.C * g.H * g.W);
}

// ---------------------------------------------------------------- prediction

// the same pixel of the band before: its value px and its neighbours pa, pb, pd (unused by the plain modes)
P3_HD int predict_mode(int ru, int j, int a, int b, int d, int px, int pa, int pb, int pd, int mode)
{
    const int m = mode & (NSPATIAL - 1);
    int p = predict(ru, j, a, b, d, m);
    if (mode >= NSPATIAL) p += px - predict(ru, j, pa, pb, pd, m);
    return p;
}

// ---------------------------------------------------------------- mode words

P3_HD uint32_t put_mode(uint32_t word, int c, int mode) { return word | ((uint32_t)mode << (3 * (c % MODES_PER_WORD))); }
P3_HD int get_mode(uint32_t word, int c) { return (int)((word >> (3 * (c % MODES_PER_WORD))) & 7u); }
// word w of a pass's mode words: nothing set beyond the bands it holds, and band 0 plain
P3_HD bool mode_word_ok(uint32_t word, int w, int C)
{
    const int held = C - w * MODES_PER_WORD < MODES_PER_WORD ? C - w * MODES_PER_WORD : MODES_PER_WORD;
    if (word >> (3 * held)) return false;
    return w != 0 || (word & 7u) < (uint32_t)NSPATIAL;
}

// ---------------------------------------------------------------- header and table

P3_HD uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// Host: the header and the unit table against the body's length.  0, or -1 and a message.
inline int check_body(const uint8_t* body, size_t n, Geom* g, char* msg, size_t cap)
{
    if (n % 4 || n < 4 * (size_t)HEADER_WORDS || le32(body) != MAGIC) {
        snprintf(msg, cap, "not an LBB3 body (%zu bytes; magic or length)", n);
        return -1;
    }
    const uint32_t C = le32(body + 4), H = le32(body + 8), W = le32(body + 12), S = le32(body + 16);
    if (S % T || S < (uint32_t)T) {
        snprintf(msg, cap, "LBB3 unit height S = %u is not a multiple of 64 from 64 up", S);
        return -1;
    }
    if (!make_geom(C, H, W, S, g)) {
        snprintf(msg, cap, "LBB3 geometry %u x %u x %u (S = %u) is out of range", C, H, W, S);
        return -1;
    }
    const size_t words = n / 4 - HEADER_WORDS;
    if (words < (size_t)g->nunits) {
        snprintf(msg, cap, "LBB3 body of %zu bytes cannot hold the table of %lld units", n, (long long)g->nunits);
        return -1;
    }
    const uint8_t* table = body + 4 * HEADER_WORDS;
    const size_t data = words - (size_t)g->nunits;
    size_t off = 0;
    for (int64_t u = 0; u < g->nunits; ++u) {
        const Unit r = unit_of(*g, u);
        const uint32_t cnt = le32(table + 4 * u);
        if (cnt > data - off) {
            snprintf(msg, cap, "LBB3 unit %lld: its %u words overrun the body", (long long)u, cnt);
            return -1;
        }
        if (cnt < min_unit_words(g->C, r.uh) || cnt > max_unit_words(g->C, r.uh, r.tw)) {
            snprintf(msg, cap, "LBB3 unit %lld: %u words are not what %d x %d x %d samples can take", (long long)u, cnt, g->C, r.uh, r.tw);
            return -1;
        }
        off += cnt;
    }
    if (off != data) {
        snprintf(msg, cap, "LBB3 unit table does not add up: %zu words behind the last unit", data - off);
        return -1;
    }
    return 0;
}

}  // namespace plane3
