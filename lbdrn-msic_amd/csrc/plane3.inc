// The LBB3 payload's format text (include/lbdrn_plane3.h), written once for the device and the host: geometry and bounds,
// the predictors and the eight modes, the fold, the lane coder in both directions, the mode words, the header and the
// host-side validation of a body's table.  csrc/plane3.hip compiles it for the kernels, tests/plane3_host_shim.cpp and
// tests/plane3_damage_main.cpp compile the same text with a host compiler.  No state, no allocation, no I/O.
//
// The predictors, the fold and the lane coder are LBB2's (csrc/plane_codec.hip), copied: LBB2's bytes are pinned by its own
// tests and must not move with this file.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#if defined(__HIPCC__)
#define P3_HD __host__ __device__ inline
#else
#define P3_HD inline
#endif

namespace plane3 {

constexpr int T = 64;                 // columns of a unit = lanes = rows of a pass
constexpr int NSPATIAL = 4;           // MED / mean / plane / mix
constexpr int NMODES = 8;             // each of them plain or differential
constexpr int QESC = 15;              // unary length that announces a raw 16-bit value
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

P3_HD int inner(int a, int b, int d, int m)
{
    if (m == 0) {
        const int mn = a < b ? a : b, mx = a < b ? b : a;
        return d >= mx ? mn : (d <= mn ? mx : a + b - d);
    }
    if (m == 1) return (a + b) >> 1;
    if (m == 2) return a + b - d;
    return ((3 * (a + b) - 2 * d + (1 << 20)) >> 2) - (1 << 18);
}
// ru: row in the unit, j: column in the unit; a left, b up, d up-left
P3_HD int predict(int ru, int j, int a, int b, int d, int m)
{
    if (ru == 0) return j == 0 ? 0 : a;
    if (j == 0) return b;
    return inner(a, b, d, m);
}
// the same pixel of the band before: its value px and its neighbours pa, pb, pd (unused by the plain modes)
P3_HD int predict_mode(int ru, int j, int a, int b, int d, int px, int pa, int pb, int pd, int mode)
{
    const int m = mode & (NSPATIAL - 1);
    int p = predict(ru, j, a, b, d, m);
    if (mode >= NSPATIAL) p += px - predict(ru, j, pa, pb, pd, m);
    return p;
}
P3_HD uint32_t fold(int x, int pred)
{
    const int e = (int)(short)(unsigned short)(x - pred);
    return e >= 0 ? 2u * (uint32_t)e : (uint32_t)(-2 * e - 1);
}
P3_HD int unfold(uint32_t v) { return (v & 1u) ? -(int)((v + 1u) >> 1) : (int)(v >> 1); }

// ---------------------------------------------------------------- the lane coder

struct Lane {
    uint32_t A, N;
    int left;
    bool zero;
    P3_HD void init(int k0, int z0)
    {
        N = 4;
        A = z0 == 2 ? 0u : (z0 == 1 ? 1u : 6u << k0);
        left = 0;
        zero = false;
    }
    P3_HD void row() { left = 0; zero = false; }        // groups do not cross rows
    P3_HD int k() const
    {
        int kk = 0;
        while (kk < 15 && (N << (kk + 1)) < A) ++kk;
        return kk;
    }
    P3_HD int group() const { return 16 * A < N ? 16 : (2 * A < N ? 4 : 1); }
    P3_HD void update(uint32_t v)
    {
        left -= 1;
        A += v;
        N += 1;
        if (N == 32) { A = (A + 1) >> 1; N = 16; }
    }
};

P3_HD void start_parameters(uint32_t best, uint32_t count, int* k0, int* z0)
{
    int k = 0;
    while (k < 15 && ((uint64_t)count << (k + 1)) < best) ++k;
    *k0 = k;
    *z0 = 16ull * best < count ? 2 : (2ull * best < count ? 1 : 0);
}
P3_HD uint32_t head_word(int k0, int z0) { return (uint32_t)k0 | ((uint32_t)z0 << 12); }
P3_HD bool read_head_word(uint32_t w, int* k0, int* z0)
{
    *k0 = (int)(w & 0xFFu); *z0 = (int)(w >> 12);
    if (*k0 > 15 || *z0 > 2 || (w & 0xF00u)) { *k0 = 0; *z0 = 0; return false; }
    return true;
}

// Sample j of a row of tw folded residuals v[0 .. tw): its bits (at most 32, right-aligned in *code) and their number;
// advances the lane's state.
P3_HD int encode_symbol(Lane& st, const uint16_t* v, int j, int tw, uint32_t* code_out)
{
    uint32_t code = 0;
    int len = 0;
    if (st.left == 0) {
        int gsz = st.group();
        st.zero = false;
        if (gsz > 1) {
            gsz = gsz < tw - j ? gsz : tw - j;
            bool all0 = true;
            for (int u = 0; u < gsz; ++u) all0 = all0 && v[j + u] == 0;
            code = all0 ? 0u : 1u;
            len = 1;
            st.zero = all0;
        }
        st.left = gsz;
    }
    const uint32_t x = v[j];
    if (!st.zero) {
        const int kk = st.k();
        const uint32_t q = x >> kk;
        if (q < (uint32_t)QESC) {
            code = (code << (q + 1 + kk)) | (((1u << q) - 1u) << (kk + 1)) | (x & ((1u << kk) - 1u));
            len += (int)q + 1 + kk;
        } else {
            code = (code << 31) | (0x7FFFu << 16) | x;
            len += 31;
        }
    }
    st.update(x);
    *code_out = code;
    return len;
}

P3_HD int leading_ones(uint32_t top)
{
    const uint32_t inv = ~top;
    return inv ? __builtin_clz(inv) : 32;
}
// The inverse: top holds the lane's next 32 unread bits, MSB first.  Returns the folded residual, *len the bits it took.
P3_HD uint32_t decode_symbol(Lane& st, uint32_t top, int j, int tw, int* len_out)
{
    uint32_t v = 0;
    int len = 0;
    if (st.left == 0) {
        int gsz = st.group();
        st.zero = false;
        if (gsz > 1) {
            gsz = gsz < tw - j ? gsz : tw - j;
            st.zero = !(top >> 31);
            top <<= 1;
            len = 1;
        }
        st.left = gsz;
    }
    if (!st.zero) {
        const int kk = st.k();
        int q = leading_ones(top);
        if (q >= QESC) { v = (top >> 1) & 0xFFFFu; len += 31; }
        else { v = ((uint32_t)q << kk) | ((top >> (31 - q - kk)) & ((1u << kk) - 1u)); len += q + 1 + kk; }
    }
    st.update(v);
    *len_out = len;
    return v;
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
