// The lane coder of the MSB-plane payloads, LBB2 (csrc/plane_codec.hip) and LBB3 (csrc/plane3.inc, csrc/plane3.hip): the
// four spatial predictors and their edge rules, the fold of the 16-bit wrapped residual, a lane's adaptive Golomb-Rice
// state with its zero-group flags, the start parameters and the head word that carries them, and one symbol in both
// directions.  One text for both formats and for the device and the host: the kernels of both libraries compile it, and
// so do tests/plane3_host_shim.cpp and tests/plane3_damage_main.cpp with a host compiler.  A change here moves the bytes
// of both formats; oracle/plane_codec.c and tests/plane3_reference.py restate them independently and pin them.
// No state, no allocation, no I/O.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PL_HD __host__ __device__ inline
#else
#define PL_HD inline
#endif

namespace plane_lane {

constexpr int T = 64;                 // columns of a strip or unit = lanes = rows of a pass
constexpr int NSPATIAL = 4;           // MED / mean / plane / mix
constexpr int QESC = 15;              // unary length that announces a raw 16-bit value

// ---------------------------------------------------------------- prediction

PL_HD int inner(int a, int b, int d, int m)
{
    if (m == 0) {
        const int mn = a < b ? a : b, mx = a < b ? b : a;
        return d >= mx ? mn : (d <= mn ? mx : a + b - d);
    }
    if (m == 1) return (a + b) >> 1;
    if (m == 2) return a + b - d;
    return ((3 * (a + b) - 2 * d + (1 << 20)) >> 2) - (1 << 18);
}
// r: row in the strip or unit, j: column in it; a left, b up, d up-left
PL_HD int predict(int r, int j, int a, int b, int d, int m)
{
    if (r == 0) return j == 0 ? 0 : a;
    if (j == 0) return b;
    return inner(a, b, d, m);
}
PL_HD uint32_t fold(int x, int pred)
{
    const int e = (int)(short)(unsigned short)(x - pred);
    return e >= 0 ? 2u * (uint32_t)e : (uint32_t)(-2 * e - 1);
}
PL_HD int unfold(uint32_t v) { return (v & 1u) ? -(int)((v + 1u) >> 1) : (int)(v >> 1); }

// ---------------------------------------------------------------- the lane coder

struct Lane {
    uint32_t A, N;
    int left;
    bool zero;
    PL_HD void init(int k0, int z0)
    {
        N = 4;
        A = z0 == 2 ? 0u : (z0 == 1 ? 1u : 6u << k0);
        left = 0;
        zero = false;
    }
    PL_HD void row() { left = 0; zero = false; }        // groups do not cross rows
    PL_HD int k() const
    {
        int kk = 0;
        while (kk < 15 && (N << (kk + 1)) < A) ++kk;
        return kk;
    }
    PL_HD int group() const { return 16 * A < N ? 16 : (2 * A < N ? 4 : 1); }
    PL_HD void update(uint32_t v)
    {
        left -= 1;
        A += v;
        N += 1;
        if (N == 32) { A = (A + 1) >> 1; N = 16; }
    }
};

// best: the smallest residual sum of the first pass's count samples
PL_HD void start_parameters(uint32_t best, uint32_t count, int* k0, int* z0)
{
    int k = 0;
    while (k < 15 && ((uint64_t)count << (k + 1)) < best) ++k;
    *k0 = k;
    *z0 = 16ull * best < count ? 2 : (2ull * best < count ? 1 : 0);
}
PL_HD uint32_t head_word(int k0, int z0) { return (uint32_t)k0 | ((uint32_t)z0 << 12); }
PL_HD bool read_head_word(uint32_t w, int* k0, int* z0)
{
    *k0 = (int)(w & 0xFFu); *z0 = (int)(w >> 12);
    if (*k0 > 15 || *z0 > 2 || (w & 0xF00u)) { *k0 = 0; *z0 = 0; return false; }
    return true;
}

// Sample j of a row of tw folded residuals v[0 .. tw): its bits (at most 32, right-aligned in *code) and their number;
// advances the lane's state.
PL_HD int encode_symbol(Lane& st, const uint16_t* v, int j, int tw, uint32_t* code_out)
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

// the leading one-bits of top, counted up to 16: the escape is QESC = 15 of them and no code has more (no branch, and
// never the count of an all-zero word)
PL_HD int leading_ones(uint32_t top) { return __builtin_clz(~top | 0xFFFFu); }
// The inverse: top holds the lane's next 32 unread bits, MSB first.  Returns the folded residual, *len the bits it took.
PL_HD uint32_t decode_symbol(Lane& st, uint32_t top, int j, int tw, int* len_out)
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

}  // namespace plane_lane
