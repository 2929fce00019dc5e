// The quality report's text, shared by the device (csrc/quality.hip) and the host tests (tests/quality_host_shim.cpp):
// the result's layout, the cut of a raster into workgroups, the per-sample statistics, the SSIM window weights and the
// SSIM value of one window from its five moments, the spectral angle of one pixel.  Every function here is
// __host__ __device__ and touches nothing but its arguments.  Definitions: include/lbdrn_quality.h.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define QUALITY_HD __host__ __device__ inline
#else
#define QUALITY_HD inline
#endif

namespace quality {

// ---- the result: C band records, then one pixel record; every field 8 bytes
constexpr int HIST_BINS = 257;                    // |e| = 0 .. 255, and |e| >= 256
constexpr int F_N = 0, F_SSE = 1, F_SAE = 2, F_SUM_ERR = 3, F_MAX_ABS = 4, F_HIST = 5;
constexpr int F_SSIM_N = F_HIST + HIST_BINS, F_SSIM_SUM = F_SSIM_N + 1;
constexpr int BAND_WORDS = F_SSIM_SUM + 1;        // 264 words = 2112 bytes
constexpr int P_SAM_N = 0, P_SAM_UNDEFINED = 1, P_SAM_SUM = 2, P_SAM_MAX = 3;
constexpr int PIXEL_WORDS = 4;

constexpr uint32_t WHAT_SSIM = 1u, WHAT_SAM = 2u;
constexpr int MAX_BANDS = 65535, MAX_SIDE = 1 << 20;
constexpr int64_t MAX_PLANE = (int64_t)1 << 31;   // H * W of a plane: a band's sse stays below 2^63
constexpr int SAM_MIN_BANDS = 2, SAM_MAX_BANDS = 16;

// ---- the cut into workgroups: a function of (C, H, W) alone
constexpr int STAT_ROWS = 4;                      // rows of all bands one workgroup of the statistics pass takes
constexpr int STAT_BANDS = 16;                    // bands a workgroup keeps histograms for (C > 16: several band blocks)
constexpr int TAPS = 11, HALO = TAPS / 2;         // the SSIM window
constexpr int SSIM_TILE = 32;                     // windows per tile side; the tile reads (32 + 10)^2 samples of each raster
constexpr int SSIM_IN = SSIM_TILE + TAPS - 1;

struct Geom {
    int C, H, W;
    int64_t stat_groups;      // ceil(H / STAT_ROWS)
    int tiles_x, tiles_y;     // SSIM tiles per band; 0 where H < 11 or W < 11
    int64_t windows;          // (H - 10)(W - 10) or 0
};

QUALITY_HD bool make_geom(int C, int H, int W, Geom* g)
{
    if (C < 1 || H < 1 || W < 1 || C > MAX_BANDS || H > MAX_SIDE || W > MAX_SIDE || (int64_t)H * W > MAX_PLANE) return false;
    g->C = C; g->H = H; g->W = W;
    g->stat_groups = ((int64_t)H + STAT_ROWS - 1) / STAT_ROWS;
    const bool any = H >= TAPS && W >= TAPS;
    g->tiles_x = any ? (W - 2 * HALO + SSIM_TILE - 1) / SSIM_TILE : 0;
    g->tiles_y = any ? (H - 2 * HALO + SSIM_TILE - 1) / SSIM_TILE : 0;
    g->windows = any ? (int64_t)(H - 2 * HALO) * (W - 2 * HALO) : 0;
    return true;
}

QUALITY_HD bool sam_active(const Geom& g, uint32_t what) { return (what & WHAT_SAM) && g.C >= SAM_MIN_BANDS && g.C <= SAM_MAX_BANDS; }
QUALITY_HD bool ssim_active(const Geom& g, uint32_t what) { return (what & WHAT_SSIM) && g.windows > 0; }

QUALITY_HD size_t result_bytes(int C) { return ((size_t)C * BAND_WORDS + PIXEL_WORDS) * 8; }

// the float64 partial sums: one per statistics workgroup (SAM), one per SSIM tile and band
QUALITY_HD size_t workspace_bytes(const Geom& g, uint32_t what)
{
    size_t n = 0;
    if (sam_active(g, what)) n += (size_t)g.stat_groups;
    if (ssim_active(g, what)) n += (size_t)g.C * g.tiles_x * g.tiles_y;
    return n * 8;
}

// ---- per-sample statistics of one band
struct BandAcc {
    uint64_t sse, sae, zeros;
    int64_t sum;
    uint32_t max_abs;
};

QUALITY_HD void acc_init(BandAcc* s) { s->sse = s->sae = s->zeros = 0; s->sum = 0; s->max_abs = 0; }

// e = a - b of one sample; returns |e| for the histogram
QUALITY_HD uint32_t acc_sample(BandAcc* s, uint32_t a, uint32_t b)
{
    const int32_t e = (int32_t)a - (int32_t)b;
    const uint32_t m = (uint32_t)(e < 0 ? -e : e);
    s->sse += (uint64_t)m * m;
    s->sae += m;
    s->sum += e;
    s->zeros += m == 0;
    if (m > s->max_abs) s->max_abs = m;
    return m;
}

QUALITY_HD int hist_bin(uint32_t m) { return m < 256u ? (int)m : 256; }

// ---- SSIM
struct Weights {
    double w[TAPS];
};

// Gaussian of sigma 1.5 over 11 taps, normalised to sum 1; evaluated on the host only (the kernels receive the table), so
// that every consumer multiplies by the same eleven doubles
inline void gauss_weights(Weights* g)
{
    double sum = 0.0;
    for (int k = 0; k < TAPS; ++k) {
        const double x = (double)(k - HALO);
        g->w[k] = exp(-(x * x) / (2.0 * 1.5 * 1.5));
        sum += g->w[k];
    }
    for (int k = 0; k < TAPS; ++k) g->w[k] /= sum;
}

// the five moments of one row (or column) of a window: taps in order
struct Moments {
    double a, b, aa, bb, ab;
};

QUALITY_HD void moments_zero(Moments* m) { m->a = m->b = m->aa = m->bb = m->ab = 0.0; }

QUALITY_HD void moments_tap(Moments* m, double w, double a, double b)
{
    m->a += w * a;
    m->b += w * b;
    m->aa += w * (a * a);
    m->bb += w * (b * b);
    m->ab += w * (a * b);
}

QUALITY_HD void moments_tap5(Moments* m, double w, double a, double b, double aa, double bb, double ab)
{
    m->a += w * a;
    m->b += w * b;
    m->aa += w * aa;
    m->bb += w * bb;
    m->ab += w * ab;
}

QUALITY_HD double ssim_point(const Moments& m, double c1, double c2)
{
    const double va = m.aa - m.a * m.a, vb = m.bb - m.b * m.b, cov = m.ab - m.a * m.b;
    return ((2.0 * m.a * m.b + c1) * (2.0 * cov + c2)) / ((m.a * m.a + m.b * m.b + c1) * (va + vb + c2));
}

QUALITY_HD double ssim_c1(double peak) { return (0.01 * peak) * (0.01 * peak); }
QUALITY_HD double ssim_c2(double peak) { return (0.03 * peak) * (0.03 * peak); }

// ---- SAM: one pixel's C samples of a and of b
// one term of cross = sum over i < j of (a_i b_j - a_j b_i)^2, from the samples as doubles.  Both products are integers below
// 2^32 and their difference is an integer below 2^33 in magnitude: each of the three operations is exact in float64, so d is the
// exact integer difference; only its square is rounded
QUALITY_HD double sam_term(double ai, double bi, double aj, double bj)
{
    const double d = ai * bj - aj * bi;
    return d * d;
}

// theta = atan2(sqrt(cross), dot).  any_a / any_b: the OR of the pixel's samples.  Returns false (the pixel is undefined)
// where exactly one of the two is zero in every band; both zero: theta = 0
QUALITY_HD bool sam_angle(double cross, uint64_t dot, uint32_t any_a, uint32_t any_b, double* theta)
{
    const double th = atan2(sqrt(cross), (double)dot);      // (cross = 0 and dot = 0 where either is zero in every band)
    *theta = (any_a | any_b) ? th : 0.0;
    return (any_a != 0) == (any_b != 0);
}

}  // namespace quality
