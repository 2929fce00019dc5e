// The host build of the quality report's text: csrc/quality.inc compiled by a host compiler behind a few C functions for
// tests/test_quality_host.py, tests/test_gpu_quality.py (ctypes) and tests/quality_main.cpp.  The per-sample, per-window and
// per-pixel functions are the device's; the loops around them are plain and sequential here.  TEST INFRASTRUCTURE.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "quality.inc"

namespace {

template <class T>
void compare(const T* a, int64_t a_row, int64_t a_plane, const T* b, int64_t b_row, int64_t b_plane, const quality::Geom& g, double peak,
             uint32_t what, uint64_t* result)
{
    const int C = g.C, H = g.H, W = g.W;
    memset(result, 0, quality::result_bytes(C));
    for (int c = 0; c < C; ++c) {
        uint64_t* rec = result + (size_t)c * quality::BAND_WORDS;
        quality::BandAcc s;
        quality::acc_init(&s);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const uint32_t m = quality::acc_sample(&s, a[c * a_plane + y * a_row + x], b[c * b_plane + y * b_row + x]);
                rec[quality::F_HIST + quality::hist_bin(m)] += 1;
            }
        rec[quality::F_N] = (uint64_t)H * W;
        rec[quality::F_SSE] = s.sse;
        rec[quality::F_SAE] = s.sae;
        rec[quality::F_SUM_ERR] = (uint64_t)s.sum;
        rec[quality::F_MAX_ABS] = s.max_abs;
    }
    if (quality::ssim_active(g, what)) {
        quality::Weights wt;
        quality::gauss_weights(&wt);
        const double c1 = quality::ssim_c1(peak), c2 = quality::ssim_c2(peak);
        const int ow = W - 2 * quality::HALO, oh = H - 2 * quality::HALO;
        std::vector<quality::Moments> hm((size_t)H * ow);
        for (int c = 0; c < C; ++c) {
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < ow; ++x) {
                    quality::Moments m;
                    quality::moments_zero(&m);
                    for (int k = 0; k < quality::TAPS; ++k)
                        quality::moments_tap(&m, wt.w[k], (double)a[c * a_plane + y * a_row + x + k], (double)b[c * b_plane + y * b_row + x + k]);
                    hm[(size_t)y * ow + x] = m;
                }
            double sum = 0.0;
            for (int y = 0; y < oh; ++y)
                for (int x = 0; x < ow; ++x) {
                    quality::Moments m;
                    quality::moments_zero(&m);
                    for (int k = 0; k < quality::TAPS; ++k) {
                        const quality::Moments& h = hm[(size_t)(y + k) * ow + x];
                        quality::moments_tap5(&m, wt.w[k], h.a, h.b, h.aa, h.bb, h.ab);
                    }
                    sum += quality::ssim_point(m, c1, c2);
                }
            uint64_t* rec = result + (size_t)c * quality::BAND_WORDS;
            rec[quality::F_SSIM_N] = (uint64_t)g.windows;
            memcpy(&rec[quality::F_SSIM_SUM], &sum, 8);
        }
    }
    if (quality::sam_active(g, what)) {
        uint64_t n = 0, undefined = 0;
        double sum = 0.0, mx = 0.0;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                double cross = 0.0;
                uint64_t dot = 0;
                uint32_t any_a = 0, any_b = 0;
                for (int i = 0; i < C; ++i) {
                    const uint32_t ai = a[i * a_plane + y * a_row + x], bi = b[i * b_plane + y * b_row + x];
                    dot += (uint64_t)ai * bi;
                    any_a |= ai;
                    any_b |= bi;
                    for (int j = i + 1; j < C; ++j)
                        cross += quality::sam_term((double)ai, (double)bi, (double)a[j * a_plane + y * a_row + x], (double)b[j * b_plane + y * b_row + x]);
                }
                double th;
                if (quality::sam_angle(cross, dot, any_a, any_b, &th)) {
                    ++n;
                    sum += th;
                    mx = th > mx ? th : mx;
                } else {
                    ++undefined;
                }
            }
        uint64_t* rec = result + (size_t)C * quality::BAND_WORDS;
        rec[quality::P_SAM_N] = n;
        rec[quality::P_SAM_UNDEFINED] = undefined;
        memcpy(&rec[quality::P_SAM_SUM], &sum, 8);
        memcpy(&rec[quality::P_SAM_MAX], &mx, 8);
    }
}

}  // namespace

extern "C" {

uint64_t quality_shim_result_bytes(int C) { return C >= 1 && C <= quality::MAX_BANDS ? quality::result_bytes(C) : 0; }

uint64_t quality_shim_workspace(int C, int H, int W, uint32_t what)
{
    quality::Geom g;
    return quality::make_geom(C, H, W, &g) ? quality::workspace_bytes(g, what) : 0;
}

int quality_shim_stat_rows(void) { return quality::STAT_ROWS; }
int quality_shim_ssim_tile(void) { return quality::SSIM_TILE; }

void quality_shim_weights(double* w)
{
    quality::Weights wt;
    quality::gauss_weights(&wt);
    memcpy(w, wt.w, sizeof wt.w);
}

// the whole comparison on host rasters: result[0 .. result_bytes(C) / 8); returns 0, or -1 for arguments the library refuses too
int quality_shim_compare(const void* a, int64_t a_row, int64_t a_plane, const void* b, int64_t b_row, int64_t b_plane, int bits, int C, int H,
                         int W, double peak, uint32_t what, uint64_t* result)
{
    quality::Geom g;
    if (!a || !b || !result || (bits != 8 && bits != 16) || !quality::make_geom(C, H, W, &g) || a_row < W || b_row < W || a_plane < 0 ||
        b_plane < 0 || !(peak > 0.0))
        return -1;
    if (bits == 8) compare<uint8_t>((const uint8_t*)a, a_row, a_plane, (const uint8_t*)b, b_row, b_plane, g, peak, what, result);
    else compare<uint16_t>((const uint16_t*)a, a_row, a_plane, (const uint16_t*)b, b_row, b_plane, g, peak, what, result);
    return 0;
}

}  // extern "C"
