// A stand-alone program for the sanitizers: the host build of the quality report (tests/quality_host_shim.cpp over
// csrc/quality.inc) on seeded rasters of the tests' shapes, 8- and 16-bit, contiguous and as windows of a larger scene; every
// raster a heap buffer of exactly the samples its strides reach and the result a heap buffer of exactly result_bytes(C), so a
// read or write behind either is a finding.  Each result is checked against sums this file forms itself.  Built by
// tests/test_quality_host.py with -fsanitize=address,undefined; exits non-zero on any finding.  TEST INFRASTRUCTURE.
#include <stdio.h>

#include "quality_host_shim.cpp"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}

static int g_failed = 0, g_run = 0;

template <class T>
static void run(int C, int H, int W, int pad_row, int pad_plane, int kind)
{
    const int64_t row = W + pad_row, plane = (int64_t)H * row + pad_plane;
    const size_t n = (size_t)((C - 1) * plane + (H - 1) * row + W);      // the last sample the strides reach, and no more
    T* a = (T*)malloc(n * sizeof(T));
    T* b = (T*)malloc(n * sizeof(T));
    const uint32_t top = sizeof(T) == 1 ? 255u : 65535u;
    for (size_t i = 0; i < n; ++i) {
        a[i] = (T)(kind == 2 ? (rnd() & 1 ? top : 0) : rnd() & top);
        b[i] = (T)(kind == 0 ? a[i] : kind == 1 ? (a[i] & ~31u) | (rnd() & 31u) : (rnd() & 1 ? top : 0));
    }
    const size_t words = quality::result_bytes(C) / 8;
    uint64_t* res = (uint64_t*)malloc(words * 8);
    memset(res, 0xA5, words * 8);
    const int rc = quality_shim_compare(a, row, plane, b, row, plane, 8 * (int)sizeof(T), C, H, W, sizeof(T) == 1 ? 255.0 : 10000.0, 3u, res);
    ++g_run;
    bool ok = rc == 0;
    for (int c = 0; ok && c < C; ++c) {
        uint64_t sse = 0, hist = 0;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const int64_t e = (int64_t)a[c * plane + y * row + x] - (int64_t)b[c * plane + y * row + x];
                sse += (uint64_t)(e * e);
            }
        const uint64_t* rec = res + (size_t)c * quality::BAND_WORDS;
        for (int k = 0; k < quality::HIST_BINS; ++k) hist += rec[quality::F_HIST + k];
        double ssim;
        memcpy(&ssim, &rec[quality::F_SSIM_SUM], 8);
        ok = rec[quality::F_N] == (uint64_t)H * W && rec[quality::F_SSE] == sse && hist == (uint64_t)H * W &&
             rec[quality::F_SSIM_N] == (H >= 11 && W >= 11 ? (uint64_t)(H - 10) * (W - 10) : 0) && ssim <= (double)rec[quality::F_SSIM_N] + 1e-6 &&
             (kind != 0 || (sse == 0 && (rec[quality::F_SSIM_N] == 0 || fabs(ssim / (double)rec[quality::F_SSIM_N] - 1.0) < 1e-12)));
    }
    const uint64_t* px = res + (size_t)C * quality::BAND_WORDS;
    if (ok && C >= 2 && C <= 16) ok = px[quality::P_SAM_N] + px[quality::P_SAM_UNDEFINED] == (uint64_t)H * W;
    if (!ok) {
        ++g_failed;
        printf("FAILED: %d x %d x %d, %d-bit, strides +%d +%d, kind %d\n", C, H, W, 8 * (int)sizeof(T), pad_row, pad_plane, kind);
    }
    free(res);
    free(b);
    free(a);
}

int main()
{
    static const int shapes[][3] = {{1, 1, 1}, {1, 10, 40}, {1, 11, 11}, {3, 12, 75}, {8, 48, 80}, {4, 65, 129}, {16, 33, 70}, {1, 41, 43},
                                    {2, 3, 20}, {3, 5, 9}, {17, 2, 5}};
    for (const auto& s : shapes)
        for (int kind = 0; kind < 3; ++kind) {
            run<uint16_t>(s[0], s[1], s[2], 0, 0, kind);
            run<uint8_t>(s[0], s[1], s[2], 0, 0, kind);
            run<uint16_t>(s[0], s[1], s[2], 7, 13, kind);
        }
    printf("%d comparisons, %d failed\n", g_run, g_failed);
    return g_failed ? 1 : 0;
}
