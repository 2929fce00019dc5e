// A stand-alone program for the sanitizers: the host build of the overview pyramid (tests/pyramid_host_shim.cpp over
// csrc/pyramid.inc) on seeded rasters of the tests' shapes, 8- and 16-bit, both resamplings, with and without nodata,
// contiguous and as windows of a larger scene; every raster a heap buffer of exactly the samples its pitches reach and the
// output a heap buffer of exactly output_bytes, so a read or write behind either is a finding.  Each level is checked
// against a reduction this file forms itself, from the level before it.  Built by tests/test_pyramid_host.py with
// -fsanitize=address,undefined; exits non-zero on any finding.  TEST INFRASTRUCTURE.
#include <stdio.h>

#include "pyramid_host_shim.cpp"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}

static int g_failed = 0, g_run = 0;

template <class T>
static bool level_ok(const T* src, int64_t row, int64_t plane, int C, int Hs, int Ws, const T* dst, int resampling, int has_nodata, uint32_t nodata)
{
    const int Hd = (Hs + 1) / 2, Wd = (Ws + 1) / 2;
    for (int c = 0; c < C; ++c)
        for (int y = 0; y < Hd; ++y)
            for (int x = 0; x < Wd; ++x) {
                uint64_t s = 0, n = 0;
                for (int dy = 0; dy < 2; ++dy)
                    for (int dx = 0; dx < 2; ++dx) {
                        if (2 * y + dy >= Hs || 2 * x + dx >= Ws) continue;
                        const uint32_t v = src[c * plane + (int64_t)(2 * y + dy) * row + 2 * x + dx];
                        if (has_nodata && v == nodata) continue;
                        s += v;
                        ++n;
                    }
                const uint64_t want = resampling == 1 ? src[c * plane + (int64_t)(2 * y) * row + 2 * x] : n ? (s + n / 2) / n : nodata;
                if (dst[((int64_t)c * Hd + y) * Wd + x] != want) return false;
            }
    return true;
}

template <class T>
static void run(int C, int H, int W, int pad_row, int pad_plane, int kind, int resampling, int has_nodata, uint32_t nodata)
{
    const int64_t row = W + pad_row, plane = (int64_t)H * row + pad_plane;
    const size_t n = (size_t)((C - 1) * plane + (H - 1) * row + W);      // the last sample the pitches reach, and no more
    T* a = (T*)malloc(n * sizeof(T));
    const uint32_t top = sizeof(T) == 1 ? 255u : 65535u;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t r = rnd();
        a[i] = (T)(kind == 1 ? top : kind == 2 ? nodata : r % 15 < 5 ? 0u : r % 15 >= 12 ? top : (r >> 8) & top);
    }
    const int levels = pyramid::max_levels(H, W);
    const size_t bytes = pyramid::output_bytes(C, H, W, levels, (int)sizeof(T));
    unsigned char* out = (unsigned char*)malloc(bytes);
    memset(out, 0xA5, bytes);
    bool ok = pyr_shim_build(a, row, plane, 8 * (int)sizeof(T), C, H, W, resampling, has_nodata, nodata, levels, out) == 0;
    ++g_run;
    const T* from = a;
    int64_t r = row, p = plane;
    int Hs = H, Ws = W;
    for (int k = 1; ok && k <= levels; ++k) {
        const T* to = (const T*)(out + pyramid::level_offset(C, H, W, k, (int)sizeof(T)));
        ok = level_ok<T>(from, r, p, C, Hs, Ws, to, resampling, has_nodata, nodata);
        Hs = (Hs + 1) / 2;
        Ws = (Ws + 1) / 2;
        from = to;
        r = Ws;
        p = (int64_t)Hs * Ws;
    }
    ok = ok && Hs == 1 && Ws == 1;
    if (!ok) {
        ++g_failed;
        printf("FAILED: %d x %d x %d, %d-bit, pitches +%d +%d, kind %d, resampling %d, nodata %d / %u\n", C, H, W, 8 * (int)sizeof(T), pad_row,
               pad_plane, kind, resampling, has_nodata, nodata);
    }
    free(out);
    free(a);
}

template <class T>
static void run_all(const int* s, int pad_row, int pad_plane)
{
    const uint32_t top = sizeof(T) == 1 ? 255u : 65535u;
    for (int kind = 0; kind < 3; ++kind)
        for (int resampling = 0; resampling < 2; ++resampling) {
            run<T>(s[0], s[1], s[2], pad_row, pad_plane, kind, resampling, 0, top);
            run<T>(s[0], s[1], s[2], pad_row, pad_plane, kind, resampling, 1, 0u);
            run<T>(s[0], s[1], s[2], pad_row, pad_plane, kind, resampling, 1, top);
        }
}

int main()
{
    static const int shapes[][3] = {{1, 1, 2}, {1, 2, 1}, {1, 1, 200}, {1, 3, 3}, {2, 37, 53}, {8, 75, 130}, {3, 5, 130}, {1, 64, 64}, {1, 65, 129}};
    for (const auto& s : shapes) {
        run_all<uint16_t>(s, 0, 0);
        run_all<uint8_t>(s, 0, 0);
        run_all<uint16_t>(s, 7, 13);
    }
    printf("%d builds, %d failed\n", g_run, g_failed);
    return g_failed ? 1 : 0;
}
