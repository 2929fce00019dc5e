// A stand-alone program for the sanitizers: the host build of the TIFF writer's Deflate encoder (csrc/tiffw.inc) on its hard
// cases and on 200 seeded random segments, each into a heap buffer of exactly bound(n) bytes, its state a heap allocation of
// exactly its size filled with 0xA5, and every stream decoded again by the reader's host text (csrc/tiff.inc) into a buffer
// of exactly n bytes.  Built by tests/test_tiff_write_host.py with -fsanitize=address,undefined; exits non-zero on any
// finding.  TEST INFRASTRUCTURE.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "tiffw.inc"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}

static int g_failed = 0, g_run = 0;
static uint32_t g_kinds = 0;

static void run(const char* name, const std::vector<uint8_t>& data)
{
    const size_t n = data.size(), cap = tiffw::bound(n);
    uint8_t* in = (uint8_t*)malloc(n);      // exactly n: a read behind the segment is a finding
    memcpy(in, data.data(), n);
    uint8_t* out = (uint8_t*)malloc(cap);
    tiffw::DeflateState* st = (tiffw::DeflateState*)malloc(sizeof(tiffw::DeflateState));
    memset(st, 0xA5, sizeof *st);
    const size_t got = tiffw::deflate(in, n, out, cap, st, 0, 1);
    g_kinds |= st->stats[2];
    ++g_run;
    bool ok = got <= cap;
    if (ok) {
        tiff::InflateTables* t = (tiff::InflateTables*)malloc(sizeof(tiff::InflateTables));
        memset(t, 0xA5, sizeof *t);
        uint8_t* zin = (uint8_t*)malloc(got);
        memcpy(zin, out, got);
        uint8_t* back = (uint8_t*)malloc(n);
        const int status = tiff::inflate(zin, got, back, n, t, 0, 1);
        ok = status == 0 && memcmp(back, in, n) == 0;
        if (!ok) printf("FAILED %s: %zu bytes -> %zu, reader status %d\n", name, n, got, status);
        free(back); free(zin); free(t);
    } else {
        printf("FAILED %s: %zu bytes -> %zu, above the bound of %zu\n", name, n, got, cap);
    }
    g_failed += !ok;
    free(st); free(out); free(in);
}

// five statistics: noise, a constant, a random walk of 16-bit samples (what predictor 2 leaves), text-like repeats, sparse
static std::vector<uint8_t> make(int kind, size_t n)
{
    std::vector<uint8_t> v(n);
    if (kind == 0) for (size_t i = 0; i < n; ++i) v[i] = (uint8_t)rnd();
    else if (kind == 1) { const uint8_t c = (uint8_t)rnd(); for (size_t i = 0; i < n; ++i) v[i] = c; }
    else if (kind == 2) for (size_t i = 0; i < n; ++i) v[i] = (i & 1) ? (uint8_t)((rnd() % 16 == 0) ? 0xFF : 0) : (uint8_t)(rnd() % 41 - 20);
    else if (kind == 3) {
        static const char* words[] = {"tile ", "strip ", "raster ", "band ", "predictor ", "deflate ", "0123456789 ", "\n"};
        size_t i = 0;
        while (i < n) { const char* w = words[rnd() % 8]; for (size_t k = 0; w[k] && i < n; ++k) v[i++] = (uint8_t)w[k]; }
    } else for (size_t i = 0; i < n; ++i) v[i] = rnd() % 50 == 0 ? (uint8_t)rnd() : 0;
    return v;
}

int main()
{
    char name[64];
    for (size_t n = 1; n <= 4; ++n) { snprintf(name, sizeof name, "%zu bytes", n); run(name, make(0, n)); }
    run("constant 128 KiB", std::vector<uint8_t>(131072, 7));
    {
        std::vector<uint8_t> block = make(0, 32768), v;
        for (int k = 0; k < 3; ++k) v.insert(v.end(), block.begin(), block.end());
        run("32 KiB of noise three times", v);
    }
    run("128 KiB of noise", make(0, 131072));
    run("one token more than a block", make(0, (size_t)tiffw::TOKCAP + 1));
    {
        std::vector<uint8_t> v(6000);
        for (size_t i = 0; i < v.size(); ++i) v[i] = (uint8_t)(i * 7 + (i >> 8));      // literals only
        run("literals", v);
        for (size_t i = 0; i < v.size(); ++i) v[i] = (uint8_t)(i % 5);                 // one distance
        run("one distance", v);
        for (int gap : {139, 140}) {
            for (size_t i = 0; i < v.size(); ++i) v[i] = (uint8_t)(rnd() & 1 ? 10 : 10 + gap);
            snprintf(name, sizeof name, "zero run of %d", gap - 1);
            run(name, v);
        }
    }
    run("0xFF over 5552 bytes", std::vector<uint8_t>(70000, 0xFF));
    for (int k = 0; k < 200; ++k) {
        const size_t n = 1 + rnd() % (160u << 10);
        snprintf(name, sizeof name, "random %d (statistic %d, %zu bytes)", k, k % 5, n);
        run(name, make(k % 5, n));
    }
    printf("%d segments, %d failed, block kinds %u\n", g_run, g_failed, g_kinds);
    return g_failed || g_kinds != 7u ? 1 : 0;
}
