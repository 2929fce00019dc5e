// A stand-alone program (its own main) that feeds damaged TIFF segments to the host build of the segment decoders
// (csrc/tiff.inc through tests/tiff_host_shim.cpp).  tests/test_tiff_host.py compiles it with -fsanitize=address,undefined
// and runs it as a process of its own: every stream, every output buffer and every table is a heap allocation of exactly
// its size, so a read or write outside one ends the program.  TEST INFRASTRUCTURE.
//
//     tiff_damage CASES
//
// CASES is a file of records the test writes with tests/tiff_reference.py's encoders, all integers little-endian u32:
//     kind | compression | expected bytes | stream bytes | the stream | the expected bytes (kind 1 only)
// kind 1: a sound stream.  It must decode to the expected bytes; then `cuts` truncations and `flips` single-byte
//         corruptions of it are decoded (400 and 1,000 per codec, shared among the codec's streams).
// kind 2: a damaged stream of the fixed lists (tiff_reference.damage_cases, tiff_big_cases.damage_rows).  It must end in a
//         non-zero status.
// kind 3: a sound stream of a scene-sized segment (tiff_big_cases.rows; the expected bytes follow as for kind 1).  It must
//         decode to the expected bytes and is decoded once: the random damage is drawn on the small streams of kind 1.
// Exit 0 and a line of counts when every damaged stream ended in a status or in a completed decode, non-zero otherwise.
#include <stdio.h>

#include "tiff_host_shim.cpp"

static uint32_t g_seed = 20240611u;
static uint32_t rnd() { return g_seed = g_seed * 1664525u + 1013904223u; }

static int run(int comp, const std::vector<uint8_t>& stream, size_t expect, std::vector<uint8_t>* keep = nullptr)
{
    uint8_t* exact = (uint8_t*)malloc(stream.size() ? stream.size() : 1);      // exactly the stream's bytes
    if (!stream.empty()) memcpy(exact, stream.data(), stream.size());
    uint8_t* out = (uint8_t*)malloc(expect);
    const int st = tiff_shim_decode(comp, exact, stream.size(), out, expect);
    if (keep) keep->assign(out, out + expect);
    free(out);
    free(exact);
    return st;
}

static bool get32(FILE* f, uint32_t* v)
{
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) return false;
    *v = b[0] | b[1] << 8 | b[2] << 16 | (uint32_t)b[3] << 24;
    return true;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    struct Case { uint32_t kind, comp, expect; std::vector<uint8_t> stream, want; };
    std::vector<Case> cases;
    uint32_t kind;
    while (get32(f, &kind)) {
        Case c;
        uint32_t n;
        c.kind = kind;
        if (!get32(f, &c.comp) || !get32(f, &c.expect) || !get32(f, &n)) return 2;
        c.stream.resize(n);
        if (n && fread(c.stream.data(), 1, n, f) != n) return 2;
        if (kind == 1 || kind == 3) {
            c.want.resize(c.expect);
            if (fread(c.want.data(), 1, c.expect, f) != c.expect) return 2;
        }
        cases.push_back(c);
    }
    fclose(f);
    const int comps[3] = {tiff::COMP_DEFLATE, tiff::COMP_LZW, tiff::COMP_PACKBITS};
    int flagged = 0, passed = 0, fixed = 0, sound = 0;
    for (int ci = 0; ci < 3; ++ci) {
        int streams = 0;
        for (const Case& c : cases) streams += c.kind == 1 && (int)c.comp == comps[ci];
        if (!streams) return 3;
        const int cuts = (400 + streams - 1) / streams, flips = (1000 + streams - 1) / streams;
        for (const Case& c : cases) {
            if ((int)c.comp != comps[ci]) continue;
            if (c.kind == 2) {      // the fixed list: a status, every time
                if (run((int)c.comp, c.stream, c.expect) == 0) { fprintf(stderr, "a case of the fixed list decoded without a status\n"); return 4; }
                ++fixed;
                continue;
            }
            std::vector<uint8_t> got;
            if (run((int)c.comp, c.stream, c.expect, &got) != 0 || got != c.want) { fprintf(stderr, "a sound stream did not decode\n"); return 5; }
            ++sound;
            if (c.kind == 3) continue;
            const uint32_t n = (uint32_t)c.stream.size();
            for (int t = 0; t < cuts; ++t) {
                std::vector<uint8_t> cut(c.stream.begin(), c.stream.begin() + (size_t)(rnd() % n));
                run((int)c.comp, cut, c.expect) ? ++flagged : ++passed;
            }
            for (int t = 0; t < flips; ++t) {
                std::vector<uint8_t> bad = c.stream;
                const uint32_t where = t % 4 == 0 ? rnd() % (n < 64u ? n : 64u) : rnd() % n;      // a quarter in the headers
                const uint8_t v = (uint8_t)(t % 3 == 0 ? rnd() : bad[where] ^ (1u << (rnd() % 8u)));
                bad[where] = v == bad[where] ? (uint8_t)~v : v;
                run((int)c.comp, bad, c.expect) ? ++flagged : ++passed;
            }
        }
    }
    printf("tiff_damage: %d sound streams, %d of the fixed list flagged; %d damaged streams: %d flagged, %d decoded to the end\n", sound, fixed,
           flagged + passed, flagged, passed);
    return 0;
}
