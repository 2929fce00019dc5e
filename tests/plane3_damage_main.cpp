// A stand-alone program (its own main) that feeds damaged LBB3 bodies to the host build of the decoder (csrc/plane3.inc
// through tests/plane3_host_shim.cpp).  tests/test_plane3_host.py compiles it with -fsanitize=address,undefined and runs it
// as a process of its own: every body, every unit's words and every raster is a heap allocation of exactly its size, so a
// read or write outside one ends the program.  TEST INFRASTRUCTURE.
//
// argv[1]: the fixed list of damaged units (tests/plane3_reference.py, damaged_units) as a file -- u32 count, then per entry
// C, H, W, S as i32, the body's byte count as u32 and the body.  Beside it the program cuts and corrupts a few small bodies
// of its own.  Exit 0 and a line of counts when every damaged body ended in a status, a refusal or a raster.
#include <stdlib.h>

#include "plane3_host_shim.cpp"

static uint32_t g_seed = 20250911u;
static uint32_t rnd() { return g_seed = g_seed * 1664525u + 1013904223u; }

static int run(const std::vector<uint8_t>& body, int C, int H, int W, int S)
{
    uint8_t* exact = (uint8_t*)malloc(body.size() ? body.size() : 1);      // exactly the body's bytes
    memcpy(exact, body.data(), body.size());
    uint16_t* planes = (uint16_t*)calloc((size_t)C * H * W, 2);
    int64_t out[4];
    char msg[64];
    plane3_shim_info(exact, body.size(), out, msg, sizeof msg);
    const int st = plane3_shim_decode(exact, body.size(), C, H, W, S, planes);
    free(planes);
    free(exact);
    return st;
}

int main(int argc, char** argv)
{
    int flagged = 0, passed = 0, refused = 0, total = 0, listed = 0;
    if (argc > 1) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 5;
        uint32_t count = 0;
        if (fread(&count, 4, 1, f) != 1) return 5;
        for (uint32_t i = 0; i < count; ++i) {
            int32_t geom[4];
            uint32_t n;
            if (fread(geom, 4, 4, f) != 4 || fread(&n, 4, 1, f) != 1) return 5;
            std::vector<uint8_t> body(n);
            if (n && fread(body.data(), 1, n, f) != n) return 5;
            const int st = run(body, geom[0], geom[1], geom[2], geom[3]);
            if (i == 0 && st != 0) return 6;      // the list starts with the sound body
            ++total; ++listed; st < 0 ? ++refused : (st ? ++flagged : ++passed);
        }
        fclose(f);
    }
    const int shapes[3][4] = {{2, 70, 66, 64}, {3, 130, 65, 128}, {16, 5, 9, 256}};
    for (int si = 0; si < 3; ++si) {
        const int C = shapes[si][0], H = shapes[si][1], W = shapes[si][2], S = shapes[si][3];
        std::vector<uint16_t> planes((size_t)C * H * W);
        for (int c = 0; c < C; ++c)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const uint32_t r = rnd();
                    int v = 700 + 11 * x + 6 * y + 90 * c + (int)(r % 9u);
                    if ((r >> 8) % 97u == 0) v = (int)(r >> 16);                 // escapes
                    if (y < 3) v = 1000;                                         // flat rows: the zero groups
                    planes[((size_t)c * H + y) * W + x] = (uint16_t)v;
                }
        std::vector<uint8_t> body((size_t)plane3_shim_bound(C, H, W, S));
        const int64_t n = plane3_shim_encode(planes.data(), C, H, W, S, body.data(), (int64_t)body.size());
        if (n <= 0) return 2;
        body.resize((size_t)n);
        {   // the sound body decodes to the planes
            std::vector<uint16_t> back(planes.size(), 0);
            if (plane3_shim_decode(body.data(), body.size(), C, H, W, S, back.data()) != 0) return 3;
            if (memcmp(back.data(), planes.data(), 2 * planes.size())) return 4;
        }
        for (int t = 0; t < 120; ++t) {      // truncations
            std::vector<uint8_t> cut(body.begin(), body.begin() + (size_t)(rnd() % (uint32_t)n));
            const int st = run(cut, C, H, W, S);
            ++total; st < 0 ? ++refused : (st ? ++flagged : ++passed);
        }
        for (int t = 0; t < 400; ++t) {      // corruptions: header, table, head and mode words, the lanes' words
            std::vector<uint8_t> bad = body;
            const uint32_t where = t % 3 == 0 ? rnd() % 60u : (t % 3 == 1 ? 20u + rnd() % 120u : rnd() % (uint32_t)n);
            const int flips = 1 + (int)(rnd() % 3u);
            for (int f = 0; f < flips; ++f) bad[(where + (uint32_t)f * (rnd() % 7u)) % (uint32_t)n] ^= (uint8_t)(1u << (rnd() % 8u));
            if (t % 5 == 0) bad[where % (uint32_t)n] = 0xFF;
            const int st = run(bad, C, H, W, S);
            ++total; st < 0 ? ++refused : (st ? ++flagged : ++passed);
        }
    }
    printf("plane3_damage: %d damaged bodies (%d listed): %d flagged, %d refused on the host, %d decoded to a raster\n", total, listed, flagged,
           refused, passed);
    return 0;
}
