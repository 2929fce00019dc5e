// A stand-alone program (its own main) that feeds damaged LBR1 bodies to the host build of the residual decoder
// (csrc/resid.inc through tests/resid_host_shim.cpp).  tests/test_resid_host.py compiles it with
// -fsanitize=address,undefined and runs it as a process of its own: every body, every raster and every row buffer is a
// heap allocation of exactly its size, so a read or write outside one ends the program.  TEST INFRASTRUCTURE.
//
// Exit 0 and a line of counts when every damaged body ended in a status or in a raster, non-zero otherwise.
#include <stdlib.h>

#include "resid_host_shim.cpp"

static uint32_t g_seed = 20240607u;
static uint32_t rnd() { return g_seed = g_seed * 1664525u + 1013904223u; }

static int run(const std::vector<uint8_t>& body, int C, int H, int W, int x0, int y0, int w, int h)
{
    uint8_t* exact = (uint8_t*)malloc(body.size() ? body.size() : 1);      // exactly the body's bytes
    memcpy(exact, body.data(), body.size());
    uint16_t* rec = (uint16_t*)calloc((size_t)C * h * w, 2);
    int64_t out[4];
    char msg[64];
    resid_shim_info(exact, body.size(), out, msg, sizeof msg);
    const int st = resid_shim_decode_body(exact, body.size(), C, H, W, x0, y0, w, h, rec);
    free(rec);
    free(exact);
    return st;
}

int main()
{
    const int C = 2, H = 70, W = 300, taus[3] = {0, 1, 700};
    int flagged = 0, passed = 0, refused = 0, total = 0;
    for (int ti = 0; ti < 3; ++ti) {
        const int tau = taus[ti];
        std::vector<uint16_t> orig((size_t)C * H * W), recon(orig.size());
        for (size_t i = 0; i < orig.size(); ++i) {
            const uint32_t r = rnd();
            recon[i] = (uint16_t)(r >> 8);
            const int spread = (r & 7u) == 0 ? 65535 : ((r & 7u) < 4 ? 3 : 300);      // escapes, small and middling residuals
            int v = (int)recon[i] + (int)(rnd() % (2u * spread + 1u)) - spread;
            if ((r & 0xF0u) == 0) v = recon[i];
            orig[i] = (uint16_t)(v < 0 ? 0 : (v > 65535 ? 65535 : v));
        }
        for (size_t i = 0; i < (size_t)W * 3; ++i) orig[i] = recon[i];                // rows of zeros
        std::vector<uint8_t> body((size_t)resid_shim_bound(C, H, W));
        const int64_t n = resid_shim_encode_body(orig.data(), recon.data(), C, H, W, tau, body.data(), (int64_t)body.size());
        if (n <= 0) return 2;
        body.resize((size_t)n);
        {   // the sound body decodes to within tau
            std::vector<uint16_t> rec = recon;
            if (resid_shim_decode_body(body.data(), body.size(), C, H, W, 0, 0, W, H, rec.data()) != 0) return 3;
            for (size_t i = 0; i < rec.size(); ++i)
                if (abs((int)rec[i] - (int)orig[i]) > tau) return 4;
        }
        for (int t = 0; t < 200; ++t) {      // truncations
            std::vector<uint8_t> cut(body.begin(), body.begin() + (size_t)(rnd() % (uint32_t)n));
            const int st = run(cut, C, H, W, 0, 0, W, H);
            ++total; st < 0 ? ++refused : (st ? ++flagged : ++passed);
        }
        for (int t = 0; t < 600; ++t) {      // corruptions: header, tables, row lengths, row bits
            std::vector<uint8_t> bad = body;
            const uint32_t where = t % 3 == 0 ? rnd() % 40u : (t % 3 == 1 ? 20u + rnd() % 200u : rnd() % (uint32_t)n);
            const int flips = 1 + (int)(rnd() % 3u);
            for (int f = 0; f < flips; ++f) bad[(where + (uint32_t)f * (rnd() % 7u)) % (uint32_t)n] ^= (uint8_t)(1u << (rnd() % 8u));
            if (t % 5 == 0) bad[where % (uint32_t)n] = 0xFF;
            const int whole = run(bad, C, H, W, 0, 0, W, H);
            const int part = run(bad, C, H, W, 250, 60, 20, 8);      // straddles a block corner
            ++total; whole < 0 ? ++refused : (whole ? ++flagged : ++passed);
            ++total; part < 0 ? ++refused : (part ? ++flagged : ++passed);
        }
    }
    printf("resid_damage: %d damaged bodies: %d flagged, %d refused on the host, %d decoded to a raster\n", total, flagged, refused, passed);
    return 0;
}
