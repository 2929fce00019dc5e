// The LBB3 payload's host-compilable text (csrc/plane3.inc: geometry, predictors and modes, fold, lane coder, mode words,
// table validation) behind a C ABI, compiled by a host C++ compiler into a temporary directory by
// tests/test_plane3_host.py, which judges it against tests/plane3_reference.py without a GPU.  TEST INFRASTRUCTURE.
//
// The only product text restated here is what the kernels of csrc/plane3.hip do around that text: the walk over units,
// passes, bands and steps, the lanes' bit buffers, and the hand-out of a unit's words (lanes in order where the kernel
// has a ballot).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "plane3.inc"

namespace {

using plane3::T;

struct Window {     // a band's pass: row 0 = the row above
    uint16_t px[T + 1][T + 2];
};

inline int pred_at(const Window& w, const Window& prev, int ru, int lane, int j, int mode)
{
    const int a = j ? w.px[lane + 1][j - 1] : 0, b = ru ? w.px[lane][j] : 0, d = (j && ru) ? w.px[lane][j - 1] : 0;
    int pv = 0, pa = 0, pb = 0, pd = 0;
    if (mode >= plane3::NSPATIAL) {
        pv = prev.px[lane + 1][j];
        pa = j ? prev.px[lane + 1][j - 1] : 0; pb = ru ? prev.px[lane][j] : 0; pd = (j && ru) ? prev.px[lane][j - 1] : 0;
    }
    return plane3::predict_mode(ru, j, a, b, d, pv, pa, pb, pd, mode);
}

void encode_unit(const uint16_t* planes, const plane3::Geom& g, const plane3::Unit& un, std::vector<uint32_t>& out)
{
    const int C = g.C, tw = un.tw, np = plane3::passes(un.uh), lanes = un.uh < T ? un.uh : T;
    std::vector<Window> win(2);
    memset(win.data(), 0, 2 * sizeof(Window));
    std::vector<plane3::Lane> st((size_t)C * T);
    std::vector<uint32_t> head(C);
    std::vector<int> modes((size_t)np * C);
    std::vector<uint8_t> lens((size_t)np * C * T * T, 0);
    std::vector<std::vector<uint32_t>> priv(T);
    uint64_t acc[T] = {0};
    int nb[T] = {0};
    for (int p = 0; p < np; ++p) {
        const int rows = un.uh - p * T < T ? un.uh - p * T : T;
        for (int c = 0; c < C; ++c) {
            Window& w = win[c & 1];
            const Window& prev = win[(c & 1) ^ 1];
            const uint16_t* band = planes + ((size_t)c * g.H + un.y0) * g.W + un.x0;
            for (int rr = (p == 0 ? 1 : 0); rr <= rows; ++rr)
                for (int j = 0; j < tw; ++j) w.px[rr][j] = band[(size_t)(p * T - 1 + rr) * g.W + j];
            uint32_t sum[plane3::NMODES] = {0};
            const int nm = c ? plane3::NMODES : plane3::NSPATIAL;
            for (int lane = 0; lane < rows; ++lane)
                for (int j = 0; j < tw; ++j)
                    for (int m = 0; m < nm; ++m) sum[m] += plane3::fold(w.px[lane + 1][j], pred_at(w, prev, p * T + lane, lane, j, m));
            int mode = 0;
            for (int m = 1; m < nm; ++m)
                if (sum[m] < sum[mode]) mode = m;
            modes[(size_t)p * C + c] = mode;
            if (p == 0) {
                int k0, z0;
                plane3::start_parameters(sum[mode], (uint32_t)(rows * tw), &k0, &z0);
                head[c] = plane3::head_word(k0, z0);
                for (int lane = 0; lane < T; ++lane) st[(size_t)c * T + lane].init(k0, z0);
            }
            for (int lane = 0; lane < rows; ++lane) {
                plane3::Lane& s = st[(size_t)c * T + lane];
                s.row();
                uint16_t v[T];
                for (int j = 0; j < tw; ++j) v[j] = (uint16_t)plane3::fold(w.px[lane + 1][j], pred_at(w, prev, p * T + lane, lane, j, mode));
                for (int j = 0; j < tw; ++j) {
                    uint32_t code;
                    const int len = plane3::encode_symbol(s, v, j, tw, &code);
                    lens[(((size_t)p * C + c) * T + lane) * T + j] = (uint8_t)len;
                    if (len) {
                        acc[lane] = (acc[lane] << len) | code;
                        nb[lane] += len;
                        if (nb[lane] >= 32) {
                            priv[lane].push_back((uint32_t)(acc[lane] >> (nb[lane] - 32)));
                            nb[lane] -= 32;
                        }
                    }
                }
            }
        }
    }
    for (int lane = 0; lane < lanes; ++lane) priv[lane].push_back(nb[lane] ? (uint32_t)(acc[lane] << (32 - nb[lane])) : 0u);
    // the decoder's request order
    for (int c = 0; c < C; ++c) out.push_back(head[c]);
    int fill[T] = {0};
    size_t taken[T] = {0};
    const int mw = plane3::mode_words(C);
    for (int p = 0; p < np; ++p) {
        const int rows = un.uh - p * T < T ? un.uh - p * T : T;
        for (int w = 0; w < mw; ++w) {
            uint32_t word = 0;
            for (int c = w * plane3::MODES_PER_WORD; c < C && c < (w + 1) * plane3::MODES_PER_WORD; ++c) word = plane3::put_mode(word, c, modes[(size_t)p * C + c]);
            out.push_back(word);
        }
        for (int c = 0; c < C; ++c)
            for (int d = 0; d < rows + tw - 1; ++d)
                for (int lane = 0; lane < rows; ++lane) {
                    const int j = d - lane;
                    if (j < 0 || j >= tw) continue;
                    if (fill[lane] < 32) {
                        out.push_back(taken[lane] < priv[lane].size() ? priv[lane][taken[lane]] : 0u);
                        taken[lane] += 1;
                        fill[lane] += 32;
                    }
                    fill[lane] -= lens[(((size_t)p * C + c) * T + lane) * T + j];
                }
    }
}

// ws[0 .. nws): the unit's words.  Writes the unit's samples into planes; true where the unit is damaged.
bool decode_unit(const uint32_t* ws, uint32_t nws, const plane3::Geom& g, const plane3::Unit& un, uint16_t* planes)
{
    const int C = g.C, tw = un.tw, np = plane3::passes(un.uh), mw = plane3::mode_words(C);
    bool bad = false;
    std::vector<Window> win(2);
    memset(win.data(), 0, 2 * sizeof(Window));
    std::vector<uint16_t> above((size_t)C * T, 0);
    std::vector<plane3::Lane> st((size_t)C * T);
    for (int c = 0; c < C; ++c) {
        int k0, z0;
        if ((uint32_t)c >= nws || !plane3::read_head_word(ws[c], &k0, &z0)) { bad = true; k0 = 0; z0 = 0; }
        for (int lane = 0; lane < T; ++lane) st[(size_t)c * T + lane].init(k0, z0);
    }
    uint64_t buf[T] = {0};
    int nb[T] = {0};
    uint32_t cur = (uint32_t)C;
    for (int p = 0; p < np; ++p) {
        const int rows = un.uh - p * T < T ? un.uh - p * T : T;
        uint32_t mword[2] = {0u, 0u};
        for (int i = 0; i < mw; ++i) {
            if (cur + i < nws) mword[i] = ws[cur + i]; else bad = true;
            if (!plane3::mode_word_ok(mword[i], i, C)) { bad = true; mword[i] = 0u; }
        }
        cur += (uint32_t)mw;
        for (int c = 0; c < C; ++c) {
            Window& w = win[c & 1];
            const Window& prev = win[(c & 1) ^ 1];
            const int mode = plane3::get_mode(c < plane3::MODES_PER_WORD ? mword[0] : mword[1], c);
            if (p)
                for (int j = 0; j < tw; ++j) w.px[0][j] = above[(size_t)c * T + j];
            for (int lane = 0; lane < T; ++lane) st[(size_t)c * T + lane].row();
            for (int d = 0; d < rows + tw - 1; ++d)
                for (int lane = 0; lane < rows; ++lane) {       // (a lane reads what its neighbours wrote at earlier steps only)
                    const int j = d - lane;
                    if (j < 0 || j >= tw) continue;
                    if (nb[lane] < 32) {
                        if (cur >= nws) bad = true;
                        buf[lane] |= (uint64_t)(cur < nws ? ws[cur] : 0u) << (32 - nb[lane]);
                        nb[lane] += 32;
                        cur += 1;
                    }
                    int len;
                    const uint32_t v = plane3::decode_symbol(st[(size_t)c * T + lane], (uint32_t)(buf[lane] >> 32), j, tw, &len);
                    buf[lane] <<= len;
                    nb[lane] -= len;
                    w.px[lane + 1][j] = (uint16_t)(pred_at(w, prev, p * T + lane, lane, j, mode) + plane3::unfold(v));
                }
            uint16_t* band = planes + ((size_t)c * g.H + un.y0 + (size_t)p * T) * g.W + un.x0;
            for (int rr = 1; rr <= rows; ++rr)
                for (int j = 0; j < tw; ++j) band[(size_t)(rr - 1) * g.W + j] = w.px[rr][j];
            for (int j = 0; j < tw; ++j) above[(size_t)c * T + j] = w.px[T][j];
        }
    }
    return bad || cur != nws;
}

}  // namespace

extern "C" {

int64_t plane3_shim_bound(int32_t C, int32_t H, int32_t W, int32_t S)
{
    plane3::Geom g;
    return plane3::make_geom(C, H, W, S, &g) ? (int64_t)plane3::body_bound(g) : 0;
}

// the whole body on the host, the way k_p3_encode / k_p3_scan / k_p3_compact build it; returns its bytes (-1: cap too small)
int64_t plane3_shim_encode(const uint16_t* planes, int32_t C, int32_t H, int32_t W, int32_t S, uint8_t* out, int64_t cap)
{
    plane3::Geom g;
    if (!plane3::make_geom(C, H, W, S, &g)) return -2;
    std::vector<uint32_t> body = {plane3::MAGIC, (uint32_t)C, (uint32_t)H, (uint32_t)W, (uint32_t)S};
    body.resize((size_t)plane3::HEADER_WORDS + (size_t)g.nunits);
    for (int64_t u = 0; u < g.nunits; ++u) {
        const size_t before = body.size();
        const plane3::Unit un = plane3::unit_of(g, u);
        encode_unit(planes, g, un, body);
        const size_t n = body.size() - before;
        if (n > plane3::max_unit_words(C, un.uh, un.tw)) return -3;
        body[plane3::HEADER_WORDS + (size_t)u] = (uint32_t)n;
    }
    if ((int64_t)(4 * body.size()) > cap) return -1;
    for (size_t i = 0; i < body.size(); ++i)
        for (int b = 0; b < 4; ++b) out[4 * i + b] = (uint8_t)(body[i] >> (8 * b));
    return (int64_t)(4 * body.size());
}

// {C, H, W, S}; 0, or -1 and a message
int plane3_shim_info(const uint8_t* body, size_t n, int64_t out[4], char* msg, size_t cap)
{
    plane3::Geom g;
    char local[256] = "";
    const int rc = plane3::check_body(body, n, &g, local, sizeof local);
    if (msg && cap) snprintf(msg, cap, "%s", local);
    if (rc) return rc;
    out[0] = g.C; out[1] = g.H; out[2] = g.W; out[3] = g.S;
    return 0;
}

// The body for the geometry and S the caller states, the way lbdrn_plane3_decode and k_p3_decode read it.  Returns the status
// (0 = sound, 1 = damaged), -1 for what lbdrn_plane3_decode refuses on the host.
int plane3_shim_decode(const uint8_t* body, size_t n, int32_t C, int32_t H, int32_t W, int32_t S, uint16_t* planes)
{
    plane3::Geom g;
    if (!plane3::make_geom(C, H, W, S, &g)) return -1;
    if (n % 4 || n / 4 < (size_t)plane3::HEADER_WORDS + (size_t)g.nunits) return -1;
    std::vector<uint32_t> words(n / 4);
    for (size_t i = 0; i < words.size(); ++i) words[i] = plane3::le32(body + 4 * i);
    bool bad = words[0] != plane3::MAGIC || words[1] != (uint32_t)C || words[2] != (uint32_t)H || words[3] != (uint32_t)W || words[4] != (uint32_t)S;
    const uint64_t total = words.size() - plane3::HEADER_WORDS - (size_t)g.nunits;
    const uint32_t* data = words.data() + plane3::HEADER_WORDS + g.nunits;
    uint64_t off = 0;
    for (int64_t u = 0; u < g.nunits; ++u) {
        uint32_t nws = words[plane3::HEADER_WORDS + (size_t)u];
        const uint64_t mine = off;
        off += nws;
        bool over = false;
        if (mine > total || nws > total - mine) { nws = 0; over = true; }
        // exactly the unit's words, in a buffer of their own: a read beyond them is a read outside an allocation
        std::vector<uint32_t> own(data + (over ? 0 : mine), data + (over ? 0 : mine) + nws);
        if (decode_unit(own.data(), nws, g, plane3::unit_of(g, u), planes) || over) bad = true;
    }
    if (off != total) bad = true;      // the counts do not add up to the body
    return bad ? 1 : 0;
}

}  // extern "C"
