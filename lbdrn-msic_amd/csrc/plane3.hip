// liblbdrn_plane3.so (include/lbdrn_plane3.h): "LBB3", the lossless payload of the MSB planes with inter-band prediction,
// coded and decoded on the GPU.  The format's text (geometry, modes, mode words, header and table validation, and through
// csrc/plane_lane.inc the predictors, the fold and the lane coder) is csrc/plane3.inc, shared with the host tests; the full
// description is in the header.
//
// LBB3 is LBB2 (csrc/plane_codec.hip) with another unit -- 64 columns x S rows x all C bands instead of 64 columns x the full
// height x one band -- and eight modes instead of four: each of LBB2's spatial predictors either plain or with the band
// before's residual at the same pixel carried over.  The entropy stage and the word hand-out are LBB2's, one text for
// both: plane_lane.inc, and plane_wave.hpp for the bit writer, the replay and the hand-out.  What is here is LBB3's own: the
// unit, two pixel windows, the packed mode words, a lane's coder state of a band parked in LDS.
//
//   k_p3_encode    one 64-lane workgroup per unit.  Phase A walks pass -> band: stage the band's 65 x 64 window in LDS beside
//                  the band before's (two windows, used in turn), the eight residual sums (wave reduction), code the lane's
//                  row into its private stream in the workspace and record each symbol's length.  A lane's coder state of
//                  a band lives in LDS between passes (an array indexed by the band: registers would need a dynamic index).
//                  Phase B replays the decoder's requests from the recorded lengths and emits the unit's words in that order.
//   k_p3_scan      exclusive sum of the units' word counts (one workgroup: a tile has a few hundred units)
//   k_p3_compact   header, and the units back to back behind the table
//   k_p3_decode    one wave per unit: head and mode words, the unit's next words and the two windows in LDS, the
//                  anti-diagonal walk with a ballot + mbcnt hand-out per step; the last row of every band is kept in LDS for
//                  the next pass.
#include <string.h>

#include "common.hpp"
#include "error_buffer.inc"
#include "../../include/lbdrn_plane3.h"
#include "plane3.inc"
#include "plane_wave.hpp"

namespace lbdrn {

constexpr int P3_T = plane3::T;
constexpr int P3_SCAN_THREADS = 256;

struct P3Sizes {
    int npmax;      // passes of a full unit
    size_t pw;      // private words per lane: a word a symbol at the most, and the tail
    size_t capw;    // words per unit before compaction (worst case)
};

static P3Sizes p3_sizes(const plane3::Geom& g)
{
    P3Sizes z;
    const int uh = std::min(g.S, g.H);
    z.npmax = plane3::passes(uh);
    z.pw = (size_t)z.npmax * g.C * P3_T + 1;
    z.capw = plane3::max_unit_words(g.C, uh, P3_T);
    return z;
}

struct P3Ws {
    uint64_t* offsets;  // [nunits + 1]
    uint32_t* priv;     // [nunits][64][pw]
    uint8_t* lens;      // [nunits][npmax * C][64][64]
    int* modes;         // [nunits][npmax * C]
    uint32_t* words;    // [nunits][capw]
    size_t total;
};

static void carve_p3(const plane3::Geom& g, void* ws, P3Ws* w, bool decoder)
{
    const P3Sizes z = p3_sizes(g);
    char* p = (char*)ws;
    w->offsets = (uint64_t*)p; p += align_up((size_t)(g.nunits + 1) * 8, 256);
    w->priv = nullptr; w->lens = nullptr; w->modes = nullptr; w->words = nullptr;
    if (!decoder) {
        w->priv = (uint32_t*)p; p += align_up((size_t)g.nunits * P3_T * z.pw * 4, 256);
        w->lens = (uint8_t*)p; p += align_up((size_t)g.nunits * z.npmax * g.C * P3_T * P3_T, 256);
        w->modes = (int*)p; p += align_up((size_t)g.nunits * z.npmax * g.C * 4, 256);
        w->words = (uint32_t*)p; p += align_up((size_t)g.nunits * z.capw * 4, 256);
    }
    w->total = (size_t)(p - (char*)ws);
}

// ------------------------------------------------------------------ encoder

__global__ void __launch_bounds__(P3_T) k_p3_encode(const uint16_t* __restrict__ planes, plane3::Geom g, P3Sizes z, P3Ws w,
                                                     uint32_t* __restrict__ counts)
{
    __shared__ uint16_t px[2][P3_T + 1][P3_T + 2];   // the band's window and the band before's; row 0 = the row above the pass
    __shared__ uint16_t vrow[P3_T][P3_T + 2];        // folded residuals of the lane's row
    __shared__ __attribute__((aligned(16))) uint8_t lensw[P3_T][P3_T];
    __shared__ uint32_t pwin[P3_T][P3_T + 1];
    __shared__ uint32_t stA[plane3::MAX_C][P3_T], stN[plane3::MAX_C][P3_T];
    __shared__ uint32_t head[plane3::MAX_C];
    const int lane = threadIdx.x;
    const int64_t unit = blockIdx.x;
    const plane3::Unit un = plane3::unit_of(g, unit);
    const int tw = un.tw, np = plane3::passes(un.uh), C = g.C;
    uint32_t* priv = w.priv + ((size_t)unit * P3_T + lane) * z.pw;
    uint8_t* glens = w.lens + (size_t)unit * z.npmax * C * P3_T * P3_T;
    int* gmodes = w.modes + (size_t)unit * z.npmax * C;
    uint32_t* wout = w.words + (size_t)unit * z.capw;

    // ---- phase A: private streams
    BitWriter bits;
    for (int p = 0; p < np; ++p) {
        const int rows = min(P3_T, un.uh - p * P3_T);
        const int ru = p * P3_T + lane;
        for (int c = 0; c < C; ++c) {
            const int cb = c & 1;
            const uint16_t* band = planes + ((size_t)c * g.H + un.y0) * g.W + un.x0;
            __syncthreads();
            for (int rr = (p == 0 ? 1 : 0); rr <= rows; ++rr)
                px[cb][rr][lane] = lane < tw ? band[(size_t)(p * P3_T - 1 + rr) * g.W + lane] : (uint16_t)0;
            __syncthreads();
            uint32_t sum[plane3::NMODES] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (lane < rows)
                for (int j = 0; j < tw; ++j) {
                    const int a = j ? px[cb][lane + 1][j - 1] : 0, b = ru ? px[cb][lane][j] : 0, d = (j && ru) ? px[cb][lane][j - 1] : 0;
                    const int x = px[cb][lane + 1][j];
                    if (c == 0) {
#pragma unroll
                        for (int m = 0; m < plane3::NSPATIAL; ++m) sum[m] += plane3::fold(x, plane3::predict(ru, j, a, b, d, m));
                    } else {
                        const int pa = j ? px[cb ^ 1][lane + 1][j - 1] : 0, pb = ru ? px[cb ^ 1][lane][j] : 0;
                        const int pd = (j && ru) ? px[cb ^ 1][lane][j - 1] : 0, pv = px[cb ^ 1][lane + 1][j];
#pragma unroll
                        for (int m = 0; m < plane3::NSPATIAL; ++m) {
                            const int pm = plane3::predict(ru, j, a, b, d, m);
                            sum[m] += plane3::fold(x, pm);
                            sum[plane3::NSPATIAL + m] += plane3::fold(x, pm + pv - plane3::predict(ru, j, pa, pb, pd, m));
                        }
                    }
                }
            int mode = 0;
            uint32_t best = wave_sum(sum[0]);
#pragma unroll
            for (int m = 1; m < plane3::NMODES; ++m) {
                const uint32_t s = wave_sum(sum[m]);
                if ((c != 0 || m < plane3::NSPATIAL) && s < best) { best = s; mode = m; }
            }
            if (lane == 0) gmodes[p * C + c] = mode;
            plane3::Lane st;
            if (p == 0) {
                int k0, z0;
                plane3::start_parameters(best, (uint32_t)(rows * tw), &k0, &z0);
                if (lane == 0) head[c] = plane3::head_word(k0, z0);
                st.init(k0, z0);
            } else {
                st.A = stA[c][lane]; st.N = stN[c][lane];
            }
            st.row();
            if (lane < rows) {
                for (int j = 0; j < tw; ++j) {
                    const int a = j ? px[cb][lane + 1][j - 1] : 0, b = ru ? px[cb][lane][j] : 0, d = (j && ru) ? px[cb][lane][j - 1] : 0;
                    int pv = 0, pa = 0, pb = 0, pd = 0;
                    if (mode >= plane3::NSPATIAL) {
                        pv = px[cb ^ 1][lane + 1][j];
                        pa = j ? px[cb ^ 1][lane + 1][j - 1] : 0; pb = ru ? px[cb ^ 1][lane][j] : 0; pd = (j && ru) ? px[cb ^ 1][lane][j - 1] : 0;
                    }
                    vrow[lane][j] = (uint16_t)plane3::fold(px[cb][lane + 1][j], plane3::predict_mode(ru, j, a, b, d, pv, pa, pb, pd, mode));
                }
                for (int j = 0; j < tw; ++j) {
                    uint32_t code;
                    const int len = plane3::encode_symbol(st, &vrow[lane][0], j, tw, &code);
                    lensw[lane][j] = (uint8_t)len;
                    bits.put(priv, code, len);
                }
            }
            stA[c][lane] = st.A; stN[c][lane] = st.N;
            __syncthreads();
            copy_lens_tile(glens + (size_t)(p * C + c) * P3_T * P3_T, &lensw[0][0], lane);
        }
    }
    if (lane < un.uh) bits.tail(priv);
    __threadfence_block();
    __syncthreads();

    // ---- phase B: the decoder's request order
    const int mw = plane3::mode_words(C);
    if (lane < C) wout[lane] = head[lane];
    Replay rp;
    rp.nw = (uint32_t)C;
    for (int p = 0; p < np; ++p) {
        const int rows = min(P3_T, un.uh - p * P3_T);
        if (lane < mw) {
            uint32_t word = 0;
            for (int c = lane * plane3::MODES_PER_WORD; c < min(C, (lane + 1) * plane3::MODES_PER_WORD); ++c)
                word = plane3::put_mode(word, c, gmodes[p * C + c]);
            wout[rp.nw + lane] = word;
        }
        rp.nw += (uint32_t)mw;
        for (int c = 0; c < C; ++c)
            rp.band(glens + (size_t)(p * C + c) * P3_T * P3_T, priv, bits.pwords, rows, tw, lane, lensw, pwin, wout);
    }
    if (lane == 0) counts[unit] = rp.nw;
}

// counts[0 .. n) -> offsets[0 .. n]: the exclusive sum and, behind it, the total
__global__ void __launch_bounds__(P3_SCAN_THREADS) k_p3_scan(const uint32_t* __restrict__ counts, int64_t n, uint64_t* __restrict__ offsets)
{
    __shared__ uint64_t part[P3_SCAN_THREADS];
    const int tid = threadIdx.x;
    const int64_t per = (n + P3_SCAN_THREADS - 1) / P3_SCAN_THREADS;
    const int64_t lo = min(n, tid * per), hi = min(n, lo + per);
    uint64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += counts[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        uint64_t run = 0;
        for (int t = 0; t < P3_SCAN_THREADS; ++t) {
            const uint64_t v = part[t];
            part[t] = run;
            run += v;
        }
        offsets[n] = run;
    }
    __syncthreads();
    s = part[tid];
    for (int64_t i = lo; i < hi; ++i) {
        offsets[i] = s;
        s += counts[i];
    }
}

__global__ void __launch_bounds__(256) k_p3_compact(const uint32_t* __restrict__ units, size_t capw, plane3::Geom g,
                                                     const uint64_t* __restrict__ offsets, uint32_t* __restrict__ body,
                                                     uint64_t* __restrict__ body_bytes)
{
    const int64_t u = blockIdx.x;
    const uint32_t* counts = body + plane3::HEADER_WORDS;
    const uint32_t n = counts[u];
    const uint32_t* src = units + (size_t)u * capw;
    uint32_t* dst = body + plane3::HEADER_WORDS + g.nunits + offsets[u];
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
    if (u == 0 && threadIdx.x == 0) {
        body[0] = plane3::MAGIC; body[1] = (uint32_t)g.C; body[2] = (uint32_t)g.H; body[3] = (uint32_t)g.W; body[4] = (uint32_t)g.S;
        *body_bytes = ((uint64_t)plane3::HEADER_WORDS + (uint64_t)g.nunits + offsets[g.nunits]) * 4;
    }
}

// ------------------------------------------------------------------ decoder

constexpr int P3_WWIN = P3_T * P3_T;  // the most words one band of one pass can take: a word a lane and step

__global__ void __launch_bounds__(P3_T) k_p3_decode(const uint32_t* __restrict__ body, uint64_t body_words, plane3::Geom g,
                                                     const uint64_t* __restrict__ offsets, uint16_t* __restrict__ planes,
                                                     int* __restrict__ status)
{
    __shared__ uint16_t px[2][P3_T + 1][P3_T + 2];
    __shared__ uint16_t above[plane3::MAX_C][P3_T];      // every band's last row of the pass before
    __shared__ uint32_t wwin[P3_WWIN];
    __shared__ uint32_t stA[plane3::MAX_C][P3_T], stN[plane3::MAX_C][P3_T];
    const int lane = threadIdx.x;
    const int64_t unit = blockIdx.x;
    const plane3::Unit un = plane3::unit_of(g, unit);
    const int tw = un.tw, np = plane3::passes(un.uh), C = g.C;
    const int mw = plane3::mode_words(C);
    const uint32_t* counts = body + plane3::HEADER_WORDS;
    const uint64_t total_words = body_words - (uint64_t)plane3::HEADER_WORDS - (uint64_t)g.nunits;   // (the host checked the table fits)
    bool bad = body[0] != plane3::MAGIC || body[1] != (uint32_t)g.C || body[2] != (uint32_t)g.H || body[3] != (uint32_t)g.W ||
               body[4] != (uint32_t)g.S;
    const uint64_t off = offsets[unit];
    uint32_t nws = counts[unit];
    if (off > total_words || nws > total_words - off) { nws = 0; bad = true; }   // counts that overrun the body
    if (offsets[g.nunits] != total_words) bad = true;                            // or do not add up to it
    const uint32_t* ws = body + plane3::HEADER_WORDS + g.nunits + (nws ? off : 0);
    for (int c = 0; c < C; ++c) {
        int k0, z0;
        if ((uint32_t)c >= nws || !plane3::read_head_word(ws[c], &k0, &z0)) { bad = true; k0 = 0; z0 = 0; }
        plane3::Lane st;
        st.init(k0, z0);
        stA[c][lane] = st.A; stN[c][lane] = st.N;
    }
    WordReader rd;
    rd.cur = (uint32_t)C;
    for (int p = 0; p < np; ++p) {
        const int rows = min(P3_T, un.uh - p * P3_T);
        const int ru = p * P3_T + lane;
        uint32_t mword[2] = {0u, 0u};
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (i < mw) {
                if (rd.cur + i < nws) mword[i] = ws[rd.cur + i]; else bad = true;
                if (!plane3::mode_word_ok(mword[i], i, C)) { bad = true; mword[i] = 0u; }
            }
        rd.cur += (uint32_t)mw;
        for (int c = 0; c < C; ++c) {
            const int cb = c & 1;
            const int mode = plane3::get_mode(c < plane3::MODES_PER_WORD ? mword[0] : mword[1], c);
            __syncthreads();
            rd.stage(wwin, P3_WWIN, ws, nws, lane);
            if (p && lane < tw) px[cb][0][lane] = above[c][lane];
            __syncthreads();
            plane3::Lane st;
            st.A = stA[c][lane]; st.N = stN[c][lane];
            st.row();
            for (int d = 0; d < rows + tw - 1; ++d) {
                const int j = d - lane;
                const bool active = lane < rows && j >= 0 && j < tw;
                if (!rd.refill(active, wwin, P3_WWIN, nws)) bad = true;
                if (active) {
                    int len;
                    const uint32_t v = plane3::decode_symbol(st, rd.top(), j, tw, &len);
                    rd.drop(len);
                    const int a = j ? px[cb][lane + 1][j - 1] : 0, b = ru ? px[cb][lane][j] : 0, dd = (j && ru) ? px[cb][lane][j - 1] : 0;
                    int pv = 0, pa = 0, pb = 0, pd = 0;
                    if (mode >= plane3::NSPATIAL) {
                        pv = px[cb ^ 1][lane + 1][j];
                        pa = j ? px[cb ^ 1][lane + 1][j - 1] : 0; pb = ru ? px[cb ^ 1][lane][j] : 0; pd = (j && ru) ? px[cb ^ 1][lane][j - 1] : 0;
                    }
                    px[cb][lane + 1][j] = (uint16_t)(plane3::predict_mode(ru, j, a, b, dd, pv, pa, pb, pd, mode) + plane3::unfold(v));
                }
                __syncthreads();   // one wave: orders this step's LDS write before the neighbours' reads of the next
            }
            stA[c][lane] = st.A; stN[c][lane] = st.N;
            uint16_t* band = planes + ((size_t)c * g.H + un.y0 + (size_t)p * P3_T) * g.W + un.x0;
            for (int rr = 1; rr <= rows; ++rr)
                if (lane < tw) band[(size_t)(rr - 1) * g.W + lane] = px[cb][rr][lane];
            if (lane < tw) above[c][lane] = px[cb][P3_T][lane];   // the next pass's row above (unused after a short pass)
        }
    }
    if (rd.cur != nws) bad = true;
    if (bad) atomicOr(status, 1);
}

// ------------------------------------------------------------------ host entry points

static int p3_encode(const uint16_t* planes, int C, int H, int W, void* body, size_t cap, uint64_t* body_bytes, void* ws,
                     size_t ws_bytes, hipStream_t s)
{
    LBDRN_REQUIRE(planes && body && body_bytes, "lbdrn_plane3_encode: null pointer");
    plane3::Geom g;
    LBDRN_REQUIRE(plane3::make_geom(C, H, W, plane3::WRITER_S, &g), "lbdrn_plane3_encode: geometry %d x %d x %d is out of range (1..%d bands)",
                  C, H, W, plane3::MAX_C);
    LBDRN_REQUIRE(((uintptr_t)body & 3u) == 0, "lbdrn_plane3_encode: the body buffer is not 4-byte aligned");
    P3Ws w;
    carve_p3(g, ws, &w, false);
    if (!ws || ws_bytes < w.total) {
        set_error("LBB3 encoder workspace too small: %zu < %zu", ws_bytes, w.total);
        return LBDRN_E_WORKSPACE;
    }
    if (cap < plane3::body_bound(g)) {
        set_error("LBB3 body buffer too small: %zu < %zu", cap, plane3::body_bound(g));
        return LBDRN_E_WORKSPACE;
    }
    uint32_t* counts = (uint32_t*)body + plane3::HEADER_WORDS;
    k_p3_encode<<<(unsigned)g.nunits, P3_T, 0, s>>>(planes, g, p3_sizes(g), w, counts);
    LBDRN_LAUNCH_CHECK();
    k_p3_scan<<<1, P3_SCAN_THREADS, 0, s>>>(counts, g.nunits, w.offsets);
    LBDRN_LAUNCH_CHECK();
    k_p3_compact<<<(unsigned)g.nunits, 256, 0, s>>>(w.words, p3_sizes(g).capw, g, w.offsets, (uint32_t*)body, body_bytes);
    LBDRN_LAUNCH_CHECK();
    return 0;
}

static int p3_decode(const void* body, size_t n, int C, int H, int W, int S, uint16_t* planes, int* status, void* ws, size_t ws_bytes,
                     hipStream_t s)
{
    LBDRN_REQUIRE(body && planes && status, "lbdrn_plane3_decode: null pointer");
    plane3::Geom g;
    LBDRN_REQUIRE(plane3::make_geom(C, H, W, S, &g), "lbdrn_plane3_decode: geometry %d x %d x %d, S = %d is out of range (1..%d bands, S a multiple of 64)",
                  C, H, W, S, plane3::MAX_C);
    LBDRN_REQUIRE(((uintptr_t)body & 3u) == 0, "lbdrn_plane3_decode: the body is not 4-byte aligned");
    LBDRN_REQUIRE(n % 4 == 0 && n / 4 >= (size_t)plane3::HEADER_WORDS + (size_t)g.nunits,
                  "lbdrn_plane3_decode: a body of %zu bytes cannot hold the table of %lld units", n, (long long)g.nunits);
    P3Ws w;
    carve_p3(g, ws, &w, true);
    if (!ws || ws_bytes < w.total) {
        set_error("LBB3 decoder workspace too small: %zu < %zu", ws_bytes, w.total);
        return LBDRN_E_WORKSPACE;
    }
    const uint32_t* words = (const uint32_t*)body;
    LBDRN_HIP_TRY(hipMemsetAsync(status, 0, sizeof(int), s));
    k_p3_scan<<<1, P3_SCAN_THREADS, 0, s>>>(words + plane3::HEADER_WORDS, g.nunits, w.offsets);
    LBDRN_LAUNCH_CHECK();
    k_p3_decode<<<(unsigned)g.nunits, P3_T, 0, s>>>(words, (uint64_t)(n / 4), g, w.offsets, planes, status);
    LBDRN_LAUNCH_CHECK();
    return 0;
}

}  // namespace lbdrn

extern "C" {

const char* lbdrn_plane3_last_error(void) { return lbdrn::last_error(); }
int lbdrn_plane3_abi_version(void) { return LBDRN_PLANE3_ABI_VERSION; }

size_t lbdrn_plane3_bound(int32_t C, int32_t H, int32_t W)
{
    plane3::Geom g;
    return plane3::make_geom(C, H, W, plane3::WRITER_S, &g) ? plane3::body_bound(g) : 0;
}

size_t lbdrn_plane3_encode_workspace(int32_t C, int32_t H, int32_t W)
{
    plane3::Geom g;
    lbdrn::P3Ws w;
    if (!plane3::make_geom(C, H, W, plane3::WRITER_S, &g)) return 0;
    lbdrn::carve_p3(g, nullptr, &w, false);
    return w.total;
}

size_t lbdrn_plane3_decode_workspace(int32_t C, int32_t H, int32_t W)
{
    plane3::Geom g;
    lbdrn::P3Ws w;
    if (!plane3::make_geom(C, H, W, plane3::T, &g)) return 0;      // the finest cut has the most units
    lbdrn::carve_p3(g, nullptr, &w, true);
    return w.total;
}

int lbdrn_plane3_encode(const uint16_t* planes, int32_t C, int32_t H, int32_t W, void* body, size_t capacity, uint64_t* body_bytes,
                        void* workspace, size_t workspace_bytes, void* stream)
{
    return lbdrn::p3_encode(planes, C, H, W, body, capacity, body_bytes, workspace, workspace_bytes, (hipStream_t)stream);
}

int lbdrn_plane3_info(const void* body, size_t n, int32_t* C, int32_t* H, int32_t* W, int32_t* S)
{
    LBDRN_REQUIRE(body && C && H && W && S, "lbdrn_plane3_info: null pointer");
    plane3::Geom g;
    char msg[256];
    if (plane3::check_body((const uint8_t*)body, n, &g, msg, sizeof msg)) {
        lbdrn::set_error("lbdrn_plane3_info: %s", msg);
        return LBDRN_E_ARG;
    }
    *C = g.C; *H = g.H; *W = g.W; *S = g.S;
    return 0;
}

int lbdrn_plane3_decode(const void* body, size_t n, int32_t C, int32_t H, int32_t W, int32_t S, uint16_t* planes, int32_t* status,
                        void* workspace, size_t workspace_bytes, void* stream)
{
    return lbdrn::p3_decode(body, n, C, H, W, S, planes, status, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
