// liblbdrn_quality.so (include/lbdrn_quality.h): two rasters in HBM compared -- exact per-band error statistics and
// histogram, SSIM per band in float64, the spectral angle per pixel.  The per-sample, per-window and per-pixel text is
// csrc/quality.inc, shared with the host tests.
//
//   k_quality_stats   one workgroup per 4 rows of all bands (and per block of 16 bands where C > 16).  The rows are cut
//                     into vectors of 16 bytes, one per lane and step, read once with 16-byte loads (sample by sample at a
//                     row's tail and where a row does not start on 16 bytes).  Per band and step: the lane's partial sums in
//                     registers, a wave reduction, one LDS add per wave; |e| > 0 goes to the band's histogram in LDS by an
//                     LDS atomic (|e| = 0 is counted in registers: the bin every lane would hit on a near-lossless pair).
//                     Where SAM runs, the lane keeps its vectors of all bands in LDS slots of its own (no barrier: nobody
//                     else reads them), then walks the band pairs with ds_read_b128 for 8 pixels at once (an 8-bit vector's
//                     16 pixels in two halves) and evaluates the angles in one rolled loop.  One flush per workgroup: integer
//                     atomics into the result, the workgroup's float64 angle sum into the workspace.
//   k_quality_ssim    one workgroup per tile of 32 x 32 windows and band: the 42 x 42 samples of both rasters staged in
//                     LDS once (7 KB), the horizontal pass of the five moments to LDS in float64 (42 x 32 x 5 x 8 = 52.5 KB),
//                     the vertical pass from there.  59.4 KB of LDS: two workgroups per CU.  The tile's sum goes to the
//                     workspace.
//   k_quality_finish  one workgroup per band and one for the pixel record: n, ssim_n, and the float64 partial sums added in
//                     a fixed order (lane t takes partials t, t + 256, ...; then a tree over the 256 lanes).
#include <string.h>

#include "common.hpp"
#include "error_buffer.inc"
#include "../../include/lbdrn_quality.h"
#include "quality.inc"

namespace lbdrn {

constexpr int QT = 256;      // threads of every workgroup here

struct V16 {
    uint32_t w[4];
};

template <class T>
__device__ __forceinline__ uint32_t vec_get(const V16& v, int k)      // (k is a constant after unrolling)
{
    constexpr int per = 4 / (int)sizeof(T), bits = 8 * (int)sizeof(T);
    return (v.w[k / per] >> (bits * (k % per))) & ((1u << bits) - 1u);
}

// nv samples from p, 0 < nv <= 16 / sizeof(T); nothing behind p[nv - 1] is read
template <class T>
__device__ __forceinline__ V16 vec_load(const T* __restrict__ p, int nv)
{
    constexpr int N = 16 / (int)sizeof(T), per = 4 / (int)sizeof(T), bits = 8 * (int)sizeof(T);
    V16 v;
    if (nv == N && ((uintptr_t)p & 15u) == 0) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        v.w[0] = q.x; v.w[1] = q.y; v.w[2] = q.z; v.w[3] = q.w;
    } else {
        v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) {      // (every lane loads a sample it owns, p[min(k, nv - 1)], and keeps it where k < nv)
            const uint32_t x = (uint32_t)p[k < nv ? k : nv - 1];
            v.w[k / per] |= (k < nv ? x : 0u) << (bits * (k % per));
        }
    }
    return v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v)      // a fixed tree: the same bits every run
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// the LDS of k_quality_stats behind the lanes' sample slots
struct StatLds {
    uint32_t hist[quality::STAT_BANDS][quality::HIST_BINS];      // |e| > 0 only
    uint32_t max_abs[quality::STAT_BANDS];
    unsigned long long acc[quality::STAT_BANDS][4];               // sse, sae, sum_err, zeros
    unsigned long long sam_n, sam_undefined, sam_max;
    double sam_sum[QT / 64];
};

static size_t stat_lds_bytes(int C, bool sam)
{
    return (sam ? (size_t)C * 2 * QT * sizeof(V16) : 0) + sizeof(StatLds);
}

// the angles of SAM_PIXELS pixels of the lane's vector: the band pairs are walked once for all of them
constexpr int SAM_PIXELS = 8;

struct SamAcc {
    uint32_t n, undefined;
    double sum, max;
};

// pixel p of the vector's half: 8-bit vectors hold two halves of 8 pixels, 16-bit ones a single half
template <class T>
__device__ __forceinline__ uint32_t half_get(const V16& v, int half, int p)      // (p is a constant after unrolling)
{
    if (sizeof(T) == 2) return vec_get<T>(v, p);
    const uint32_t w = p < 4 ? (half ? v.w[2] : v.w[0]) : (half ? v.w[3] : v.w[1]);
    return (w >> (8 * (p & 3))) & 255u;
}

template <class T>
__device__ __forceinline__ void sam_pixels(const V16* __restrict__ slots, int tid, int cb, int nv, int half, SamAcc* out)
{
    constexpr int N = SAM_PIXELS;
    const int P0 = half * SAM_PIXELS;
    double cross[N];
    unsigned long long dot[N];
    uint32_t any_a[N], any_b[N];
#pragma unroll
    for (int p = 0; p < N; ++p) { cross[p] = 0.0; dot[p] = 0; any_a[p] = any_b[p] = 0; }
    for (int i = 0; i < cb; ++i) {
        const V16 ai = slots[(i * 2 + 0) * QT + tid], bi = slots[(i * 2 + 1) * QT + tid];
        double da[N], db[N];
#pragma unroll
        for (int p = 0; p < N; ++p) {
            const uint32_t x_a = half_get<T>(ai, half, p), x_b = half_get<T>(bi, half, p);
            dot[p] += (unsigned long long)x_a * x_b;
            any_a[p] |= x_a;
            any_b[p] |= x_b;
            da[p] = (double)x_a;
            db[p] = (double)x_b;
        }
        for (int j = i + 1; j < cb; ++j) {
            const V16 aj = slots[(j * 2 + 0) * QT + tid], bj = slots[(j * 2 + 1) * QT + tid];
#pragma unroll
            for (int p = 0; p < N; ++p)
                cross[p] += quality::sam_term(da[p], db[p], (double)half_get<T>(aj, half, p), (double)half_get<T>(bj, half, p));
        }
    }
#pragma unroll 1
    for (int p = 0; p < N; ++p) {      // one copy of the angle's code: the pixels pass through element 0 (selects, not branches)
        double th;
        const bool defined = quality::sam_angle(cross[0], dot[0], any_a[0], any_b[0], &th), mine = P0 + p < nv;
        const bool take = defined && mine;
        out->n += take ? 1u : 0u;
        out->undefined += !defined && mine ? 1u : 0u;
        out->sum += take ? th : 0.0;
        out->max = take && th > out->max ? th : out->max;
#pragma unroll
        for (int k = 0; k + 1 < N; ++k) { cross[k] = cross[k + 1]; dot[k] = dot[k + 1]; any_a[k] = any_a[k + 1]; any_b[k] = any_b[k + 1]; }
    }
}

template <class T, bool SAM>
__global__ void __launch_bounds__(QT) k_quality_stats(const T* __restrict__ a, int64_t a_row, int64_t a_plane,
                                                       const T* __restrict__ b, int64_t b_row, int64_t b_plane, quality::Geom g,
                                                       unsigned long long* __restrict__ result, double* __restrict__ sam_partial)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    constexpr int N = 16 / (int)sizeof(T);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (SAM) {      // the rasters' addresses and strides live in vector registers: the scalar file is what the angle's atan2 needs
        asm volatile("" : "+v"(a), "+v"(b), "+v"(a_row), "+v"(a_plane), "+v"(b_row), "+v"(b_plane));
    }
    const int c0 = (int)blockIdx.y * quality::STAT_BANDS;
    const int cb = min(quality::STAT_BANDS, g.C - c0);
    V16* slots = reinterpret_cast<V16*>(lds_raw);      // [cb][2][QT], SAM only
    StatLds& L = *reinterpret_cast<StatLds*>(lds_raw + (SAM ? (size_t)cb * 2 * QT * sizeof(V16) : 0));

    for (int i = tid; i < quality::STAT_BANDS * quality::HIST_BINS; i += QT) (&L.hist[0][0])[i] = 0;
    if (tid < quality::STAT_BANDS) {
        L.max_abs[tid] = 0;
        L.acc[tid][0] = L.acc[tid][1] = L.acc[tid][2] = L.acc[tid][3] = 0;
    }
    if (tid == 0) L.sam_n = L.sam_undefined = L.sam_max = 0;
    __syncthreads();

    const int y0 = (int)blockIdx.x * quality::STAT_ROWS;
    const int rows = min(quality::STAT_ROWS, g.H - y0);
    const int vpr = (g.W + N - 1) / N;
    const int items = rows * vpr;
    uint32_t sam_n = 0, sam_undef = 0;
    double sam_sum = 0.0, sam_max = 0.0;

    for (int base = 0; base < items; base += QT) {
        const int q = base + tid;
        const bool active = q < items;
        const int r = active ? q / vpr : 0;
        const int x = active ? (q - r * vpr) * N : 0;
        const int nv = active ? min(N, g.W - x) : 0;
        for (int c = 0; c < cb; ++c) {
            V16 va = {{0, 0, 0, 0}}, vb = {{0, 0, 0, 0}};
            if (nv > 0) {
                va = vec_load<T>(a + (int64_t)(c0 + c) * a_plane + (int64_t)(y0 + r) * a_row + x, nv);
                vb = vec_load<T>(b + (int64_t)(c0 + c) * b_plane + (int64_t)(y0 + r) * b_row + x, nv);
            }
            quality::BandAcc s;
            quality::acc_init(&s);
#pragma unroll
            for (int k = 0; k < N; ++k) {      // (samples behind nv are 0 in both vectors: e = 0, taken out of the zero count below)
                const uint32_t m = quality::acc_sample(&s, vec_get<T>(va, k), vec_get<T>(vb, k));
                if (m) atomicAdd(&L.hist[c][quality::hist_bin(m)], 1u);
            }
            s.zeros -= (uint64_t)(N - nv);
            if (SAM) {
                slots[(c * 2 + 0) * QT + tid] = va;
                slots[(c * 2 + 1) * QT + tid] = vb;
            }
            const unsigned long long sse = wave_sum((unsigned long long)s.sse);
            const uint32_t sae = wave_sum((uint32_t)s.sae);                   // at most 64 * 16 * 65535
            const int32_t sum = (int32_t)wave_sum((uint32_t)(int32_t)s.sum);
            const uint32_t zeros = wave_sum((uint32_t)s.zeros);
            const uint32_t mx = wave_max(s.max_abs);
            if (lane == 0) {
                atomicAdd(&L.acc[c][0], sse);
                atomicAdd(&L.acc[c][1], (unsigned long long)sae);
                atomicAdd(&L.acc[c][2], (unsigned long long)(long long)sum);
                atomicAdd(&L.acc[c][3], (unsigned long long)zeros);
                atomicMax(&L.max_abs[c], mx);
            }
        }
        if (SAM && nv > 0) {
            SamAcc sa = {sam_n, sam_undef, sam_sum, sam_max};
#pragma unroll 1
            for (int half = 0; half < N / SAM_PIXELS; ++half) sam_pixels<T>(slots, tid, cb, nv, half, &sa);
            sam_n = sa.n; sam_undef = sa.undefined; sam_sum = sa.sum; sam_max = sa.max;
        }
    }

    if (SAM) {
        const uint32_t n = wave_sum(sam_n), u = wave_sum(sam_undef);
        const unsigned long long mx = wave_max((unsigned long long)__double_as_longlong(sam_max));      // (angles are >= 0: their bits order them)
        const double sum = wave_sum(sam_sum);
        if (lane == 0) {
            atomicAdd(&L.sam_n, (unsigned long long)n);
            atomicAdd(&L.sam_undefined, (unsigned long long)u);
            atomicMax(&L.sam_max, mx);
            L.sam_sum[wave] = sum;
        }
    }
    __syncthreads();

    for (int i = tid; i < cb * quality::HIST_BINS; i += QT) {
        const int c = i / quality::HIST_BINS, k = i - c * quality::HIST_BINS;
        const unsigned long long n = k == 0 ? L.acc[c][3] : (unsigned long long)L.hist[c][k];
        if (n) atomicAdd(&result[(size_t)(c0 + c) * quality::BAND_WORDS + quality::F_HIST + k], n);
    }
    if (tid < cb) {
        unsigned long long* rec = result + (size_t)(c0 + tid) * quality::BAND_WORDS;
        atomicAdd(&rec[quality::F_SSE], L.acc[tid][0]);
        atomicAdd(&rec[quality::F_SAE], L.acc[tid][1]);
        atomicAdd(&rec[quality::F_SUM_ERR], L.acc[tid][2]);      // (two's complement: the sum of the int64 values)
        atomicMax(&rec[quality::F_MAX_ABS], (unsigned long long)L.max_abs[tid]);
    }
    if (SAM && tid == 0) {
        unsigned long long* rec = result + (size_t)g.C * quality::BAND_WORDS;
        atomicAdd(&rec[quality::P_SAM_N], L.sam_n);
        atomicAdd(&rec[quality::P_SAM_UNDEFINED], L.sam_undefined);
        atomicMax(&rec[quality::P_SAM_MAX], L.sam_max);
        sam_partial[blockIdx.x] = ((L.sam_sum[0] + L.sam_sum[1]) + L.sam_sum[2]) + L.sam_sum[3];
    }
}

template <class T>
__global__ void __launch_bounds__(QT, 2) k_quality_ssim(const T* __restrict__ a, int64_t a_row, int64_t a_plane, const T* __restrict__ b,
                                                         int64_t b_row, int64_t b_plane, quality::Geom g, quality::Weights wt, double c1,
                                                         double c2, double* __restrict__ partial)
{
    constexpr int IN = quality::SSIM_IN, TS = quality::SSIM_TILE, TAPS = quality::TAPS;
    __shared__ uint16_t sa[IN * IN], sb[IN * IN];
    __shared__ double hm[5][IN][TS];
    __shared__ double wsum[QT / 64];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x, ty = blockIdx.y, c = blockIdx.z;
    const int gx0 = tx * TS, gy0 = ty * TS;
    const T* pa = a + (int64_t)c * a_plane;
    const T* pb = b + (int64_t)c * b_plane;

    for (int i = tid; i < IN * IN; i += QT) {
        const int r = i / IN, col = i - r * IN;
        const int gy = gy0 + r, gx = gx0 + col;
        const bool in = gy < g.H && gx < g.W;
        sa[i] = in ? (uint16_t)pa[(int64_t)gy * a_row + gx] : (uint16_t)0;
        sb[i] = in ? (uint16_t)pb[(int64_t)gy * b_row + gx] : (uint16_t)0;
    }
    __syncthreads();
    for (int i = tid; i < IN * TS; i += QT) {
        const int r = i / TS, x = i - r * TS;
        quality::Moments m;
        quality::moments_zero(&m);
#pragma unroll
        for (int k = 0; k < TAPS; ++k) quality::moments_tap(&m, wt.w[k], (double)sa[r * IN + x + k], (double)sb[r * IN + x + k]);
        hm[0][r][x] = m.a; hm[1][r][x] = m.b; hm[2][r][x] = m.aa; hm[3][r][x] = m.bb; hm[4][r][x] = m.ab;
    }
    __syncthreads();
    double sum = 0.0;
    for (int i = tid; i < TS * TS; i += QT) {
        const int y = i / TS, x = i - y * TS;
        if (gy0 + y < g.H - 2 * quality::HALO && gx0 + x < g.W - 2 * quality::HALO) {
            quality::Moments m;
            quality::moments_zero(&m);
#pragma unroll
            for (int k = 0; k < TAPS; ++k)
                quality::moments_tap5(&m, wt.w[k], hm[0][y + k][x], hm[1][y + k][x], hm[2][y + k][x], hm[3][y + k][x], hm[4][y + k][x]);
            sum += quality::ssim_point(m, c1, c2);
        }
    }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) wsum[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0)
        partial[((size_t)c * g.tiles_y + ty) * g.tiles_x + tx] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// block c < C: band c's n, ssim_n and ssim_sum; block C: sam_sum
__global__ void __launch_bounds__(QT) k_quality_finish(quality::Geom g, int ssim, int sam, const double* __restrict__ ssim_partial,
                                                        const double* __restrict__ sam_partial, unsigned long long* __restrict__ result)
{
    __shared__ double tree[QT];
    const int tid = threadIdx.x, blk = blockIdx.x;
    const bool band = blk < g.C;
    if (band ? !ssim : !sam) {
        if (band && tid == 0) result[(size_t)blk * quality::BAND_WORDS + quality::F_N] = (unsigned long long)g.H * g.W;
        return;
    }
    const int64_t n = band ? (int64_t)g.tiles_x * g.tiles_y : g.stat_groups;
    const double* src = band ? ssim_partial + (size_t)blk * n : sam_partial;
    double s = 0.0;
    for (int64_t i = tid; i < n; i += QT) s += src[i];
    tree[tid] = s;
    __syncthreads();
    for (int o = QT / 2; o > 0; o >>= 1) {
        if (tid < o) tree[tid] += tree[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        if (band) {
            unsigned long long* rec = result + (size_t)blk * quality::BAND_WORDS;
            rec[quality::F_N] = (unsigned long long)g.H * g.W;
            rec[quality::F_SSIM_N] = (unsigned long long)g.windows;
            rec[quality::F_SSIM_SUM] = (unsigned long long)__double_as_longlong(tree[0]);
        } else {
            result[(size_t)g.C * quality::BAND_WORDS + quality::P_SAM_SUM] = (unsigned long long)__double_as_longlong(tree[0]);
        }
    }
}

template <class T>
static int launch(const T* a, int64_t a_row, int64_t a_plane, const T* b, int64_t b_row, int64_t b_plane, const quality::Geom& g,
                  double peak, uint32_t what, unsigned long long* result, double* ws, hipStream_t s)
{
    const bool sam = quality::sam_active(g, what), ssim = quality::ssim_active(g, what);
    double* sam_partial = ws;
    double* ssim_partial = ws + (sam ? g.stat_groups : 0);
    LBDRN_HIP_TRY(hipMemsetAsync(result, 0, quality::result_bytes(g.C), s));
    const dim3 grid((unsigned)g.stat_groups, (unsigned)((g.C + quality::STAT_BANDS - 1) / quality::STAT_BANDS));
    const size_t lds = stat_lds_bytes(g.C, sam);
    if (sam) {
        static std::atomic<unsigned long long> configured{0};      // (one per kernel instance)
        if (int rc = configure_lds_once(k_quality_stats<T, true>, 160 * 1024, configured)) return rc;
        k_quality_stats<T, true><<<grid, QT, lds, s>>>(a, a_row, a_plane, b, b_row, b_plane, g, result, sam_partial);
    } else {
        k_quality_stats<T, false><<<grid, QT, lds, s>>>(a, a_row, a_plane, b, b_row, b_plane, g, result, sam_partial);
    }
    LBDRN_LAUNCH_CHECK();
    if (ssim) {
        quality::Weights wt;
        quality::gauss_weights(&wt);
        k_quality_ssim<T><<<dim3((unsigned)g.tiles_x, (unsigned)g.tiles_y, (unsigned)g.C), QT, 0, s>>>(
            a, a_row, a_plane, b, b_row, b_plane, g, wt, quality::ssim_c1(peak), quality::ssim_c2(peak), ssim_partial);
        LBDRN_LAUNCH_CHECK();
    }
    k_quality_finish<<<(unsigned)g.C + 1u, QT, 0, s>>>(g, ssim ? 1 : 0, sam ? 1 : 0, ssim_partial, sam_partial, result);
    LBDRN_LAUNCH_CHECK();
    return 0;
}

static int quality_compare(const void* a, int64_t a_row, int64_t a_plane, const void* b, int64_t b_row, int64_t b_plane, int bits, int C,
                           int H, int W, double peak, uint32_t what, void* result, void* ws, size_t ws_bytes, hipStream_t s)
{
    LBDRN_REQUIRE(a && b && result, "lbdrn_quality_compare: null pointer");
    LBDRN_REQUIRE(bits == 8 || bits == 16, "lbdrn_quality_compare: %d-bit samples: 8 or 16", bits);
    quality::Geom g;
    LBDRN_REQUIRE(quality::make_geom(C, H, W, &g), "lbdrn_quality_compare: geometry %d x %d x %d is out of range", C, H, W);
    LBDRN_REQUIRE(a_row >= W && b_row >= W, "lbdrn_quality_compare: row strides %lld and %lld are below the width %d", (long long)a_row,
                  (long long)b_row, W);
    LBDRN_REQUIRE(a_plane >= 0 && b_plane >= 0, "lbdrn_quality_compare: negative plane stride");
    LBDRN_REQUIRE(peak > 0.0 && peak <= 1.0e300, "lbdrn_quality_compare: peak must be a positive finite number");
    LBDRN_REQUIRE((what & ~(quality::WHAT_SSIM | quality::WHAT_SAM)) == 0, "lbdrn_quality_compare: unknown bits in what = %u", what);
    LBDRN_REQUIRE(((uintptr_t)result & 7u) == 0, "lbdrn_quality_compare: result is not 8-byte aligned");
    const size_t need = quality::workspace_bytes(g, what);
    if (need && (!ws || ws_bytes < need || ((uintptr_t)ws & 7u))) {
        set_error("quality workspace too small or not 8-byte aligned: %zu < %zu", ws_bytes, need);
        return LBDRN_E_WORKSPACE;
    }
    if (bits == 8)
        return launch<uint8_t>((const uint8_t*)a, a_row, a_plane, (const uint8_t*)b, b_row, b_plane, g, peak, what,
                               (unsigned long long*)result, (double*)ws, s);
    return launch<uint16_t>((const uint16_t*)a, a_row, a_plane, (const uint16_t*)b, b_row, b_plane, g, peak, what,
                            (unsigned long long*)result, (double*)ws, s);
}

}  // namespace lbdrn

extern "C" {

const char* lbdrn_quality_last_error(void) { return lbdrn::last_error(); }
int lbdrn_quality_abi_version(void) { return LBDRN_QUALITY_ABI_VERSION; }

size_t lbdrn_quality_result_bytes(int32_t C) { return C >= 1 && C <= quality::MAX_BANDS ? quality::result_bytes(C) : 0; }

size_t lbdrn_quality_workspace(int32_t C, int32_t H, int32_t W, uint32_t what)
{
    quality::Geom g;
    return quality::make_geom(C, H, W, &g) ? quality::workspace_bytes(g, what) : 0;
}

int lbdrn_quality_compare(const void* a, int64_t a_row, int64_t a_plane, const void* b, int64_t b_row, int64_t b_plane, int32_t bits,
                          int32_t C, int32_t H, int32_t W, double peak, uint32_t what, void* result, void* workspace,
                          size_t workspace_bytes, void* stream)
{
    return lbdrn::quality_compare(a, a_row, a_plane, b, b_row, b_plane, bits, C, H, W, peak, what, result, workspace, workspace_bytes,
                                  (hipStream_t)stream);
}

}  // extern "C"
