// Fused apply kernel for gfx950: neighbourhood gather + normalise + nl x (Linear -> sin(30 z)) +
// Linear -> sigmoid, then either integer reconstruction (decode.py:122-134) or the squared error
// against the labels (LBDRNperformance.py:18-21), in ONE pass over the image with no feature
// matrix in HBM (the reference materialises [N,F] float32 = 3.36 GB at 2048^2x8, D=2).
//
// Mapping to CDNA4
//  * one wave = one 32-pixel row segment; every layer is computed transposed,
//    H^T[neuron][pixel] = W[neuron][k] * X^T[k][pixel], on v_mfma_f32_32x32x2_f32: A = weights
//    (one VGPR), B = inputs (one VGPR), accumulator tile = 32 neurons x 32 pixels (16 VGPRs).
//  * an f32 MFMA is a k-ordered fmaf chain seeded by the C operand, so seeding C with the bias
//    and walking k = 0,1,2,... reproduces the generic kernels / the oracle bit for bit.
//  * the accumulator layout (row = (r&3)+8(r>>2)+4(lane>>5), col = lane&31) is turned into the
//    next layer's B operand without any data movement: tile row i is assigned neuron
//    pi(i) = 2*((i&3)+4*(i>>3)) + ((i>>2)&1), so register r of lane-half h holds neuron 2r+h --
//    exactly the k = 2s+h the next MFMA step s consumes from that lane.  The permutation is
//    applied once when the weights are packed into "fragment order".
//  * weights (76 KB for F=200, bc=64) live in LDS in fragment order, so every A operand is one
//    conflict-free ds_read_b64; the D-ring of normalised MSB values is staged per 16x64 tile in
//    channel-planar LDS (conflict-free for 32 consecutive pixels) with reflect padding applied.
//  * 8 waves per CU (2 per SIMD): one wave's sin() VALU work overlaps the other's MFMAs.
#include <cstdlib>

#include "common.hpp"
#include "lbdrn_math.hpp"

namespace lbdrn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int APPLY_CHUNK = 20;   // layer-0 steps whose B operands are made in one go, a multiple of 4; eval pass on the
                                  // 8 x 2048^2 tile: 1.79-1.82 ms at 20, 1.87 at 52, 1.845 with none (round 2's loop: four at a time)
constexpr int APPLY_WAVES = 8;
constexpr int APPLY_THREADS = APPLY_WAVES * 64;
constexpr int TILE_W = 64;

// tile row i of a hidden accumulator tile carries neuron pi(i) (+32*tile)
__host__ __device__ inline int tile_row_to_neuron(int i)
{
    return 2 * ((i & 3) + 4 * (i >> 3)) + ((i >> 2) & 1);
}
// accumulator register r of lane-half h is tile row:
__host__ __device__ inline int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

enum ApplyMode { MODE_DECODE = 0, MODE_EVAL = 1, MODE_EVAL_FAST = 2,   // _FAST: the evaluation pass in the tolerance arithmetic (lbdrn_math.hpp)
                 MODE_EVAL_X16 = 3 };   // _FAST with the colour features of layer 0 on the f16 matrix pipe, exact operands (opt-in)
__host__ __device__ constexpr bool mode_fast(int mode) { return mode == MODE_EVAL_FAST || mode == MODE_EVAL_X16; }

// ---- the instances of the fused apply pass: every kernel that is compiled, each list stated once.  The planners, the mode a
// request is served in and the two dispatch functions all come from these lists.
//
// k_apply_mfma<NT, MODE, RELU> (NT = bc / 32 hidden tiles, weights resident in LDS), both activations.  No (4, MODE_EVAL_FAST): at
// bc = 128 the tolerance arithmetic's extra operands spill at two waves per SIMD (88 registers, 356 B of scratch when it was
// instantiated), and the canonical pass IS within the 1e-6 the flag promises.  No (4, MODE_EVAL_X16): ApplyPlan::pair stops at NT = 2.
#define APPLY_INSTANCES(X) \
    X(1, MODE_DECODE)    X(2, MODE_DECODE)    X(4, MODE_DECODE) \
    X(1, MODE_EVAL)      X(2, MODE_EVAL)      X(4, MODE_EVAL)   \
    X(1, MODE_EVAL_FAST) X(2, MODE_EVAL_FAST)                   \
    X(1, MODE_EVAL_X16)  X(2, MODE_EVAL_X16)
// k_apply_wide<NT, NL, MODE> (apply_wide.inc: NT = bc / 16 unit tiles, weights streamed; the Sine network), each row in MODE_DECODE,
// MODE_EVAL and MODE_EVAL_FAST: the streaming kernel has no exact-operand layer 0.
#define WAPPLY_INSTANCES(X) X(8, 1) X(8, 2) X(16, 1) X(16, 2)

// What the rest reads off the lists: whether a row names (nt, mode) / (nt, nl); a negative mode or nl stands for any.
#define X(NT, MODE) if (nt == NT && (mode < 0 || mode == MODE)) return true;
constexpr bool apply_row(int nt, int mode = -1) { APPLY_INSTANCES(X) return false; }
#undef X
#define X(NT, NL) if (nt == NT && (nl < 0 || nl == NL)) return true;
constexpr bool wapply_row(int nt, int nl = -1) { WAPPLY_INSTANCES(X) return false; }
#undef X
// The mode of the instance that serves a requested mode on nt tiles (x16: the plan has ApplyPlan::x16; never on the wide kernel):
// the exact-operand pass where the plan and a row have it, else the fast pass; the fast pass where a row has it, else the canonical one.
constexpr int serving_mode(int mode, int nt, bool x16)
{
    if (mode == MODE_EVAL_X16 && !(x16 && apply_row(nt, MODE_EVAL_X16))) mode = MODE_EVAL_FAST;
    if (mode == MODE_EVAL_FAST && !(apply_row(nt, MODE_EVAL_FAST) || wapply_row(nt))) mode = MODE_EVAL;
    return mode;
}
// requested mode x {NT 1 / 2, NT 4, wide} x {plan without / with x16}: the whole domain
#define SERVES(mode, x16, nt12, nt4, wide)                                                                                          \
    static_assert(serving_mode(mode, 1, x16) == nt12 && serving_mode(mode, 2, x16) == nt12 && serving_mode(mode, 4, x16) == nt4 && \
                  serving_mode(mode, 8, x16) == wide && serving_mode(mode, 16, x16) == wide, #mode);
SERVES(MODE_DECODE, false, MODE_DECODE, MODE_DECODE, MODE_DECODE)          SERVES(MODE_DECODE, true, MODE_DECODE, MODE_DECODE, MODE_DECODE)
SERVES(MODE_EVAL, false, MODE_EVAL, MODE_EVAL, MODE_EVAL)                  SERVES(MODE_EVAL, true, MODE_EVAL, MODE_EVAL, MODE_EVAL)
SERVES(MODE_EVAL_FAST, false, MODE_EVAL_FAST, MODE_EVAL, MODE_EVAL_FAST)   SERVES(MODE_EVAL_FAST, true, MODE_EVAL_FAST, MODE_EVAL, MODE_EVAL_FAST)
SERVES(MODE_EVAL_X16, false, MODE_EVAL_FAST, MODE_EVAL, MODE_EVAL_FAST)    SERVES(MODE_EVAL_X16, true, MODE_EVAL_X16, MODE_EVAL, MODE_EVAL_FAST)
#undef SERVES

struct ApplyPlan {
    int NT;          // hidden tiles = bc/32
    int S0;          // MFMA steps of layer 0: P positional + colour steps padded to a multiple of 4
                     // (pad steps carry zero weights: fmaf(0, finite, acc) == acc)
    int TH;          // tile rows
    int SH, SW;      // staged rows / pitch = TH+2D, TILE_W+2D
    int ncolor;      // colour features = F - 2P
    int pair;        // 1: the tolerance-arithmetic pass walks the colour features in CHANNEL PAIRS (k_apply_mfma, layer0_pair):
                     // step (c, r) multiplies window position r of channel c in lane half 0 and of channel c + C/2 in lane
                     // half 1; with RELATIVE the window centre -- an exact zero -- is not a step
    int RS;          // pair: steps per channel pair = (2D+1)^2, minus the centre with RELATIVE
    int x16;         // 1 (opt-in, LBDRN_EVAL_X16): the colour features of layer 0 on the f16 matrix pipe with EXACT operands
                     // (layer0_pair_x16): integer window differences x W_0 in three fp16 pieces, f32 accumulation
    int M16;         // x16: MFMAs per channel pair and weight piece = RS / 8
    int off_scale;   // x16: one float, 2^-s / msb_max (what turns the scaled integer accumulator into the pre-activation)
    // float offsets inside the packed buffer == inside LDS
    int off_w0, off_wh, off_wl, off_bh, off_bl, pack_floats;
    // further LDS regions (float offsets)
    int off_ktab, off_rowt, off_colt, off_tile, lds_floats;
    int tiles_x, tiles_y;
};

constexpr int X16_PIECES = 3;   // fp16 pieces of a float32 weight: 3 x 11 bits hold all 24 of its mantissa

static bool make_plan(const lbdrn_geom& g, const lbdrn_net& net, ApplyPlan* p, bool fast = false, bool x16 = false)
{
    // hidden activation: Sine(30) (LBDRNmodel.py:37) or nn.ReLU (the alternative of encode.py:75 / decode.py:108): a template
    // parameter of k_apply_mfma
    if (net.act != LBDRN_ACT_SINE && net.act != LBDRN_ACT_RELU) return false;
    if (net.bc % 32 != 0 || !apply_row(net.bc / 32)) return false;   // (bc = 96 would be NT = 3: no such kernel, the generic ones)
    if (net.C > 32 || net.nl < 1 || net.nl > 15) return false;
    ApplyPlan q;
    q.NT = net.bc / 32;
    q.ncolor = net.F - 2 * g.P;
    if (q.ncolor < 0) return false;
    q.S0 = g.P + ((q.ncolor + 1) / 2 + 3) / 4 * 4;
    // the evaluation pass in the tolerance arithmetic may take the features in any order (the sum is held to 1e-6, not to
    // a bit pattern): channel pairs, and no step for the window centres, which are exact zeros with RELATIVE
    // (LBDRNdataset.py:126-128) -- 96 MFMA steps instead of 100 at the headline shape.
    const int side = 2 * g.D + 1;
    q.pair = fast && q.NT <= 2 && g.use_colors && g.D >= 1 && g.D <= 3 && (g.C % 2) == 0 && q.ncolor == g.C * side * side;
    // (NT = 4, bc = 128: the pair's 24 operands on top of 128 accumulator / activation registers would spill at two waves per SIMD)
    q.RS = side * side - ((g.relative && g.D > 0) ? 1 : 0);
    if (q.pair) q.S0 = g.P + (g.C / 2) * q.RS;
    // the exact-operand f16 layer 0: relative colours only (the differences of two MSB values are integers; (2D+1)^2 - 1 is a
    // multiple of 8), no positional features, MSB values that fp16 holds exactly (<= 2047: any 16-bit image at K >= 5)
    q.x16 = x16 && q.pair && g.relative && g.P == 0 && g.msb_max >= 1 && g.msb_max <= 2047 && (q.RS % 8) == 0;
    q.M16 = q.RS / 8;
    const int half = net.bc / 2;
    int o = 0;
    q.off_w0 = o; o += q.x16 ? (g.C / 2) * q.M16 * X16_PIECES * 64 * q.NT * 4 : q.S0 * 64 * q.NT;
    q.off_wh = o; o += (net.nl - 1) * half * 64 * q.NT;
    q.off_wl = o; o += half * 64;
    q.off_bh = o; o += net.nl * q.NT * 32;
    q.off_bl = o; o += 32;
    q.off_scale = o; o += 4;
    q.pack_floats = o;
    q.off_ktab = o; o += 2 * 2 * (q.S0 - g.P) + 2;
    q.SW = TILE_W + 2 * g.D;
    const int fixed = o;
    int th = 16;
    for (;; th >>= 1) {
        if (th == 0) return false;
        q.TH = th;
        q.SH = th + 2 * g.D;
        o = fixed;
        q.off_rowt = o; o += th * g.P;
        q.off_colt = o; o += TILE_W * g.P;
        q.off_tile = o; o += (g.use_colors ? g.C * q.SH * q.SW : 0);
        q.lds_floats = std::max(o, q.off_rowt + 2 * APPLY_THREADS + 4);   // the per-tile regions double as the SSE reduction's doubles
        if ((size_t)q.lds_floats * 4 <= 160 * 1024) break;
    }
    q.tiles_x = (g.W + TILE_W - 1) / TILE_W;
    q.tiles_y = (g.H + q.TH - 1) / q.TH;
    *p = q;
    return true;
}

constexpr int MFMA_PARTIALS = 1024;

// ------------------------------------------------------------------ weight packing

// params (state_dict order) -> fragment order; one thread per packed float
// max |W_0| (x16: fixes the power of two that brings the weights into fp16's range); one block
__global__ void __launch_bounds__(256) k_w0_absmax(const float* __restrict__ params, int n, float* __restrict__ out)
{
    __shared__ float red[256];
    float m = 0.0f;
    for (int e = threadIdx.x; e < n; e += 256) m = fmaxf(m, fabsf(params[e]));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

// x16: the power of two s with max |W_0| 2^s < 2^15 (fp16 holds every scaled weight; 0 for an all-zero layer)
__device__ __forceinline__ int x16_shift(float amax)
{
    if (!(amax > 0.0f) || !(amax < 3.0e38f)) return 0;
    int ex;
    (void)frexpf(amax, &ex);      // amax = m 2^ex, 0.5 <= m < 1
    return 15 - ex;
}

__global__ void __launch_bounds__(256)
    k_pack_apply(const float* __restrict__ params, lbdrn_net net, ApplyPlan p, int P, int C, int msb_max, const float* __restrict__ amax,
                 float* __restrict__ out)
{
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.pack_floats) return;
    const int NT = p.NT, half = net.bc / 2;
    float v = 0.0f;
    if (p.x16 && e < p.off_wh) {
        // layer 0, exact-operand f16 (layer0_pair_x16): [channel pair][MFMA m][piece][lane][tile][8 halfs]; this thread: two
        // halfs.  Lane (row i = lane & 31, half h = lane >> 5) of MFMA m holds W_0[neuron(i, tile)][channel cp + h C/2][window
        // positions 8 m .. 8 m + 7, the centre left out], scaled by 2^s and cut into three fp16 pieces whose sum IS the float32
        // weight (3 x 11 bits of mantissa)
        const int j = e & 3, q4 = e >> 2;
        const int t = q4 % NT, lane = (q4 / NT) % 64, rest = q4 / (NT * 64);
        const int piece = rest % X16_PIECES, m = (rest / X16_PIECES) % p.M16, cp = rest / (X16_PIECES * p.M16);
        const int s2 = p.ncolor / C, cen = s2 / 2, sh = x16_shift(*amax);
        const int neuron = tile_row_to_neuron(lane & 31) + 32 * t, ch = cp + (lane >> 5) * (C / 2);
        _Float16 hv[2];
        for (int u = 0; u < 2; ++u) {
            const int pos = 8 * m + 2 * j + u, r = pos + (pos >= cen ? 1 : 0);
            const float w = ldexpf(params[(int64_t)neuron * net.F + ch * s2 + r], sh);
            const _Float16 hi = (_Float16)w;
            const float r1 = w - (float)hi;
            const _Float16 mid = (_Float16)r1;
            const float r2 = r1 - (float)mid;
            hv[u] = piece == 0 ? hi : piece == 1 ? mid : (_Float16)r2;
        }
        f16x2 pk = {hv[0], hv[1]};
        out[e] = __builtin_bit_cast(float, pk);
        return;
    }
    if (e >= p.off_scale) {   // x16: acc * this = the pre-activation's sum (acc = sum of (w 2^s) x integer difference)
        out[e] = (p.x16 && e == p.off_scale) ? ldexpf(1.0f, -x16_shift(*amax)) / (float)msb_max : 0.0f;
        return;
    }
    if (e < p.off_wh) {  // layer 0: [S0][64][NT]
        int t = e % NT, lane = (e / NT) % 64, s = e / (NT * 64);
        int k = 2 * s + (lane >> 5);
        if (p.pair && s >= P) {   // step (c, r'): channel c + (C/2) * lane half, window position r' (the centre left out)
            const int s2 = (p.ncolor / C), sp = s - P, c = sp / p.RS, rr = sp - c * p.RS;
            const int r = rr + ((p.RS < s2 && rr >= s2 / 2) ? 1 : 0);
            k = 2 * P + (c + (lane >> 5) * (C / 2)) * s2 + r;
        }
        int neuron = tile_row_to_neuron(lane & 31) + 32 * t;
        if (k < net.F) v = params[(int64_t)neuron * net.F + k];
    } else if (e < p.off_wl) {  // hidden layers 1..nl-1: [l-1][half][64][NT]
        int q = e - p.off_wh;
        int t = q % NT, lane = (q / NT) % 64, s = (q / (NT * 64)) % half, l = 1 + q / (NT * 64 * half);
        int k = 2 * s + (lane >> 5);
        int neuron = tile_row_to_neuron(lane & 31) + 32 * t;
        int64_t base = (int64_t)net.bc * net.F + net.bc + (int64_t)(l - 1) * ((int64_t)net.bc * net.bc + net.bc);
        v = params[base + (int64_t)neuron * net.bc + k];
    } else if (e < p.off_bh) {  // last layer: [half][64], rows = channels (identity order)
        int q = e - p.off_wl;
        int lane = q % 64, s = q / 64;
        int k = 2 * s + (lane >> 5), ch = lane & 31;
        int64_t base = (int64_t)net.bc * net.F + net.bc + (int64_t)(net.nl - 1) * ((int64_t)net.bc * net.bc + net.bc);
        if (ch < net.C) v = params[base + (int64_t)ch * net.bc + k];
    } else if (e < p.off_bl) {  // hidden biases: [l][t][h][16]
        int q = e - p.off_bh;
        int r = q % 16, h = (q / 16) % 2, t = (q / 32) % NT, l = q / (32 * NT);
        int neuron = 2 * r + h + 32 * t;
        int64_t wbase = l == 0 ? 0 : (int64_t)net.bc * net.F + net.bc + (int64_t)(l - 1) * ((int64_t)net.bc * net.bc + net.bc);
        int64_t nin = l == 0 ? net.F : net.bc;
        v = params[wbase + (int64_t)net.bc * nin + neuron];
    } else {  // last bias: [h][16]
        int q = e - p.off_bl;
        int r = q % 16, h = q / 16;
        int ch = acc_row(r, h);
        int64_t base = (int64_t)net.bc * net.F + net.bc + (int64_t)(net.nl - 1) * ((int64_t)net.bc * net.bc + net.bc);
        if (ch < net.C) v = params[base + (int64_t)net.C * net.bc + ch];
    }
    out[e] = v;
}

// ------------------------------------------------------------------ the fused kernel

struct ApplyArgs {
    lbdrn_geom g;
    lbdrn_net net;
    ApplyPlan p;
    const float* packed;
    const uint16_t* msb;
    const uint16_t* img;  // EVAL: original image (labels)
    uint16_t* out;        // DECODE
    float* y_out;         // DECODE, optional
    double* partial;      // EVAL: [nvirt]
    int nvirt;            // virtual workgroups: virtual workgroup v takes tiles v, v + nvirt, .. and owns partial[v]; a
                          // launch of fewer real workgroups walks them in turn -- same sums bit for bit on any grid
    int nodata;           // EVAL (LBDRN_EVAL_VALID): samples of img equal to it add no term; -1, which no sample equals: none
    int decoded;          // EVAL (LBDRN_EVAL_DECODED): a term is (img - out)^2, out the sample the decode pass writes; canonical instances only
    unsigned long long* stamps;  // diagnostic build (-DLBDRN_APPLY_STAMPS): [gridDim.x][8] cycle sums of wave 0
};

#ifdef LBDRN_APPLY_STAMPS
#define ASTAMP(k)                                                                    \
    do {                                                                              \
        unsigned long long t_;                                                        \
        __builtin_amdgcn_sched_barrier(0);                                            \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");   \
        __builtin_amdgcn_sched_barrier(0);                                            \
        acc_t[k] += t_ - last_t;                                                      \
        last_t = t_;                                                                  \
    } while (0)
#else
#define ASTAMP(k)
#endif

template <int NT>
__device__ __forceinline__ void load_a(const float* w, int idx, float (&a)[NT])
{
    if constexpr (NT == 1) {
        a[0] = w[idx];
    } else if constexpr (NT == 2) {
        float2 v = *reinterpret_cast<const float2*>(w + (size_t)idx * 2);
        a[0] = v.x; a[1] = v.y;
    } else {
        float4 v = *reinterpret_cast<const float4*>(w + (size_t)idx * 4);
        a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
    }
}

// Layer 0 of the tolerance-arithmetic evaluation pass over the colour features, in channel pairs (ApplyPlan::pair): lane
// half h walks the window of channel c + h C/2, so one per-lane base address serves every step of a pair and what
// changes from step to step is a compile-time offset: per step ONE LDS read of the window (the canonical loop reads an
// offset pair out of a table, the neighbour AND the centre: three reads), the centre of the pair's channel is read once
// and held in a register, and the window centre itself -- centre minus centre, an exact zero -- is not a step.
// wc: the pair's first fragment (w0 + ((P + c RS) 64 + lane) NT); tp: tile + c plane + (h C/2) plane + ly SW + lx + j.
template <int NT, int D, bool REL>
__device__ __forceinline__ void layer0_pair(f32x16 (&acc)[NT], const float* wc, const float* tp)
{
    constexpr int side = 2 * D + 1, S2 = side * side, CEN = D * side + D, SW = TILE_W + 2 * D, RS = S2 - (REL ? 1 : 0);
    const float cen = tp[D * SW + D];
    float bq[RS];
#pragma unroll
    for (int r = 0; r < S2; ++r) {
        if (REL && r == CEN) continue;
        const float nb = tp[(r / side) * SW + (r % side)];
        bq[r - ((REL && r > CEN) ? 1 : 0)] = REL ? nb - cen : nb;   // minus centre, LBDRNdataset.py:126-128
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < RS; ++k) {
        float a[NT];
        load_a<NT>(wc, k * 64, a);
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tt], bq[k], acc[tt], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
}

// Layer 0 over the colour features on the f16 matrix pipe, operands EXACT (MODE_EVAL_X16; ApplyPlan::x16).  A relative colour
// feature is (msb_nbr - msb_ctr) / max: the numerator an integer of at most 11 bits -- exactly an fp16 --, and a float32
// weight is exactly the sum of three fp16 pieces once a power of two has brought it into range (k_pack_apply).  So
//     sum_k W[n][k] x[k]  =  (2^-s / max)  sum_pieces sum_k piece[n][k] * int[k]
// with every product exact (11 x 11 bits) and the sums taken in float32 by v_mfma_f32_32x32x16_f16: the same real numbers as
// the float32 MFMA of layer0_pair, with fewer roundings (the reference rounds nbr / max, ctr / max and their difference; this
// rounds none of them), at 3/16 of its matrix-pipe cycles.  Lane half h walks channel c + h C/2 as in layer0_pair; one MFMA
// takes eight window positions of both channels (k = 8 h + i).  tp: the STAGED INTEGERS of this lane's pixel (tile holds
// float(msb), not msb / max, in this mode); wc: the pair's first fragment + lane NT 4 floats.
template <int NT, int D>
__device__ __forceinline__ void layer0_pair_x16(f32x16 (&acc)[NT], const float* wc, const float* tp)
{
    constexpr int side = 2 * D + 1, S2 = side * side, CEN = D * side + D, SW = TILE_W + 2 * D, RS = S2 - 1, M = RS / 8;
    static_assert(RS % 8 == 0, "(2D+1)^2 - 1 = 4 D (D+1)");
    const float cen = tp[D * SW + D];
    float bq[RS];
#pragma unroll
    for (int r = 0; r < S2; ++r) {
        if (r == CEN) continue;
        bq[r - (r > CEN ? 1 : 0)] = tp[(r / side) * SW + (r % side)] - cen;     // an integer in [-2047, 2047]: exact
    }
    f16x8 b[M];
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f16x2 pk = __builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_pkrtz(bq[8 * m + 2 * j], bq[8 * m + 2 * j + 1]));   // (exact: integers)
            b[m][2 * j] = pk[0];
            b[m][2 * j + 1] = pk[1];
        }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int pc = 0; pc < X16_PIECES; ++pc) {
            const float4* ap = reinterpret_cast<const float4*>(wc + (size_t)((m * X16_PIECES + pc) * 64) * NT * 4);
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, ap[tt]), b[m], acc[tt], 0, 0, 0);
        }
    __builtin_amdgcn_sched_barrier(0);
}

// hidden activation of one accumulator entry.  RELU: z where z > 0, else 0 (torch.nn.ReLU: the same in every arithmetic)
template <int MODE, bool RELU>
__device__ __forceinline__ float apply_hidden_act(float z)
{
    if constexpr (RELU) return z > 0.0f ? z : 0.0f;
    else return mode_fast(MODE) ? fast_sin(30.0f * z) : siren_act(z);
}

// The last layer (bc -> C, C <= 8) of the tolerance-arithmetic pass on v_mfma_f32_4x4x1_16B_f32: sixteen independent 4x4 outer
// products per instruction, block b = lane / 4, D_b[i][j] += A_b[i] B_b[j] with A_b[i] in lane 4 b + i, B_b[j] in lane 4 b + j and
// D_b[i][j] in register i of lane 4 b + j (scripts/mfma4_probe.hip checks the map and times the instruction).  The hidden
// activations already sit where B wants them -- lane 32 h + j holds pixel j, register r unit 2 r + h --, so with
// A = W_last[4 g + (lane & 3)][unit] every lane collects four channels of ITS pixel over the units of ITS half's parity:
// NG = (C + 3) / 4 instructions per hidden register where the 32x32x2 tile spends 64 cycles of the matrix pipe on 32 rows, 24 of
// them padding at C = 8.  The A operand comes out of the fragments as they are packed for the 32x32x2 step: row 4 g + (lane & 3)
// of lane half h is entry 32 h + 4 g + (lane & 3) of step s (four addresses per half, broadcast: no bank conflict).  The halves
// are joined by one v_permlane32_swap and one add per register, after which half h holds channels 4 h .. 4 h + 3 complete -- the
// channels the epilogue finishes in that half, out of registers 0..3 of o as before.  The sum's order: bias + even units
// ascending, the odd units ascending from zero, then the two (held to 1e-6 of the canonical sum, not to its bits).
// wl: the [bc/2][64] fragments; bl: the last bias as packed, [h][16] with entry r < 4 of half g = bias[4 g + r].
template <int NT, int NG>
__device__ __forceinline__ void last_layer_4x4(f32x16& o, const f32x16 (&hid)[NT], const float* wl, const float* bl, int lane)
{
    const bool lo = lane < 32;
    f32x4 part[NG];
#pragma unroll
    for (int gq = 0; gq < NG; ++gq) {
        const float4 b4 = *reinterpret_cast<const float4*>(bl + gq * 16);
        part[gq][0] = lo ? b4.x : 0.0f; part[gq][1] = lo ? b4.y : 0.0f;
        part[gq][2] = lo ? b4.z : 0.0f; part[gq][3] = lo ? b4.w : 0.0f;
    }
    // every fragment is read before the first product: an instruction this short (4.5 cycles of the pipe, 16 until its result
    // can be accumulated on) hides no LDS latency behind itself the way a 64-cycle 32x32x2 does
    const float* wq = wl + (lane & 32) + (lane & 3);
    float a[NT * 16][NG];
#pragma unroll
    for (int s = 0; s < NT * 16; ++s)
#pragma unroll
        for (int gq = 0; gq < NG; ++gq) a[s][gq] = wq[s * 64 + 4 * gq];
    __builtin_amdgcn_sched_barrier(0);   // (or the scheduler sinks each read to just before its product again)
#pragma unroll
    for (int s = 0; s < NT * 16; ++s) {
        const float b = hid[s / 16][s % 16];
#pragma unroll
        for (int gq = 0; gq < NG; ++gq) part[gq] = __builtin_amdgcn_mfma_f32_4x4x1f32(a[s][gq], b, part[gq], 0, 0, 0);
    }
    // swap(x, y): lanes 32..63 of x <-> lanes 0..31 of y.  x = group 0, y = group NG - 1: afterwards x is [group 0 | group NG-1]
    // of the even units, y the same of the odd units
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float x = part[0][i], y = part[NG - 1][i];   // (scalars first: a bit cast of a vector ELEMENT reads element 0)
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
        const unsigned even = sw[0], odd = sw[1];
        o[i] = __uint_as_float(even) + __uint_as_float(odd);
    }
}

template <int NT, int MODE, bool RELU>
__global__ void __launch_bounds__(APPLY_THREADS) k_apply_mfma(ApplyArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const lbdrn_geom& g = A.g;
    const ApplyPlan& p = A.p;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int half = A.net.bc / 2;
    const int P = g.P, D = g.D, C = g.C;

    // ---- once per workgroup: weights (fragment order) and the colour offset table into LDS
    for (int e = tid * 4; e < p.pack_floats; e += APPLY_THREADS * 4) {
        if (e + 3 < p.pack_floats) {
            *reinterpret_cast<float4*>(lds + e) = *reinterpret_cast<const float4*>(A.packed + e);
        } else {
            for (int q = e; q < p.pack_floats; ++q) lds[q] = A.packed[q];
        }
    }
    int* ktab = reinterpret_cast<int*>(lds + p.off_ktab);
    {
        const int side = 2 * D + 1, plane = p.SH * p.SW;
        for (int k = tid; k < 2 * (p.S0 - P) + 1; k += APPLY_THREADS) {
            int kk = min(k, p.ncolor - 1);  // pad entries repeat the last feature (their weight is 0)
            kk = max(kk, 0);
            int c = kk / (side * side), r = kk - c * side * side;
            int dy = r / side, dx = r - dy * side;
            ktab[2 * k] = c * plane + (dy - D) * p.SW + (dx - D);
            ktab[2 * k + 1] = c * plane;
        }
    }
    const float* w0 = lds + p.off_w0;
    const float* wh = lds + p.off_wh;
    const float* wl = lds + p.off_wl;
    const float* bh = lds + p.off_bh;
    const float* bl = lds + p.off_bl;
    float* rowt = lds + p.off_rowt;
    float* colt = lds + p.off_colt;
    float* tile = lds + p.off_tile;
    const bool rel = g.relative && D > 0;
    const float maxf = (float)g.msb_max;
    const int64_t HW = (int64_t)g.H * g.W;
    const float scale = (float)((1 << g.K) - 1);
    const int lmask = (1 << g.K) - 1;
#ifdef LBDRN_APPLY_STAMPS
    unsigned long long acc_t[8] = {}, last_t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(last_t)::"memory");
#endif
    const int ntiles = p.tiles_x * p.tiles_y;
    for (int v = blockIdx.x; v < A.nvirt; v += gridDim.x) {
    double sse = 0.0;
    for (int t = v; t < ntiles; t += A.nvirt) {
        const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
        const int y0 = ty * p.TH, x0 = tx * TILE_W;
        __syncthreads();  // previous tile fully consumed (and the weight copy landed)
        // ---- stage the (TH+2D) x (64+2D) ring: p = float(msb)/max, reflect-padded (LBDRNdataset.py:120-123)
        if (g.use_colors) {
            // element e = (c, sy, sx) in LDS order, consecutive lanes = consecutive columns of one row, so a
            // wave load is one or two full 128-byte lines of the uint16 plane.  Eight loads are issued
            // before the first division (a load -> divide -> store loop paid the memory latency once per
            // element: 27 % of the kernel).  Index split by multiply-high (exact for e < 2^16, SW,SH < 2^8).
            const int plane = p.SH * p.SW, total = C * plane;
            const unsigned msw = 0xFFFFFFFFu / (unsigned)p.SW + 1u, msh = 0xFFFFFFFFu / (unsigned)p.SH + 1u;
            // (SH == 1 would need the multiplier 2^32: such single-row tiles take the dividing path)
            const bool simple = D < g.H && D < g.W && total < 65536 && p.SH > 1;
            constexpr int UB = 8;
            for (int base = 0; base < total; base += APPLY_THREADS * UB) {
                unsigned short raw[UB];
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    const int e = min(base + u * APPLY_THREADS + tid, total - 1);
                    int row, sx, c, sy, yy, xx;
                    if (simple) {
                        row = (int)__umulhi((unsigned)e, msw); sx = e - row * p.SW;
                        c = (int)__umulhi((unsigned)row, msh); sy = row - c * p.SH;
                        yy = y0 + sy - D; xx = x0 + sx - D;
                        yy = yy < 0 ? -yy : yy; yy = yy >= g.H ? 2 * (g.H - 1) - yy : yy;
                        xx = xx < 0 ? -xx : xx; xx = xx >= g.W ? 2 * (g.W - 1) - xx : xx;
                        yy = max(0, min(yy, g.H - 1));  // rows / columns past a ragged last tile feed only
                        xx = max(0, min(xx, g.W - 1));  // masked outputs: any valid pixel will do
                    } else {
                        row = e / p.SW; sx = e - row * p.SW; c = row / p.SH; sy = row - c * p.SH;
                        yy = reflect_idx(y0 + sy - D, g.H); xx = reflect_idx(x0 + sx - D, g.W);
                    }
                    // (the fast evaluation pass is internal to a fit, whose MSB plane IS img >> K: one plane read per pass
                    //  instead of two; the API's canonical pass and the decode pass read the plane they are given)
                    raw[u] = mode_fast(MODE) ? (unsigned short)(A.img[(int64_t)c * HW + (int64_t)yy * g.W + xx] >> g.K)
                                             : A.msb[(int64_t)c * HW + (int64_t)yy * g.W + xx];
                }
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    const int e = base + u * APPLY_THREADS + tid;
                    if (e < total) tile[e] = MODE == MODE_EVAL_X16 ? (float)raw[u] : (float)raw[u] / maxf;   // (x16: the integers themselves)
                }
            }
        }
        for (int e = tid; e < p.TH * P; e += APPLY_THREADS) {
            int yy = min(y0 + e / P, g.H - 1);
            rowt[e] = g.rowtab[(int64_t)yy * P + e % P];
        }
        for (int e = tid; e < TILE_W * P; e += APPLY_THREADS) {
            int xx = min(x0 + e / P, g.W - 1);
            colt[e] = g.coltab[(int64_t)xx * P + e % P];
        }
        __syncthreads();

        ASTAMP(0);  // staging + barriers
        const int nseg = p.TH * (TILE_W / 32);
        for (int seg = wave; seg < nseg; seg += APPLY_WAVES) {
            const int ly = seg / (TILE_W / 32), lx = (seg % (TILE_W / 32)) * 32;
            const int pixbase = (ly + D) * p.SW + (lx + j + D);
            // what the epilogue needs from HBM (the label source or the MSB to rebuild) is requested now, so
            // that its latency hides behind the layer-0 MFMAs instead of ending the block
            const int yy = y0 + ly, xx = x0 + lx + j;
            const bool inside = yy < g.H && xx < g.W;
            const int64_t pix = (int64_t)min(yy, g.H - 1) * g.W + min(xx, g.W - 1);
            const int nreg = 4 * ((C + 7) / 8);  // accumulator registers that hold real channels
            unsigned short pre[16];
            {
                const uint16_t* src = (MODE == MODE_DECODE) ? A.msb : A.img;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    pre[r] = 0;
                    if (r < nreg) pre[r] = src[(int64_t)min(acc_row(r, h), C - 1) * HW + pix];
                }
            }
            f32x16 acc[NT];
            f32x16 hid[NT];
            // ---- layer 0: C operand = bias, then k = 0..F-1 in order
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    float4 b4 = *reinterpret_cast<const float4*>(bh + (tt * 2 + h) * 16 + q4 * 4);
                    acc[tt][q4 * 4 + 0] = b4.x; acc[tt][q4 * 4 + 1] = b4.y;
                    acc[tt][q4 * 4 + 2] = b4.z; acc[tt][q4 * 4 + 3] = b4.w;
                }
            if constexpr (MODE == MODE_EVAL_X16) {
                // exact-operand f16 layer 0 (the plan guarantees P == 0, relative colours, D in 1..3): the accumulator starts at
                // zero, collects sum (w 2^s) x integer, and becomes the pre-activation as fma(acc, 2^-s / max, bias)
                f32x16 bias0[NT];
#pragma unroll
                for (int tt = 0; tt < NT; ++tt) {
                    bias0[tt] = acc[tt];
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[tt][r] = 0.0f;
                }
                const int plane = p.SH * p.SW;
                const float* tp = tile + h * (C / 2) * plane + ly * p.SW + lx + j;
                const float* wc = w0 + (size_t)lane * NT * 4;
                const size_t wstep = (size_t)p.M16 * X16_PIECES * 64 * NT * 4;
                for (int c = 0; c < C / 2; ++c, tp += plane, wc += wstep) {
                    if (D == 1) layer0_pair_x16<NT, 1>(acc, wc, tp);
                    else if (D == 2) layer0_pair_x16<NT, 2>(acc, wc, tp);
                    else layer0_pair_x16<NT, 3>(acc, wc, tp);
                }
                const float cs = lds[p.off_scale];
#pragma unroll
                for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[tt][r] = fmaf(acc[tt][r], cs, bias0[tt][r]);
            }
            for (int s = 0; s < (MODE == MODE_EVAL_X16 ? 0 : P); ++s) {  // positional features, k = 2s+h < 2P
                int k = 2 * s + h;
                float b = (k < P) ? rowt[ly * P + k] : colt[(lx + j) * P + (k - P)];
                float a[NT];
                load_a<NT>(w0, s * 64 + lane, a);
#pragma unroll
                for (int tt = 0; tt < NT; ++tt)
                    acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tt], b, acc[tt], 0, 0, 0);
            }
            bool paired = MODE == MODE_EVAL_X16;
            if constexpr (MODE == MODE_EVAL_FAST) {
                if (p.pair) {
                    paired = true;
                    const int plane = p.SH * p.SW;
                    const float* tp = tile + h * (C / 2) * plane + ly * p.SW + lx + j;
                    const float* wc = w0 + ((size_t)P * 64 + lane) * NT;
                    for (int c = 0; c < C / 2; ++c, tp += plane, wc += (size_t)p.RS * 64 * NT) {
                        if (rel) {
                            if (D == 1) layer0_pair<NT, 1, true>(acc, wc, tp);
                            else if (D == 2) layer0_pair<NT, 2, true>(acc, wc, tp);
                            else layer0_pair<NT, 3, true>(acc, wc, tp);
                        } else {
                            if (D == 1) layer0_pair<NT, 1, false>(acc, wc, tp);
                            else if (D == 2) layer0_pair<NT, 2, false>(acc, wc, tp);
                            else layer0_pair<NT, 3, false>(acc, wc, tp);
                        }
                    }
                }
            }
            if (!paired) {
                // colour features in chunks of CH steps: the chunk's B operands (window gather, minus centre) are all made
                // first -- vector and LDS work only --, then its 2 CH MFMAs run with nothing but their A-operand reads
                // between them: an f32 MFMA and vector work of the SAME wave never overlap, those of the two waves
                // sharing a SIMD do once their streams are not both a fine mix of the two (scripts/pipe_probe.hip)
                constexpr int CH = APPLY_CHUNK;
                static_assert(CH % 4 == 0, "the steps left behind the chunks are taken four at a time");
                int s4 = P;
                for (; s4 + CH <= p.S0; s4 += CH) {
                    float bq[CH];
#pragma unroll
                    for (int u = 0; u < CH; ++u) {
                        const int kk = 2 * (s4 + u - P) + h;
                        const int2 e = *reinterpret_cast<const int2*>(ktab + 2 * kk);
                        const float nb = tile[pixbase + e.x];
                        const float ct = tile[pixbase + e.y];
                        bq[u] = rel ? nb - ct : nb;  // minus centre, LBDRNdataset.py:126-128
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int u = 0; u < CH; ++u) {
                        float a[NT];
                        load_a<NT>(w0, (s4 + u) * 64 + lane, a);
#pragma unroll
                        for (int tt = 0; tt < NT; ++tt)
                            acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tt], bq[u], acc[tt], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                for (; s4 < p.S0; s4 += 4) {  // the colour features left behind the chunks, four MFMA steps per trip
                    float bq[4];
                    float aq[4][NT];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        int kk = 2 * (s4 + u - P) + h;
                        int2 e = *reinterpret_cast<const int2*>(ktab + 2 * kk);
                        float nb = tile[pixbase + e.x];
                        float ct = tile[pixbase + e.y];
                        bq[u] = rel ? nb - ct : nb;  // minus centre, LBDRNdataset.py:126-128
                        load_a<NT>(w0, (s4 + u) * 64 + lane, aq[u]);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int tt = 0; tt < NT; ++tt)
                            acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[u][tt], bq[u], acc[tt], 0, 0, 0);
                }
            }
            ASTAMP(1);  // layer 0
#pragma unroll
            for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                for (int r = 0; r < 16; ++r) hid[tt][r] = apply_hidden_act<MODE, RELU>(acc[tt][r]);
            ASTAMP(2);  // sin
            // ---- hidden layers 1..nl-1: B operand = previous activations, straight from registers
            for (int l = 1; l < A.net.nl; ++l) {
                const float* wlayer = wh + (size_t)(l - 1) * half * 64 * NT;
#pragma unroll
                for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) {
                        float4 b4 = *reinterpret_cast<const float4*>(bh + ((l * NT + tt) * 2 + h) * 16 + q4 * 4);
                        acc[tt][q4 * 4 + 0] = b4.x; acc[tt][q4 * 4 + 1] = b4.y;
                        acc[tt][q4 * 4 + 2] = b4.z; acc[tt][q4 * 4 + 3] = b4.w;
                    }
#pragma unroll
                for (int s = 0; s < NT * 16; ++s) {
                    float b = hid[s / 16][s % 16];
                    float a[NT];
                    load_a<NT>(wlayer, s * 64 + lane, a);
#pragma unroll
                    for (int tt = 0; tt < NT; ++tt)
                        acc[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tt], b, acc[tt], 0, 0, 0);
                }
#pragma unroll
                for (int tt = 0; tt < NT; ++tt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) hid[tt][r] = apply_hidden_act<MODE, RELU>(acc[tt][r]);
            }
            ASTAMP(3);  // hidden layers incl. their sin
            // ---- last layer: rows = channels
            f32x16 o;
            if (mode_fast(MODE)) {   // (C <= 8: run_apply) 4x4 blocks, no padded rows (registers 0..3 of o: channels 4 h .. 4 h + 3, as below)
                if (C > 4) last_layer_4x4<NT, 2>(o, hid, wl, bl, lane);
                else last_layer_4x4<NT, 1>(o, hid, wl, bl, lane);
            } else {
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    float4 b4 = *reinterpret_cast<const float4*>(bl + h * 16 + q4 * 4);
                    o[q4 * 4 + 0] = b4.x; o[q4 * 4 + 1] = b4.y; o[q4 * 4 + 2] = b4.z; o[q4 * 4 + 3] = b4.w;
                }
#pragma unroll
                for (int s = 0; s < NT * 16; ++s) {
                    float b = hid[s / 16][s % 16];
                    float a = wl[s * 64 + lane];
                    o = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, o, 0, 0, 0);
                }
            }
            ASTAMP(4);  // last layer
            // ---- epilogue (the 4x4-block last layer writes o[0..3] only: it runs with C <= 8, where nreg is 4 and no other entry is read)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ch = acc_row(r, h);
                if (r < nreg && ch < C && inside) {
                    float yv = mode_fast(MODE) ? fast_sigmoid(o[r]) : canon_sigmoid(o[r]);
                    if (MODE == MODE_DECODE) {
                        float rr = __builtin_rintf(yv * scale);  // torch.round, decode.py:131
                        int base = (int)pre[r] << g.K;             // decode.py:134
                        A.out[(int64_t)ch * HW + pix] = (uint16_t)(base + (int)rr);
                        if (A.y_out) A.y_out[pix * C + ch] = yv;
                    } else if ((int)pre[r] != A.nodata) {   // (a nodata sample: a term not added)
                        if (MODE == MODE_EVAL && A.decoded) {   // (uniform over the launch; the centre sample of msb, as the decode pass reads it)
                            // (opaque: the band's 64-bit offset is formed here; left to the compiler, sixteen of them are held in
                            //  registers over the loops -- 30 more VGPRs, which the flagless pass would pay too)
                            int band = ch;
                            asm volatile("" : "+v"(band));
                            sse += decoded_term((int)pre[r], (int)A.msb[(int64_t)band * HW + pix], yv, scale, g.K);
                            continue;
                        }
                        float lab = (float)((int)pre[r] & lmask) / scale;
                        float d = yv - lab;
                        sse += (double)(d * d);
                    }
                }
            }
            ASTAMP(5);  // epilogue
        }
    }
    if (MODE != MODE_DECODE) {
        __syncthreads();
        double* red = reinterpret_cast<double*>(lds + ((p.off_rowt + 3) & ~3));  // the per-tile regions: consumed
        red[tid] = sse;
        __syncthreads();
        for (int o2 = APPLY_THREADS / 2; o2 > 0; o2 >>= 1) {
            if (tid < o2) red[tid] += red[tid + o2];
            __syncthreads();
        }
        if (tid == 0) A.partial[v] = red[0];
    }
    }
#ifdef LBDRN_APPLY_STAMPS
    if (tid == 0 && A.stamps)
        for (int k = 0; k < 8; ++k) A.stamps[(size_t)blockIdx.x * 8 + k] = acc_t[k];
#endif
}

// one wave: lane l sums partial[l], partial[l + 64], .. in index order, then the 64 lane sums pairwise in a fixed tree
// (the same value every run; a single thread walking 256 partials took 13 us)
__global__ void k_sum_partials_mfma(const double* __restrict__ partial, int n, double* dst)
{
    const int lane = threadIdx.x;
    double s = 0.0;
    for (int i = lane; i < n; i += 64) s += partial[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if (lane == 0) *dst = s;
}

#include "apply_wide.inc"

static size_t wapply_workspace(const lbdrn_geom& g, const lbdrn_net& net)
{
    WApplyPlan p;
    if (!make_wapply_plan(g, net, &p)) return 0;
    return align_up((size_t)p.pack_floats * 4, 256) + align_up(MFMA_PARTIALS * sizeof(double), 256);
}

bool mfma_apply_supported(const lbdrn_geom& g, const lbdrn_net& net)
{
    ApplyPlan p;
    WApplyPlan w;
    return make_plan(g, net, &p) || make_wapply_plan(g, net, &w);
}

// the packed weights of the largest of a shape's plans | the SSE partials | one float: max |W_0| (x16)
static size_t apply_pack_bytes(const lbdrn_geom& g, const lbdrn_net& net)
{
    ApplyPlan p{}, q{};
    if (!make_plan(g, net, &p)) return 0;
    lbdrn_geom gx = g;
    gx.msb_max = 1;                     // (the workspace is sized before the image's maximum is known to the caller's struct)
    const bool x = make_plan(gx, net, &q, true, true) && q.x16;
    return align_up((size_t)std::max(p.pack_floats, x ? q.pack_floats : 0) * 4, 256);
}

size_t mfma_apply_workspace(const lbdrn_geom& g, const lbdrn_net& net)
{
    ApplyPlan p;
    if (!make_plan(g, net, &p)) return wapply_workspace(g, net);
    return apply_pack_bytes(g, net) + align_up(MFMA_PARTIALS * sizeof(double), 256) + 256;
}

// Launch either kernel.  ALWAYS_160K: the kernel may use the whole 160 KB of a CU's LDS (k_apply_mfma; k_apply_wide's own map
// stays under the 64 KB no kernel has to ask for).  whole_lds (a fit's background evaluation pass): the workgroup asks for 125 of
// the CU's 128 LDS granules of 1,280 bytes whatever it needs, so that the k_reduce_adam launches of the training chain beside it
// (4 granules) are placed on the CUs the chain's own training step has just left, not next to this pass's waves -- there they
// took 14.4 instead of 4.9 us (kernel trace of a fit alone, scripts/lone_timeline.py; bc = 256, one tile alone: 569.5 -> 558.5 ms)
template <auto KERN, int THREADS, bool ALWAYS_160K, class Args>
static int launch_pass(const Args& A, int grid, hipStream_t s, bool whole_lds)
{
    const size_t lds_bytes = std::max((size_t)A.p.lds_floats * 4, whole_lds ? (size_t)125 * 1280 : (size_t)0);
    static std::atomic<unsigned long long> configured{0};   // (one per kernel instance)
    if (ALWAYS_160K || whole_lds)
        if (int rc = configure_lds_once(KERN, 160 * 1024, configured)) return rc;
    KERN<<<grid, THREADS, lds_bytes, s>>>(A);
    LBDRN_LAUNCH_CHECK();
    return 0;
}

// The one place a kernel of each list is named for launching.  A (NT, mode) or (NT, nl) that no row names is one the planners do
// not plan and serving_mode does not answer: it is refused, never run on some other instance.
static int dispatch_apply(const ApplyArgs& A, int mode, int grid, hipStream_t s, bool whole_lds)
{
    const bool relu = A.net.act == LBDRN_ACT_RELU;
    if (mode_fast(mode) && A.net.C > 8) {   // (last_layer_4x4 finishes channels 0..7)
        set_error("the fast instances of the fused apply pass take at most 8 bands, not %d", A.net.C);
        return LBDRN_E_UNSUPPORTED;
    }
#define X(nt, m)                                                                                                       \
    if (A.p.NT == nt && mode == m)                                                                                     \
        return relu ? launch_pass<k_apply_mfma<nt, m, true>, APPLY_THREADS, true>(A, grid, s, whole_lds)               \
                    : launch_pass<k_apply_mfma<nt, m, false>, APPLY_THREADS, true>(A, grid, s, whole_lds);
    APPLY_INSTANCES(X)
#undef X
    set_error("no fused apply pass is built for NT = %d, mode %d", A.p.NT, mode);
    return LBDRN_E_UNSUPPORTED;
}

static int dispatch_wapply(const WApplyArgs& A, int mode, int grid, hipStream_t s, bool whole_lds)
{
#define LAUNCH(nt, n, m) if (mode == m) return launch_pass<k_apply_wide<nt, n, m>, WA_THREADS, false>(A, grid, s, whole_lds);
#define X(nt, n) if (A.p.NT == nt && A.net.nl == n) { LAUNCH(nt, n, MODE_DECODE) LAUNCH(nt, n, MODE_EVAL) LAUNCH(nt, n, MODE_EVAL_FAST) }
    WAPPLY_INSTANCES(X)
#undef X
#undef LAUNCH
    set_error("no streamed apply pass is built for NT = %d, nl = %d, mode %d", A.p.NT, A.net.nl, mode);
    return LBDRN_E_UNSUPPORTED;
}

struct ApplyCall {   // what an entry point hands the driver
    const lbdrn_geom& g;
    const lbdrn_net& net;
    const uint16_t *img, *msb;   // img: EVAL only
    const float* params;
    uint16_t* out;   // DECODE
    float* y_out;    // DECODE, optional
    double* sse;     // EVAL
    int nodata;      // EVAL: the sample value left out of the sum (LBDRN_EVAL_VALID), or -1
    bool decoded;    // EVAL: the closed-loop sum (LBDRN_EVAL_DECODED); the canonical instance serves it
    void* ws;
    size_t ws_bytes;
    bool background;
    hipStream_t s;
};

static int workspace_holds(const ApplyCall& c, size_t need)
{
    if (c.ws && c.ws_bytes >= need) return 0;
    set_error("apply workspace too small: %zu < %zu", c.ws_bytes, need);
    return LBDRN_E_WORKSPACE;
}

// diagnostic build: wave 0's cycle sums of every workgroup, read back and printed per pass
template <class Args>
static int report_stamps(const Args& A, int grid, hipStream_t s)
{
#ifdef LBDRN_APPLY_STAMPS
    LBDRN_HIP_TRY(hipStreamSynchronize(s));
    unsigned long long h[1024 * 8];
    LBDRN_HIP_TRY(hipMemcpy(h, A.stamps, (size_t)grid * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    double sum[8] = {};
    for (int b = 0; b < grid; ++b) for (int k = 0; k < 8; ++k) sum[k] += (double)h[b * 8 + k];
    if constexpr (std::is_same<Args, WApplyArgs>::value) {
        const double segs = (double)A.p.tiles_x * A.p.tiles_y * A.p.TH * (TILE_W / 16) / 4 / grid;
        double rtmin = 1e30, rtmax = 0;
        for (int b = 0; b < grid; ++b) { rtmin = std::min(rtmin, (double)h[b * 8 + 6]); rtmax = std::max(rtmax, (double)h[b * 8 + 6]); }
        fprintf(stderr, "[lbdrn wide apply stamps] wave lifetime %.2f .. %.2f ms (mean %.2f); per wave: tiles-staging %.0f total; per 16-px segment: L0 %.0f sin %.0f L1 %.0f last %.0f epilogue %.0f\n",
                rtmin / 1e5, rtmax / 1e5, sum[6] / grid / 1e5, sum[0] / grid, sum[1] / grid / segs, sum[2] / grid / segs, sum[3] / grid / segs, sum[4] / grid / segs, sum[5] / grid / segs);
    } else {
        const double blocks = (double)A.p.tiles_x * A.p.tiles_y * A.p.TH * (TILE_W / 32) / APPLY_WAVES / grid;
        fprintf(stderr, "[lbdrn apply stamps] per wave: tiles-staging %.0f total; per 32-px block: L0 %.0f sin %.0f hidden %.0f last %.0f epilogue %.0f\n",
                sum[0] / grid, sum[1] / grid / blocks, sum[2] / grid / blocks, sum[3] / grid / blocks, sum[4] / grid / blocks, sum[5] / grid / blocks);
    }
#endif
    return 0;
}

// What a pass of either kernel does once its plan is made and its weights are packed: fill the args, size the launch, run the
// instance that serves `mode`, sum the evaluation's partials.
template <class Args>
static int run_pass(Args& A, const ApplyCall& c, int mode, const float* packed, double* partial,
                    int (*dispatch)(const Args&, int, int, hipStream_t, bool))
{
    A.g = c.g; A.net = c.net; A.packed = packed; A.msb = c.msb; A.img = c.img; A.out = c.out; A.y_out = c.y_out; A.partial = partial; A.nodata = c.nodata; A.decoded = c.decoded;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess)
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    A.nvirt = std::min(std::min(A.p.tiles_x * A.p.tiles_y, cus), MFMA_PARTIALS);
    // a background pass (beside a training stream that holds the other half of the CUs) launches half as many
    // workgroups, each walking two virtual ones
    const int grid = c.background ? std::max(1, A.nvirt / 2) : A.nvirt;   // (a quarter / a sixth: 3 / 10 ms per tile slower)
    A.stamps = nullptr;
#ifdef LBDRN_APPLY_STAMPS
    static unsigned long long* stamp_buf = nullptr;
    if (!stamp_buf) LBDRN_HIP_TRY(hipMalloc(&stamp_buf, 1024 * 8 * sizeof(unsigned long long)));
    A.stamps = stamp_buf;
#endif
    // evaluation claims the whole LDS exactly when it runs in the background; the decode pass never does
    if (int rc = dispatch(A, mode, grid, c.s, c.background && mode != MODE_DECODE)) return rc;
    if (mode != MODE_DECODE) {
        k_sum_partials_mfma<<<1, 64, 0, c.s>>>(partial, A.nvirt, c.sse);
        LBDRN_LAUNCH_CHECK();
    }
    return report_stamps(A, grid, c.s);
}

// The streaming kernel's plan for a requested mode and the mode of the instance that serves it there; false: the shape has no
// streaming instance.  Host arithmetic: run_wapply launches what this says, mfma_eval_reads_msb answers from it.
static bool resolve_wapply(const lbdrn_geom& g, const lbdrn_net& net, int mode, WApplyPlan* plan, int* serving)
{
    if (!make_wapply_plan(g, net, plan, mode_fast(mode))) return false;
    *serving = serving_mode(mode, plan->NT, false);
    return true;
}

static int run_wapply(const ApplyCall& c, int mode)
{
    WApplyArgs A;
    int serving = mode;
    if (!resolve_wapply(c.g, c.net, mode, &A.p, &serving)) {
        set_error("shape not supported by the MFMA apply kernels");
        return LBDRN_E_UNSUPPORTED;
    }
    if (int rc = workspace_holds(c, wapply_workspace(c.g, c.net))) return rc;
    float* packed = (float*)c.ws;
    double* partial = (double*)((char*)c.ws + align_up((size_t)A.p.pack_floats * 4, 256));
    k_pack_apply_wide<<<(A.p.pack_floats + 255) / 256, 256, 0, c.s>>>(c.params, c.net, A.p, 2 * c.g.P, packed);
    LBDRN_LAUNCH_CHECK();
    return run_pass(A, c, serving, packed, partial, dispatch_wapply);
}

// Which kernel serves a requested mode for this shape, and in which mode: k_apply_mfma on *plan in the mode returned (*wide_mode
// < 0), or the streaming kernel (apply_wide.inc), to be asked for *wide_mode.  Host arithmetic only: run_apply launches what this
// says, and mfma_eval_reads_msb answers lbdrn_eval_sse's NULL-msb check from it before anything is launched.
static int resolve_apply(const lbdrn_geom& g, const lbdrn_net& net, int mode, ApplyPlan* plan, int* wide_mode)
{
    if (mode == MODE_EVAL_X16) {   // (a hint: where the x16 weight pack does not fit in LDS -- C = 8, D = 3, bc = 64 --, or fits only at a
                                   //  shorter tile than the fast plan's -- C = 6, D = 3, bc = 64, two layers --, the pass is the fast one)
        ApplyPlan fp, xp;
        if (make_plan(g, net, &fp, true, false) && (!make_plan(g, net, &xp, true, true) || xp.TH < fp.TH)) mode = MODE_EVAL_FAST;
    }
    // The fast instances of k_apply_mfma carry the 4x4-block last layer only (C <= 8; with the 32x32x2 one beside it <2, 2, *> needs
    // 256 registers and spills three): with more bands than that NO fast plan is made for this kernel -- the pass is the canonical
    // one, which IS within the 1e-6 the flag promises (DESIGN.md 4.6 prices it), and where the canonical plan does not fit, the
    // streaming kernel's or none.  dispatch_apply refuses a fast launch with C > 8 should one ever be asked for.
    const int requested = mode;
    if (mode_fast(mode) && net.C > 8) mode = MODE_EVAL;
    *wide_mode = -1;
    if (!make_plan(g, net, plan, mode_fast(mode), mode == MODE_EVAL_X16)) {   // too wide for LDS-resident weights: the streaming kernel
        *wide_mode = requested;
        return requested;
    }
    return serving_mode(mode, plan->NT, plan->x16);   // (x16 is a hint: where the shape or the image does not qualify, the pass is the fast one)
}

// lbdrn_hip.h at LBDRN_EVAL_FAST: msb may be NULL exactly where this says false -- the serving instance is a fast one (the
// colour window comes from img >> K: `mode_fast(MODE) ? A.img ... >> g.K : A.msb ...` in both kernels' staging loops).
bool mfma_eval_reads_msb(const lbdrn_geom& g, const lbdrn_net& net, bool fast, bool x16)
{
    ApplyPlan plan;
    int wide_mode = -1;
    int mode = resolve_apply(g, net, fast ? (x16 ? MODE_EVAL_X16 : MODE_EVAL_FAST) : MODE_EVAL, &plan, &wide_mode);
    if (wide_mode >= 0) {
        WApplyPlan wp;
        if (!resolve_wapply(g, net, wide_mode, &wp, &mode)) return true;   // (no fused instance: the call is refused later)
    }
    return !mode_fast(mode);
}

// lbdrn_apply_instance (lbdrn_hip.h): what run_apply would launch for the request, read off the same two functions and launched
// nowhere.  request: 0 decode, 1 evaluation, 2 with LBDRN_EVAL_FAST, 3 with LBDRN_EVAL_X16 too (ApplyMode).  false: no fused instance.
bool mfma_apply_instance(const lbdrn_geom& g, const lbdrn_net& net, int request, int32_t out[8])
{
    ApplyPlan p;
    int wide_mode = -1;
    const int serving = resolve_apply(g, net, request, &p, &wide_mode);
    if (wide_mode < 0) {
        const int32_t v[8] = {1, p.NT, net.act == LBDRN_ACT_RELU, serving, p.TH, p.pair, p.x16, p.tiles_x * p.tiles_y};
        std::copy(v, v + 8, out);
        return true;
    }
    WApplyPlan w;
    int wserving = wide_mode;
    if (!resolve_wapply(g, net, wide_mode, &w, &wserving)) return false;
    const int32_t v[8] = {2, w.NT, net.nl, wserving, w.TH, w.skip, 0, w.tiles_x * w.tiles_y};
    std::copy(v, v + 8, out);
    return true;
}

static int run_apply(const ApplyCall& c, int mode)
{
    const lbdrn_geom& g = c.g;
    const lbdrn_net& net = c.net;
    ApplyArgs A;
    int wide_mode = -1;
    mode = resolve_apply(g, net, mode, &A.p, &wide_mode);
    if (wide_mode >= 0) return run_wapply(c, wide_mode);
    if (int rc = workspace_holds(c, mfma_apply_workspace(g, net))) return rc;
    float* packed = (float*)c.ws;
    const size_t pack_bytes = apply_pack_bytes(g, net);
    double* partial = (double*)((char*)c.ws + pack_bytes);
    float* amax = (float*)((char*)c.ws + pack_bytes + align_up(MFMA_PARTIALS * sizeof(double), 256));
    if (A.p.x16) {
        k_w0_absmax<<<1, 256, 0, c.s>>>(c.params, net.bc * net.F, amax);
        LBDRN_LAUNCH_CHECK();
    }
    k_pack_apply<<<(A.p.pack_floats + 255) / 256, 256, 0, c.s>>>(c.params, net, A.p, g.P, g.C, g.msb_max, amax, packed);
    LBDRN_LAUNCH_CHECK();
    return run_pass(A, c, mode, packed, partial, dispatch_apply);
}

int mfma_decode(const lbdrn_geom& g, const lbdrn_net& net, const uint16_t* msb, const float* params,
                uint16_t* out, float* y_out, void* ws, size_t ws_bytes, hipStream_t s)
{
    return run_apply({g, net, nullptr, msb, params, out, y_out, nullptr, -1, false, ws, ws_bytes, false, s}, MODE_DECODE);
}

int mfma_eval_sse(const lbdrn_geom& g, const lbdrn_net& net, const uint16_t* img,
                  const uint16_t* msb, const float* params, double* sse, void* ws, size_t ws_bytes,
                  bool background, bool fast, bool x16, int nodata, bool decoded, hipStream_t s)
{
    return run_apply({g, net, img, msb, params, nullptr, nullptr, sse, nodata, decoded, ws, ws_bytes, background, s},
                     fast ? (x16 ? MODE_EVAL_X16 : MODE_EVAL_FAST) : MODE_EVAL);
}

}  // namespace lbdrn
