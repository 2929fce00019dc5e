// Training step for wide networks (bc = 128 or 256: BASELINE.json configs[2], ref LBDRNmodel.py:62-77 at dim_hidden = 256),
// included into train_mfma.hip (one translation unit: it shares k_reduce_adam, the row matrix and the store helpers).
// No layer's weights fit near a CU at this width (W1 alone is 256 KB), and a per-workgroup gradient slab would be 494 KB
// (61 MB per step), so the step is three launches:
//   1. k_train_half: rows -> forward -> loss -> backward on 32-row workgroups, the units of every layer halved between
//      two waves, weights streamed L2 -> VGPR; what the gradient products need leaves row-major, [sample][unit], as
//      16-byte stores: the rows' features X, the activations H_l, dz_l of every layer and dz_out; cos(30 z_0) waits in LDS;
//   2. k_dw_wide: dW_l = dz_l^T H_{l-1} as a batch-dimension GEMM over the WHOLE minibatch -- 64 x 64 output blocks
//      (4 x 4 MFMA tiles in a wave's registers) x slices of 1024 samples, a quarter of the slice per wave = 232
//      workgroups / 928 equal wave-tasks on all 256 CUs, operands straight L2 -> VGPR through buffer loads with scalar
//      offsets, bias gradients from the A operands as they pass; the four waves' blocks meet in LDS (fixed order) and
//      leave as one partial slab per SLICE (8 x 477 KB), tile order;
//   3. k_reduce_adam over the 8 slices (fixed order: bitwise reproducible, no atomics).
// Training parity is a tolerance contract (1e-5 relative on the loss), as for the other fused steps.
// (Rounds 2-3 ran this width on one fused kernel per 64-row workgroup, k_train_wide; the history keeps it.)

struct WidePlan {
    FeatMap fm;   // the features the step multiplies (window centres skipped: train_mfma.hip)
    int LQ, NT0, RP, NT, bc, nl;
    int64_t NP;
    int64_t offW[3], offB[3];
    int pk_w0, pk_wh, pk_wl, pk_wht, pk_wlt, pack_floats;
    int sl_hid, sl_out, sl_bias, slab_floats;
    int w_dp, w_df;
    int lds_floats;
    int xo;       // row pitch of the features the step hands to k_dw_wide (16 NT0 rounded up to blocks of 64)
};

constexpr int DW_KS = 1024;    // samples per slice of the weight-gradient launch = per workgroup; a quarter per wave (a multiple of 64)
constexpr int HB = 32;       // rows per workgroup of k_train_half

static bool make_wide_plan(const lbdrn_geom& g, const lbdrn_net& net, WidePlan* out)
{
    if (net.act != LBDRN_ACT_SINE || (net.bc != 128 && net.bc != 256) || net.nl < 1 || net.nl > 2 || net.C > 16 || net.F < 1) return false;
    WidePlan p;
    p.bc = net.bc; p.NT = net.bc / 16; p.nl = net.nl;
    p.fm = centre_skipping_map(g, net);
    p.RP = (p.fm.Fe + net.C + 3) / 4 * 4;
    p.LQ = 0;
    for (int lq : {16, 32, 48, 52, 64})
        if (p.fm.Fe <= 4 * lq && p.RP <= wave_xp(lq)) { p.LQ = lq; break; }
    if (!p.LQ) return false;
    p.NT0 = (p.fm.Fe + 15) / 16;
    if (16 * p.NT0 > wave_xp(p.LQ)) return false;
    p.RP = wave_xp(p.LQ);   // matrix row pitch = LDS row pitch: the rows come in by LDS-DMA (see make_train_plan)
    p.NP = param_count(net);
    int64_t o = 0;
    for (int l = 0; l < net.nl; ++l) {
        const int nin = l ? net.bc : net.F;
        p.offW[l] = o; o += (int64_t)net.bc * nin;
        p.offB[l] = o; o += net.bc;
    }
    p.offW[net.nl] = o; o += (int64_t)net.C * net.bc;
    p.offB[net.nl] = o;
    int k = 0;
    p.pk_w0 = k; k += p.NT * p.LQ * 64;                   // [NT tiles][LQ/4 blocks][64 lanes][4]
    p.pk_wh = k; k += (net.nl - 1) * p.NT * p.NT * 256;   // [out tile][k tile] blocks
    p.pk_wl = k; k += p.NT * 256;
    p.pk_wht = k; k += (net.nl - 1) * p.NT * p.NT * 256;  // [in tile][out tile] blocks
    p.pk_wlt = k; k += p.NT * 256;
    p.pack_floats = k;
    int s = p.NT * p.NT0 * 256;
    p.sl_hid = s; s += (net.nl - 1) * p.NT * p.NT * 256;
    p.sl_out = s; s += p.NT * 256;
    p.sl_bias = s; s += net.nl * net.bc + 16;
    p.slab_floats = (s + 127) / 128 * 128;
    const int rp4 = p.RP / 4;
    p.w_dp = 64 / rp4;
    p.w_df = 64 % rp4;
    p.xo = (16 * p.NT0 + 63) / 64 * 64;   // k_dw_wide reads the features in blocks of 64
    {   // k_train_half: rows / exchange buffer (aliased), cos(30 z_0), output partials, loss partials
        const int ep = net.bc + 4, r0 = std::max(HB * wave_xp(p.LQ), HB * ep);
        p.lds_floats = r0 + (net.nl > 1 ? HB * ep : 0) + 2 * HB * 20 + 4;
    }
    if ((size_t)p.lds_floats * 4 > 160 * 1024) return false;
    if (p.xo > 256) return false;   // k_train_half copies a row of X as one 16-byte piece per lane
    *out = p;
    return true;
}

static int wide_plan_features(const WidePlan& p) { return p.fm.Fe; }

struct WideWsLayout { size_t off_rows, off_pack, off_slab, off_loss, off_map, off_x, off_h[2], off_dz[2], off_dzo, total; };

static WideWsLayout wide_ws_layout(const lbdrn_geom& g, const lbdrn_net& net, const WidePlan& p, int bs)
{
    WideWsLayout L;
    size_t o = 0;
    const size_t rpw = HB;
    const size_t nwg = ((size_t)bs + rpw - 1) / rpw;
    L.off_rows = o; o += align_up((size_t)g.H * g.W * p.RP * sizeof(float), 256);
    L.off_pack = o; o += align_up((size_t)p.pack_floats * sizeof(float), 256);
    const size_t nrows = (nwg * rpw + 63) / 64 * 64, nslabs = (nrows + DW_KS - 1) / DW_KS;   // (k_dw_wide walks blocks of 64 rows)
    L.off_slab = o; o += align_up(nslabs * (size_t)p.slab_floats * sizeof(float), 256);
    L.off_loss = o; o += align_up(nwg * sizeof(double), 256);
    L.off_map = o; o += align_up((size_t)p.slab_floats * 4 * sizeof(int), 256);
    // what k_dw_wide multiplies, row-major [sample][..]
    L.off_x = o; o += align_up(nrows * (size_t)p.xo * sizeof(float), 256);
    L.off_h[1] = L.off_dz[1] = o;
    for (int l = 0; l < net.nl; ++l) {
        L.off_h[l] = o; o += align_up(nrows * (size_t)p.bc * sizeof(float), 256);
        L.off_dz[l] = o; o += align_up(nrows * (size_t)p.bc * sizeof(float), 256);
    }
    L.off_dzo = o; o += align_up(nrows * (size_t)WOP * sizeof(float), 256);
    L.total = o;
    return L;
}

// canonical parameter index -> positions in the fragment-order buffer: .x forward copy, .y transposed copy
__device__ __forceinline__ int2 wide_frag_pos(int64_t idx, const WidePlan& p, int F, int C)
{
    const int NT = p.NT, bc = p.bc, nl = p.nl;
    if (idx < p.offB[0]) {  // W0[n][k]: quarter q walks k = q*LQ .. q*LQ+LQ-1
        const int n = (int)(idx / F), k = slot_of_feat((int)(idx - (int64_t)n * F), p.fm);
        if (k < 0) return make_int2(-1, -1);   // a column the step skips
        const int q = k / p.LQ, s = k - q * p.LQ;
        return make_int2(p.pk_w0 + ((((n >> 4) * (p.LQ >> 2) + (s >> 2)) * 64 + q * 16 + (n & 15)) * 4 + (s & 3)), -1);
    }
    for (int l = 1; l < nl; ++l)
        if (idx >= p.offW[l] && idx < p.offB[l]) {  // W_l[n][k]: step (k tile, r) multiplies k = 16 tk + 4 q + r
            const int e = (int)(idx - p.offW[l]);
            const int n = e / bc, k = e - n * bc;
            const int fwd = p.pk_wh + (((((l - 1) * NT + (n >> 4)) * NT + (k >> 4)) * 64 + ((k >> 2) & 3) * 16 + (n & 15)) * 4 + (k & 3));
            const int bwd = p.pk_wht + (((((l - 1) * NT + (k >> 4)) * NT + (n >> 4)) * 64 + ((n >> 2) & 3) * 16 + (k & 15)) * 4 + (n & 3));
            return make_int2(fwd, bwd);
        }
    if (idx >= p.offW[nl] && idx < p.offB[nl]) {  // W_last[c][k]
        const int e = (int)(idx - p.offW[nl]);
        const int c = e / bc, k = e - c * bc;
        return make_int2(p.pk_wl + (((k >> 4) * 64 + ((k >> 2) & 3) * 16 + c) * 4 + (k & 3)),
                         p.pk_wlt + (((k >> 4) * 64 + (c >> 2) * 16 + (k & 15)) * 4 + (c & 3)));
    }
    return make_int2(-1, -1);
}

// slab element (tile order) -> canonical parameter index (or -1: padding)
__device__ __forceinline__ int64_t wide_slab_to_param(int e, const WidePlan& p, int F, int C)
{
    const int NT = p.NT, bc = p.bc, nl = p.nl;
    if (e >= p.sl_bias) {
        const int b = e - p.sl_bias;
        if (b < nl * bc) return p.offB[b / bc] + (b % bc);
        const int ch = b - nl * bc;
        return ch < C ? p.offB[nl] + ch : -1;
    }
    const int tile = e >> 8, lane = (e >> 2) & 63, r = e & 3;
    const int row = 4 * (lane >> 4) + r, col = lane & 15;
    if (e < p.sl_hid) {   // dW0 tile (unit tile t, input strip nt)
        const int t = tile / p.NT0, nt = tile - t * p.NT0;
        const int k = 16 * nt + col;
        return k < p.fm.Fe ? p.offW[0] + (int64_t)(16 * t + row) * F + feat_of_slot(k, p.fm) : -1;
    }
    if (e < p.sl_out) {   // dW_1 tile (unit tile t, input tile nt)
        const int t2 = tile - NT * p.NT0;
        const int t = t2 / NT, nt = t2 - t * NT;
        return p.offW[1] + (int64_t)(16 * t + row) * bc + 16 * nt + col;
    }
    const int wt = tile - (p.sl_out >> 8);   // output layer: rows = channel slots, hidden column tile wt
    return row < C ? p.offW[nl] + (int64_t)row * bc + 16 * wt + col : -1;
}

__global__ void __launch_bounds__(256)
    k_pack_wide(const float* __restrict__ params, WidePlan p, int F, int C, float* __restrict__ packed)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= p.NP) return;
    const int2 pos = wide_frag_pos(idx, p, F, C);
    if (pos.x >= 0) packed[pos.x] = params[idx];
    if (pos.y >= 0) packed[pos.y] = params[idx];
}

__global__ void __launch_bounds__(256) k_build_map_wide(WidePlan p, int F, int C, int4* __restrict__ map)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.slab_floats) return;
    const int64_t idx = e < p.sl_bias + p.nl * p.bc + 16 ? wide_slab_to_param(e, p, F, C) : -1;
    const int2 pos = idx >= 0 ? wide_frag_pos(idx, p, F, C) : make_int2(-1, -1);
    map[e] = make_int4((int)idx, pos.x, pos.y, 0);
}

struct WideArgs {
    lbdrn_net net;
    WidePlan p;
    const float* rows;
    int64_t npix;
    const int64_t* perm;
    int batch_n;
    const float* params;
    const float* packed;
    float* slabs;
    double* loss_part;
    float inv;
    float *oX, *oH[2], *oDZ[2], *oDZO;   // the operands of k_dw_wide, [rows][xo / bc / bc / 16]
    unsigned long long* stamps;  // diagnostic build only (-DLBDRN_TRAIN_STAMPS): [nwg][4][16] s_memtime
};

// ---- the forward / backward launch, units halved between two waves ------------------------------------------------------
// A workgroup is 32 samples = two sample tiles x two UNIT HALVES: wave (s, u) computes units 8u .. 8u + 7 (tiles of 16) of
// every layer for the 16 samples of tile s.  What a product needs from the other half of the units crosses LDS -- h_0
// before the hidden layer, dz_1 before its backward product, [sample][unit] rows read back as the 16-byte pieces that ARE
// the B operand of step (k tile, r) --, the output layer's two partial sums meet in LDS and are finished by both waves.
// Per wave 1,472 MFMAs and half the activations; 256 workgroups per 8192-row minibatch (every CU for a lone fit); 72 KB of
// LDS and <= 256 registers: two workgroups fit on a CU, so with two fits in flight one workgroup's activation / prologue
// phases run under the other's MFMAs.  (A wave on 16 samples x ALL units -- round 3's shape -- is 2,944 MFMAs behind
// 35 k cycles of phases without a single MFMA, one wave per SIMD at 412 registers, and holds half of the chip for 62 us.)
constexpr int HALF_NP = 2;  // unit tiles per pass of a product (A/B: 8 = one pass, everything behind a product exposed)

// sched_group_barrier recipe of one iteration of a k_train_half product: M MFMAs; ND LDS reads (the next iteration's B
// operand / a row of X) and NV fragment requests (for a later iteration) go out one behind each of the first MFMAs; with
// PIECES the rest of the MFMAs each take a few vector instructions of the previous pass's activation along
template <int M, int NV, int ND, bool PIECES>
__device__ __forceinline__ void half_deal()
{
    constexpr int nd = ND < M ? ND : M, nv = NV < M - nd ? NV : M - nd, left = M - nd - nv;
#pragma unroll
    for (int k = 0; k < nd; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
    }
#pragma unroll
    for (int k = 0; k < nv; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
    }
    if constexpr (PIECES) {
#pragma unroll
        for (int k = 0; k < left; ++k) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);   // VALU
        }
    } else if constexpr (left > 0) {
        __builtin_amdgcn_sched_group_barrier(0x008, left, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
}

template <int LQ, int NL, int NT>
__global__ void __launch_bounds__(WAVE_THREADS, 2) k_train_half(WideArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const WidePlan& p = A.p;
    constexpr int XP = wave_xp(LQ), OP = WOP, G0 = LQ / 4, BC = 16 * NT, NH = NT / 2, EP = BC + 4, PP = 20;
    constexpr int R0 = HB * XP > HB * EP ? HB * XP : HB * EP;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int st = wv >> 1, uh = wv & 1;       // sample tile, unit half
    const int i = lane & 15, q = lane >> 4;
    const int C = A.net.C, F = p.fm.Fe;
    float* Xs = lds;                           // [32][XP] features | labels; dead after the first barriers:
    float* E = lds;                            // [32][EP] h_0, later dz_1, of all units (the exchange between unit halves)
    float* CS = lds + R0;                      // [32][EP] cos(30 z_0) (NL > 1)
    float* P = CS + (NL > 1 ? HB * EP : 0);    // [2 halves][32][PP] partial pre-activations of the output layer
    float* red = P + 2 * HB * PP;              // [2] loss partials of the two sample tiles
    const int wg = blockIdx.x, first = wg * HB;
    const int nvalid = min(HB, A.batch_n - first);
    const int srow = 16 * st + i;
    const size_t orow = (size_t)first + srow;
    const int t0 = NH * uh;                    // this wave's first unit tile
#ifdef LBDRN_TRAIN_STAMPS
    unsigned long long stamp[16] = {};
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp[14])::"memory");
#endif
    STAMP(0);

    auto clamp_pix = [&](int64_t pix) -> int { return (int)(pix < 0 ? 0 : (pix >= A.npix ? A.npix - 1 : pix)); };
    const int64_t raw_mine = A.perm[min(first + 16 * st + i, A.batch_n - 1)];
    f32x4 bias_last;
#pragma unroll
    for (int r = 0; r < 4; ++r) bias_last[r] = (4 * q + r) < C ? A.params[p.offB[NL] + 4 * q + r] : 0.0f;
    auto ldbias = [&](int l, int t) -> f32x4 {
        const float4 b4 = *reinterpret_cast<const float4*>(A.params + p.offB[l] + 16 * t + 4 * q);
        f32x4 b = {b4.x, b4.y, b4.z, b4.w};
        return b;
    };
    f32x4 acc[NH];
#pragma unroll
    for (int t = 0; t < NH; ++t) acc[t] = ldbias(0, t0 + t);

    // ---- rows of this pair's 16 samples by LDS-DMA (matrix row pitch = LDS row pitch), the requests dealt between the
    //      two waves of the pair
    constexpr int NLD = (16 * (XP / 4) + 63) / 64;
    const int rp4 = p.RP >> 2, nchunk = 16 * rp4;
    const int pix_mine = clamp_pix(raw_mine);
    {
        float* dst = Xs + 16 * st * XP;
        const int row0 = lane / rp4, col0 = lane - row0 * rp4;
        int row = row0, col = col0;
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const float* src = A.rows + (size_t)__shfl(pix_mine, min(row, 15)) * p.RP + 4 * col;
            if ((k & 1) == uh && lane + 64 * k < nchunk)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(dst + k * 256), 16, 0, 0);
            row += p.w_dp; col += p.w_df;
            if (col >= rp4) { col -= rp4; row += 1; }
        }
    }
    // ---- the weight stream: 1 KB blocks (64 lanes x 16 B) by buffer loads with scalar block offsets
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A.packed), (short)0,
                                                                         p.pack_floats * 4, 0x00020000);
    const int lane16 = lane * 16;
    auto ldw = [&](int float_base, int block) -> float4 {
        const v4i32 x = __builtin_amdgcn_raw_buffer_load_b128(wrs, lane16, float_base * 4 + block * 1024, 0);
        return make_float4(__int_as_float(x[0]), __int_as_float(x[1]), __int_as_float(x[2]), __int_as_float(x[3]));
    };
    // Every product of this wave runs in NPASS passes of NP unit tiles (round 4, second half): what follows a product --
    // sin / cos of its accumulators, the stores -- is vector work whose LATENCIES (transcendental results, LDS stores,
    // address arithmetic waiting on each other) can only hide under MFMAs of the same wave: one wave per SIMD for a lone
    // fit, and f32 MFMAs and vector instructions do not execute together anyway (DESIGN 4.2: issue cycles add).  With all
    // NH tiles finishing together all of it stood in the open (stamps: 3.4 k + 3.1 k + 1.6 k cycles of a 70 k-cycle wave);
    // now the tiles of pass p are activated under the
    // MFMAs of pass p + 1, one sin/cos pair per iteration, and only the last pass's are left over.  A pass re-reads the B
    // operand (registers / 16 LDS reads) and fetches its own NP fragment blocks per iteration: the same bytes as before,
    // in a ring of RING iterations (the request of iteration it + DIST goes out in iteration it: ~1.5 k cycles ahead).
    constexpr int NP = NH % HALF_NP == 0 ? HALF_NP : NH, NPASS = NH / NP;
    constexpr int DIST = NP >= 8 ? 2 : NP >= 4 ? 4 : 6, RING = DIST + 1;   // (NP = 2: 6 against 8 / 12 iterations ahead: 332.4 / 334.1 / 336.7 ms per tile)
    constexpr int IT0 = NPASS * G0, IT1 = NPASS * NT;
    static_assert(DIST * NP < 48, "requests in flight behind the rows: vmcnt is a 6-bit counter");
    float4 wq[RING][NP];
    auto sel4 = [](const float4& x, int e) -> float { return e == 0 ? x.x : e == 1 ? x.y : e == 2 ? x.z : x.w; };
    // block (tile t0 + .., step ..) of a product = a per-product scalar base (this wave's first tile; opaque, so that the
    // compiler neither merges the offsets of different products nor keeps 128 of them alive in SGPRs) + a constant
    auto ldwc = [&](int sbase, int block) -> float4 {
        const v4i32 x = __builtin_amdgcn_raw_buffer_load_b128(wrs, lane16, sbase + block * 1024, 0);
        return make_float4(__int_as_float(x[0]), __int_as_float(x[1]), __int_as_float(x[2]), __int_as_float(x[3]));
    };
    auto opaque_base = [&](int float_base, int stride) -> int {
        int b = __builtin_amdgcn_readfirstlane(float_base * 4 + t0 * stride * 1024);
        asm volatile("" : "+s"(b));
        return b;
    };
    auto blk0 = [](int it, int t) -> int { return ((it / G0) * NP + t) * G0 + (it % G0); };
    auto blk1 = [](int it, int t) -> int { return ((it / NT) * NP + t) * NT + (it % NT); };   // W_1 [out][k] and W_1^T [in][out] alike
    const int sb0 = opaque_base(p.pk_w0, G0);
    constexpr int PRE0 = DIST < IT0 ? DIST : IT0, PRE1 = DIST < IT1 ? DIST : IT1;
    stream_for<PRE0>([&](auto j_) {
        constexpr int j = decltype(j_)::value;
#pragma unroll
        for (int t = 0; t < NP; ++t) wq[j % RING][t] = ldwc(sb0, blk0(j, t));
    });
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PRE0 * NP) : "memory");   // the rows (the fragment blocks may stay in flight)
    __syncthreads();   // both waves' requests of the pair have landed
    float bx[LQ];   // the B operand of layer 0: features q*LQ .. q*LQ+LQ-1 of sample srow
#pragma unroll
    for (int g = 0; g < G0; ++g) {
        const float4 x = *reinterpret_cast<const float4*>(Xs + srow * XP + q * LQ + 4 * g);
        bx[4 * g] = x.x; bx[4 * g + 1] = x.y; bx[4 * g + 2] = x.z; bx[4 * g + 3] = x.w;
    }
    float4 lab4;   // labels of channels 4 q .. 4 q + 3 (one float at a time: F need not be a multiple of four)
    {
        const float* lr = Xs + srow * XP + F + 4 * q;
        lab4 = make_float4(lr[0], lr[1], lr[2], lr[3]);
    }
    __builtin_amdgcn_sched_barrier(0);
    STAMP(1);
    // the features of the pair's 16 rows leave row-major for the first layer's gradient product: a row per iteration of
    // the first pass (this wave: rows 2 j + uh; one LDS read, stored an iteration later), under its MFMAs -- it used to
    // be a loop of its own in front of layer 0
    constexpr int NXC = 8;
    float* xdst = A.oX + ((size_t)first + 16 * st) * p.xo;
    const int xq = p.xo >> 2;
    float4 xr[2];
    auto xrow_read = [&](int j) {
        xr[j & 1] = 4 * lane < XP ? *reinterpret_cast<const float4*>(Xs + (16 * st + 2 * j + uh) * XP + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto xrow_store = [&](int j) {
        if (lane < xq) *reinterpret_cast<float4*>(xdst + (size_t)(2 * j + uh) * p.xo + 4 * lane) = xr[j & 1];
    };

    float h[NH][4];       // this wave's activations of the current layer, accumulator layout
    f32x4 csl[NH];        // cos(30 z) of the LAST hidden layer
    // sin / cos of one accumulator register; a tile's activations leave row-major for k_dw_wide, h_0 also into the exchange buffer
    auto act_piece = [&](int t, int r) {
        float sn, co;
        train_sincos(30.0f * acc[t][r], sn, co);
        h[t][r] = sn;
        csl[t][r] = co;
    };
    auto act_store = [&](int l, int t) {
        const float4 h4 = make_float4(h[t][0], h[t][1], h[t][2], h[t][3]);
        *reinterpret_cast<float4*>(A.oH[l] + orow * BC + 16 * (t0 + t) + 4 * q) = h4;
        if (NL > 1 && l == 0) {
            *reinterpret_cast<float4*>(E + srow * EP + 16 * (t0 + t) + 4 * q) = h4;
            *reinterpret_cast<float4*>(CS + srow * EP + 16 * (t0 + t) + 4 * q) = make_float4(csl[t][0], csl[t][1], csl[t][2], csl[t][3]);
        }
    };
    // the pieces (tile, register) of the NP tiles of pass ps that iteration k of NIT of the next pass carries
    auto act_under = [&](int l, int ps, int k, int nit) {
#pragma unroll
        for (int e = 0; e < 4 * NP; ++e)
            if (e * nit / (4 * NP) == k) {
                act_piece(ps * NP + (e >> 2), e & 3);
                if ((e & 3) == 3) act_store(l, ps * NP + (e >> 2));
            }
    };
    auto act_rest = [&](int l) {   // the last pass's tiles: nothing left to hide them under
#pragma unroll
        for (int t = (NPASS - 1) * NP; t < NH; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) act_piece(t, r);
            act_store(l, t);
        }
    };

    // ---- layer 0, this wave's unit tiles: iteration (pass, group g) = 4 steps x NP tiles
    stream_for<IT0>([&](auto it_) {
        constexpr int it = decltype(it_)::value, ps = it / G0, g = it % G0;
        if constexpr (it + DIST < IT0) {
#pragma unroll
            for (int t = 0; t < NP; ++t) wq[(it + DIST) % RING][t] = ldwc(sb0, blk0(it + DIST, t));
        }
        if constexpr (ps == 0) {
            if constexpr (g < NXC) xrow_read(g);
            if constexpr (g >= 1 && g <= NXC) xrow_store(g - 1);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int t = 0; t < NP; ++t) acc[ps * NP + t] = MFMA16(sel4(wq[it % RING][t], e), bx[4 * g + e], acc[ps * NP + t]);
        if constexpr (ps > 0) act_under(0, ps - 1, g, G0);
        half_deal<4 * NP, (it + DIST < IT0 ? NP : 0), (ps == 0 && g < NXC ? 1 : 0), (ps > 0)>();
        if constexpr (ps == 0 && g == G0 - 1) {
            // (short rows: what the first pass's iterations did not reach)
            stream_for<(G0 <= NXC ? NXC + 1 - G0 : 0)>([&](auto j_) {
                constexpr int j = G0 + decltype(j_)::value;
                if constexpr (j < NXC) xrow_read(j);
                xrow_store(j - 1);
            });
            __syncthreads();   // every wave has what it needs from the rows: the space becomes the exchange buffer
        }
    });

    STAMP(2);
    f32x4 b1[NL > 1 ? NH : 1];
    int sbh = 0, sbt = 0;
    if (NL > 1) {   // the hidden layer's bias and first fragment groups: in flight under the activation's arithmetic
#pragma unroll
        for (int t = 0; t < NH; ++t) b1[t] = ldbias(1, t0 + t);
        sbh = opaque_base(p.pk_wh, NT);
        stream_for<PRE1>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
#pragma unroll
            for (int t = 0; t < NP; ++t) wq[j % RING][t] = ldwc(sbh, blk1(j, t));
        });
        __builtin_amdgcn_sched_barrier(0);
    }
    act_rest(0);
    STAMP(3);

    if (NL > 1) {
        __syncthreads();   // h_0 of all units of this pair's samples is in the exchange buffer
        STAMP(4);
        // ---- hidden layer: step (tk, r) multiplies unit 16 tk + 4 q + r of sample i = the 16-byte piece at E[srow][16 tk + 4 q]
#pragma unroll
        for (int t = 0; t < NH; ++t) acc[t] = b1[t];
        float4 hk[2];
        hk[0] = *reinterpret_cast<const float4*>(E + srow * EP + 4 * q);
        stream_for<IT1>([&](auto it_) {
            constexpr int it = decltype(it_)::value, ps = it / NT, tk = it % NT;
            if constexpr (it + DIST < IT1) {
#pragma unroll
                for (int t = 0; t < NP; ++t) wq[(it + DIST) % RING][t] = ldwc(sbh, blk1(it + DIST, t));
            }
            if constexpr (it + 1 < IT1) hk[(it + 1) & 1] = *reinterpret_cast<const float4*>(E + srow * EP + 16 * ((it + 1) % NT) + 4 * q);
            const float4 hb = hk[it & 1];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int to = 0; to < NP; ++to)
                    acc[ps * NP + to] = MFMA16(sel4(wq[it % RING][to], r), sel4(hb, r), acc[ps * NP + to]);
            if constexpr (ps > 0) act_under(1, ps - 1, tk, NT);
            half_deal<4 * NP, (it + DIST < IT1 ? NP : 0), (it + 1 < IT1 ? 1 : 0), (ps > 0)>();
        });
    }
    STAMP(5);
    // the output layer's fragments (this wave's k tiles) and W_last^T, requested before the last activation's arithmetic
    float4 wl[NH], wlt[NH];
#pragma unroll
    for (int t = 0; t < NH; ++t) wl[t] = ldw(p.pk_wl, t0 + t);
#pragma unroll
    for (int t = 0; t < NH; ++t) wlt[t] = ldw(p.pk_wlt, t0 + t);
    __builtin_amdgcn_sched_barrier(0);
    if (NL > 1) act_rest(1);
    STAMP(6);

    // ---- output layer: this half's partial sums -> LDS; both waves of the pair finish (bias + half 0) + half 1
    {
        f32x4 oe = {0.f, 0.f, 0.f, 0.f}, oo = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NH; ++t) {
            const float4 x = wl[t];
            oe = MFMA16(x.x, h[t][0], oe);
            oo = MFMA16(x.y, h[t][1], oo);
            oe = MFMA16(x.z, h[t][2], oe);
            oo = MFMA16(x.w, h[t][3], oo);
        }
        *reinterpret_cast<float4*>(P + (uh * HB + srow) * PP + 4 * q) = make_float4(oe[0] + oo[0], oe[1] + oo[1], oe[2] + oo[2], oe[3] + oo[3]);
    }
    if (NL > 1) {   // the first fragment groups of W_1^T for the product after next
        sbt = opaque_base(p.pk_wht, NT);
        stream_for<PRE1>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
#pragma unroll
            for (int t = 0; t < NP; ++t) wq[j % RING][t] = ldwc(sbt, blk1(j, t));
        });
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();   // both halves' partial sums are in LDS (and every wave is through the hidden layer: E is free)
    float dzo[4];
    {
        const float4 p0 = *reinterpret_cast<const float4*>(P + srow * PP + 4 * q);
        const float4 p1 = *reinterpret_cast<const float4*>(P + (HB + srow) * PP + 4 * q);
        const float z4[4] = {(bias_last[0] + p0.x) + p1.x, (bias_last[1] + p0.y) + p1.y, (bias_last[2] + p0.z) + p1.z, (bias_last[3] + p0.w) + p1.w};
        const float labv[4] = {lab4.x, lab4.y, lab4.z, lab4.w};
        const bool live = srow < nvalid;
        float lsum = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool ok = live && (4 * q + r) < C;
            const float y = train_sigmoid(z4[r]);
            const float d = y - ((4 * q + r) < C ? labv[r] : 0.0f);
            lsum += ok ? d * d : 0.0f;                                      // ref LBDRNloss.py:9
            dzo[r] = ok ? ((2.0f * d) * A.inv) * (y * (1.0f - y)) : 0.0f;    // mse + sigmoid backward
        }
        if (uh == 0) {   // (both waves of a pair hold the same numbers)
            *reinterpret_cast<float4*>(A.oDZO + orow * OP + 4 * q) = make_float4(dzo[0], dzo[1], dzo[2], dzo[3]);
            lsum = wave_sum(lsum);
            if (lane == 0) red[st] = lsum;
        }
    }
    STAMP(7);
    // ---- backward through the output layer: dz of this half's units of the last hidden layer
    float dzu[NH][4];
    {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NH; ++t) acc[t] = zero;
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int t = 0; t < NH; ++t) {
                const float4 x = wlt[t];
                acc[t] = MFMA16(s4 == 0 ? x.x : s4 == 1 ? x.y : s4 == 2 ? x.z : x.w, dzo[s4], acc[t]);
            }
        float* zrow = A.oDZ[NL - 1] + orow * BC;
#pragma unroll
        for (int t = 0; t < NH; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dzu[t][r] = (acc[t][r] * csl[t][r]) * 30.0f;
            const float4 z4 = make_float4(dzu[t][0], dzu[t][1], dzu[t][2], dzu[t][3]);
            *reinterpret_cast<float4*>(zrow + 16 * (t0 + t) + 4 * q) = z4;
            if (NL > 1) *reinterpret_cast<float4*>(E + srow * EP + 16 * (t0 + t) + 4 * q) = z4;
        }
    }
    STAMP(8);
    if (NL > 1) {
        __syncthreads();   // dz_1 of all units of this pair's samples is in the exchange buffer
        STAMP(9);
        // ---- dh_0 = W_1^T dz_1 for this half's input units: step (to, r) multiplies dz_1 of unit 16 to + 4 q + r; in passes
        //      like the forward products: dz_0 of a pass's tiles (x cos(30 z_0) out of LDS, x 30, a 16-byte store) leaves
        //      under the next pass's MFMAs
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NH; ++t) acc[t] = zero;
        float* zrow = A.oDZ[0] + orow * BC;
        auto dz0_tile = [&](int t) {
            const float4 cc = *reinterpret_cast<const float4*>(CS + srow * EP + 16 * (t0 + t) + 4 * q);
            *reinterpret_cast<float4*>(zrow + 16 * (t0 + t) + 4 * q) =
                make_float4((acc[t][0] * cc.x) * 30.0f, (acc[t][1] * cc.y) * 30.0f, (acc[t][2] * cc.z) * 30.0f, (acc[t][3] * cc.w) * 30.0f);
        };
        float4 zk[2];
        zk[0] = *reinterpret_cast<const float4*>(E + srow * EP + 4 * q);
        stream_for<IT1>([&](auto it_) {
            constexpr int it = decltype(it_)::value, ps = it / NT, to = it % NT;
            if constexpr (it + DIST < IT1) {
#pragma unroll
                for (int t = 0; t < NP; ++t) wq[(it + DIST) % RING][t] = ldwc(sbt, blk1(it + DIST, t));
            }
            if constexpr (it + 1 < IT1) zk[(it + 1) & 1] = *reinterpret_cast<const float4*>(E + srow * EP + 16 * ((it + 1) % NT) + 4 * q);
            const float4 zb = zk[it & 1];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int ti = 0; ti < NP; ++ti)
                    acc[ps * NP + ti] = MFMA16(sel4(wq[it % RING][ti], r), sel4(zb, r), acc[ps * NP + ti]);
            if constexpr (ps > 0) {
#pragma unroll
                for (int e = 0; e < NP; ++e)
                    if (e * NT / NP == to) dz0_tile((ps - 1) * NP + e);
            }
            half_deal<4 * NP, (it + DIST < IT1 ? NP : 0), (it + 1 < IT1 ? 1 : 0), (ps > 0)>();
        });
#pragma unroll
        for (int t = (NPASS - 1) * NP; t < NH; ++t) dz0_tile(t);
    }
    STAMP(10);
    __syncthreads();
    if (tid == 0) A.loss_part[wg] = (double)red[0] + (double)red[1];
#ifdef LBDRN_TRAIN_STAMPS
    STAMP(11); STAMP(12); STAMP(13);
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp[15])::"memory");
    if (lane == 0 && A.stamps)
        for (int e = 0; e < 16; ++e) A.stamps[((size_t)wg * 4 + wv) * 16 + e] = stamp[e];
#endif
    // k_dw_wide walks the rows in blocks of 64: an odd number of workgroups leaves half a block, which the last workgroup
    // fills with zeros (dz = 0 there, and whatever a zero multiplies must be finite: the scratch is not initialised)
    if (wg == (int)gridDim.x - 1 && (gridDim.x & 1)) {
        const size_t r0 = (size_t)first + HB;
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int e = tid; e < HB * (p.xo >> 2); e += WAVE_THREADS) reinterpret_cast<float4*>(A.oX + r0 * p.xo)[e] = z4;
        for (int l = 0; l < NL; ++l)
            for (int e = tid; e < HB * (BC >> 2); e += WAVE_THREADS) {
                reinterpret_cast<float4*>(A.oH[l] + r0 * BC)[e] = z4;
                reinterpret_cast<float4*>(A.oDZ[l] + r0 * BC)[e] = z4;
            }
        for (int e = tid; e < HB * (OP >> 2); e += WAVE_THREADS) reinterpret_cast<float4*>(A.oDZO + r0 * OP)[e] = z4;
    }
}

// ---- the weight gradients of the split form: dW_l = dz_l^T H_{l-1} over the whole minibatch (see the head of the file)
struct DwArgs {
    WidePlan p;
    int nrows;        // rows the step wrote, a multiple of 64 (rows past the minibatch carry dz = 0)
    int nslices;      // ceil(nrows / DW_KS): one partial slab each
    const float* X;   // [nrows][p.xo]
    const float* H[2];    // [nrows][bc]
    const float* DZ[2];   // [nrows][bc]
    const float* DZO;     // [nrows][16]
    float* slabs;     // [nslices][p.slab_floats], tile order
};

// One workgroup-task of k_dw_wide: a block of 64 units (AV: a block of dz_l; !AV: the 16 channel slots of dz_out) x NBK
// blocks of 64 inputs, summed over a slice of DW_KS samples, a quarter of the slice in each of the four waves.
//
// Operands come straight L2 -> VGPR out of the row-major [sample][unit] arrays as 16-BYTE loads: in MFMA step j lane
// (i, q) reads units 4 i .. 4 i + 3 of sample 4 j + q -- a wave-load is four whole 256-byte row pieces (the first version
// read one float per lane: four 64-byte pieces of four cache lines per wave-load, and the launch spent as long loading as
// multiplying).  A 16 x 16 MFMA tile is then made of every FOURTH unit: "tile" e of a block = units {4 i + e}, which is
// legal because rows and columns of an outer-product sum can be taken in any order as long as the result is put back
// where it belongs -- and it is, on the way through LDS: every wave scatters its accumulators to the slab's tile order
// (16-byte pieces), the four waves' partial blocks are summed there in wave order ((0 + 1) + 2) + 3, wave w finishing
// every fourth tile.  ONE partial slab per slice of 1024 samples (8 x 477 KB per step at bs = 8192).
// Buffers: NB register buffers of SB steps, a later buffer's loads dealt out between this buffer's MFMAs.
constexpr int DW_TS = 260;   // floats per tile in LDS (256 + 4: the scatter of a wave meets 4 banks per tile, tiles 4 banks apart)

__device__ __forceinline__ float4 dw_ld4(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    const v4i32 x = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    return make_float4(__int_as_float(x[0]), __int_as_float(x[1]), __int_as_float(x[2]), __int_as_float(x[3]));
}
__device__ __forceinline__ float dw_ld1(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    return __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ float f4e(const float4& x, int e) { return e == 0 ? x.x : e == 1 ? x.y : e == 2 ? x.z : x.w; }

// out_off(ut, vt): float offset in the slab of the 16 x 16 tile (unit tile ut of the block, input tile vt of the NBK blocks),
// or -1 where the layer has no such tile; bias_out: where the block's 64 (16) column sums of A go, or null
template <bool AV, int NBK, int SB, int NB, class OutOff>
__device__ __forceinline__ void dw_task(const float* Aarr, int pitchA, int a_col0, const float* Barr, int pitchB, int b_col0,
                                        int nrows, int k0, int nsteps, float* slab, OutOff out_off, float* bias_out, int lane,
                                        int w, float* lds)
{
    constexpr int MU = AV ? 4 : 1, MI = 4 * NBK, NTILE = MU * MI;
    const int i = lane & 15, q = lane >> 4;
    const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Aarr), (short)0, nrows * pitchA * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Barr), (short)0, nrows * pitchB * 4, 0x00020000);
    const int vA = (q * pitchA + (AV ? 4 * i : i)) * 4, vB = (q * pitchB + 4 * i) * 4;
    const int sA0 = __builtin_amdgcn_readfirstlane((k0 * pitchA + a_col0) * 4);
    const int sB0 = __builtin_amdgcn_readfirstlane((k0 * pitchB + b_col0) * 4);
    const int dA = 4 * pitchA * 4, dB = 4 * pitchB * 4;   // bytes per step (four samples)
    f32x4 acc[MU][MI];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < MU; ++u)
#pragma unroll
        for (int v = 0; v < MI; ++v) acc[u][v] = zero;
    float bsum[MU];
#pragma unroll
    for (int u = 0; u < MU; ++u) bsum[u] = 0.0f;
    float4 a[NB][SB], b[NB][SB][NBK];   // (!AV: only .x of a)
    auto ld = [&](float4 (&aa)[SB], float4 (&bb)[SB][NBK], int it) {
        const int oa = sA0 + it * SB * dA, ob = sB0 + it * SB * dB;
#pragma unroll
        for (int s = 0; s < SB; ++s) {
            if constexpr (AV) aa[s] = dw_ld4(rA, vA, oa + s * dA);
            else aa[s].x = dw_ld1(rA, vA, oa + s * dA);
#pragma unroll
            for (int k = 0; k < NBK; ++k) bb[s][k] = dw_ld4(rB, vB, ob + s * dB + 256 * k);
        }
    };
    auto mm = [&](const float4 (&aa)[SB], const float4 (&bb)[SB][NBK]) {
#pragma unroll
        for (int s = 0; s < SB; ++s) {
#pragma unroll
            for (int u = 0; u < MU; ++u) {
                const float av = AV ? f4e(aa[s], u) : aa[s].x;
#pragma unroll
                for (int v = 0; v < MI; ++v) acc[u][v] = MFMA16(av, f4e(bb[s][v >> 2], v & 3), acc[u][v]);
                bsum[u] += av;
            }
        }
    };
    auto deal = [&]() {   // this buffer's MFMAs with another buffer's loads between them
        constexpr int NM = MU * MI * SB, NLD = (1 + NBK) * SB, R = NM / NLD > 0 ? NM / NLD : 1, K = NLD < NM ? NLD : NM;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            __builtin_amdgcn_sched_group_barrier(0x008, R, 0);   // MFMA
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
        }
        if constexpr (NM - K * R > 0) __builtin_amdgcn_sched_group_barrier(0x008, NM - K * R, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    const int niter = nsteps / SB;   // a multiple of NB: a wave's range is a multiple of 64 samples = 16 steps (or empty), NB SB divides 16
    static_assert(16 % (NB * SB) == 0, "buffer rotation");
    if (niter > 0) {
#pragma unroll
        for (int k = 0; k < NB - 1; ++k) ld(a[k], b[k], k);
        for (int it = 0; it < niter; it += NB) {
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                ld(a[(k + NB - 1) % NB], b[(k + NB - 1) % NB], min(it + k + NB - 1, niter - 1));   // (no branch: the last trips re-read the last rows)
                mm(a[k], b[k]);
                deal();
            }
        }
    }
    // ---- the wave's accumulators -> LDS in the slab's tile order.  acc[u][v], lane (i, q), register r is
    //      AV:  unit 16 q + 4 r + u of the block, input 4 i + (v & 3) of input block v >> 2:
    //           tile (q, 4 (v >> 2) + i / 4), row 4 r + u, column 4 (i % 4) + (v & 3) -> lane 16 r + column, register u:
    //           for fixed (v, r) the four u are 16 consecutive bytes;
    //      !AV: slot 4 q + r, input as above: tile (0, 4 (v >> 2) + i / 4), lane 16 q + column, register r: a tile register
    //           quadruple as it stands.
    float* part = lds + (size_t)w * NTILE * DW_TS;
    const int col = 4 * (i & 3);
    if constexpr (AV) {
#pragma unroll
        for (int v = 0; v < MI; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                *reinterpret_cast<float4*>(part + (q * MI + 4 * (v >> 2) + (i >> 2)) * DW_TS + (16 * r + col + (v & 3)) * 4) =
                    make_float4(acc[0][v][r], acc[1][v][r], acc[2][v][r], acc[3][v][r]);
    } else {
#pragma unroll
        for (int v = 0; v < MI; ++v)
            *reinterpret_cast<float4*>(part + (4 * (v >> 2) + (i >> 2)) * DW_TS + (16 * q + col + (v & 3)) * 4) =
                make_float4(acc[0][v][0], acc[0][v][1], acc[0][v][2], acc[0][v][3]);
    }
    float* bpart = lds + 4 * NTILE * DW_TS;   // [wave][64] column sums of A (AV: unit 4 i + u at 4 i + u; !AV: slot i)
    if (bias_out) {   // lane (i, q) holds samples 4 j + q; quarters (0 + 1) + (2 + 3)
#pragma unroll
        for (int u = 0; u < MU; ++u) {
            float t = bsum[u];
            t += __shfl_xor(t, 16);
            t += __shfl_xor(t, 32);
            if (lane < 16) bpart[w * 64 + (AV ? 4 * lane + u : lane)] = t;
        }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < (NTILE + 3) / 4; ++t) {
        const int tile = 4 * t + w;
        const int off = tile < NTILE ? out_off(tile / MI, tile % MI) : -1;
        if (off >= 0) {
            const float* base = lds + tile * DW_TS + lane * 4;
            const float4 p0 = *reinterpret_cast<const float4*>(base), p1 = *reinterpret_cast<const float4*>(base + NTILE * DW_TS);
            const float4 p2 = *reinterpret_cast<const float4*>(base + 2 * NTILE * DW_TS), p3 = *reinterpret_cast<const float4*>(base + 3 * NTILE * DW_TS);
            *reinterpret_cast<float4*>(slab + off + lane * 4) =
                make_float4(((p0.x + p1.x) + p2.x) + p3.x, ((p0.y + p1.y) + p2.y) + p3.y,
                            ((p0.z + p1.z) + p2.z) + p3.z, ((p0.w + p1.w) + p2.w) + p3.w);
        }
    }
    if (bias_out && w == 0 && lane < 16 * MU)
        bias_out[lane] = ((bpart[lane] + bpart[64 + lane]) + bpart[128 + lane]) + bpart[192 + lane];
}

constexpr int DW_LDS_FLOATS = 4 * 16 * DW_TS + 4 * 64;   // four waves x 16 tiles + the bias partials
constexpr int DW_SB = 4;   // MFMA steps per register buffer of the 64 x 64 blocks (four buffers).  At 2: 212 registers
                           // instead of 284, two workgroups of this launch fit on a CU -- measured, same box, interleaved:
                           // 22.8 against 22.6 us alone, 337.3 against 338.5 ms per tile with three fits in flight: no
                           // difference, the deeper ring stays

template <int NT, int NL>
__global__ void __launch_bounds__(WAVE_THREADS, 1) k_dw_wide(DwArgs A)
{
    __shared__ __attribute__((aligned(16))) float dw_lds[DW_LDS_FLOATS];
    const WidePlan& p = A.p;
    constexpr int UM = NT / 4, BC = 16 * NT;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int NT0 = p.NT0, IM0 = (NT0 + 3) / 4;
    const int T0 = UM * IM0, T1 = NL > 1 ? UM * UM : 0, T = T0 + T1 + 1;   // workgroup-tasks per slice
    // blockIdx -> XCD is round-robin on this part (speed only, never correctness): the workgroups of one XCD take the
    // slices x, x + 8, .. so that an XCD's L2 fetches every operand row once (at bs = 8192: one slice per XCD)
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int ns_x = (A.nslices - xcd + 7) >> 3;
    if (j >= ns_x * T) return;
    const int sl = j / T, task = j - sl * T, slice = xcd + 8 * sl;
    // this wave's quarter of the slice (the last slice of a short minibatch may leave waves without rows)
    const int k0 = min(slice * DW_KS + w * (DW_KS / 4), A.nrows), k1 = min(k0 + DW_KS / 4, A.nrows);
    const int nsteps = (k1 - k0) >> 2;
    float* slab = A.slabs + (size_t)slice * p.slab_floats;
    if (task < T0) {   // first layer: dz_0 (unit block um) x the rows' features (input block im)
        const int um = task / IM0, im = task - um * IM0;
        auto off = [&](int ut, int vt) { return 4 * im + vt < NT0 ? ((4 * um + ut) * NT0 + 4 * im + vt) * 256 : -1; };
        dw_task<true, 1, DW_SB, 4>(A.DZ[0], BC, 64 * um, A.X, p.xo, 64 * im, A.nrows, k0, nsteps, slab, off,
                               im == 0 ? slab + p.sl_bias + 64 * um : nullptr, lane, w, dw_lds);
    } else if (NL > 1 && task < T0 + T1) {   // hidden layer: dz_1 x H_0
        const int t1 = task - T0, um = t1 / UM, im = t1 - um * UM;
        auto off = [&](int ut, int vt) { return p.sl_hid + ((4 * um + ut) * NT + 4 * im + vt) * 256; };
        dw_task<true, 1, DW_SB, 4>(A.DZ[1], BC, 64 * um, A.H[0], BC, 64 * im, A.nrows, k0, nsteps, slab, off,
                               im == 0 ? slab + p.sl_bias + BC + 64 * um : nullptr, lane, w, dw_lds);
    } else {   // output layer: dz_out (the 16 channel slots) x H_last, all of its units
        auto off = [&](int ut, int vt) { return p.sl_out + vt * 256; };
        dw_task<false, NT / 4, 2, 4>(A.DZO, WOP, 0, A.H[NL - 1], BC, 0, A.nrows, k0, nsteps, slab, off, slab + p.sl_bias + NL * BC, lane, w, dw_lds);
    }
}

template <int LQ, int NL, int NT>
static int launch_wide(const WideArgs& A, int nwg, hipStream_t s, bool configure)
{
    auto kern = k_train_half<LQ, NL, NT>;
    if (configure) {   // once per device and kernel (a cache of an idempotent setting)
        static std::atomic<unsigned long long> configured{0};
        return configure_lds_once(kern, A.p.lds_floats * 4, configured);
    }
    kern<<<nwg, WAVE_THREADS, (size_t)A.p.lds_floats * 4, s>>>(A);
    LBDRN_LAUNCH_CHECK();
    return 0;
}

template <int LQ>
static int dispatch_wide_lq(const WideArgs& A, int nwg, hipStream_t s, bool configure)
{
    const bool one = A.net.nl == 1;
    if (A.p.NT == 16) return one ? launch_wide<LQ, 1, 16>(A, nwg, s, configure) : launch_wide<LQ, 2, 16>(A, nwg, s, configure);
    return one ? launch_wide<LQ, 1, 8>(A, nwg, s, configure) : launch_wide<LQ, 2, 8>(A, nwg, s, configure);
}

static int dispatch_wide(const WideArgs& A, int nwg, hipStream_t s, bool configure)
{
    switch (A.p.LQ) {
        case 16: return dispatch_wide_lq<16>(A, nwg, s, configure);
        case 32: return dispatch_wide_lq<32>(A, nwg, s, configure);
        case 48: return dispatch_wide_lq<48>(A, nwg, s, configure);
        case 52: return dispatch_wide_lq<52>(A, nwg, s, configure);
        default: return dispatch_wide_lq<64>(A, nwg, s, configure);
    }
}

static int dispatch_dw(const DwArgs& A, hipStream_t s)
{
    const int NT = A.p.NT, NL = A.p.nl;
    const int IM0 = (A.p.NT0 + 3) / 4, UM = NT / 4;
    const int T = UM * IM0 + (NL > 1 ? UM * UM : 0) + 1;
    const int ns_max = (A.nslices + 7) / 8;                    // slices of the busiest XCD
    const unsigned grid = 8u * (unsigned)(ns_max * T);
    if (NT == 16) {
        if (NL == 1) k_dw_wide<16, 1><<<grid, WAVE_THREADS, 0, s>>>(A); else k_dw_wide<16, 2><<<grid, WAVE_THREADS, 0, s>>>(A);
    } else {
        if (NL == 1) k_dw_wide<8, 1><<<grid, WAVE_THREADS, 0, s>>>(A); else k_dw_wide<8, 2><<<grid, WAVE_THREADS, 0, s>>>(A);
    }
    LBDRN_LAUNCH_CHECK();
    return 0;
}

static int wide_train_epoch(const lbdrn_geom& g, const lbdrn_net& net, const int64_t* perm, int64_t n, int bs,
                            float* params, float* m, float* v, int64_t step0, double lr, float* losses, void* ws,
                            size_t ws_bytes, hipStream_t s)
{
    WideArgs A;
    if (!make_wide_plan(g, net, &A.p)) {
        set_error("shape not supported by the wide MFMA train kernel");
        return LBDRN_E_UNSUPPORTED;
    }
    const WideWsLayout L = wide_ws_layout(g, net, A.p, bs);
    if (!ws || ws_bytes < L.total) {
        set_error("train workspace too small: %zu < %zu", ws_bytes, L.total);
        return LBDRN_E_WORKSPACE;
    }
    float* packed = (float*)((char*)ws + L.off_pack);
    LBDRN_HIP_TRY(hipMemsetAsync(packed, 0, (size_t)A.p.pack_floats * sizeof(float), s));
    k_pack_wide<<<(unsigned)((A.p.NP + 255) / 256), 256, 0, s>>>(params, A.p, net.F, net.C, packed);
    LBDRN_LAUNCH_CHECK();
    int4* map = (int4*)((char*)ws + L.off_map);
    k_build_map_wide<<<(unsigned)((A.p.slab_floats + 255) / 256), 256, 0, s>>>(A.p, net.F, net.C, map);
    LBDRN_LAUNCH_CHECK();
    A.net = net; A.rows = (float*)((char*)ws + L.off_rows); A.npix = (int64_t)g.H * g.W; A.params = params;
    A.packed = packed; A.slabs = (float*)((char*)ws + L.off_slab); A.loss_part = (double*)((char*)ws + L.off_loss);
    A.oX = (float*)((char*)ws + L.off_x);
    A.oDZO = (float*)((char*)ws + L.off_dzo);
    for (int l = 0; l < 2; ++l) { A.oH[l] = (float*)((char*)ws + L.off_h[l]); A.oDZ[l] = (float*)((char*)ws + L.off_dz[l]); }
    if (int rc = dispatch_wide(A, 0, s, true)) return rc;
    DwArgs Dw;
    Dw.p = A.p; Dw.X = A.oX; Dw.DZO = A.oDZO; Dw.slabs = A.slabs;
    for (int l = 0; l < 2; ++l) { Dw.H[l] = A.oH[l]; Dw.DZ[l] = A.oDZ[l]; }
    A.stamps = nullptr;
#ifdef LBDRN_TRAIN_STAMPS
    const int max_wg = (bs + HB - 1) / HB;
    LBDRN_HIP_TRY(hipMalloc(&A.stamps, (size_t)max_wg * 4 * 16 * sizeof(unsigned long long)));
#endif
    int64_t step = step0;
    int si = 0;
    for (int64_t first = 0; first < n; first += bs, ++si) {
        const int B = (int)std::min<int64_t>(bs, n - first);
        const int rpw = HB;
        const int nwg = (B + rpw - 1) / rpw;
        A.perm = perm + first;
        A.batch_n = B;
        A.inv = 1.0f / ((float)B * (float)net.C);
        if (int rc = dispatch_wide(A, nwg, s, false)) return rc;
        if (g_prof_mode == 2)   // measurement only (lbdrn_train_profile_mode): the same launch again
            if (int rc = dispatch_wide(A, nwg, s, false)) return rc;
        // the weight gradients: one partial slab per slice of DW_KS samples
        Dw.nrows = (nwg * rpw + 63) / 64 * 64;
        const int nslabs = Dw.nslices = (Dw.nrows + DW_KS - 1) / DW_KS;
        if (g_prof_mode != 4)
            if (int rc = dispatch_dw(Dw, s)) return rc;
        if (g_prof_mode == 5)   // measurement only: the same launch again
            if (int rc = dispatch_dw(Dw, s)) return rc;
        ++step;
        const double bc1 = 1.0 - std::pow(0.9, (double)step), bc2 = 1.0 - std::pow(0.999, (double)step);
        ReduceArgs R;
        for (int f = 0; f < MAX_GROUP; ++f)
            R.fit[f] = ReduceFit{A.slabs, params, m, v, packed, A.loss_part, losses ? losses + si : nullptr};
        R.nloss = nwg;
        R.tl = nullptr;
        if (g_prof_mode != 3 && g_prof_mode != 4)
            launch_reduce(R, A.p.slab_floats / (4 * RED_LANES), 1, false, nslabs, A.p.slab_floats, map, (float)(lr / bc1), (float)std::sqrt(bc2), (double)B * net.C, s);
        if (g_prof_mode == 1) {   // measurement only: the same launch again with a zero step
            for (int f = 0; f < MAX_GROUP; ++f) R.fit[f].loss_out = nullptr;
            launch_reduce(R, A.p.slab_floats / (4 * RED_LANES), 1, false, nslabs, A.p.slab_floats, map, 0.0f, (float)std::sqrt(bc2), (double)B * net.C, s);
        }
        LBDRN_LAUNCH_CHECK();
    }
#ifdef LBDRN_TRAIN_STAMPS
    {
        LBDRN_HIP_TRY(hipStreamSynchronize(s));
        const int nw = ((int)std::min<int64_t>(bs, n) + HB - 1) / HB * 4;
        std::vector<unsigned long long> h((size_t)nw * 16);
        LBDRN_HIP_TRY(hipMemcpy(h.data(), A.stamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        (void)hipFree(A.stamps);
        double d[14] = {}, clk = 0;
        for (int k = 0; k < nw; ++k) {
            for (int j = 1; j <= 13; ++j) d[j] += (double)(h[k * 16 + j] - h[k * 16 + j - 1]);
            clk += (double)(h[k * 16 + 13] - h[k * 16 + 0]) / (double)(h[k * 16 + 15] - h[k * 16 + 14]) * 100.0;
        }
        fprintf(stderr, "[lbdrn stamps, half kernel] clock %.0f MHz; wave lifetime %.0f cycles; mean cycles: rows landed, operands read %.0f | layer 0 (X copy and the earlier passes' act0 under it) %.0f | "
                        "act0 + stores of the last pass %.0f | barrier (h0 exchanged) %.0f | hidden layer (earlier passes' act1 under it) %.0f | act1 + stores of the last pass %.0f | output partials, barrier, loss %.0f | "
                        "dz1 product + stores %.0f | barrier (dz1 exchanged) %.0f | dh0 product + dz0 %.0f | tail %.0f\n",
                clk / nw, (d[1] + d[2] + d[3] + d[4] + d[5] + d[6] + d[7] + d[8] + d[9] + d[10] + d[11] + d[12] + d[13]) / nw,
                d[1] / nw, d[2] / nw, d[3] / nw, d[4] / nw, d[5] / nw, d[6] / nw, d[7] / nw, d[8] / nw, d[9] / nw, d[10] / nw,
                (d[11] + d[12] + d[13]) / nw);
    }
#endif
    return 0;
}
