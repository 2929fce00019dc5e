// k_apply_wide: the fused apply pass (decode / evaluation) of networks too wide for k_apply_mfma's LDS-resident
// weights -- bc = 256 (BASELINE.json configs[2]) and bc = 128 shapes whose weights + window do not fit 160 KB.
// Included by apply_mfma.hip.
//
// Same contract as k_apply_mfma: neighbourhood gather + normalise + nl x (Linear -> sin(30 z)) + Linear -> sigmoid
// in one pass, no feature matrix in HBM, every dot product a k-ascending fmaf chain seeded by the bias (bit for bit the
// generic kernels and the oracle).  What the width changes is where the weights live: W1 alone is 256 KB, so nothing
// stays near the CU and every product STREAMS its fragments L2 -> VGPR (1 KB blocks, scalar-offset buffer loads,
// one group of NT blocks ahead of the MFMAs that use them, one request dealt out per three MFMAs), as k_train_wide's
// forward half does.  The rest is the wave-local scheme on v_mfma_f32_16x16x4_f32:
//  * one wave = 16 pixels of a row; a layer is NT = bc/16 accumulator tiles [16 units][16 pixels];
//  * MFMA step s, lane quarter q multiplies k = 4 s + q: ascending over the steps and inside a step -- the order of a
//    scalar loop.  The accumulator of tile t holds, in register r of lane quarter q, tile row 4 q + r; the weights are
//    packed so that tile row m carries unit 16 t + 4 (m & 3) + (m >> 2), i.e. that register holds unit
//    16 t + 4 r + q = 4 (4 t + r) + q: exactly the k that step 4 t + r of the next product takes from that lane.  No data
//    movement between layers, and the canonical order is kept;
//  * layer-0 B operands are made on the fly from the LDS-staged window (offset table per colour feature), the
//    positional ones from the row / column tables, one group of four steps ahead of the MFMAs;
//  * the last layer is one chain of 4 NT dependent MFMAs (a second accumulator would change the summation order).
// A workgroup = 4 waves walks 64 x TH pixel tiles (staging as in k_apply_mfma); evaluation partials per virtual
// workgroup, so the sum does not depend on the launch shape.

constexpr int WA_THREADS = 256;

struct WApplyPlan {
    int NT;          // unit tiles = bc/16
    int G0;          // layer-0 groups of four MFMA steps = ceil(F/16), rounded up to even
    int TH, SH, SW, ncolor;
    int skip;        // 1 (the tolerance-arithmetic pass with RELATIVE, D > 0): the window centres -- centre minus centre, exact
                     // zeros -- are not features of layer 0: Fe = F - C of them, slot j <-> feature wa_feat_of_slot(j)
    int Fe, S2;      // features layer 0 multiplies; (2D+1)^2
    int pk_w0, pk_wh, pk_wl, pk_bh, pk_bl, pack_floats;   // fragment-order buffer (floats)
    int off_ktab, off_rowt, off_colt, off_tile, lds_floats;
    int tiles_x, tiles_y;
};

// slot j of the compacted feature order <-> feature index (identity without `skip`): positional features first, then per
// band the window positions without the centre
__host__ __device__ __forceinline__ int wa_feat_of_slot(int j, int P2, int S2, bool skip)
{
    if (!skip || j < P2) return j;
    const int cj = j - P2, c = cj / (S2 - 1), r = cj - c * (S2 - 1);
    return P2 + c * S2 + r + (r >= S2 / 2 ? 1 : 0);
}

static bool make_wapply_plan(const lbdrn_geom& g, const lbdrn_net& net, WApplyPlan* p, bool fast = false)
{
    if (net.act != LBDRN_ACT_SINE || net.bc % 16 != 0 || !wapply_row(net.bc / 16)) return false;
    if (net.C > 16 || net.nl < 1 || net.nl > 2 || net.F < 1) return false;
    WApplyPlan q;
    q.NT = net.bc / 16;
    q.ncolor = net.F - 2 * g.P;
    if (q.ncolor < 0) return false;
    // the evaluation pass in the tolerance arithmetic leaves the always-zero window centres out (LBDRNdataset.py:126-128;
    // its sum is held to 1e-6, not to a bit pattern): F = 200 -> 192 = twelve groups of 16 instead of the fourteen that
    // 200 pads to.
    q.S2 = (2 * g.D + 1) * (2 * g.D + 1);
    q.skip = fast && g.use_colors && g.relative && g.D > 0 && q.ncolor == g.C * q.S2;
    q.Fe = q.skip ? net.F - g.C : net.F;
    q.G0 = ((q.Fe + 15) / 16 + 1) & ~1;   // even: the kernel walks the groups in pairs (a padding group carries zero weights)
    if (q.ncolor < 1) return false;        // (USE_COLORS off: the generic kernels)
    int k = 0;
    q.pk_w0 = k; k += q.NT * q.G0 * 256;
    q.pk_wh = k; k += (net.nl - 1) * q.NT * q.NT * 256;
    q.pk_wl = k; k += q.NT * 256;
    q.pk_bh = k; k += net.nl * q.NT * 16;
    q.pk_bl = k; k += 16;
    q.pack_floats = k;
    q.SW = TILE_W + 2 * g.D;
    int o = 0;
    q.off_ktab = o; o += 2 * std::max(q.ncolor, 1) + 2;
    const int fixed = o;
    int th = 16;
    for (;; th >>= 1) {
        if (th == 0) return false;
        q.TH = th;
        q.SH = th + 2 * g.D;
        o = fixed;
        q.off_rowt = o; o += th * g.P;
        q.off_colt = o; o += TILE_W * g.P;
        o = (o + 3) & ~3;
        q.off_tile = o; o += (g.use_colors ? g.C * q.SH * q.SW : 0);
        q.lds_floats = std::max(o, q.off_rowt + 2 * WA_THREADS + 4);   // (the per-tile regions double as the SSE reduction's doubles)
        if ((size_t)q.lds_floats * 4 <= 64 * 1024) break;
    }
    q.tiles_x = (g.W + TILE_W - 1) / TILE_W;
    q.tiles_y = (g.H + q.TH - 1) / q.TH;
    *p = q;
    return true;
}

// params (state_dict order) -> fragment order; one thread per packed float
__global__ void __launch_bounds__(256)
    k_pack_apply_wide(const float* __restrict__ params, lbdrn_net net, WApplyPlan p, int P2, float* __restrict__ out)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= p.pack_floats) return;
    const int NT = p.NT, bc = net.bc, F = net.F;
    const int64_t offB0 = (int64_t)bc * F;
    auto offW = [&](int l) -> int64_t { return l == 0 ? 0 : offB0 + bc + (int64_t)(l - 1) * ((int64_t)bc * bc + bc); };
    const int64_t offWl = offW(net.nl), offBl = offWl + (int64_t)net.C * bc;
    float v = 0.0f;
    if (e < p.pk_bh) {
        const int blk = e >> 8, lane = (e >> 2) & 63, c = e & 3;
        const int i = lane & 15, q = lane >> 4;
        const int row_unit = 4 * (i & 3) + (i >> 2);   // tile row i carries unit 16 t + row_unit
        if (e < p.pk_wh) {            // layer 0: block t*G0 + g, k = 16 g + 4 c + q
            const int t = blk / p.G0, g = blk - t * p.G0;
            const int k = 16 * g + 4 * c + q;
            if (k < p.Fe) v = params[(int64_t)(16 * t + row_unit) * F + wa_feat_of_slot(k, P2, p.S2, p.skip)];
        } else if (e < p.pk_wl) {     // hidden layer l: block ((l-1) NT + to) NT + tk, k = 16 tk + 4 c + q
            const int b = blk - (p.pk_wh >> 8);
            const int l = 1 + b / (NT * NT), to = (b / NT) % NT, tk = b % NT;
            v = params[offW(l) + (int64_t)(16 * to + row_unit) * bc + 16 * tk + 4 * c + q];
        } else {                      // last layer: block tk, row i = channel i
            const int tk = blk - (p.pk_wl >> 8);
            if (i < net.C) v = params[offWl + (int64_t)i * bc + 16 * tk + 4 * c + q];
        }
    } else if (e < p.pk_bl) {         // hidden biases [l][t][q][r]: unit 16 t + 4 r + q
        const int b = e - p.pk_bh;
        const int r = b & 3, q = (b >> 2) & 3, t = (b >> 4) % NT, l = b / (16 * NT);
        v = params[offW(l) + (int64_t)bc * (l == 0 ? F : bc) + 16 * t + 4 * r + q];
    } else {                          // last bias [q][r]: channel 4 q + r
        const int ch = e - p.pk_bl;
        if (ch < net.C) v = params[offBl + ch];
    }
    out[e] = v;
}

struct WApplyArgs {
    lbdrn_geom g;
    lbdrn_net net;
    WApplyPlan p;
    const float* packed;
    const uint16_t* msb;
    const uint16_t* img;  // EVAL: original image (labels)
    uint16_t* out;        // DECODE
    float* y_out;         // DECODE, optional
    double* partial;      // EVAL: [nvirt]
    int nvirt;
    int nodata;           // EVAL (LBDRN_EVAL_VALID): samples of img equal to it add no term; -1: none
    int decoded;          // EVAL (LBDRN_EVAL_DECODED): a term is (img - out)^2, out the sample the decode pass writes; canonical instance only
    unsigned long long* stamps;  // diagnostic build (-DLBDRN_APPLY_STAMPS): [gridDim.x][8] cycle sums of wave 0
};

typedef float wa_f32x4 __attribute__((ext_vector_type(4)));
typedef int wa_v4i32 __attribute__((ext_vector_type(4)));
#define WA_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
// phase boundary: nothing is scheduled across it (left free, the compiler mixes the phases -- sines into the MFMA
// streams, the next product's requests ahead of them -- and the pass takes 28 ms instead of 10); the diagnostic build
// also stamps the clock here
#ifdef LBDRN_APPLY_STAMPS
#define WA_PHASE(k) ASTAMP(k)
#else
#define WA_PHASE(k) __builtin_amdgcn_sched_barrier(0)
#endif

template <int NT, int NL, int MODE>
__global__ void __launch_bounds__(WA_THREADS, 1) k_apply_wide(WApplyArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const lbdrn_geom& g = A.g;
    const WApplyPlan& p = A.p;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, q = lane >> 4;
    const int P = g.P, D = g.D, C = g.C, F = p.Fe, G0 = p.G0;   // (F: the features layer 0 walks, WApplyPlan::skip)
    const int ncolor = p.skip ? p.ncolor - C : p.ncolor;
    int* ktab = reinterpret_cast<int*>(lds + p.off_ktab);
    {   // offset table of the colour features into the staged window: (neighbour, centre)
        const int side = 2 * D + 1, plane = p.SH * p.SW;
        for (int k = tid; k < max(ncolor, 1); k += WA_THREADS) {
            const int kk = wa_feat_of_slot(2 * P + min(k, max(ncolor - 1, 0)), 2 * P, p.S2, p.skip) - 2 * P;
            const int c = kk / (side * side), r = kk - c * side * side;
            const int dy = r / side, dx = r - dy * side;
            ktab[2 * k] = c * plane + (dy - D) * p.SW + (dx - D);
            ktab[2 * k + 1] = c * plane;
        }
    }
    float* rowt = lds + p.off_rowt;
    float* colt = lds + p.off_colt;
    float* tile = lds + p.off_tile;
    const bool rel = g.relative && D > 0;
    const float maxf = (float)g.msb_max;
    const int64_t HW = (int64_t)g.H * g.W;
    const float scale = (float)((1 << g.K) - 1);
    const int lmask = (1 << g.K) - 1;
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A.packed), (short)0,
                                                                         p.pack_floats * 4, 0x00020000);
    const int lane16 = lane * 16;
    auto ldw = [&](int byte_base, int block) -> float4 {
        const wa_v4i32 x = __builtin_amdgcn_raw_buffer_load_b128(wrs, lane16, byte_base + block * 1024, 0);
        return make_float4(__int_as_float(x[0]), __int_as_float(x[1]), __int_as_float(x[2]), __int_as_float(x[3]));
    };

#ifdef LBDRN_APPLY_STAMPS
    unsigned long long acc_t[8] = {}, last_t, rt0, rt1;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt0)::"memory");
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(last_t)::"memory");
#endif
    const int ntiles = p.tiles_x * p.tiles_y;
    for (int v = blockIdx.x; v < A.nvirt; v += gridDim.x) {
        double sse = 0.0;
        for (int t = v; t < ntiles; t += A.nvirt) {
            const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
            const int y0 = ty * p.TH, x0 = tx * TILE_W;
            __syncthreads();  // previous tile fully consumed (and the offset table written)
            // ---- stage the (TH+2D) x (64+2D) ring: p = float(msb)/max, reflect-padded (LBDRNdataset.py:120-123)
            if (g.use_colors) {
                const int plane = p.SH * p.SW, total = C * plane;
                constexpr int UB = 8;
                for (int base = 0; base < total; base += WA_THREADS * UB) {
                    unsigned short raw[UB];
#pragma unroll
                    for (int u = 0; u < UB; ++u) {
                        const int e = min(base + u * WA_THREADS + tid, total - 1);
                        const int row = e / p.SW, sx = e - row * p.SW, c = row / p.SH, sy = row - c * p.SH;
                        int yy = reflect_fast(y0 + sy - D, g.H), xx = reflect_fast(x0 + sx - D, g.W);
                        // (rows / columns past a ragged last tile feed only masked outputs: reflect_fast keeps them valid)
                        raw[u] = MODE == MODE_EVAL_FAST ? (unsigned short)(A.img[(int64_t)c * HW + (int64_t)yy * g.W + xx] >> g.K)   // (a fit's MSB plane IS img >> K)
                                                        : A.msb[(int64_t)c * HW + (int64_t)yy * g.W + xx];
                    }
#pragma unroll
                    for (int u = 0; u < UB; ++u) {
                        const int e = base + u * WA_THREADS + tid;
                        if (e < total) tile[e] = (float)raw[u] / maxf;
                    }
                }
            }
            for (int e = tid; e < p.TH * P; e += WA_THREADS) {
                const int yy = min(y0 + e / P, g.H - 1);
                rowt[e] = g.rowtab[(int64_t)yy * P + e % P];
            }
            for (int e = tid; e < TILE_W * P; e += WA_THREADS) {
                const int xx = min(x0 + e / P, g.W - 1);
                colt[e] = g.coltab[(int64_t)xx * P + e % P];
            }
            __syncthreads();

            WA_PHASE(0);  // staging + barriers
            const int nseg = p.TH * (TILE_W / 16);
            for (int seg = wave; seg < nseg; seg += WA_THREADS / 64) {
                const int ly = seg / (TILE_W / 16), lx = (seg % (TILE_W / 16)) * 16;
                const int pixbase = (ly + D) * p.SW + (lx + i + D);
                const int yy = y0 + ly, xx = x0 + lx + i;
                const bool inside = yy < g.H && xx < g.W;
                const int64_t pix = (int64_t)min(yy, g.H - 1) * g.W + min(xx, g.W - 1);
                // B operand of layer 0, step 4 g + e: feature k = 16 g + 4 e + q of this lane's pixel.  Branch-free (a
                // branch would cut the MFMA stream into basic blocks the dealt schedule cannot cross): indices are clamped
                // into their tables, the value past F is 0 by select (its weight is 0, but it must be finite)
                auto colour = [&](int k) __attribute__((always_inline)) -> float {
                    const int2 e2 = *reinterpret_cast<const int2*>(ktab + 2 * min(max(k - 2 * P, 0), ncolor - 1));
                    const float nb = tile[pixbase + e2.x];
                    const float ct = tile[pixbase + e2.y];
                    const float vcol = rel ? nb - ct : nb;   // minus centre, LBDRNdataset.py:126-128
                    return k < F ? vcol : 0.0f;
                };
                auto feature = [&](int k) __attribute__((always_inline)) -> float {   // groups that hold positional features
                    const float vr = rowt[ly * P + min(k, P - 1)];
                    const float vc = colt[(lx + i) * P + min(max(k - P, 0), P - 1)];
                    const float vcol = colour(k);
                    return k < P ? vr : k < 2 * P ? vc : vcol;
                };
                const int gpos = P > 0 ? min(G0, (2 * P + 15) / 16) : 0;
                // section starts of the fragment buffer, made opaque per segment: everything fetched through them (biases,
                // 16 + 256 + 16 block offsets) would otherwise be hoisted out of this loop and held -- or spilled -- across it
                int o_w0 = p.pk_w0 * 4, o_wh = p.pk_wh * 4, o_wl = p.pk_wl * 4, o_bh = p.pk_bh, o_bl = p.pk_bl;
                asm volatile("" : "+s"(o_w0), "+s"(o_wh), "+s"(o_wl), "+s"(o_bh), "+s"(o_bl));
                auto ldbias = [&](int l, int t) -> wa_f32x4 {
                    const float4 b4 = *reinterpret_cast<const float4*>(A.packed + o_bh + ((l * NT + t) * 4 + q) * 4);
                    wa_f32x4 b = {b4.x, b4.y, b4.z, b4.w};
                    return b;
                };
                wa_f32x4 acc[NT];
#pragma unroll
                for (int tt = 0; tt < NT; ++tt) acc[tt] = ldbias(0, tt);
                float4 wq[2][NT];   // the group being multiplied and the one in flight behind it
#pragma unroll
                for (int tt = 0; tt < NT; ++tt) wq[0][tt] = ldw(o_w0, tt * G0);
                float bq[2][4];
                if (gpos > 0) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) bq[0][e] = feature(4 * e + q);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) bq[0][e] = colour(4 * e + q);
                }
                // ---- layer 0: k = 0 .. F-1 in order, two groups per trip (the ring indices stay compile-time); the
                //      request behind the last group re-reads it (harmless) instead of branching
#define WA_L0_PAIR(FEATURE)                                                                                             \
    _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                                    \
        const int gn = min(gg + u + 1, G0 - 1);                                                                        \
        _Pragma("unroll") for (int tt = 0; tt < NT; ++tt) wq[u ^ 1][tt] = ldw(o_w0, tt * G0 + gn);                     \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) bq[u ^ 1][e] = FEATURE(16 * gn + 4 * e + q);                     \
        _Pragma("unroll") for (int e = 0; e < 4; ++e)                                                                  \
            _Pragma("unroll") for (int tt = 0; tt < NT; ++tt) {                                                        \
                const float4 x = wq[u][tt];                                                                            \
                acc[tt] = WA_MFMA(e == 0 ? x.x : e == 1 ? x.y : e == 2 ? x.z : x.w, bq[u][e], acc[tt]);                \
            }                                                                                                          \
        _Pragma("unroll") for (int k = 0; k < NT; ++k) {                                                               \
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); /* MFMA */                                              \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); /* LDS read */                                          \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                         \
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); /* VMEM read */                                         \
        }                                                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
    }
                int gg = 0;
                for (; gg < gpos; gg += 2) { WA_L0_PAIR(feature) }
                for (; gg < G0; gg += 2) { WA_L0_PAIR(colour) }
#undef WA_L0_PAIR
                WA_PHASE(1);  // layer 0
                float h[NT][4];
                auto activate = [&]() __attribute__((always_inline)) {   // (tile by tile: 64 sines scheduled at once hold hundreds of temporaries)
#pragma unroll
                    for (int tt = 0; tt < NT; ++tt) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) h[tt][r] = MODE == MODE_EVAL_FAST ? fast_sin(30.0f * acc[tt][r]) : siren_act(acc[tt][r]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                };
                // ---- hidden layer 1: B = the activations where they stand (step 4 tk + r multiplies unit 16 tk + 4 r + q)
                if constexpr (NL > 1) {
#pragma unroll
                    for (int tt = 0; tt < NT; ++tt) wq[0][tt] = ldw(o_wh, tt * NT);   // requested under the sines
                    activate();
                    WA_PHASE(2);  // sin
#pragma unroll
                    for (int tt = 0; tt < NT; ++tt) acc[tt] = ldbias(1, tt);
#pragma unroll
                    for (int tk = 0; tk < NT; ++tk) {
                        if (tk + 1 < NT) {
#pragma unroll
                            for (int tt = 0; tt < NT; ++tt) wq[(tk + 1) & 1][tt] = ldw(o_wh, tt * NT + tk + 1);
                        } else {
#pragma unroll
                            for (int tt = 0; tt < NT; ++tt) wq[(tk + 1) & 1][tt] = ldw(o_wl, tt);   // the last layer's blocks
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int to = 0; to < NT; ++to) {
                                const float4 x = wq[tk & 1][to];
                                acc[to] = WA_MFMA(r == 0 ? x.x : r == 1 ? x.y : r == 2 ? x.z : x.w, h[tk][r], acc[to]);
                            }
#pragma unroll
                        for (int k = 0; k < NT; ++k) {
                            __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
                            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    WA_PHASE(3);  // layer 1
                    activate();
                    WA_PHASE(2);
                } else {
#pragma unroll
                    for (int tt = 0; tt < NT; ++tt) wq[NT & 1][tt] = ldw(o_wl, tt);
                    activate();
                }
                // what the epilogue needs from HBM (label source / the MSB to rebuild): requested under the last layer's chain
                unsigned short pre[4];
                {
                    const uint16_t* src = (MODE == MODE_DECODE) ? A.msb : A.img;
#pragma unroll
                    for (int r = 0; r < 4; ++r) pre[r] = src[(int64_t)min(4 * q + r, C - 1) * HW + pix];
                }
                // ---- last layer: rows = channels, one k-ordered chain
                wa_f32x4 o;
                {
                    const float4 b4 = *reinterpret_cast<const float4*>(A.packed + o_bl + 4 * q);
                    o[0] = b4.x; o[1] = b4.y; o[2] = b4.z; o[3] = b4.w;
                }
#pragma unroll
                for (int tk = 0; tk < NT; ++tk) {
                    const float4 x = wq[NT & 1][tk];
                    o = WA_MFMA(x.x, h[tk][0], o);
                    o = WA_MFMA(x.y, h[tk][1], o);
                    o = WA_MFMA(x.z, h[tk][2], o);
                    o = WA_MFMA(x.w, h[tk][3], o);
                }
                WA_PHASE(4);  // last layer
                // ---- epilogue: lane (pixel i, quarter q), register r = channel 4 q + r
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ch = 4 * q + r;
                    if (ch < C && inside) {
                        const float yv = MODE == MODE_EVAL_FAST ? fast_sigmoid(o[r]) : canon_sigmoid(o[r]);
                        if (MODE == MODE_DECODE) {
                            const float rr = __builtin_rintf(yv * scale);  // torch.round, decode.py:131
                            const int base = (int)pre[r] << g.K;           // decode.py:134
                            A.out[(int64_t)ch * HW + pix] = (uint16_t)(base + (int)rr);
                            if (A.y_out) A.y_out[pix * C + ch] = yv;
                        } else if ((int)pre[r] != A.nodata) {   // (a nodata sample: a term not added)
                            if (MODE == MODE_EVAL && A.decoded) {   // (uniform over the launch; the centre sample of msb, as the decode pass reads it)
                                int band = ch;   // (opaque: the band's 64-bit offset is formed here, not held in registers over the loops: k_apply_mfma)
                                asm volatile("" : "+v"(band));
                                sse += decoded_term((int)pre[r], (int)A.msb[(int64_t)band * HW + pix], yv, scale, g.K);
                                continue;
                            }
                            const float lab = (float)((int)pre[r] & lmask) / scale;
                            const float d = yv - lab;
                            sse += (double)(d * d);
                        }
                    }
                }
                WA_PHASE(5);  // epilogue
            }
        }
        if (MODE != MODE_DECODE) {
            __syncthreads();
            double* red = reinterpret_cast<double*>(lds + ((p.off_rowt + 3) & ~3));  // the per-tile regions: consumed
            red[tid] = sse;
            __syncthreads();
            for (int o2 = WA_THREADS / 2; o2 > 0; o2 >>= 1) {
                if (tid < o2) red[tid] += red[tid + o2];
                __syncthreads();
            }
            if (tid == 0) A.partial[v] = red[0];
        }
    }
#ifdef LBDRN_APPLY_STAMPS
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt1)::"memory");
    acc_t[6] = rt1 - rt0;   // 100 MHz ticks
    acc_t[7] = wave;
    if (lane == 0 && A.stamps && wave == (int)(blockIdx.x & 3))   // a different wave of each workgroup reports
        for (int k = 0; k < 8; ++k) A.stamps[(size_t)blockIdx.x * 8 + k] = acc_t[k];
#endif
}
#undef WA_MFMA
#undef WA_PHASE
