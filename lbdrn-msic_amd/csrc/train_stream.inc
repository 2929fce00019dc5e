// k_train_stream: the wave-local training step (k_train_wave, above) with its memory prologue turned into a stream
// that runs UNDER the first layer's MFMAs (ref modified_ignite_engine.py:18-27; LBDRNdataset.py:151-155 for the gather).
//
// What round 2's kernel left on the table (in-kernel stamps, 39.7 k cycles per wave): 9.9 k cycles in which the four
// waves of a workgroup do nothing but wait for 106 KB -- their 64 rows and the layer-0 weight fragments -- to arrive at
// the ~18 B/clk a CU takes in, followed by 6.8 k cycles of layer-0 MFMAs during which the memory path carries only
// the 160 KB of small-matrix fragments (40 KB per wave, four times the same bytes).  Here:
//  * the row matrix is stored in the order layer 0 eats it: a row is G0 = LQ/4 groups of 64 B, group g = the four
//    features each lane quarter multiplies in MFMA group g (k = q LQ + 4 g + e), then one group of labels.  A wave's
//    request g is then "64 B of each of my 16 rows" (lane = 4 row + quarter), lands lane-linear in LDS, and is all
//    that MFMA group g needs from the rows: nothing waits for a whole row any more;
//  * requests are issued a few stages ahead (stage = two groups: two row requests + two fragment blocks per wave)
//    and consumed behind counted waits (s_waitcnt vmcnt(N): requests complete in order) and one workgroup barrier per
//    stage (the fragment blocks of a group are fetched once per workgroup, a quarter by each wave);
//  * LDS-DMA is issued by inline assembly: the compiler's waitcnt pass parks an s_waitcnt vmcnt(0) in front of the
//    first LDS read behind a builtin LDS-DMA (it cannot tell which bytes a request writes); with the requests out of its
//    sight the LDS reads stay free and the waits are the counted ones written here.  Extra vector-memory operations
//    the compiler issues in between can only make a counted wait stricter (completion is in order), never wrong;
//  * W_1 and W_1^T fragments (the same for all four waves) are fetched once per workgroup into LDS behind the last
//    stages (8 requests per wave instead of 32 L2 -> VGPR loads) where LDS has room for them (LQ <= 52);
//  * dz^T is parked [unit][sample] with the samples in order and lane quarter q of the weight-gradient products
//    takes the 16 samples of wave q: the 32 transposed stores per wave and layer are conflict-free (round 2's
//    column permutation made them 4-way: the 323 k LDS bank-conflict cycles per launch of r02_sq_a.csv); the
//    row-major operands (rows, H, dz_out) keep rows of different waves 16 banks apart.
// LDS map (floats, LQ = 52, NL = 2; 150.6 KB = 118 of the CU's 128 allocation granules of 1280 B -- LQ = 48: 146.5 KB =
// 115 granules --: the reduce / Adam launch of another fit, 4 KB, fits beside it): rows X' [4 waves][14 groups][260] | layer-0 fragments [13 groups][4
// tiles][256], whose first six groups become H0 + the loss partials after the last stage barrier and whose rest, after
// the barrier behind layer 0, takes H1, dz_out and dz^T -- dz^T running over the W_1 fragments once the barrier behind
// the hidden layer has passed | W_1 fragments | W_1^T fragments.
constexpr int SGP = 260;   // floats per (wave, group) piece of X': 64 lanes x 16 B + 16 B (group g starts 4 g banks on)
__host__ __device__ constexpr int stream_groups(int LQ) { return LQ / 4 + 1; }             // feature groups + labels
__host__ __device__ constexpr int stream_rp(int LQ) { return 16 * stream_groups(LQ); }     // matrix row pitch, floats
__host__ __device__ constexpr int stream_wpx(int LQ)   // one wave's X' piece, = 16 (mod 32): waves 16 banks apart
{
    const int n = stream_groups(LQ) * SGP;
    return n + ((16 - n % 32) + 32) % 32;
}
// row pitches of the row-major operands: = 4 (mod 32) multiples of 4 floats, so that the 16-byte stores of a
// layer's activations / of dz_out (eight lanes = eight consecutive rows per LDS cycle) spread over all 32 banks (at
// the pitches 80 / 16 of k_train_wave they were 4-way conflicts: half of the 233 k conflict cycles per launch that
// were left after dz^T); the one-float reads of the gradient products take one row per step, lanes along it, and
// find the rows of the other lane quarter 16 banks on through the per-wave offset
constexpr int SHP = 68, SOP = 20;
constexpr int SHSZ = WB * SHP + 48;       // H [64][68], each wave's 16 rows 16 floats further on
constexpr int SZOSZ = WB * SOP + 48;      // dz_out [64][20], likewise
constexpr int SZTSZ = TBC_W * WPT;        // one layer's dz^T [64 units][68]

constexpr int SRED = 8 + 2 * 64;        // loss partials [parity][wave] | output-bias partials [parity][wave][slot]
struct StreamLds { int x, stage, h0, red, h1, zo, zt, wh, wht, idx, total, small; };
__host__ __device__ constexpr StreamLds stream_lds(int LQ, int NL)
{
    StreamLds L{};
    const int G0 = LQ / 4, NST = (G0 + 2) / 2;
    L.x = 0;
    L.stage = 4 * stream_wpx(LQ);
    const int stage_end = L.stage + 4 * G0 * 256;
    // H0 + loss partials over the first fragment groups: dead once a wave has passed the last stage barrier (every wave
    // has then issued its reads of all stages but the last, groups <= 2 (NST - 1) - 1)
    const bool alias = 2 * (NST - 1) - 1 >= (SHSZ + SRED + 1023) / 1024 - 1;
    int r = alias ? L.stage + ((SHSZ + SRED + 3) & ~3) : L.stage;   // (what follows is written behind the barrier after layer 0)
    L.h1 = r; r += (NL - 1) * SHSZ;
    L.zo = r; r += SZOSZ;
    L.zt = r; r += NL * SZTSZ;
    const int small_floats = (NL - 1) * 16 * 256;
    int total = r > stage_end ? r : stage_end;
    L.small = 0;
    if (NL > 1) {
        const int wht = r > stage_end + small_floats ? r : stage_end + small_floats;
        const int h0_extra = alias ? 0 : SHSZ + SRED;
        if ((wht + small_floats + h0_extra) * 4 <= 160 * 1024) {
            L.small = 1;
            L.wh = stage_end;
            L.wht = wht;
            total = wht + small_floats;
        }
    }
    if (alias) { L.h0 = L.stage; L.red = L.stage + SHSZ; }
    else { L.h0 = total; L.red = total + SHSZ; total += SHSZ + SRED; }
    L.idx = total; total += 256;     // the loader's landing place for the workgroup's 64 pixel indices (512 B; the request writes 1 KB)
    L.total = total;
    return L;
}

// ---- the request schedule, all of it known at compile time (the loops over stages are unrolled).  ONE wave of the
// workgroup, the fifth, does nothing but issue requests and wait for them: an LDS-DMA request costs its issuing wave
// ~60 cycles among MFMAs (35 per compute wave and step were 2 k cycles of a 35 k-cycle lifetime), and a vector-memory
// instruction of one wave issues beside another wave's MFMA.  Iteration s of the layer-0 loop consumes stage s (two
// groups: for each of the four compute waves two row requests, and the eight fragment blocks); the loader has issued
// stages 0 .. PD-1 up front (fragment blocks first: they do not wait for the pixel indices), then in iteration k the
// stage k + PD or, past the last stage, a batch of the small-matrix blocks.
__host__ __device__ constexpr int stream_row_cnt(int LQ, int s)   // row requests of stage s, per compute wave
{
    int c = 0;
    for (int g = 2 * s; g < 2 * s + 2; ++g) c += g < LQ / 4 + 1;
    return c;
}
__host__ __device__ constexpr int stream_frag_cnt(int LQ, int s)   // fragment groups of stage s (four blocks each)
{
    int c = 0;
    for (int g = 2 * s; g < 2 * s + 2; ++g) c += g < LQ / 4;
    return c;
}
__host__ __device__ constexpr int stream_small_batch(int LQ, int NL, int PD, int k)   // W_1 / W_1^T blocks issued in iteration k
{
    const int NST = (LQ / 4 + 2) / 2;
    if (!stream_lds(LQ, NL).small || k + PD < NST) return 0;
    const int nsw = (NL - 1) * 32, per = (nsw + PD - 1) / PD, done = per * (k + PD - NST);
    return done >= nsw ? 0 : (nsw - done < per ? nsw - done : per);
}
__host__ __device__ constexpr int stream_vg(int LQ, int NL, int k)   // loads to registers a compute wave issues in iteration k
{
    const int NST = (LQ / 4 + 2) / 2;
    if (stream_lds(LQ, NL).small) return k == NST - 1 ? 8 : 0;   // W_last, W_last^T
    const int nv = (NL - 1) * 32 + 8;                            // everything, dealt over the iterations
    const int per = (nv + NST - 1) / NST, done = per * k;
    return done >= nv ? 0 : (nv - done < per ? nv - done : per);
}
// N of the loader's s_waitcnt vmcnt(N) in iteration s: the requests it has issued behind the last one of stage s
// (requests complete in order).  The order is replayed here exactly as the loader issues it.
__host__ __device__ constexpr int stream_allow(int LQ, int NL, int PD, int s)
{
    const int NST = (LQ / 4 + 2) / 2;
    int total = 0, last = 0;
    for (int k = 0; k < PD && k < NST; ++k) { total += 4 * stream_frag_cnt(LQ, k); if (k == s) last = total; }
    for (int k = 0; k < PD && k < NST; ++k) { total += 4 * stream_row_cnt(LQ, k); if (k == s) last = total; }
    for (int it = 0; it < s; ++it) {
        if (it + PD < NST) {
            total += 4 * stream_row_cnt(LQ, it + PD) + 4 * stream_frag_cnt(LQ, it + PD);
            if (it + PD == s) last = total;
        } else {
            total += stream_small_batch(LQ, NL, PD, it);
        }
    }
    return total - last;
}

template <int N>
__device__ __forceinline__ void stream_wait_vm()
{
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void stream_barrier() { asm volatile("s_barrier" ::: "memory"); }
// one LDS-DMA request: 64 lanes x 16 B from per-lane global addresses to 1 KB of LDS at byte address lds_byte.
// The statement writes M0 and says so (ADVICE round 3): M0 is a reserved register for the compiler -- it is never
// allocated, the compiler writes it right in front of each instruction of its own that reads it -- but its pass that
// merges equal M0 initialisations looks at what the instructions in between define, and the clobber is what puts M0 on
// this statement's list (clang notes that a clobber of a reserved register is not a promise to preserve it: nothing
// here wants it preserved).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void stream_dma(const float* g, unsigned lds_byte)
{
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds_byte), "v"(g) : "memory", "m0");
}
// the same for 4 bytes a lane: 256 B of LDS at lds_byte
__device__ __forceinline__ void stream_dma_dword(const float* g, unsigned lds_byte)
{
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dword %1, off" ::"s"(lds_byte), "v"(g) : "memory", "m0");
}
#pragma clang diagnostic pop
template <int... Is, class F>
__device__ __forceinline__ void stream_for_impl(std::integer_sequence<int, Is...>, F&& f)
{
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void stream_for(F&& f)
{
    stream_for_impl(std::make_integer_sequence<int, N>{}, f);
}

constexpr int TAIL_PLAIN = 1;   // the last strips of the first layer's gradient whose tiles leave as plain stores (the rest written through)
constexpr int STREAM_PD = 3;    // k_train_stream's prefetch depth: stages the loader wave issues up front

constexpr int STREAM_THREADS = WAVE_THREADS + 64;   // four compute waves + the loader

// in-kernel stamps (diagnostic build): SE = the phases up to the weight-gradient barrier, SD = inside the first layer's
// weight-gradient strips (-DLBDRN_STAMP_DW: slot 0 is then the barrier, 1 = operands in registers, 2/3 4/5 6/7 = a
// strip's MFMAs / its stores)
#ifdef LBDRN_STAMP_DW
#define SE(k) do { if ((k) == 9) STAMP(0); } while (0)
#define SD(k) STAMP(k)
#else
#define SE(k) STAMP(k)
#define SD(k)
#endif

// sched_group_barrier recipe of one scheduling region: M MFMAs with R LDS reads (requested for a later region) dealt
// one behind each of the first MFMAs, then S tile stores (of the region before) spread over the rest
template <int M, int R, int S>
__device__ __forceinline__ void stream_deal()
{
    constexpr int RR = R < M ? R : M;
#pragma unroll
    for (int k = 0; k < RR; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
    }
    constexpr int left = M - RR, per = S > 0 ? (left / (S + 1) > 0 ? left / (S + 1) : 1) : 0;
#pragma unroll
    for (int k = 0; k < S; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, per, 0);
        __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);   // VMEM write
    }
    if constexpr (left - S * per > 0) __builtin_amdgcn_sched_group_barrier(0x008, left - S * per, 0);
    __builtin_amdgcn_sched_barrier(0);
}

// sums over the eight rows 2 j + h (j = 0..7) of a wave's 16, both parities at once, ONE tree for this kernel and
// k_train_split (split_sum8):  ((x7 + x6) + (x5 + x4)) + ((x3 + x2) + (x1 + x0))  over j; lanes 14 + h hold the totals.
__device__ __forceinline__ float stream_sum8(float x)
{
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x112, 0xf, 0xf, true));   // row_shr:2
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x114, 0xf, 0xf, true));   // row_shr:4
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x118, 0xf, 0xf, true));   // row_shr:8
    return x;
}
// the two chains of a weight-gradient tile -- the rows of even and of odd step (parity 0 / 1: see k_train_split) -- added
__device__ __forceinline__ f32x4 stream_join(const f32x4& even, const f32x4& odd)
{
    f32x4 g = {even[0] + odd[0], even[1] + odd[1], even[2] + odd[2], even[3] + odd[3]};
    return g;
}

// NT0C > 0: the first layer's strip count ceil(F / 16), known at compile time (the headline shapes: F = 200 -> 13,
// F = 250 -> 16; two hidden-layer networks): the weight-gradient half of the kernel is then one straight-line
// schedule (below).  NT0C == 0: any strip count, a loop.
// ACT: the hidden activation (train_act: Sine(30), or nn.ReLU -- no sines, the 1 / 0 derivative in the slot of the cosine).
template <int LQ, int NL, int PD, int NT0C, int ACT>
__global__ void __launch_bounds__(STREAM_THREADS, 1) k_train_stream(TrainArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const TrainPlan& p = A.p;
    const TrainFit& F = A.fit[blockIdx.y];   // the fits of a group step side by side: one launch, blockIdx.y = fit
    constexpr int G0 = LQ / 4, NGR = G0 + 1, NST = (NGR + 1) / 2, WPX = stream_wpx(LQ), RPM = stream_rp(LQ);
    constexpr int HP = SHP, OP = SOP, PT = WPT;
    constexpr StreamLds L = stream_lds(LQ, NL);
    constexpr bool SMALL = L.small != 0;
    constexpr int NH = (NL - 1) * 16;     // fragment blocks of the hidden layers' weights (and as many transposed)
    static_assert(L.total * 4 <= 160 * 1024, "LDS map does not fit");
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, q = lane >> 4;
    const int C = A.net.C;
    float* Xs = lds + L.x;
    const float* ST = lds + L.stage;
    float* H0 = lds + L.h0;
    float* red = lds + L.red;
    float* ZT = lds + L.zt;
    float* Zo = lds + L.zo;
    auto Hl = [&](int l) -> float* { return l == 0 ? H0 : lds + L.h1 + (size_t)(l - 1) * SHSZ; };
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) void*)lds;
    const int wg = blockIdx.x, first = wg * WB;
    const int nvalid = min(WB, A.batch_n - first);
    const int srow = 16 * w + i;
    float* slab = F.slabs + (size_t)wg * p.slab_floats;
    const WtBuf slabw(slab, (size_t)p.slab_floats * 4);
    if (w == 4) {
        // ---- the loader wave.  Lane j fetches the pixel index of the workgroup's row j (rows past the end of a short
        //      minibatch repeat its last row: finite values, masked out of the loss); request g of compute wave v's
        //      rows: lane = 4 row + quarter reads 16 B at row base + 64 g + 16 quarter.
        const float* fsrc = F.packed + p.pk_w0 + lane * 4;      // fragment block (tile t, group g) at 256 (t G0 + g)
        auto issue_frags = [&](int s) {
#pragma unroll
            for (int g = 2 * s; g < 2 * s + 2; ++g)
                if (g < G0)
#pragma unroll
                    for (int t = 0; t < 4; ++t) stream_dma(fsrc + 256 * (t * G0 + g), lds0 + 4u * (unsigned)(L.stage + (g * 4 + t) * 256));
        };
        // The pixel indices are requested first -- by LDS-DMA like everything else this wave asks for: 64 indices = 512 B, lane
        // l < 32 fetches elements 2 l, 2 l + 1 of the workgroup's rows (or the minibatch's last two, past its end), lanes
        // 32 .. 63 repeat them into the second half of the request's 1 KB -- and waited for with the fragment requests of
        // the first stages already behind them (a load the compiler knows of would be waited for with vmcnt(0): those
        // requests included; a register written by an inline-asm load -- this code until round 5 -- is written whenever the
        // data arrives, whatever the compiler has done with it meanwhile).
        if (A.batch_n >= 2) {
            const int64_t* isrc = F.perm + min(first + 2 * (lane & 31), A.batch_n - 2);
            stream_dma(reinterpret_cast<const float*>(isrc), lds0 + 4u * (unsigned)L.idx);
        } else {   // a minibatch of ONE row (the tail of an epoch of n = 1 (mod batch size) rows): its index as two 4-byte pieces,
                   // not a byte past the end of the caller's permutation (ADVICE round 5); one request either way
            stream_dma_dword(reinterpret_cast<const float*>(F.perm) + (lane & 1), lds0 + 4u * (unsigned)L.idx);
        }
        stream_for<PD>([&](auto s_) { if (decltype(s_)::value < NST) issue_frags(decltype(s_)::value); });
        {
            constexpr int up = 4 * (stream_frag_cnt(LQ, 0) + (PD > 1 ? stream_frag_cnt(LQ, 1) : 0) + (PD > 2 ? stream_frag_cnt(LQ, 2) : 0) +
                                    (PD > 3 ? stream_frag_cnt(LQ, 3) : 0));
            static_assert(PD <= 4, "prefetch depth");
            stream_wait_vm<up>();
        }
        int64_t raw;
        {   // row j of the workgroup (rows past the end of a short minibatch repeat its last row) and where its index landed
            const int g = min(first + lane, A.batch_n - 1), l = (g - first) >> 1;
            raw = reinterpret_cast<const int64_t*>(lds + L.idx)[2 * l + (g - max(min(first + 2 * l, A.batch_n - 2), 0))];
        }
        const int pix = (int)(raw < 0 ? 0 : (raw >= A.npix ? A.npix - 1 : raw));
        const float* rsrc[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) rsrc[v] = F.rows + (size_t)__shfl(pix, 16 * v + (lane >> 2)) * RPM + 4 * (lane & 3);
        auto issue_rows = [&](int s) {
#pragma unroll
            for (int g = 2 * s; g < 2 * s + 2; ++g)
                if (g < NGR)
#pragma unroll
                    for (int v = 0; v < 4; ++v) stream_dma(rsrc[v] + 16 * g, lds0 + 4u * (unsigned)(L.x + v * WPX + g * SGP));
        };
        stream_for<PD>([&](auto s_) { if (decltype(s_)::value < NST) issue_rows(decltype(s_)::value); });
        // W_l / W_l^T blocks (SMALL): block j of 2 NH goes where it is read from
        auto issue_small = [&](int k) {
            constexpr int nsw = 2 * NH, per = (nsw + PD - 1) / PD;
            const int b = k + PD - NST;
#pragma unroll
            for (int u = 0; u < per; ++u) {
                const int j = b * per + u;
                if (j < NH) stream_dma(F.packed + p.pk_wh + lane * 4 + 256 * j, lds0 + 4u * (unsigned)(L.wh + 256 * j));
                else if (j < nsw) stream_dma(F.packed + p.pk_wht + lane * 4 + 256 * (j - NH), lds0 + 4u * (unsigned)(L.wht + 256 * (j - NH)));
            }
        };
        stream_for<NST>([&](auto s_) {
            constexpr int s = decltype(s_)::value;
            stream_wait_vm<stream_allow(LQ, NL, PD, s)>();     // stage s has landed
            stream_barrier();
            if (s + PD < NST) { issue_rows(s + PD); issue_frags(s + PD); }
            else if (SMALL) issue_small(s);
        });
        stream_wait_vm<0>();   // the small matrices too
        stream_barrier();
        // This wave's work is done a quarter of the way into the kernel.  Before it goes it touches the 512 bytes it will
        // want first in the NEXT launch -- the pixel indices of the same workgroup's rows of the next minibatch (same
        // block index, so the same XCD) --: that launch opens with two dependent cold trips, indices then rows, and the
        // first one now ends in a cache.  The load's latency is nobody's: the compute waves run for another 25 k cycles.
        // (The same touch from the reduce / Adam launch: -0.65 ms per tile with four fits in flight, +3.6 ms for a fit
        // alone, whose chain waits for that launch; touching the ROWS ahead of time costs more than it returns, DESIGN 4.4.)
        if (A.next_n > 0) {
            const long long t = F.perm[A.batch_n + min(first + lane, A.next_n - 1)];
            // ... and, behind them, the head of each of those rows -- what the next launch's first stages will ask for --
            // where the host says so (touch_row_bytes of the row's 832): a fit that steps ALONE leaves the memory system
            // idle most of the time and gains 1-2 %; with several fits in flight the extra random reads cost more than
            // the shorter trip returns (58.0 -> 60.6 ms per tile), and the host asks for none
            const int touch_bytes = min(A.touch_row_bytes, RPM * 4);
            if (touch_bytes > 0) {
                const int pn = (int)(t < 0 ? 0 : (t >= A.npix ? A.npix - 1 : t));
                const float* rn = F.rows + (size_t)pn * RPM;
                // ordinary loads whose values are "used" once, behind all of them (an asm load's destination would be
                // written whenever its data arrives -- into whatever the register holds by then); offsets past the
                // requested bytes fall back onto the last requested line
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 7; ++k) acc += rn[min(128 * k, touch_bytes - 4) / 4];   // (rows are not aligned to cache lines)
                asm volatile("" ::"v"(acc));
            } else {
                asm volatile("" ::"v"(t));   // (the load has to be made; its value is not used)
            }
        }
        return;                // (a wave that has ended no longer counts at the workgroup's barriers)
    }
#ifdef LBDRN_TRAIN_STAMPS
    unsigned long long stamp[16] = {};
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp[14])::"memory");
#endif
#ifdef LBDRN_TIMELINE
    if (lane == 0 && w == 0 && wg == 0 && blockIdx.y == 0) timeline_store(A.tl, 0, false);
#endif
    SE(0);

    f32x4 bias[NL][4];
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float4 b4 = *reinterpret_cast<const float4*>(F.params + p.offB[l] + 16 * t + 4 * q);
            bias[l][t][0] = b4.x; bias[l][t][1] = b4.y; bias[l][t][2] = b4.z; bias[l][t][3] = b4.w;
        }
    f32x4 bias_last;
#pragma unroll
    for (int r = 0; r < 4; ++r) bias_last[r] = (4 * q + r) < C ? F.params[p.offB[NL] + 4 * q + r] : 0.0f;
    SE(1);

    // small matrices that stay L2 -> VGPR (fragment order): W_last and W_last^T always, the hidden layers' too where LDS
    // has no room for them (LQ = 64)
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(F.packed), (short)0,
                                                                         p.pack_floats * 4, 0x00020000);
    const int lane16 = lane * 16;
    auto ldw = [&](int float_base, int block) -> float4 {
        const v4i32 x = __builtin_amdgcn_raw_buffer_load_b128(wrs, lane16, float_base * 4 + block * 1024, 0);
        return make_float4(__int_as_float(x[0]), __int_as_float(x[1]), __int_as_float(x[2]), __int_as_float(x[3]));
    };
    float4 wh[NL > 1 ? NL - 1 : 1][4][4];    // W_l fragments [out tile][k tile]
    float4 wl[4];                            // W_last fragments [k tile]
    float4 wlt[4];                           // W_last^T [hidden tile]
    float4 wht[NL > 1 ? NL - 1 : 1][4][4];   // W_l^T [in tile][out tile]
    auto vg_load = [&](int j) {   // j-th register load of the list: (W_l, W_l^T unless SMALL), W_last, W_last^T
        constexpr int NHV = SMALL ? 0 : NH;
        if (j < NHV) wh[j / 16][(j >> 2) & 3][j & 3] = ldw(p.pk_wh, j);
        else if (j < 2 * NHV) { const int k = j - NHV; wht[k / 16][(k >> 2) & 3][k & 3] = ldw(p.pk_wht, k); }
        else if (j < 2 * NHV + 4) wl[j - 2 * NHV] = ldw(p.pk_wl, j - 2 * NHV);
        else if (j < 2 * NHV + 8) wlt[j - 2 * NHV - 4] = ldw(p.pk_wlt, j - 2 * NHV - 4);
    };

    // ---- layer 0 under the stream: z^T[64 units][16 samples] = b0 + W0 X^T, lane quarter q walks k = q LQ + 4 g + e.
    //      Group g: four fragment blocks (one per unit tile) + this wave's X' piece of the group, five ds_read_b128
    //      requested one group ahead of their 16 MFMAs and dealt out among the previous group's.
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = bias[0][t];
    {
        const float* wbase = ST + lane * 4;
        const float* xbase = Xs + w * WPX + (i * 4 + q) * 4;
        float4 aq[2][4], bq[2];
        auto reads = [&](int g) {
#pragma unroll
            for (int t = 0; t < 4; ++t) aq[g & 1][t] = *reinterpret_cast<const float4*>(wbase + (g * 4 + t) * 256);
            bq[g & 1] = *reinterpret_cast<const float4*>(xbase + g * SGP);
        };
        auto mfmas = [&](int g) {
            const float bx[4] = {bq[g & 1].x, bq[g & 1].y, bq[g & 1].z, bq[g & 1].w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float4 x = aq[g & 1][t];
                    acc[t] = MFMA16(e == 0 ? x.x : e == 1 ? x.y : e == 2 ? x.z : x.w, bx[e], acc[t]);
                }
        };
        int vgj = 0;
        stream_for<NST>([&](auto s_) {
            constexpr int s = decltype(s_)::value;
            stream_barrier();                                  // the loader has seen stage s land
#ifdef LBDRN_TRAIN_STAMPS
            if (s == 0) { SE(1); SE(2); }
#endif
#pragma unroll
            for (int u = 0; u < stream_vg(LQ, NL, s); ++u) vg_load(vgj + u);
            vgj += stream_vg(LQ, NL, s);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 2 * s; g < 2 * s + 2; ++g)
                if (g < G0) {
                    reads(g);
                    if (g > 0) {
                        mfmas(g - 1);
#pragma unroll
                        for (int k = 0; k < 5; ++k) {
                            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
                            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);   // MFMA
                        }
                        __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
        });
        mfmas(G0 - 1);
        __builtin_amdgcn_sched_barrier(0);
    }
    SE(3);
    float h[4][4];        // the current layer's activations, accumulator layout
    f32x4 cs[NL][4];      // cos(30 z) of every hidden layer, for the backward pass
    auto activate_tile = [&](int l, int t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float sn, co;
            train_act<ACT>(acc[t][r], sn, co);
            h[t][r] = sn;
            cs[l][t][r] = co;
        }
        *reinterpret_cast<float4*>(Hl(l) + srow * HP + 16 * w + 16 * t + 4 * q) = make_float4(h[t][0], h[t][1], h[t][2], h[t][3]);
    };
    auto activate = [&](int l) {
#pragma unroll
        for (int t = 0; t < 4; ++t) activate_tile(l, t);
    };
    // the first half of the activation needs nothing from memory: it runs while the last requests (the small matrices)
    // land.  (H0 goes over fragment groups every wave has read: see stream_lds.)
    activate_tile(0, 0);
    activate_tile(0, 1);
    __builtin_amdgcn_sched_barrier(0);
    // every request has landed and every wave is through layer 0: the small matrices are in LDS, the fragment space is dead
    stream_barrier();
    SE(4);
    if constexpr (SMALL) {   // requested here, they arrive under the second half of the activation
#pragma unroll
        for (int l = 1; l < NL; ++l)
#pragma unroll
            for (int j = 0; j < 16; ++j)
                wh[l - 1][j >> 2][j & 3] = *reinterpret_cast<const float4*>(lds + L.wh + ((l - 1) * 16 + j) * 256 + lane * 4);
    }
    activate_tile(0, 2);
    activate_tile(0, 3);
    SE(5);

    // ---- hidden layers: B = the activations where they stand (step (tk, r) multiplies unit 16 tk + 4 q + r).  (Two passes
    //      of two unit tiles with the first pass's sin / cos under the second's MFMAs -- what k_train_half gains 2.7 % from
    //      at bc = 256 -- were built here too: the phase came out 100 cycles longer by the stamps, the tile the same.)
#pragma unroll
    for (int l = 1; l < NL; ++l) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = bias[l][t];
#pragma unroll
        for (int tk = 0; tk < 4; ++tk) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int to = 0; to < 4; ++to) {
                    const float4 x = wh[l - 1][to][tk];
                    const float a = r == 0 ? x.x : r == 1 ? x.y : r == 2 ? x.z : x.w;
                    acc[to] = MFMA16(a, h[tk][r], acc[to]);
                }
        }
        if constexpr (SMALL) {
            if (l == NL - 1) {   // every wave has its W_l fragments in registers: dz^T may run over them from here on
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                stream_barrier();
            }
        }
        activate(l);
    }
    if constexpr (SMALL) {   // W_l^T out of LDS while the output layer and the loss run
#pragma unroll
        for (int l = 1; l < NL; ++l)
#pragma unroll
            for (int j = 0; j < 16; ++j)
                wht[l - 1][j >> 2][j & 3] = *reinterpret_cast<const float4*>(lds + L.wht + ((l - 1) * 16 + j) * 256 + lane * 4);
    }
    SE(6);

    // ---- output layer (two accumulators share the 16-step chain) + loss + d(loss)/dz_out
    float dzo[4];
    {
        f32x4 oe = bias_last, oo = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tk = 0; tk < 4; ++tk) {
            const float4 x = wl[tk];
            oe = MFMA16(x.x, h[tk][0], oe);
            oo = MFMA16(x.y, h[tk][1], oo);
            oe = MFMA16(x.z, h[tk][2], oe);
            oo = MFMA16(x.w, h[tk][3], oo);
        }
        const bool live = srow < nvalid;
        // labels: the last group of the row, lane (row i, quarter q) holds channels 4 q .. 4 q + 3
        const float4 lab = *reinterpret_cast<const float4*>(Xs + w * WPX + G0 * SGP + (i * 4 + q) * 4);
        const float labv[4] = {lab.x, lab.y, lab.z, lab.w};
        float lsum = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool ok = live && (4 * q + r) < C;
            const float y = train_sigmoid(oe[r] + oo[r]);
            const float d = y - ((4 * q + r) < C ? labv[r] : 0.0f);
            lsum += ok ? d * d : 0.0f;                                      // ref LBDRNloss.py:9
            dzo[r] = ok ? ((2.0f * d) * A.inv) * (y * (1.0f - y)) : 0.0f;    // mse + sigmoid backward
        }
        *reinterpret_cast<float4*>(Zo + srow * OP + 16 * w + 4 * q) = make_float4(dzo[0], dzo[1], dzo[2], dzo[3]);
        // Sums over samples are taken per PARITY of the row (the summation tree this kernel shares with k_train_split,
        // train_split.inc: the rows of parity h of a 64-row group are what workgroup 2 G + h of that kernel holds): the eight
        // rows 2 j + h of this wave in one fixed tree, then the four channel quarters (0 + 1) + (2 + 3); the waves' partials
        // meet in double, parity 0 plus parity 1.  32 terms in float32 (1e-7 relative).
        {
            const int li = __float_as_int(stream_sum8(lsum));
            auto rl = [&](int l) { return __int_as_float(__builtin_amdgcn_readlane(li, l)); };
            const float l0 = (rl(14) + rl(30)) + (rl(46) + rl(62)), l1 = (rl(15) + rl(31)) + (rl(47) + rl(63));
            if (lane == 0) { red[w] = l0; red[4 + w] = l1; }
        }
        // output-bias gradient of this wave's rows of either parity: lanes 14 / 15 of quarter q hold channels 4q..4q+3
        float bs[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) bs[r] = stream_sum8(dzo[r]);
        if (i >= 14) *reinterpret_cast<float4*>(red + 8 + 64 * (i - 14) + 16 * w + 4 * q) = make_float4(bs[0], bs[1], bs[2], bs[3]);
    }
    SE(7);

    // ---- backward: dh = W^T dz, dz = (dh * cos(30 z)) * 30, layer by layer, still wave-local.  dz is parked transposed,
    //      [unit][sample], samples in order: for one register the 16 lanes of a quarter write 16 consecutive floats and
    //      the quarters sit 4 rows = 16 banks apart
    float dz[4][4];
    auto backprop = [&](int l) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dz[t][r] = train_act_back<ACT>(acc[t][r], cs[l][t][r]);
                ZT[(size_t)l * SZTSZ + (16 * t + 4 * q + r) * PT + srow] = dz[t][r];
            }
    };
    {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = zero;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float4 x = wlt[t];
                const float a = s == 0 ? x.x : s == 1 ? x.y : s == 2 ? x.z : x.w;
                acc[t] = MFMA16(a, dzo[s], acc[t]);
            }
        backprop(NL - 1);
    }
    // ---- weight gradients: K = the 64 samples (16 steps; lane quarter q, step j = sample 16 q + j: wave q's row j).
    //      dW[unit tile t][input strip nt]: A = dz^T rows of tile t (16 contiguous floats per lane), B = the inputs,
    //      one float per lane and step.  Wave w takes the strips nt = w, w+4, .. of the first layer against all four
    //      unit tiles (64 MFMAs on four independent accumulators per 16 reads); the strips left over when the strip
    //      count is not a multiple of 4 go one tile to each wave; strip w of the hidden layers; tile w of the output
    //      layer.  Every finished tile leaves as one 1 KB store in the slab's tile order.
    auto ldrow = [&](const float* row, float (&dst)[16]) {   // 16 contiguous floats of a 16-byte aligned row piece
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 x = *reinterpret_cast<const float4*>(row + 4 * g);
            dst[4 * g] = x.x; dst[4 * g + 1] = x.y; dst[4 * g + 2] = x.z; dst[4 * g + 3] = x.w;
        }
    };
    auto ldx = [&](int nt, float (&dst)[16]) {   // feature 16 nt + i of wave q's 16 rows, out of X'
        const int f = 16 * nt + i;
        const int kq = f / LQ, fl = f - kq * LQ;
        const float* base = Xs + q * WPX + (fl >> 2) * SGP + kq * 4 + (fl & 3);
#pragma unroll
        for (int s = 0; s < 16; ++s) dst[s] = base[16 * s];
    };
    auto ldh = [&](const float* H, int strip, float (&dst)[16]) {   // unit 16 strip + i of wave q's 16 rows
        const float* base = H + (16 * q) * HP + 16 * q + 16 * strip + i;
#pragma unroll
        for (int s = 0; s < 16; ++s) dst[s] = base[s * HP];
    };
    auto put = [&](int off, const f32x4& g, bool early) {
        if (early) slabw.store(off + lane * 4, g[0], g[1], g[2], g[3]);
        else slabw.store_plain(off + lane * 4, g[0], g[1], g[2], g[3]);
    };
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    if constexpr (NT0C > 0) {
        // ---- the straight-line weight-gradient schedule (NL == 2, NT0C strips of the first layer).  What it buys over
        //      the loop (in-kernel stamps, cycles per wave): the operands of the first products used to arrive after
        //      the barrier with nothing to do meanwhile (1.0 k); every strip paid 16 register copies and its index
        //      arithmetic (0.4 k each), and the tail's 52 reads rode in the last strip (0.8 k); four 1 KB tile stores
        //      in a row stalled the wave at the end of every strip (0.25 k each); the bias sums re-read dz^T from
        //      LDS (0.7 k).  Here: TWO barriers -- behind dz_1^T (the hidden layer's backward product then covers
        //      the first operand requests) and behind dz_0^T (the small products cover the strips' operand
        //      requests) --, every region's reads and the previous region's stores dealt out between its MFMAs,
        //      accumulators double-buffered, bias sums taken from the A operands where they sit in registers.
        static_assert(NL == 2, "the straight-line schedule is written for two hidden layers");
        constexpr int NFS = NT0C / 4, REM = NT0C % 4;   // full strips per wave; left-over strips (one tile per wave)
        static_assert(NFS >= 1 && NFS <= 4 && REM <= 2, "strip counts of the shapes this is instantiated for");
        // the B operands of the first layer's products, in the order they are consumed: item n < NFS = strip w + 4 n (bb[n]),
        // item NFS + r = left-over strip 4 NFS + r (br[r]); item n is requested two regions ahead of its MFMAs
        constexpr int NIT = NFS + REM;
        const float* ZT1 = ZT + SZTSZ;
        __syncthreads();   // dz_1^T, H0, H1, dz_out of every wave are in LDS
        float ao[16], bo[16], bh[16], a1[4][16];
        {
            const float* base = Zo + (16 * q) * OP + 16 * q + i;
#pragma unroll
            for (int s = 0; s < 16; ++s) ao[s] = base[s * OP];
        }
        ldh(Hl(1), w, bo);
        ldh(Hl(0), w, bh);
        ldrow(ZT1 + (0 + i) * PT + 16 * q, a1[0]);
        ldrow(ZT1 + (16 + i) * PT + 16 * q, a1[1]);
        {   // backward through the hidden layer, the 56 requests above dealt out between its 64 MFMAs
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = zero;
#pragma unroll
            for (int to = 0; to < 4; ++to)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int ti = 0; ti < 4; ++ti) {
                        const float4 x = wht[0][ti][to];
                        const float a = r == 0 ? x.x : r == 1 ? x.y : r == 2 ? x.z : x.w;
                        acc[ti] = MFMA16(a, dz[to][r], acc[ti]);
                    }
            stream_deal<64, 56, 0>();
            backprop(0);
        }
        SE(8);
        __syncthreads();   // dz_0^T of every wave is in LDS
        if (tid == 0) F.loss_part[wg] = (((double)red[0] + (double)red[1]) + ((double)red[2] + (double)red[3])) +
                                        (((double)red[4] + (double)red[5]) + ((double)red[6] + (double)red[7]));
        SE(9);
        float az[4][16], azw[16], a1w[16], bb[NFS][16], br[REM > 0 ? REM : 1][16];
        auto item = [&](auto n_) {
            constexpr int n = decltype(n_)::value;
            if constexpr (n < NFS) ldx(w + 4 * n, bb[n]);
            else if constexpr (n < NIT) ldx(4 * NFS + (n - NFS), br[n - NFS]);
        };
        // region 1: tile w of the output layer + unit tiles 0, 1 of the hidden layer (48 MFMAs); requested meanwhile:
        // the other two dz_1^T tiles, the four dz_0^T tiles, the first strip of the rows (40 reads)
        ldrow(ZT1 + (32 + i) * PT + 16 * q, a1[2]);
        ldrow(ZT1 + (48 + i) * PT + 16 * q, a1[3]);
#pragma unroll
        for (int t = 0; t < 4; ++t) ldrow(ZT + (16 * t + i) * PT + 16 * q, az[t]);
        item(std::integral_constant<int, 0>{});
        // (every chain in two accumulators, even and odd steps = rows of parity 0 / 1, joined when the tile leaves)
        f32x4 go[2] = {zero4, zero4}, g1[4][2] = {{zero4, zero4}, {zero4, zero4}, {zero4, zero4}, {zero4, zero4}};
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            go[s & 1] = MFMA16(ao[s], bo[s], go[s & 1]);
            g1[0][s & 1] = MFMA16(a1[0][s], bh[s], g1[0][s & 1]);
            g1[1][s & 1] = MFMA16(a1[1][s], bh[s], g1[1][s & 1]);
        }
        stream_deal<48, 40, 0>();
        // region 2: unit tiles 2, 3 of the hidden layer (32 MFMAs); requested: the second strip, this wave's own tile
        // of both dz^T (bias sums, left-over strip: 24 reads); stored: region 1's three tiles
        item(std::integral_constant<int, 1>{});
        ldrow(ZT + (16 * w + i) * PT + 16 * q, azw);
        ldrow(ZT1 + (16 * w + i) * PT + 16 * q, a1w);
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            g1[2][s & 1] = MFMA16(a1[2][s], bh[s], g1[2][s & 1]);
            g1[3][s & 1] = MFMA16(a1[3][s], bh[s], g1[3][s & 1]);
        }
        put(p.sl_out + w * 256, stream_join(go[0], go[1]), true);
        put(p.sl_hid + (0 * 4 + w) * 256, stream_join(g1[0][0], g1[0][1]), true);
        put(p.sl_hid + (1 * 4 + w) * 256, stream_join(g1[1][0], g1[1][1]), true);
        stream_deal<32, (NIT > 1 ? 24 : 8), 3>();
        SD(1);
        // the first layer's strips nt = w + 4 k, 64 MFMAs each against the four dz_0^T tiles; strip k's region requests
        // strip k + 2 (or the left-over strip) and stores strip k - 1's tiles (the first: the hidden layer's last two)
        f32x4 gs[2][4][2];
        stream_for<NFS>([&](auto k_) {
            constexpr int k = decltype(k_)::value;
#pragma unroll
            for (int t = 0; t < 4; ++t) gs[k & 1][t][0] = gs[k & 1][t][1] = zero4;
            constexpr int nreads = k + 2 < NIT ? 16 : 0;
            item(std::integral_constant<int, k + 2>{});
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int t = 0; t < 4; ++t) gs[k & 1][t][s & 1] = MFMA16(az[t][s], bb[k][s], gs[k & 1][t][s & 1]);
            if constexpr (k == 0) {
                put(p.sl_hid + (2 * 4 + w) * 256, stream_join(g1[2][0], g1[2][1]), true);
                put(p.sl_hid + (3 * 4 + w) * 256, stream_join(g1[3][0], g1[3][1]), true);
                stream_deal<64, nreads, 2>();
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    put((t * NT0C + w + 4 * (k - 1)) * 256, stream_join(gs[(k - 1) & 1][t][0], gs[(k - 1) & 1][t][1]), k - 1 < NFS - TAIL_PLAIN);
                stream_deal<64, nreads, 4>();
            }
#ifdef LBDRN_STAMP_DW
            if (k == 0) { SD(2); stamp[3] = stamp[2]; } else if (k == 1) { SD(4); stamp[5] = stamp[4]; } else if (k == 2) { SD(6); stamp[7] = stamp[6]; }
#endif
        });
        // the left-over strips (tile w of each) and the bias sums, under which the last strip's tiles leave
        f32x4 grem[REM > 0 ? REM : 1][2];
#pragma unroll
        for (int r = 0; r < (REM > 0 ? REM : 1); ++r) grem[r][0] = grem[r][1] = zero4;
        if constexpr (REM > 0) {
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int r = 0; r < REM; ++r) grem[r][s & 1] = MFMA16(azw[s], br[r][s], grem[r][s & 1]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            put((t * NT0C + w + 4 * (NFS - 1)) * 256, stream_join(gs[(NFS - 1) & 1][t][0], gs[(NFS - 1) & 1][t][1]), false);   // (written through, the last tiles cost +1 ms per tile: measured)
        stream_deal<REM * 16, 0, 4>();
        // bias gradients: sums over the 64 samples of this wave's 16 units of either layer, out of the A operands:
        // lane (unit i, quarter q) holds wave q's 16 samples; per parity of the step (the rows of k_train_split's two
        // workgroups) in step order, quarters summed (0 + 1) + (2 + 3) on every lane, parity 0 plus parity 1
        {
            float s0[2] = {0.f, 0.f}, s1[2] = {0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 16; ++s) { s0[s & 1] += azw[s]; s1[s & 1] += a1w[s]; }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                s0[h] += __shfl_xor(s0[h], 16); s1[h] += __shfl_xor(s1[h], 16);
                s0[h] += __shfl_xor(s0[h], 32); s1[h] += __shfl_xor(s1[h], 32);
            }
            if (lane < 16) {
                slab[p.sl_bias + 16 * w + lane] = s0[0] + s0[1];
                slab[p.sl_bias + TBC_W + 16 * w + lane] = s1[0] + s1[1];
            }
        }
        if constexpr (REM > 0) {
#pragma unroll
            for (int r = 0; r < REM; ++r) put((w * NT0C + 4 * NFS + r) * 256, stream_join(grem[r][0], grem[r][1]), false);
        }
#ifdef LBDRN_STAMP_DW
        SD(8); stamp[9] = stamp[8];
#endif
        STAMP(10); STAMP(11);
        if (w == 3 && lane < 16)   // output slots: the four waves' partials (loss phase), in wave order
            slab[p.sl_bias + NL * TBC_W + lane] = ((red[8 + lane] + red[24 + lane]) + (red[40 + lane] + red[56 + lane])) +
                                                  ((red[72 + lane] + red[88 + lane]) + (red[104 + lane] + red[120 + lane]));
    } else {
    #pragma unroll
        for (int l = NL - 1; l >= 1; --l) {
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    #pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = zero;
    #pragma unroll
            for (int to = 0; to < 4; ++to)
    #pragma unroll
                for (int r = 0; r < 4; ++r)
    #pragma unroll
                    for (int ti = 0; ti < 4; ++ti) {
                        const float4 x = wht[l - 1][ti][to];
                        const float a = r == 0 ? x.x : r == 1 ? x.y : r == 2 ? x.z : x.w;
                        acc[ti] = MFMA16(a, dz[to][r], acc[ti]);
                    }
            backprop(l - 1);
        }
        SE(8);
        __syncthreads();
        if (tid == 0) F.loss_part[wg] = (((double)red[0] + (double)red[1]) + ((double)red[2] + (double)red[3])) +
                                        (((double)red[4] + (double)red[5]) + ((double)red[6] + (double)red[7]));
        SE(9);

        const int NT0 = p.NT0, NF = NT0 & ~3, rem = NT0 - NF;
        float az[4][16], b[16], bn[16];
    #pragma unroll
        for (int t = 0; t < 4; ++t) ldrow(ZT + (16 * t + i) * PT + 16 * q, az[t]);
        ldx(min(w, NT0 - 1), b);
        __builtin_amdgcn_sched_barrier(0);
        SD(1);
        [[maybe_unused]] int strips_done = 0;
        auto strip = [&](int nt, int nreads) {   // 64 MFMAs of strip nt (operands in az, b), four 1 KB tile stores; the
            f32x4 g[4] = {zero4, zero4, zero4, zero4};   // nreads LDS reads requested just before are dealt out between them
    #pragma unroll
            for (int s = 0; s < 16; ++s)
    #pragma unroll
                for (int t = 0; t < 4; ++t) g[t] = MFMA16(az[t][s], b[s], g[t]);
            if (nreads <= 16) {
    #pragma unroll
                for (int k = 0; k < 16; ++k) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
            } else {
    #pragma unroll
                for (int k = 0; k < 52; ++k) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
    #ifdef LBDRN_STAMP_DW
            if (strips_done == 0) SD(2); else if (strips_done == 1) SD(4); else SD(6);
    #endif
    #pragma unroll
            for (int t = 0; t < 4; ++t) put((t * NT0 + nt) * 256, g[t], true);
    #ifdef LBDRN_STAMP_DW
            if (strips_done == 0) SD(3); else if (strips_done == 1) SD(5); else { SD(7); stamp[8] = stamp[7]; stamp[9] = stamp[7]; }
    #endif
            ++strips_done;
        };
        int nt = w;
        for (; nt + 4 < NF; nt += 4) {   // operands of the strip after this one arrive under its MFMAs
            ldx(nt + 4, bn);
            strip(nt, 16);
    #pragma unroll
            for (int s = 0; s < 16; ++s) b[s] = bn[s];
        }
        // left-over strips of the first layer (tile w of each) and tile w of the output layer: operands requested under
        // the last full strip.  dW_last[channel slot][hidden 16w..] = sum_s dzo[s][slot] * h_last[s][16w + col]
        float azw[16], ao[16], bo[16], br[16];
        ldrow(ZT + (16 * w + i) * PT + 16 * q, azw);
        {
            const float* base = Zo + (16 * q) * OP + 16 * q + i;
    #pragma unroll
            for (int s = 0; s < 16; ++s) ao[s] = base[s * OP];
        }
        ldh(Hl(NL - 1), w, bo);
        ldx(min(NF, NT0 - 1), br);
        if (nt < NF) strip(nt, 52);
        __builtin_amdgcn_sched_barrier(0);
        STAMP(10);
        // hidden layers' operands (strip w of H_{l-1}, the four unit tiles of dz_l): requested under the tail's MFMAs
        float a1[NL > 1 ? NL - 1 : 1][4][16], bh[NL > 1 ? NL - 1 : 1][16];
    #pragma unroll
        for (int l = 1; l < NL; ++l) {
    #pragma unroll
            for (int t = 0; t < 4; ++t) ldrow(ZT + (size_t)l * SZTSZ + (16 * t + i) * PT + 16 * q, a1[l - 1][t]);
            ldh(Hl(l - 1), w, bh[l - 1]);
        }
        {
            f32x4 go = zero4, g0 = zero4;
    #pragma unroll
            for (int s = 0; s < 16; ++s) {
                go = MFMA16(ao[s], bo[s], go);
                g0 = MFMA16(azw[s], br[s], g0);
            }
    #pragma unroll
            for (int k = 0; k < 32; ++k) {   // the hidden layers' 32 operand reads, one after every MFMA of the tail
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            put(p.sl_out + w * 256, go, false);
            if (rem >= 1) put((w * NT0 + NF) * 256, g0, false);
        }
        for (int k = 1; k < rem; ++k) {   // (strip counts 4n+2, 4n+3: rare shapes, one plain chain per extra strip)
            ldx(NF + k, br);
            f32x4 g1 = zero4;
    #pragma unroll
            for (int s = 0; s < 16; ++s) g1 = MFMA16(azw[s], br[s], g1);
            put((w * NT0 + NF + k) * 256, g1, false);
        }
    #pragma unroll
        for (int l = 1; l < NL; ++l) {
            f32x4 g[4] = {zero4, zero4, zero4, zero4};
    #pragma unroll
            for (int s = 0; s < 16; ++s)
    #pragma unroll
                for (int t = 0; t < 4; ++t) g[t] = MFMA16(a1[l - 1][t][s], bh[l - 1][s], g[t]);
            __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
            for (int t = 0; t < 4; ++t) put(p.sl_hid + ((l - 1) * 16 + t * 4 + w) * 256, g[t], false);
        }
        STAMP(11);
        // bias gradients: sums over the 64 samples.  Hidden units: a row of dz^T, two threads per unit (32 columns
        // each, partner = lane ^ 1, summed low half first); output slots: a column of dz_out on the last wave.
        if (tid < NL * TBC_W * 2) {
            const int u = tid >> 1, half = tid & 1;
            const float* row = ZT + (size_t)(u >> 6) * SZTSZ + (u & 63) * PT + 32 * half;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    #pragma unroll
            for (int g = 0; g < 8; ++g) {
                const float4 x = *reinterpret_cast<const float4*>(row + 4 * g);
                s0 += x.x; s1 += x.y; s2 += x.z; s3 += x.w;
            }
            const float mine = (s0 + s1) + (s2 + s3);
            const float other = __shfl_xor(mine, 1);
            if (half == 0) slab[p.sl_bias + u] = mine + other;
        }
        if (w == 3 && lane < 16)   // output slots: the four waves' partials (loss phase), in wave order
            slab[p.sl_bias + NL * TBC_W + lane] = ((red[8 + lane] + red[24 + lane]) + (red[40 + lane] + red[56 + lane])) +
                                                  ((red[72 + lane] + red[88 + lane]) + (red[104 + lane] + red[120 + lane]));
    }
    STAMP(12);
#ifdef LBDRN_TIMELINE
    if (lane == 0 && blockIdx.y == 0) timeline_store(A.tl, 2 + wg * 4 + w, true);
#endif
#ifdef LBDRN_TRAIN_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(13);
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp[15])::"memory");
    if (lane == 0 && A.stamps)
        for (int k = 0; k < 16; ++k) A.stamps[(((size_t)blockIdx.y * gridDim.x + wg) * 4 + w) * 16 + k] = stamp[k];
#endif
}
