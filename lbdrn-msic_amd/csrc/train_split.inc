// k_train_split: the bc = 64 training step of a fit that has the device to itself, on EVERY CU (round 5; ref
// modified_ignite_engine.py:18-27, LBDRNmodel.py:62-77; LBDRNdataset.py:151-155 for the gather).
//
// k_train_stream puts a minibatch of 8192 rows on 128 workgroups of 64 rows: one per CU on HALF of the chip -- the right
// shape when another fit's launch holds the other half, and 14.9 us of a 21.4 us step when nothing else is in flight
// (what every `encode.py -sr 1` call runs).  Here the minibatch is 256 workgroups of 32 rows, and -- as in k_train_half
// at bc = 256 -- the units of every layer are halved between two waves: a workgroup is two sample tiles x two UNIT
// HALVES, wave (s, u) computes unit tiles 2u, 2u + 1 of every layer for the 16 samples of tile s.  Per wave 320 MFMAs
// instead of 624 and half of the sines.  What a product needs from the other half of the units crosses LDS (h_0, h_1, dz_1:
// [sample][unit] rows, written and read back as the 16-byte pieces that ARE an accumulator tile / the B operand of a step).
//
// Ingest.  A 32-row workgroup needs the same 88 KB of weight fragments as a 64-row one, and a CU takes in 64 bytes per
// clock: every byte is requested ONCE per workgroup, by LDS-DMA, the four waves sharing the requests (the first version
// loaded each wave's operands straight into its registers: 241 KB per CU, 8.5 k cycles before the first MFMA -- and 1024
// waves asking a cold L2 for the same lines right behind the reduce / Adam launch that rewrote them).  Two landing
// phases under counted waits (requests complete in order): the first half of W_0 and of the rows, then the rest; the
// small matrices land under layer 0.  No loader wave: at the head of the kernel the compute waves have nothing else to do.
//
// THE SAME BITS AS k_train_stream.  Which of the two kernels runs a step is a matter of what else is in flight, so it
// must not show in a single number (VERDICT round 4).  Everything per sample is the same arithmetic in the same order
// (a unit's dot product stays in one wave: k ascending as before).  What sums over samples is defined ONCE, for both:
//   * rows of the 64-row group G:  rho = 16 q + 2 j + h  (q = 0..3 lane quarter of the gradient products, j = 0..7 MFMA
//     step, h = parity).  The weight gradient of the group is  dW_G = chain_0 + chain_1,  chain_h = the 8-step MFMA chain
//     over j of the rows of parity h (a 16x16x4 MFMA adds its four k slots in quarter order).  k_train_stream runs its 16
//     steps into two accumulators (even / odd steps) and adds them; here workgroup 2 G + h gathers the rows of parity h
//     and writes chain_h as its slab; k_reduce_adam adds the two slabs of a group first, then the groups in its fixed order;
//   * bias gradients and the loss partials the same way: parity h first (sums over j in one fixed tree, then over q as
//     (0 + 1) + (2 + 3)), then h = 0 plus h = 1.
// So lane i of sample tile s holds row  rho = 16 (2 s + qb) + 2 j + h  with  qb = (i >> 2) & 1,  j = (i & 3) + 4 (i >> 3):
// quarter q of a gradient product's step j then reads sample row (j & 3) + 4 (q & 1) + 8 (j >> 2) of tile q >> 1 -- rows of
// quarters 0 / 1 four rows = 16 banks apart at the row pitches used here (= 4 mod 32).
constexpr int SPB = 32;             // rows per workgroup
constexpr int SP_HP = 68;           // [sample][64 units] pitch of H_0, H_1 and the dz_1 exchange (= 4 mod 32)
constexpr int SP_OP = 20;           // [sample][16 channel slots] pitch of dz_out
constexpr int SP_PT = 36;           // [unit][32 samples] pitch of the transposed dz copies
constexpr int SP_SM = 40;           // 1 KB blocks of the small matrices: W_1 [16] | W_1^T [16] | W_last [4] | W_last^T [4]

// The wide-window shape: LQ = 96, 384 features (D = 3 windows on 8 bands with relative colours; 6 and 7 bands pad to it).
// All 24 W_0 fragment groups (96 KB) and the rows (51 KB) do not fit beside each other, so W_0 passes through a RING of
// SP_RING groups (48 KB), two halves of SP_RING / 2 groups each: quarter Q of W_0 (groups 6 Q .. 6 Q + 5) lands in half
// Q mod 2.  Quarters 0 and 1 land with the rows; quarter 2 is requested once every wave is past group 5 (a barrier at the
// top of layer 0's iteration 7: a wave's MFMAs of group g, which wait for its reads of group g, issue in iteration g + 1),
// quarter 3 once every wave is past group 11 (iteration 13); each is waited for where its first group is read (12, 18).
// The rows stay resident for dW_0.  The arithmetic is k_train_split's, unchanged: only where W_0 sits differs.
constexpr int SP_RING = 12;
__host__ __device__ constexpr bool split_ring(int LQ) { return LQ > 64; }
__host__ __device__ constexpr int split_w0_groups(int LQ) { return split_ring(LQ) ? SP_RING : LQ / 4; }   // W_0 groups resident at once
// small-matrix requests a wave has issued by the end of layer 0's iteration k (SPI per iteration from iteration 1 on)
__host__ __device__ constexpr int split_small_through(int k, int SPI) { return k * SPI < SP_SM / 4 ? k * SPI : SP_SM / 4; }

// LDS map (floats).  W_0 fragments [G0 groups][4 tiles][256] -- dead behind the barrier after layer 0, where H_1, the dz_1
// exchange, dz_out and both dz^T move in --; the small matrices; the rows X' [2 sample tiles][G0 + 1 groups][260] as the
// requests land them (lane-linear 1 KB pieces, group g 4 banks on; the labels are the last group); H_0; the partials.
struct SplitLds { int w0, sm, x, xt, h0, red, idx, bias, h1, e, zo, zt, total; };
__host__ __device__ constexpr SplitLds split_lds(int LQ)
{
    SplitLds L{};
    const int G0 = LQ / 4, RG = split_w0_groups(LQ);
    int o = 0;
    const int over = 2 * SPB * SP_HP + SPB * SP_OP + 2 * 64 * SP_PT;   // what moves in over the W_0 fragments behind layer 0
    L.w0 = o; o += RG * 4 * 256 > over ? RG * 4 * 256 : over;         // (LQ < 40: the region is as large as its second life needs it)
    L.sm = o; o += SP_SM * 256;
    L.xt = (G0 + 1) * SGP + 16;      // one sample tile's piece
    L.x = o; o += 2 * L.xt;
    L.h0 = o; o += SPB * SP_HP;
    L.red = o; o += 4 + 4 * 16 + 12; // loss partials of the four row quarters | output-bias partials [row quarter][slot] | pad to 16 B
    L.idx = o; o += 4 * 256;         // per wave: the 64 pixel indices of the group (512 B; the request writes 1 KB)
    L.bias = o; o += 4 * 64;         // b_0 | b_1 | b_last | (wave 3's request: b_last again)
    L.total = o;
    int a = L.w0;                    // over the W_0 fragments
    L.h1 = a; a += SPB * SP_HP;
    L.e = a; a += SPB * SP_HP;
    L.zo = a; a += SPB * SP_OP;
    L.zt = a; a += 2 * 64 * SP_PT;
    if (a > L.sm) L.total = -1;      // (cannot happen: see `over`)
    return L;
}

// sums over the eight rows (j = 0..7) of one row quarter and parity, ONE tree for both kernels:
//   ((x7 + x6) + (x5 + x4)) + ((x3 + x2) + (x1 + x0)).
// Here row j of quarter half qb sits in lane (j & 3) + 4 qb + 8 (j >> 2) of a 16-lane row: lanes 11 (qb = 0) and 15 (qb = 1)
// hold the totals.  (k_train_stream: row j of parity h sits in lane 2 j + h, totals in lanes 14 + h: stream_sum8.)
__device__ __forceinline__ float split_sum8(float x)
{
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x111, 0xf, 0xf, true));   // row_shr:1
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x112, 0xf, 0xf, true));   // row_shr:2
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x118, 0xf, 0xf, true));   // row_shr:8
    return x;
}
// where sample row r of a tile sits in a landed piece of X' (bits 0 and 2 swapped: the rows a gradient product's lane
// quarters 0 / 1 read in one step are four apart, and land one slot = 16 banks apart)
__host__ __device__ constexpr int split_slot(int r) { return (r & ~5) | ((r & 1) << 2) | ((r >> 2) & 1); }

// row groups g in [lo, hi) that the wave of unit half u requests (g = u mod 2)
__host__ __device__ constexpr int split_row_requests(int lo, int hi, int u)
{
    int c = 0;
    for (int g = lo; g < hi; ++g) c += (g & 1) == u;
    return c;
}

template <int LQ, int NT0C, int ACT>
__global__ void __launch_bounds__(WAVE_THREADS, 1) k_train_split(TrainArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const TrainPlan& p = A.p;
    const TrainFit& F = A.fit[blockIdx.y];
    constexpr int NL = 2, G0 = LQ / 4, NGR = G0 + 1, HP = SP_HP, OP = SP_OP, PT = SP_PT, RPM = stream_rp(LQ);
    constexpr SplitLds L = split_lds(LQ);
    static_assert(L.total > 0 && L.total * 4 <= 160 * 1024, "LDS map does not fit");
    static_assert(16 * NT0C == 4 * LQ && G0 >= 4, "the first layer's strips fill its slots");
    // strips w, w + 4, .. (NFS per wave) against all four unit tiles, then REM left-over strips, tile w of each (LQ = 24: 1 + 2)
    constexpr int NFS = NT0C / 4, REM = NT0C % 4, NIT = NFS + REM, GA = split_w0_groups(LQ) / 2;   // groups 0 .. GA-1 land first
    static_assert(NFS >= 1 && REM <= 2, "strip counts of the shapes this is instantiated for");
    // small-matrix requests per MFMA group of layer 0 (its G0 - 1 loop iterations carry SP_SM / 4 of them per wave)
    constexpr int SPI = (SP_SM / 4 + G0 - 2) / (G0 - 1);
    // the W_0 ring (SP_RING): RG groups resident, quarters of HR groups; without it W_0 lands whole, in two halves
    constexpr bool RING = split_ring(LQ);
    constexpr int RG = split_w0_groups(LQ), HR = RG / 2, W0B = RG - GA;   // W0B: groups of the first landing's second phase
    static_assert(!RING || (G0 == 2 * RG && GA == HR), "the ring holds half of W_0, its quarters land one behind the other");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int st = wv >> 1, uh = wv & 1;            // sample tile, unit half
    const int i = lane & 15, q = lane >> 4;
    const int C = A.net.C;
    const float* W0s = lds + L.w0;
    const float* SMs = lds + L.sm;
    const float* Xs = lds + L.x;
    float* H0 = lds + L.h0;
    float* H1 = lds + L.h1;
    float* E = lds + L.e;
    float* Zo = lds + L.zo;
    float* ZT = lds + L.zt;
    float* red = lds + L.red;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) void*)lds;
    const int wg = blockIdx.x, grp = wg >> 1, par = wg & 1;
    // this lane's sample: row rho of the 64-row group (see the head of the file)
    const int qb = (i >> 2) & 1, jr = (i & 3) + 4 * (i >> 3);
    const int rho = 16 * (2 * st + qb) + 2 * jr + par;
    const int grow = grp * WB + rho;                // row of the minibatch
    const bool live = grow < A.batch_n;
    const int srow = 16 * st + i;                   // row of the [sample][..] arrays in LDS
    const int sig = 8 * (2 * st + qb) + jr;         // column of the transposed arrays: 8 (row quarter) + j
    const int t0 = 2 * uh;                          // this wave's first unit tile
    float* slab = F.slabs + (size_t)wg * p.slab_floats;
    const WtBuf slabw(slab, (size_t)p.slab_floats * 4);
#ifdef LBDRN_TRAIN_STAMPS
    unsigned long long stamp[16] = {};
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp[14])::"memory");
#endif
#ifdef LBDRN_TIMELINE
    if (lane == 0 && wv == 0 && wg == 0 && blockIdx.y == 0) timeline_store(A.tl, 0, false);
#endif
    STAMP(0);

    // ---- requests.  Nothing here is a load the compiler knows of: its own waits count only what it issued itself, and a
    //      `vmcnt(3)` of its in front of the first use of a register-loaded bias would wait for all but three of the
    //      requests below (measured: layer 0 then started when everything had landed).  So the pixel indices and the biases
    //      travel by LDS-DMA like everything else, behind counted waits.  Order: this wave's copy of the group's 64 pixel
    //      indices (a trip of its own: the row addresses depend on them), the biases, this wave's share of the first half
    //      of W_0 under them; then, as they are needed: rows A | W_0 B | rows B + labels | the small matrices.
    {   // the scalars of the first requests, fetched together (left to itself the compiler fetches each when it is first
        // used: a dozen dependent trips to the scalar cache at the head of the kernel)
        const void* a0 = F.perm; const void* a1 = F.params; const void* a2 = F.packed; const void* a3 = F.rows;
        int b0 = p.pk_w0, b1 = p.pk_wh, b2 = p.pk_wht, b3 = p.pk_wl, b4 = p.pk_wlt, b5 = A.batch_n;
        long long c0 = p.offB[0], c1 = p.offB[1], c2 = p.offB[2], c3 = A.npix;
        asm volatile("" ::"s"(a0), "s"(a1), "s"(a2), "s"(a3), "s"(b0), "s"(b1), "s"(b2), "s"(b3), "s"(b4), "s"(b5), "s"(c0), "s"(c1), "s"(c2), "s"(c3));
    }
    if constexpr (RING) {   // 64 indices, the low 4 bytes of each (pixel indices are < 2^31): lane l fetches element l of the group
                            // -- or the minibatch's last one, past its end: any minibatch size, one row included
        const int64_t* isrc = F.perm + min(grp * WB + lane, A.batch_n - 1);
        stream_dma_dword(reinterpret_cast<const float*>(isrc), lds0 + 4u * (unsigned)(L.idx + 256 * wv));
    } else {   // 64 indices = 512 B: lane l < 32 fetches elements 2 l, 2 l + 1 of the group -- or the minibatch's last two, past its
        // end (the host launches this kernel on minibatches of two rows or more) --, lanes 32 .. 63 repeat them into the
        // second half of the request's 1 KB
        const int64_t* isrc = F.perm + min(grp * WB + 2 * (lane & 31), A.batch_n - 2);
        stream_dma(reinterpret_cast<const float*>(isrc), lds0 + 4u * (unsigned)(L.idx + 256 * wv));
    }
    {   // wave l: the biases of layer l (4 bytes a lane; the last layer has C <= 16 of them; wave 3 repeats the last layer's,
        // so that every wave has issued the same number of requests)
        const int l = wv < 3 ? wv : 2, n = l < 2 ? 64 : C;
        const float* bsrc = F.params + p.offB[l] + min(lane, n - 1);
        stream_dma_dword(bsrc, lds0 + 4u * (unsigned)(L.bias + 64 * wv));
    }
    const float* fsrc = F.packed + lane * 4;
    // fragment block (tile t, group g) of W_0: 256 (t G0 + g) in the packed buffer, (g 4 + t) 256 in LDS; wave w takes tile w
    auto w0_requests = [&](int g_lo, int g_hi) {
#pragma unroll
        for (int g = g_lo; g < g_hi; ++g)
            stream_dma(fsrc + p.pk_w0 + 256 * (wv * G0 + g), lds0 + 4u * (unsigned)(L.w0 + ((g % RG) * 4 + wv) * 256));
    };
    w0_requests(0, GA);
    stream_wait_vm<GA + 1>();  // the indices have landed (behind them: the biases and W_0 A)
    int64_t raw;
    if constexpr (RING) {
        raw = reinterpret_cast<const int*>(lds + L.idx + 256 * wv)[min(grow, A.batch_n - 1) - grp * WB];
    } else {   // this lane's row of the minibatch (rows past the end of a short one repeat its last row: finite values, masked out
        // of the loss) and where the request above put its index
        const int g = min(grow, A.batch_n - 1), l = (g - grp * WB) >> 1;
        const int pos = 2 * l + (g - min(grp * WB + 2 * l, A.batch_n - 2));
        raw = reinterpret_cast<const int64_t*>(lds + L.idx + 256 * wv)[pos];
    }
    const int pix = (int)(raw < 0 ? 0 : (raw >= A.npix ? A.npix - 1 : raw));
    // request g of tile st's rows: lane = 4 slot + quarter reads 16 B of the row in that slot at 64 g + 16 quarter.  The two
    // waves of a pair share a tile's requests: wave u takes the groups g = u (mod 2)
    const float* rsrc = F.rows + (size_t)__shfl(pix, 16 * q + split_slot(lane >> 2)) * RPM + 4 * (lane & 3);
    auto row_requests = [&](int g_lo, int g_hi) {
#pragma unroll
        for (int g = g_lo; g < g_hi; ++g)
            if ((g & 1) == uh) stream_dma(rsrc + 16 * g, lds0 + 4u * (unsigned)(L.x + st * L.xt + g * SGP));
    };
    row_requests(0, GA);
    w0_requests(GA, RG);
    row_requests(GA, NGR);
    // the small matrices (packed W_1 | W_last | W_1^T | W_last^T -> LDS W_1 | W_1^T | W_last | W_last^T) are not needed before
    // layer 0 is over and go out one per MFMA group of it: pushed out here, behind 25 KB per wave of requests that are, they
    // kept the wave at its issue slot -- and away from layer 0 -- while the first half had long landed
    auto small_request = [&](int b) {
        const int blk = 4 * b + wv;
        const int src = blk < 16 ? p.pk_wh + 256 * blk : blk < 32 ? p.pk_wht + 256 * (blk - 16) : blk < 36 ? p.pk_wl + 256 * (blk - 32) : p.pk_wlt + 256 * (blk - 36);
        stream_dma(fsrc + src, lds0 + 4u * (unsigned)(L.sm + 256 * blk));
    };
    // The pixel indices this workgroup will ask for first in the NEXT launch (same block index, so the same XCD): that
    // launch opens with two dependent cold trips, indices then rows, and the first one then ends in a cache (what
    // k_train_stream's loader wave does as it ends).  An ordinary load, "used" when the kernel is nearly over.
    long long touched = 0;
    if (A.next_n > 0 && wv == 0 && lane < 8) touched = F.perm[A.batch_n + min(grp * WB + 8 * lane, A.next_n - 1)];   // a 64-byte piece each
    STAMP(1);
    // requests of this wave behind the last one of phase A: W_0 B (G0 - GA) + rows B; behind phase B: the small ones issued by then
    constexpr int ROWS_B0 = split_row_requests(GA, NGR, 0), ROWS_B1 = split_row_requests(GA, NGR, 1);
    if (uh == 0) stream_wait_vm<W0B + ROWS_B0>(); else stream_wait_vm<W0B + ROWS_B1>();
    stream_barrier();          // phase A has landed: groups 0 .. GA - 1 of W_0 and of both tiles' rows
    STAMP(2);

    // ---- layer 0, this wave's two unit tiles: z^T[32 units][16 samples] = b0 + W0 X^T, lane quarter q walks k = q LQ + 4 g + e
    auto sel4 = [](const float4& x, int e) -> float { return e == 0 ? x.x : e == 1 ? x.y : e == 2 ? x.z : x.w; };
    f32x4 bias0[2], bias1[2], bias_last;
    {
        const float* B = lds + L.bias;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const float4 b4 = *reinterpret_cast<const float4*>(B + 16 * (t0 + tt) + 4 * q);
            const float4 c4 = *reinterpret_cast<const float4*>(B + 64 + 16 * (t0 + tt) + 4 * q);
            bias0[tt][0] = b4.x; bias0[tt][1] = b4.y; bias0[tt][2] = b4.z; bias0[tt][3] = b4.w;
            bias1[tt][0] = c4.x; bias1[tt][1] = c4.y; bias1[tt][2] = c4.z; bias1[tt][3] = c4.w;
        }
        const float4 l4 = *reinterpret_cast<const float4*>(B + 128 + 4 * q);
        bias_last[0] = 4 * q + 0 < C ? l4.x : 0.0f; bias_last[1] = 4 * q + 1 < C ? l4.y : 0.0f;
        bias_last[2] = 4 * q + 2 < C ? l4.z : 0.0f; bias_last[3] = 4 * q + 3 < C ? l4.w : 0.0f;
    }
    f32x4 acc[2] = {bias0[0], bias0[1]};
    {
        const float* wbase = W0s + t0 * 256 + lane * 4;
        const float* xbase = Xs + st * L.xt + (4 * split_slot(i) + q) * 4;
        float4 aq[2][2], bq[2];
        auto reads = [&](int g) {
            aq[g & 1][0] = *reinterpret_cast<const float4*>(wbase + (g % RG) * 1024);
            aq[g & 1][1] = *reinterpret_cast<const float4*>(wbase + (g % RG) * 1024 + 256);
            bq[g & 1] = *reinterpret_cast<const float4*>(xbase + g * SGP);
        };
        auto mfmas = [&](int g) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) acc[tt] = MFMA16(sel4(aq[g & 1][tt], e), sel4(bq[g & 1], e), acc[tt]);
        };
        reads(0);
#pragma unroll
        for (int g = 1; g < G0; ++g) {
            if (g == GA) {     // the rest of W_0 and of the rows (behind them: the small-matrix requests of the iterations so far)
                stream_wait_vm<((GA - 1) * SPI < SP_SM / 4 ? (GA - 1) * SPI : SP_SM / 4)>();
                stream_barrier();
            }
            if constexpr (RING) {
                if (g == GA + 1 || g == 2 * HR + 1) {   // every wave is past group g - 2: its half of the ring takes the next quarter
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    stream_barrier();
                    const int q0 = g == GA + 1 ? 2 * HR : 3 * HR;
                    w0_requests(q0, q0 + HR);
                }
                if (g == 2 * HR) {   // quarter 2 has landed (behind it: the small-matrix requests of iterations GA + 1 .. g - 1)
                    stream_wait_vm<split_small_through(2 * HR - 1, SPI) - split_small_through(GA, SPI)>();
                    stream_barrier();
                }
                if (g == 3 * HR) {   // quarter 3 has landed
                    stream_wait_vm<split_small_through(3 * HR - 1, SPI) - split_small_through(2 * HR, SPI)>();
                    stream_barrier();
                }
            }
#pragma unroll
            for (int b = (g - 1) * SPI; b < g * SPI; ++b)
                if (b < SP_SM / 4) small_request(b);
            reads(g);
            mfmas(g - 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);   // MFMA
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        mfmas(G0 - 1);
        __builtin_amdgcn_sched_barrier(0);
    }
    const float4 lab = *reinterpret_cast<const float4*>(Xs + st * L.xt + G0 * SGP + (4 * split_slot(i) + q) * 4);   // labels of channels 4 q .. 4 q + 3
    STAMP(3);
    // sin / cos of a layer's two tiles; the activations go to LDS for the other unit half (and for the gradient products)
    float hf[4][4];            // the layer's activations of ALL units of this lane's sample, accumulator layout
    f32x4 cs[NL][2];           // cos(30 z) of this wave's tiles, for the backward pass
    auto activate = [&](int l, float* H) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            float sn[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float co;
                train_act<ACT>(acc[tt][r], sn[r], co);
                cs[l][tt][r] = co;
            }
            *reinterpret_cast<float4*>(H + srow * HP + 16 * (t0 + tt) + 4 * q) = make_float4(sn[0], sn[1], sn[2], sn[3]);
        }
    };
    // all four tiles of this lane's sample out of a [sample][unit] array, the wave's own two included (which tiles those are
    // is a run-time matter: registers cannot be indexed by it)
    auto all_units = [&](const float* H, float (&dst)[4][4]) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float4 x = *reinterpret_cast<const float4*>(H + srow * HP + 16 * t + 4 * q);
            dst[t][0] = x.x; dst[t][1] = x.y; dst[t][2] = x.z; dst[t][3] = x.w;
        }
    };
    auto small = [&](int blk) -> float4 { return *reinterpret_cast<const float4*>(SMs + 256 * blk + lane * 4); };
    activate(0, H0);
    stream_wait_vm<0>();       // the small matrices
    __syncthreads();           // h_0 of all units is in LDS, the small matrices have landed, the W_0 fragments are dead
    all_units(H0, hf);
    float4 wh[2][4];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int tk = 0; tk < 4; ++tk) wh[tt][tk] = small((t0 + tt) * 4 + tk);              // W_1 [out tile][k tile]
    STAMP(4);

    // ---- hidden layer: step (tk, r) multiplies unit 16 tk + 4 q + r
    acc[0] = bias1[0]; acc[1] = bias1[1];
#pragma unroll
    for (int tk = 0; tk < 4; ++tk)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) acc[tt] = MFMA16(sel4(wh[tt][tk], r), hf[tk][r], acc[tt]);
    float4 wl[4], wlt[2];
#pragma unroll
    for (int tk = 0; tk < 4; ++tk) wl[tk] = small(32 + tk);
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) wlt[tt] = small(36 + t0 + tt);
    activate(1, H1);
    STAMP(5);
    __syncthreads();           // h_1 of all units is in LDS
    all_units(H1, hf);
    STAMP(6);

    // ---- output layer (both waves of a pair: all of it, the same numbers) + loss + d(loss)/dz_out
    float dzo[4];
    {
        f32x4 oe = bias_last, oo = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tk = 0; tk < 4; ++tk) {
            const float4 x = wl[tk];
            oe = MFMA16(x.x, hf[tk][0], oe);
            oo = MFMA16(x.y, hf[tk][1], oo);
            oe = MFMA16(x.z, hf[tk][2], oe);
            oo = MFMA16(x.w, hf[tk][3], oo);
        }
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
        if (uh == 0) {
            *reinterpret_cast<float4*>(Zo + srow * OP + 4 * q) = make_float4(dzo[0], dzo[1], dzo[2], dzo[3]);
            // loss partial of a row quarter: eight rows in the fixed tree, then the four channel quarters (0 + 1) + (2 + 3)
            const int li = __float_as_int(split_sum8(lsum));
            auto rl = [&](int l) { return __int_as_float(__builtin_amdgcn_readlane(li, l)); };
            const float l0 = (rl(11) + rl(27)) + (rl(43) + rl(59)), l1 = (rl(15) + rl(31)) + (rl(47) + rl(63));
            if (lane == 0) { red[2 * st] = l0; red[2 * st + 1] = l1; }
            // output-bias gradient of a row quarter: lanes 11 / 15 of channel quarter q hold channels 4 q .. 4 q + 3
            float bs[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) bs[r] = split_sum8(dzo[r]);
            if (i == 11 || i == 15)
                *reinterpret_cast<float4*>(red + 4 + 16 * (2 * st + (i == 15)) + 4 * q) = make_float4(bs[0], bs[1], bs[2], bs[3]);
        }
    }
    STAMP(7);

    // ---- backward through the output layer: dz_1 of this wave's units; parked transposed [unit][sample] for the
    //      gradient products and row-major for the other unit half
    float dzf[4][4], dzm[2][4];
    auto backprop = [&](int l) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dzm[tt][r] = train_act_back<ACT>(acc[tt][r], cs[l][tt][r]);
                ZT[(size_t)l * 64 * PT + (16 * (t0 + tt) + 4 * q + r) * PT + sig] = dzm[tt][r];
            }
    };
    float4 wht[2][4];
    {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        acc[0] = zero; acc[1] = zero;
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) acc[tt] = MFMA16(sel4(wlt[tt], s4), dzo[s4], acc[tt]);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int to = 0; to < 4; ++to) wht[tt][to] = small(16 + (t0 + tt) * 4 + to);    // W_1^T [in tile][out tile]
        backprop(1);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
            *reinterpret_cast<float4*>(E + srow * HP + 16 * (t0 + tt) + 4 * q) = make_float4(dzm[tt][0], dzm[tt][1], dzm[tt][2], dzm[tt][3]);
    }
    STAMP(8);
    __syncthreads();           // dz_1 of all units is in LDS (both copies); H_0, H_1, dz_out of every wave as well
    all_units(E, dzf);
    __builtin_amdgcn_sched_barrier(0);

    // ---- weight gradients: K = the 32 rows of this workgroup (8 steps; lane quarter q, step j = row (j & 3) + 4 (q & 1) +
    //      8 (j >> 2) of sample tile q >> 1).  dW[unit tile t][input strip nt]: A = dz^T rows of tile t (8 contiguous floats
    //      per lane), B = the inputs, one float per lane and step.  Wave w takes the strips nt = w, w + 4, .. of the first
    //      layer against all four unit tiles, strip w of the hidden layer, tile w of the output layer; every finished tile
    //      leaves as one 1 KB store in the slab's tile order.  The operands of the products that do not need dz_0 are
    //      requested here, under the last backward product.
    const int w = wv;
    const int rq = 16 * (q >> 1) + 4 * (q & 1);               // first row this quarter reads; step j adds (j & 3) + 8 (j >> 2)
    auto ldcol = [&](const float* base, int pitch, float (&dst)[8]) {   // one float per step out of a row-major array
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[j] = base[(rq + (j & 3) + 8 * (j >> 2)) * pitch];
    };
    auto ldx = [&](int nt, float (&dst)[8]) {   // feature slot 16 nt + i of this quarter's eight rows, out of X' as it landed
        const int f = 16 * nt + i;
        const int kq = f / LQ, fl = f - kq * LQ;
        const float* base = Xs + (q >> 1) * L.xt + (fl >> 2) * SGP + kq * 4 + (fl & 3);
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[j] = base[16 * split_slot(4 * (q & 1) + (j & 3) + 8 * (j >> 2))];
    };
    auto ldrow8 = [&](const float* row, float (&dst)[8]) {   // 8 contiguous floats of a 16-byte aligned row piece
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const float4 x = *reinterpret_cast<const float4*>(row + 4 * g);
            dst[4 * g] = x.x; dst[4 * g + 1] = x.y; dst[4 * g + 2] = x.z; dst[4 * g + 3] = x.w;
        }
    };
    auto put = [&](int off, const f32x4& g) {
        slabw.store(off + lane * 4, g[0], g[1], g[2], g[3]);
    };
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const float* ZT1 = ZT + 64 * PT;
    float az[4][8], a1[4][8], azw[8], a1w[8], ao[8], bo[8], bh[8], bb[NFS][8], br[REM > 0 ? REM : 1][8];
    // the B operands of the first layer's products in the order they are consumed (k_train_stream's list): item n < NFS =
    // strip w + 4 n, item NFS + r = left-over strip 4 NFS + r; requested two regions ahead of its MFMAs
    auto item = [&](auto n_) {
        constexpr int n = decltype(n_)::value;
        if constexpr (n < NFS) ldx(w + 4 * n, bb[n]);
        else if constexpr (n < NIT) ldx(4 * NFS + (n - NFS), br[n - NFS]);
    };
#pragma unroll
    for (int t = 0; t < 4; ++t) ldrow8(ZT1 + (16 * t + i) * PT + 8 * q, a1[t]);
    ldrow8(ZT1 + (16 * w + i) * PT + 8 * q, a1w);   // this wave's own tile once more (bias sums): registers cannot be indexed by w
    ldcol(Zo + i, OP, ao);
    ldcol(H1 + 16 * w + i, HP, bo);
    ldcol(H0 + 16 * w + i, HP, bh);
    item(std::integral_constant<int, 0>{});
    // ---- dh_0 = W_1^T dz_1 for this wave's input units: step (to, r) multiplies dz_1 of unit 16 to + 4 q + r
    {
        acc[0] = zero4; acc[1] = zero4;
#pragma unroll
        for (int to = 0; to < 4; ++to)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) acc[tt] = MFMA16(sel4(wht[tt][to], r), dzf[to][r], acc[tt]);
        stream_deal<32, 32, 0>();
        backprop(0);
    }
    STAMP(9);
    __syncthreads();           // dz_0^T of every wave is in LDS
    if (tid == 0) F.loss_part[wg] = ((double)red[0] + (double)red[1]) + ((double)red[2] + (double)red[3]);
    STAMP(10);
    // region 1: tile w of the output layer, strip w of the hidden layer (40 MFMAs); requested meanwhile: the four dz_0^T
    // tiles, this wave's own once more, the second strip of the rows (18 + 8 reads)
#pragma unroll
    for (int t = 0; t < 4; ++t) ldrow8(ZT + (16 * t + i) * PT + 8 * q, az[t]);
    ldrow8(ZT + (16 * w + i) * PT + 8 * q, azw);
    item(std::integral_constant<int, 1>{});
    f32x4 go = zero4, g1[4] = {zero4, zero4, zero4, zero4};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        go = MFMA16(ao[j], bo[j], go);
#pragma unroll
        for (int t = 0; t < 4; ++t) g1[t] = MFMA16(a1[t][j], bh[j], g1[t]);
    }
    stream_deal<40, (NIT > 1 ? 18 : 10), 0>();
    // the first layer's strips nt = w + 4 k, 32 MFMAs each against the four dz_0^T tiles; strip k's region requests strip
    // k + 2 and stores the tiles of the region before it
    f32x4 gs[2][4];
    stream_for<NFS>([&](auto k_) {
        constexpr int k = decltype(k_)::value;
#pragma unroll
        for (int t = 0; t < 4; ++t) gs[k & 1][t] = zero4;
        item(std::integral_constant<int, k + 2>{});
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) gs[k & 1][t] = MFMA16(az[t][j], bb[k][j], gs[k & 1][t]);
        if constexpr (k == 0) {
            put(p.sl_out + w * 256, go);
#pragma unroll
            for (int t = 0; t < 4; ++t) put(p.sl_hid + (t * 4 + w) * 256, g1[t]);
            stream_deal<32, (k + 2 < NIT ? 8 : 0), 5>();
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) put((t * NT0C + w + 4 * (k - 1)) * 256, gs[(k - 1) & 1][t]);
            stream_deal<32, (k + 2 < NIT ? 8 : 0), 4>();
        }
    });
    if constexpr (REM > 0) {   // the left-over strips, tile w of each: one chain per strip, under which the last full strip's tiles leave
        f32x4 grem[REM];
#pragma unroll
        for (int r = 0; r < REM; ++r) grem[r] = zero4;
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int r = 0; r < REM; ++r) grem[r] = MFMA16(azw[j], br[r][j], grem[r]);
#pragma unroll
        for (int t = 0; t < 4; ++t) put((t * NT0C + w + 4 * (NFS - 1)) * 256, gs[(NFS - 1) & 1][t]);
        stream_deal<REM * 8, 0, 4>();
#pragma unroll
        for (int r = 0; r < REM; ++r) put((w * NT0C + 4 * NFS + r) * 256, grem[r]);
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) put((t * NT0C + w + 4 * (NFS - 1)) * 256, gs[(NFS - 1) & 1][t]);
    }
    // bias gradients: sums over this workgroup's rows of the 16 units of tile w of either layer, out of the A operands:
    // lane (unit i, quarter q) holds row quarter q's eight rows -- summed in step order, quarters (0 + 1) + (2 + 3)
    {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { s0 += azw[j]; s1 += a1w[j]; }
        s0 += __shfl_xor(s0, 16); s1 += __shfl_xor(s1, 16);
        s0 += __shfl_xor(s0, 32); s1 += __shfl_xor(s1, 32);
        if (lane < 16) {
            slab[p.sl_bias + 16 * w + lane] = s0;
            slab[p.sl_bias + TBC_W + 16 * w + lane] = s1;
        }
    }
    if (w == 3 && lane < 16)   // output slots: the four row quarters' partials (loss phase), (0 + 1) + (2 + 3)
        slab[p.sl_bias + NL * TBC_W + lane] = (red[4 + lane] + red[20 + lane]) + (red[36 + lane] + red[52 + lane]);
    asm volatile("" ::"v"(touched));
    STAMP(11); STAMP(12);
#ifdef LBDRN_TIMELINE
    if (lane == 0 && uh == 0 && blockIdx.y == 0) timeline_store(A.tl, 2 + 2 * wg + st, true);   // (one wave of each pair: 512 slots)
#endif
#ifdef LBDRN_TRAIN_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(13);
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp[15])::"memory");
    if (lane == 0 && A.stamps)
        for (int k = 0; k < 16; ++k) A.stamps[(((size_t)blockIdx.y * gridDim.x + wg) * 4 + wv) * 16 + k] = stamp[k];
#endif
}
