// Lossless JPEG 2000 encoder for the MSB planes (base codec "jp2-gpu"): the reference's payload format
// (gdal_translate -of JP2OpenJPEG -co QUALITY=100 -co REVERSIBLE=YES, ref encode.py:137) written from the planes the
// fit left in HBM.  OpenJPEG spends 88-89 % of its time on these planes in tier-1, which is independent per
// code block; that and the wavelet run here, tier-2 and the container are a few hundred KB of host work (jp2k_t2.inc).
//
//   k_jp2k_shift    [C][H][W] uint16 -> per tile-component int32 slabs, DC level shift; flags a value beyond `bits`
//   k_jp2k_lift     one direction of one 5/3 decomposition: every thread computes ONE output coefficient from the five
//                   (three) inputs it depends on, symmetric extension by mirrored indices -- no thread waits for another,
//                   vertical before horizontal as T.800 F.4.2 orders it (integer lifting does not commute)
//   k_jp2k_blocks   one wave per code block: the wave zeroes the flag words, fills the two tables, stages the block into
//                   LDS as sign/magnitude in stripe-column order and finds its top bit-plane, then lane 0 runs the
//                   serial coder of jp2k_t1.inc (t1_encode_block: the coding-pass walk the decoder shares) on LDS state
//                   (19.4 KB per block -- mag 16384 + st 2376 + mqtab 376 + zc 256 + cx 32 + top 4 = 19428 bytes: eight
//                   blocks per CU) and writes the bytes into the block's slot
//   k_jp2k_compact  packs the slots back to back behind an exclusive scan of the lengths
//
// Every write is clamped: a block's bytes to its slot (an overflow is counted and reported, never written), the file to
// the caller's capacity.
#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "common.hpp"
#include "jp2k_t1.inc"
#include "jp2k_t2.inc"

namespace lbdrn {

using jp2k::Block;
using jp2k::BlockOut;
using jp2k::Geometry;

struct Jp2kDev {       // what the kernels need of the geometry
    int C, H, W, R, tw, th, ntx, nty;
    int64_t slab;      // coefficients per tile-component slab
};

__global__ __launch_bounds__(256) void k_jp2k_shift(const uint16_t* __restrict__ planes, Jp2kDev g, int bits, int32_t* __restrict__ A,
                                                    int* __restrict__ status)
{
    const int slab = blockIdx.z, c = slab % g.C, tile = slab / g.C;
    const int x0 = (tile % g.ntx) * g.tw, y0 = (tile / g.ntx) * g.th;
    const int lx = blockIdx.x * 256 + threadIdx.x, ly = blockIdx.y;
    if (lx >= g.tw || x0 + lx >= g.W || y0 + ly >= g.H) return;
    const int v = planes[((size_t)c * g.H + (y0 + ly)) * g.W + x0 + lx];
    if (v >> bits) atomicOr(status, 1);
    A[(size_t)slab * g.slab + (size_t)ly * g.tw + lx] = v - (1 << (bits - 1));
}

// level: decompositions already done (the input is the LL region of that level).  VERT: along y.
template <bool VERT>
__global__ __launch_bounds__(256) void k_jp2k_lift(const int32_t* __restrict__ src, int32_t* __restrict__ dst, Jp2kDev g, int level)
{
    const int slab = blockIdx.z, tile = slab / g.C;
    const int x0 = (tile % g.ntx) * g.tw, y0 = (tile / g.ntx) * g.th;
    const int w = min(g.tw, g.W - x0), h = min(g.th, g.H - y0);
    const int rw = jp2k::ceil_shift(w, level), rh = jp2k::ceil_shift(h, level);
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
    if (ox >= rw || oy >= rh) return;
    const int n = VERT ? rh : rw, o = VERT ? oy : ox;
    const int32_t* line = src + (size_t)slab * g.slab + (VERT ? (size_t)ox : (size_t)oy * g.tw);
    const size_t step = VERT ? (size_t)g.tw : 1;
    int out;
    if (n == 1) out = line[0];
    else {
        const int sn = (n + 1) >> 1;
        auto X = [&](int j) { return line[(size_t)jp2k::mirror(j, n) * step]; };
        if (o >= sn) {
            const int p = 2 * (o - sn) + 1;
            out = X(p) - ((X(p - 1) + X(p + 1)) >> 1);
        } else {
            const int p = 2 * o;
            const int a = X(p - 2), b = X(p - 1), cc = X(p), d = X(p + 1), e = X(p + 2);
            const int dl = b - ((a + cc) >> 1), dr = d - ((cc + e) >> 1);
            out = cc + ((dl + dr + 2) >> 2);
        }
    }
    dst[(size_t)slab * g.slab + (size_t)oy * g.tw + ox] = out;
}

__global__ __launch_bounds__(64) void k_jp2k_blocks(const int32_t* __restrict__ A, Jp2kDev g, const Block* __restrict__ blocks,
                                                    uint8_t* __restrict__ staging, BlockOut* __restrict__ outs,
                                                    uint32_t* __restrict__ lens)
{
    __shared__ uint32_t mag[16 * 64 * 4];
    __shared__ uint16_t st[jp2k::T1_NST * jp2k::T1_STW];
    __shared__ uint32_t mqtab[jp2k::MQ_ENTRIES];
    __shared__ uint8_t zc[256];
    __shared__ uint8_t cx[32];
    __shared__ uint32_t top;
    const Block b = blocks[blockIdx.x];
    const int lane = threadIdx.x;
    const int bw = min((int)b.w, 64), bh = min((int)b.h, 64);
    if (lane == 0) top = 0;
    for (int k = lane; k < jp2k::T1_NST * jp2k::T1_STW; k += 64) st[k] = 0;
    jp2k::t1_fill_tables(mqtab, zc, b.orient, lane, 64);
    __syncthreads();
    const int32_t* src = A + (size_t)b.slab * g.slab + (size_t)b.y * g.tw + b.x;
    uint32_t mx = 0;
    for (int y = 0; y < 64; ++y) {
        uint32_t m = 0;
        if (y < bh && lane < bw) {
            const int v = src[(size_t)y * g.tw + lane];
            m = v < 0 ? (0x80000000u | (uint32_t)(-v)) : (uint32_t)v;
        }
        mag[((y >> 2) * 64 + lane) * 4 + (y & 3)] = m;
        mx |= m & 0x7FFFFFFFu;
    }
    atomicOr(&top, mx);
    __syncthreads();
    if (lane == 0) {
        const int numbps = top ? 32 - __clz((int)top) : 0;
        uint8_t* out = staging + b.slot;
        const jp2k::T1Result r = jp2k::t1_encode_block(mag, st, cx, mqtab, zc, bw, bh, numbps, out, (int)b.cap);
        BlockOut o;
        o.bytes = (uint32_t)r.bytes; o.passes = (uint32_t)r.passes; o.numbps = (uint32_t)r.numbps; o.pad = 0;
        outs[blockIdx.x] = o;
        lens[blockIdx.x] = (uint32_t)min(r.bytes, (int)b.cap);
    }
}

__global__ __launch_bounds__(256) void k_jp2k_compact(const uint8_t* __restrict__ staging, const Block* __restrict__ blocks,
                                                      const uint32_t* __restrict__ lens, const uint64_t* __restrict__ offsets,
                                                      uint8_t* __restrict__ packed, uint64_t packed_cap)
{
    const Block b = blocks[blockIdx.x];
    const uint32_t n = min(lens[blockIdx.x], b.cap);
    const uint64_t off = offsets[blockIdx.x];
    if (off + n > packed_cap) return;
    for (uint32_t k = threadIdx.x; k < n; k += 256) packed[off + k] = staging[b.slot + k];
}

// ------------------------------------------------------------------ host entry points

struct Jp2kWs {
    int32_t *A, *B;       // the two coefficient buffers; once the blocks are coded their room holds the packed bytes
    uint8_t* packed;
    size_t ab_bytes;
    uint8_t* staging;
    Block* blocks;
    BlockOut* outs;
    uint32_t* lens;
    uint64_t* offsets;
    int* status;
    void* scan_tmp;
    size_t scan_bytes, total;
};

static int64_t jp2k_slab(const Geometry& g) { return (int64_t)g.tw * g.th; }

static int carve_jp2k(const Geometry& g, void* ws, Jp2kWs* w)
{
    size_t scan_bytes = 0;
    uint32_t* in = nullptr;
    uint64_t* out = nullptr;
    if (rocprim::exclusive_scan(nullptr, scan_bytes, in, out, (uint64_t)0, (size_t)std::max<int64_t>(g.nblocks, 1),
                                rocprim::plus<uint64_t>()) != hipSuccess)
        return LBDRN_E_DEVICE;
    const size_t half = align_up((size_t)g.ntx * g.nty * g.C * (size_t)jp2k_slab(g) * 4, 256);
    char* p = (char*)ws;
    w->A = (int32_t*)p;
    w->B = (int32_t*)(p + half);
    w->packed = (uint8_t*)p;
    w->ab_bytes = std::max(2 * half, align_up((size_t)g.staging, 256));
    p += w->ab_bytes;
    w->staging = (uint8_t*)p; p += align_up((size_t)g.staging, 256);
    w->blocks = (Block*)p; p += align_up((size_t)g.nblocks * sizeof(Block), 256);
    w->outs = (BlockOut*)p; p += align_up((size_t)g.nblocks * sizeof(BlockOut), 256);
    w->lens = (uint32_t*)p; p += align_up((size_t)g.nblocks * 4, 256);
    w->offsets = (uint64_t*)p; p += align_up((size_t)(g.nblocks + 1) * 8, 256);
    w->status = (int*)p; p += 256;
    w->scan_tmp = p; p += align_up(scan_bytes, 256);
    w->scan_bytes = scan_bytes;
    w->total = (size_t)(p - (char*)ws);
    return 0;
}

int64_t jp2k_block_count(int C, int H, int W)
{
    Geometry g;
    if (!jp2k::make_geometry(C, H, W, 16, false, &g)) return 0;
    return g.nblocks;
}

size_t jp2k_bound(int C, int H, int W)
{
    Geometry g;
    if (!jp2k::make_geometry(C, H, W, 16, true, &g)) return 0;
    return jp2k::overhead_bound(g) + (size_t)g.staging;
}

size_t jp2k_workspace(int C, int H, int W)
{
    Geometry g;
    Jp2kWs w;
    if (!jp2k::make_geometry(C, H, W, 16, true, &g) || carve_jp2k(g, nullptr, &w)) return 0;
    return w.total;
}

int jp2k_encode(const uint16_t* planes, int C, int H, int W, int bits, uint8_t* out, size_t cap, size_t* nbytes, void* ws,
                size_t ws_bytes, hipStream_t s)
{
    LBDRN_REQUIRE(planes && out && nbytes, "lbdrn_jp2k_encode: null pointer");
    LBDRN_REQUIRE(C >= 1 && C <= 16384 && H >= 1 && W >= 1 && H <= jp2k::MAX_SIDE && W <= jp2k::MAX_SIDE,
                  "lbdrn_jp2k_encode: %d x %d x %d is outside 1..16384 components of 1..%d x 1..%d", C, H, W, jp2k::MAX_SIDE,
                  jp2k::MAX_SIDE);
    LBDRN_REQUIRE(bits == 8 || bits == 16, "lbdrn_jp2k_encode: bits must be 8 or 16, not %d", bits);
    *nbytes = 0;
    Geometry g16, g;
    // (the workspace is sized for 16 bits, whose slots are the larger ones)
    if (!jp2k::make_geometry(C, H, W, 16, true, &g16) || !jp2k::make_geometry(C, H, W, bits, true, &g)) {
        set_error("lbdrn_jp2k_encode: bad geometry");
        return LBDRN_E_ARG;
    }
    const int64_t slabs = (int64_t)g.ntx * g.nty * C;
    if (slabs > 65535) {
        set_error("lbdrn_jp2k_encode: %lld tile-components exceed the 65535 one launch addresses", (long long)slabs);
        return LBDRN_E_UNSUPPORTED;
    }
    Jp2kWs w16, w;
    if (int rc = carve_jp2k(g16, ws, &w16)) return rc;
    if (!ws || ws_bytes < w16.total) {
        set_error("jp2k workspace too small: %zu < %zu", ws_bytes, w16.total);
        return LBDRN_E_WORKSPACE;
    }
    if (int rc = carve_jp2k(g, ws, &w)) return rc;
    const Jp2kDev d = {C, H, W, g.R, g.tw, g.th, g.ntx, g.nty, jp2k_slab(g)};
    const size_t nb = (size_t)g.nblocks;
    LBDRN_HIP_TRY(hipMemsetAsync(w.status, 0, sizeof(int), s));
    LBDRN_HIP_TRY(hipMemcpyAsync(w.blocks, g.blocks.data(), nb * sizeof(Block), hipMemcpyHostToDevice, s));
    {
        const dim3 grid((unsigned)((g.tw + 255) / 256), (unsigned)g.th, (unsigned)slabs);
        k_jp2k_shift<<<grid, 256, 0, s>>>(planes, d, bits, w.A, w.status);
        LBDRN_LAUNCH_CHECK();
    }
    for (int level = 0; level < g.R - 1; ++level) {
        const int rw = jp2k::ceil_shift(g.tw, level), rh = jp2k::ceil_shift(g.th, level);
        const dim3 grid((unsigned)((rw + 255) / 256), (unsigned)rh, (unsigned)slabs);
        k_jp2k_lift<true><<<grid, 256, 0, s>>>(w.A, w.B, d, level);
        LBDRN_LAUNCH_CHECK();
        k_jp2k_lift<false><<<grid, 256, 0, s>>>(w.B, w.A, d, level);
        LBDRN_LAUNCH_CHECK();
    }
    k_jp2k_blocks<<<(unsigned)nb, 64, 0, s>>>(w.A, d, w.blocks, w.staging, w.outs, w.lens);
    LBDRN_LAUNCH_CHECK();
    LBDRN_HIP_TRY(rocprim::exclusive_scan(w.scan_tmp, w.scan_bytes, w.lens, w.offsets, (uint64_t)0, nb, rocprim::plus<uint64_t>(), s));
    k_jp2k_compact<<<(unsigned)nb, 256, 0, s>>>(w.staging, w.blocks, w.lens, w.offsets, w.packed, (uint64_t)w.ab_bytes);
    LBDRN_LAUNCH_CHECK();
    std::vector<BlockOut> res(nb);
    int status = 0;
    LBDRN_HIP_TRY(hipMemcpyAsync(res.data(), w.outs, nb * sizeof(BlockOut), hipMemcpyDeviceToHost, s));
    LBDRN_HIP_TRY(hipMemcpyAsync(&status, w.status, sizeof(int), hipMemcpyDeviceToHost, s));
    LBDRN_HIP_TRY(hipStreamSynchronize(s));
    if (status) {
        set_error("lbdrn_jp2k_encode: a value does not fit %d bits", bits);
        return LBDRN_E_ARG;
    }
    uint64_t total = 0;
    for (size_t k = 0; k < nb; ++k) {
        if (res[k].bytes > g.blocks[k].cap) {
            set_error("lbdrn_jp2k_encode: code block %zu needs %u bytes, its slot holds %u", k, res[k].bytes, g.blocks[k].cap);
            return LBDRN_E_UNSUPPORTED;
        }
        total += res[k].bytes;
    }
    const size_t need = jp2k::assemble(g, res.data(), nullptr, 0, nullptr, 0);   // counts, writes nothing
    if (need > cap) {
        set_error("lbdrn_jp2k_encode: the stream has %zu bytes, the buffer %zu", need, cap);
        return LBDRN_E_WORKSPACE;
    }
    // the packed block bytes go to the end of the caller's buffer and are moved forward between the packet headers
    uint8_t* tail = out + (cap - (size_t)total);
    if (total) LBDRN_HIP_TRY(hipMemcpyAsync(tail, w.packed, (size_t)total, hipMemcpyDeviceToHost, s));
    LBDRN_HIP_TRY(hipStreamSynchronize(s));
    const size_t n = jp2k::assemble(g, res.data(), tail, total, out, cap);
    if (n != need) {
        set_error("lbdrn_jp2k_encode: assembled %zu bytes, counted %zu", n, need);
        return LBDRN_E_DEVICE;
    }
    *nbytes = n;
    return 0;
}

}  // namespace lbdrn
