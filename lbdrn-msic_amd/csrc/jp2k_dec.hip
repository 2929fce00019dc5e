// liblbdrn_jp2k_dec.so (include/lbdrn_jp2k_dec.h): the decoder of the lossless JPEG 2000 MSB payload -- what jp2k.hip
// writes, what OpenJPEG and Pillow write with reversible settings, precinct partitions and the reversible component
// transform included -- with the planes left in HBM.  The host parses the file into a validated table of code blocks (jp2k_t2d.inc); tier-1 and the wavelet, which
// are independent per block and per sample, run here:
//
//   k_jp2k_unblocks   one wave per code block: the wave zeroes the block's LDS state and fills the two tables, lane 0 runs
//                     the serial decoder of jp2k_t1d.inc (t1_decode_block: the coding-pass walk the coder shares) on it,
//                     reading the block's bytes from the file's copy in HBM (19.4 KB of LDS per
//                     block -- mag 16384 + st 2376 + mqtab 376 + zc 256 + cx 32 = 19424 bytes: eight blocks per CU),
//                     then the wave stores the block as signed int32 into its tile-component slab (Mallat layout);
//                     a block the file does not include stores zeros
//   k_jp2k_unlift     one direction of one 5/3 synthesis step: every thread computes ONE output sample from the three
//                     high-pass and two low-pass coefficients it depends on (an odd sample recomputes its two even
//                     neighbours), symmetric extension by mirrored indices, the parity of the line's first coordinate
//                     from the tile's place on the grid -- no thread waits for another; rows before columns, from the
//                     lowest resolution up (the reverse of F.4.2's analysis order)
//   k_jp2k_unshift    DC shift back, clamp to [0, 2^bits - 1] (G.1.2), uint16 into [C][H][W]; its RCT form (files with
//                     the reversible component transform, COD's mct = 1) first undoes the transform on components 0 - 2
//                     (G.2.2): every thread of those three reads the three slabs at its sample and keeps its own
//                     component's value -- still one thread per stored sample, and no thread waits for another
//
// The device only ever indexes with what the host has checked: block rectangles inside the slab, offset + length inside
// the file.  The kernels clamp once more.
#include <stdarg.h>
#include <string.h>

#include <vector>

#include "common.hpp"
#include "error_buffer.inc"
#include "../../include/lbdrn_jp2k_dec.h"
#include "jp2k_t1d.inc"
#include "jp2k_t2d.inc"

namespace lbdrn {

struct Jp2kdBlock {    // what the device needs of a code block (32 bytes)
    uint64_t offset;   // of its bytes in the file
    uint32_t length;
    uint32_t slab;     // tile-component index
    uint16_t x, y;     // in the slab
    uint8_t w, h, orient, numbps, passes, pad0, pad1, pad2;
    uint32_t pad3;
};
static_assert(sizeof(Jp2kdBlock) == 32, "Jp2kdBlock is copied to the device as it is");

struct Jp2kdDev {      // what the kernels need of the geometry
    int C, H, W, XT, YT, ntx, tw, th;
    int64_t slab;      // coefficients per tile-component slab
};

__global__ __launch_bounds__(64) void k_jp2k_unblocks(const uint8_t* __restrict__ file, uint64_t file_bytes,
                                                      const Jp2kdBlock* __restrict__ blocks, Jp2kdDev g, int32_t* __restrict__ A)
{
    __shared__ uint32_t mag[16 * 64 * 4];
    __shared__ uint16_t st[jp2k::T1_NST * jp2k::T1_STW];
    __shared__ uint32_t mqtab[jp2k::MQ_ENTRIES];
    __shared__ uint8_t zc[256];
    __shared__ uint8_t cx[32];
    const Jp2kdBlock b = blocks[blockIdx.x];
    const int lane = threadIdx.x;
    const int bw = min((int)b.w, 64), bh = min((int)b.h, 64);
    for (int k = lane; k < 16 * 64 * 4; k += 64) mag[k] = 0;
    for (int k = lane; k < jp2k::T1_NST * jp2k::T1_STW; k += 64) st[k] = 0;
    jp2k::t1_fill_tables(mqtab, zc, b.orient & 3, lane, 64);
    __syncthreads();
    if (lane == 0 && b.passes && b.offset <= file_bytes && b.length <= file_bytes - b.offset)
        jp2k::t1_decode_block(mag, st, cx, mqtab, zc, bw, bh, (int)b.numbps, (int)b.passes, file + b.offset, (int)b.length);
    __syncthreads();
    if ((int)b.x + bw > g.tw || (int)b.y + bh > g.th) return;
    int32_t* dst = A + (size_t)b.slab * g.slab + (size_t)b.y * g.tw + b.x;
    for (int y = 0; y < bh; ++y) {
        if (lane < bw) {
            const uint32_t m = mag[((y >> 2) * 64 + lane) * 4 + (y & 3)];
            const int v = (int)(m & 0x7FFFFFFFu);
            dst[(size_t)y * g.tw + lane] = (m >> 31) ? -v : v;
        }
    }
}

// level: the decomposition that is undone (0 the finest).  VERT: along y.  The region is the tile-component's
// resolution of that level; what lies outside it in dst is left alone.  The horizontal step comes first: it takes the
// three high-pass bands from the coefficient slab `src` and the low-pass band from `ll` -- the slab itself at the
// lowest level, the previous level's output above it --, so the coefficient slab is never written after k_jp2k_unblocks.
template <bool VERT>
__global__ __launch_bounds__(256) void k_jp2k_unlift(const int32_t* __restrict__ src, const int32_t* __restrict__ ll,
                                                     int32_t* __restrict__ dst, Jp2kdDev g, int level)
{
    const int slab = blockIdx.z, tile = slab / g.C;
    const int64_t x0 = (int64_t)(tile % g.ntx) * g.XT, y0 = (int64_t)(tile / g.ntx) * g.YT;
    const int64_t x1 = min(x0 + g.XT, (int64_t)g.W), y1 = min(y0 + g.YT, (int64_t)g.H);
    const int64_t one = (int64_t)1 << level;
    const int64_t ux0 = (x0 + one - 1) >> level, ux1 = (x1 + one - 1) >> level;
    const int64_t uy0 = (y0 + one - 1) >> level, uy1 = (y1 + one - 1) >> level;
    const int rw = (int)(ux1 - ux0), rh = (int)(uy1 - uy0);
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
    if (ox >= rw || oy >= rh) return;
    const int n = VERT ? rh : rw, o = VERT ? oy : ox;
    const int par = (int)((VERT ? uy0 : ux0) & 1);           // parity of the line's first coordinate
    const int nlow = ((par + n + 1) >> 1) - ((par + 1) >> 1);
    // (horizontal step) the rows of the low-pass half in y hold LL | HL, the others LH | HH
    const int pary = (int)(uy0 & 1);
    const bool ll_row = !VERT && oy < ((pary + rh + 1) >> 1) - ((pary + 1) >> 1);
    const size_t base = (size_t)slab * g.slab + (VERT ? (size_t)ox : (size_t)oy * g.tw);
    const int32_t* line = src + base;
    const int32_t* lowline = (ll_row ? ll : src) + base;
    const size_t step = VERT ? (size_t)g.tw : 1;
    int out;
    if (n == 1) {
        const int v = par ? line[0] : lowline[0];            // (a lone sample at an odd coordinate is a high-pass one)
        out = par ? v / 2 : v;
    } else {
        // the coefficient that stands at position k of the interleaved line
        auto IL = [&](int k) {
            const int i = par + k;
            return (i & 1) ? line[(size_t)(nlow + (i >> 1) - (par >> 1)) * step] : lowline[(size_t)((i >> 1) - ((par + 1) >> 1)) * step];
        };
        auto EVEN = [&](int m) { return IL(m) - ((IL(jp2k::mirror(m - 1, n)) + IL(jp2k::mirror(m + 1, n)) + 2) >> 2); };
        if ((par + o) & 1) out = IL(o) + ((EVEN(jp2k::mirror(o - 1, n)) + EVEN(jp2k::mirror(o + 1, n))) >> 1);
        else out = EVEN(o);
    }
    dst[(size_t)slab * g.slab + (size_t)oy * g.tw + ox] = out;
}

// RCT: g.C >= 3 (the host refuses the transform on fewer components).  A damaged file can leave any int32 in a slab: the
// transform's sums wrap around as unsigned ones, the floor is taken of a 64-bit sum, the shift is added in 64 bits.
template <bool RCT>
__global__ __launch_bounds__(256) void k_jp2k_unshift(const int32_t* __restrict__ A, Jp2kdDev g, int bits, uint16_t* __restrict__ planes)
{
    const int slab = blockIdx.z, c = slab % g.C, tile = slab / g.C;
    const int64_t x0 = (int64_t)(tile % g.ntx) * g.XT, y0 = (int64_t)(tile / g.ntx) * g.YT;
    const int lx = blockIdx.x * 256 + threadIdx.x, ly = blockIdx.y;
    if (lx >= g.tw || x0 + lx >= g.W || y0 + ly >= g.H) return;
    const int top = (1 << bits) - 1;
    int v;
    if (RCT && c < 3) {
        const int32_t* Y = A + (size_t)(slab - c) * g.slab + (size_t)ly * g.tw + lx;      // the tile's component 0
        const int32_t y0v = Y[0], y1v = Y[g.slab], y2v = Y[2 * g.slab];
        const uint32_t i1 = (uint32_t)y0v - (uint32_t)(((int64_t)y1v + y2v) >> 2);        // (G-6; >> of a negative sum: the floor)
        const uint32_t u = c == 1 ? i1 : (uint32_t)(c == 0 ? y2v : y1v) + i1;             // (G-7, G-8)
        const int64_t w = (int64_t)(int32_t)u + (1 << (bits - 1));
        v = (int)(w < 0 ? 0 : (w > top ? top : w));
    } else {
        v = A[(size_t)slab * g.slab + (size_t)ly * g.tw + lx] + (1 << (bits - 1));
        v = v < 0 ? 0 : (v > top ? top : v);
    }
    planes[((size_t)c * g.H + (size_t)(y0 + ly)) * g.W + (size_t)(x0 + lx)] = (uint16_t)v;
}

// ------------------------------------------------------------------ host side

struct Jp2kdWs {
    int32_t *A, *B, *L;    // the coefficient slabs (written by k_jp2k_unblocks only), a level's rows, a level's output
    uint8_t* file;
    Jp2kdBlock* blocks;
    size_t total;
};

static void carve_jp2kd(const jp2k::DecParams& p, int64_t nblocks, size_t n, void* ws, Jp2kdWs* w)
{
    const size_t half = align_up((size_t)p.ntx * p.nty * p.C * (size_t)p.tw * p.th * 4, 256);
    char* q = (char*)ws;
    w->A = (int32_t*)q; q += half;
    w->B = (int32_t*)q; q += half;
    w->L = (int32_t*)q; q += half;
    w->file = (uint8_t*)q; q += align_up(n, 256);
    w->blocks = (Jp2kdBlock*)q; q += align_up((size_t)(nblocks ? nblocks : 1) * sizeof(Jp2kdBlock), 256);
    w->total = (size_t)(q - (char*)ws);
}

static int dec_status(const jp2k::DecError& e, const char* who)
{
    set_error("%s: %s", who, e.msg);
    return e.code == jp2k::DEC_UNSUPPORTED ? LBDRN_E_UNSUPPORTED : LBDRN_E_ARG;
}

// headers and geometry: what every entry point starts with
static int jp2kd_open(const void* buf, size_t n, jp2k::DecStream* s, int64_t* nblocks, const char* who)
{
    jp2k::DecError e = {0, ""};
    if (jp2k::dec_read_headers((const uint8_t*)buf, n, s, &e)) return dec_status(e, who);
    const int64_t nb = jp2k::dec_count_blocks(s->p, &e);
    if (nb < 0) return dec_status(e, who);
    const int64_t slabs = (int64_t)s->p.ntx * s->p.nty * s->p.C;
    if (slabs > 65535) {
        set_error("%s: %lld tile-components exceed the 65535 one launch addresses", who, (long long)slabs);
        return LBDRN_E_UNSUPPORTED;
    }
    *nblocks = nb;
    return 0;
}

static int jp2kd_device_ok()
{
    int count = 0, dev = 0;
    hipDeviceProp_t prop;
    const hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count < 1) {
        set_error("no HIP device available (%s); liblbdrn_jp2k_dec has no CPU path", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return LBDRN_E_DEVICE;
    }
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        set_error("cannot query the current HIP device");
        return LBDRN_E_DEVICE;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; this library is built for gfx950 (MI355X) only", dev, prop.gcnArchName);
        return LBDRN_E_DEVICE;
    }
    return 0;
}

static int jp2kd_decode(const void* buf, size_t n, uint16_t* planes, int C, int H, int W, void* ws, size_t ws_bytes, hipStream_t s)
{
    LBDRN_REQUIRE(buf && planes, "lbdrn_jp2kd_decode: null pointer");
    LBDRN_REQUIRE(((uintptr_t)planes & 1u) == 0, "lbdrn_jp2kd_decode: planes is not 2-byte aligned");
    LBDRN_REQUIRE(((uintptr_t)ws & 255u) == 0, "lbdrn_jp2kd_decode: workspace is not 256-byte aligned");   // (carve_jp2kd: int32 regions from the base)
    jp2k::DecStream st;
    int64_t nblocks = 0;
    if (int rc = jp2kd_open(buf, n, &st, &nblocks, "lbdrn_jp2kd_decode")) return rc;
    const jp2k::DecParams& p = st.p;
    LBDRN_REQUIRE(C == p.C && H == p.H && W == p.W, "lbdrn_jp2kd_decode: the file holds %d x %d x %d, the planes are %d x %d x %d", p.C, p.H,
                  p.W, C, H, W);
    Jp2kdWs w;
    carve_jp2kd(p, nblocks, n, ws, &w);
    if (!ws || ws_bytes < w.total) {
        set_error("jp2k decoder workspace too small: %zu < %zu", ws_bytes, w.total);
        return LBDRN_E_WORKSPACE;
    }
    std::vector<jp2k::DecBlock> table;
    jp2k::DecError e = {0, ""};
    if (jp2k::dec_parse((const uint8_t*)buf, n, st, &table, &e)) return dec_status(e, "lbdrn_jp2kd_decode");
    std::vector<Jp2kdBlock> dev(table.size());
    for (size_t k = 0; k < table.size(); ++k) {
        const jp2k::DecBlock& t = table[k];
        Jp2kdBlock& d = dev[k];
        memset(&d, 0, sizeof d);
        d.offset = t.passes ? (uint64_t)t.offset : 0;
        d.length = t.passes ? (uint32_t)t.length : 0;
        d.slab = (uint32_t)(t.tile * p.C + t.comp);
        d.x = (uint16_t)t.x; d.y = (uint16_t)t.y; d.w = (uint8_t)t.w; d.h = (uint8_t)t.h;
        d.orient = (uint8_t)t.orient; d.numbps = (uint8_t)t.numbps; d.passes = (uint8_t)t.passes;
    }
    if (int rc = jp2kd_device_ok()) return rc;
    const Jp2kdDev g = {p.C, p.H, p.W, p.XT, p.YT, p.ntx, p.tw, p.th, (int64_t)p.tw * p.th};
    const unsigned slabs = (unsigned)(p.ntx * p.nty * p.C);
    LBDRN_HIP_TRY(hipMemcpyAsync(w.file, buf, n, hipMemcpyHostToDevice, s));
    if (!dev.empty()) {
        LBDRN_HIP_TRY(hipMemcpyAsync(w.blocks, dev.data(), dev.size() * sizeof(Jp2kdBlock), hipMemcpyHostToDevice, s));
        k_jp2k_unblocks<<<(unsigned)dev.size(), 64, 0, s>>>(w.file, (uint64_t)n, w.blocks, g, w.A);
        LBDRN_LAUNCH_CHECK();
    }
    for (int level = p.NL - 1; level >= 0; --level) {
        // (ceil(a + b) - ceil(a) <= ceil(b): no tile's resolution is larger than the nominal tile's, wherever it starts)
        const int rw = jp2k::ceil_shift(p.tw, level), rh = jp2k::ceil_shift(p.th, level);
        const dim3 grid((unsigned)((rw + 255) / 256), (unsigned)rh, slabs);
        k_jp2k_unlift<false><<<grid, 256, 0, s>>>(w.A, level == p.NL - 1 ? w.A : w.L, w.B, g, level);
        LBDRN_LAUNCH_CHECK();
        k_jp2k_unlift<true><<<grid, 256, 0, s>>>(w.B, w.B, w.L, g, level);
        LBDRN_LAUNCH_CHECK();
    }
    {
        const dim3 grid((unsigned)((p.tw + 255) / 256), (unsigned)p.th, slabs);
        if (p.mct) k_jp2k_unshift<true><<<grid, 256, 0, s>>>(p.NL ? w.L : w.A, g, p.bits, planes);
        else k_jp2k_unshift<false><<<grid, 256, 0, s>>>(p.NL ? w.L : w.A, g, p.bits, planes);
        LBDRN_LAUNCH_CHECK();
    }
    LBDRN_HIP_TRY(hipStreamSynchronize(s));     // (the host copies above were staged from memory this call owns)
    return 0;
}

}  // namespace lbdrn

extern "C" {

const char* lbdrn_jp2kd_last_error(void) { return lbdrn::last_error(); }
int lbdrn_jp2kd_abi_version(void) { return LBDRN_JP2KD_ABI_VERSION; }

int lbdrn_jp2kd_info(const void* buf, size_t n, int32_t* C, int32_t* H, int32_t* W, int32_t* bits)
{
    LBDRN_REQUIRE(buf && C && H && W && bits, "lbdrn_jp2kd_info: null pointer");
    jp2k::DecStream st;
    int64_t nblocks = 0;
    if (int rc = lbdrn::jp2kd_open(buf, n, &st, &nblocks, "lbdrn_jp2kd_info")) return rc;
    std::vector<jp2k::DecBlock> table;
    jp2k::DecError e = {0, ""};
    if (jp2k::dec_parse((const uint8_t*)buf, n, st, &table, &e)) return lbdrn::dec_status(e, "lbdrn_jp2kd_info");
    *C = st.p.C; *H = st.p.H; *W = st.p.W; *bits = st.p.bits;
    return 0;
}

size_t lbdrn_jp2kd_workspace(const void* buf, size_t n)
{
    jp2k::DecStream st;
    int64_t nblocks = 0;
    if (!buf || lbdrn::jp2kd_open(buf, n, &st, &nblocks, "lbdrn_jp2kd_workspace")) return 0;
    lbdrn::Jp2kdWs w;
    lbdrn::carve_jp2kd(st.p, nblocks, n, nullptr, &w);
    return w.total;
}

int lbdrn_jp2kd_decode(const void* buf, size_t n, uint16_t* planes, int32_t C, int32_t H, int32_t W, void* workspace,
                       size_t workspace_bytes, void* stream)
{
    return lbdrn::jp2kd_decode(buf, n, planes, C, H, W, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
