// The TIFF writer's format text (include/lbdrn_tiff_write.h), written once for the device and the host: the gather of a
// segment row (layout, zero fill, predictor 2) and the Deflate encoder (RFC 1950 / 1951) -- match finder, token buffer,
// length-limited Huffman codes, dynamic header, block choice, stored blocks, bit emission, Adler-32.  csrc/tiffw.hip
// compiles it for the kernels, tests/tiff_write_host_shim.cpp and tests/tiff_write_main.cpp compile the same text with a
// host compiler.  No state, no allocation, no I/O.  The geometry and the Adler-32 are the reader's (csrc/tiff.inc).
//
// The encoder is written for one wave.  Two kinds of loop share the work:
//   for (k = lane; k < n; k += nl)    bulk work shared out by lane (the device passes its lane and 64, the host 0 and 1)
//   TW_FOR_LANES(l, lane)             one step of 64 lanes: on the device the body runs once with l = lane, on the host it
//                                     is a loop over l = 0 .. 63.  What lanes hand to each other inside a step goes through
//                                     WaveScan / WavePrev (shuffles on the device, a running value on the host) or through
//                                     the state in LDS with a commutative update (TW_MAX, TW_ADD, TW_OR), so the result does
//                                     not depend on the order in which lanes run: the host's bytes are the device's.
// Everything else is wave-uniform: every lane runs the same control flow on the same values and lane 0 stores.
//
// Bounds: deflate() reads in[0 .. n) and writes out[0 .. cap) only, whatever happens; with cap >= bound(n) nothing is cut.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "tiff.inc"
#include "../../include/lbdrn_tiff_write.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define TW_FOR_LANES(l, lane) for (int l = (lane), once_ = 1; once_; once_ = 0)
#define TW_MAX(p, v) atomicMax((p), (v))
#define TW_ADD(p, v) atomicAdd((p), (v))
#define TW_OR(p, v) atomicOr((p), (v))
#else
#define TW_FOR_LANES(l, lane) for (int l = 0; l < 64; ++l)
#define TW_MAX(p, v) do { if (*(p) < (v)) *(p) = (v); } while (0)
#define TW_ADD(p, v) (*(p) += (v))
#define TW_OR(p, v) (*(p) |= (v))
#endif

namespace tiffw {

constexpr int WAVE = 64;
constexpr int HASH_BITS = 12, HASH_SIZE = 1 << HASH_BITS;
// The staged part of the segment: 32 KiB of history, the step's 64 positions, the longest match behind the last of them and
// the part of a chunk staged ahead: 32768 + 64 + 262 + 2047 <= RING.  Not a power of two, to leave LDS for a second wave
// on the compute unit: positions are reduced once (ring_at) and then stepped with a wrap.
constexpr uint32_t RING = 36864;
constexpr uint32_t STAGE_CHUNK = 2048;
TIFF_HD uint32_t ring_at(size_t p) { return (uint32_t)p % RING; }      // (segments are below 2^32 bytes: make_geom, the cap)
constexpr int TOKCAP = 4096;                                // tokens of one block
constexpr int MIN_MATCH = 3, MAX_MATCH = 258;
constexpr uint32_t MAX_DIST = 32768, TOO_FAR = 4096;        // a match of 3 bytes further away than TOO_FAR costs more than 3 literals
constexpr int NLL = 286, ND = 30, NCL = 19, DOFF = 288;     // alphabets; distance entries follow the literal/length ones at DOFF
constexpr int LL_LIMIT = 15, CL_LIMIT = 7;
constexpr uint32_t OBUF_WORDS = 128, OBUF_BITS = OBUF_WORDS * 32;
constexpr size_t STORED_MAX = 65535;

constexpr size_t CAP_DEFLATE = tiff::CAP_DEFLATE;           // what this writer writes the device reader reads on the device

TIFF_HD size_t segment_cap(int compression)
{
    return compression == tiff::COMP_DEFLATE ? CAP_DEFLATE : compression == tiff::COMP_NONE ? tiff::CAP_NONE : 0;
}

// Every block costs at most its stored form: 3 header bits, up to 7 bits to the byte, LEN and NLEN, for each 65535 bytes: 6
// bytes a stored block.  A block that is not the segment's last holds TOKCAP tokens, so at least TOKCAP bytes.  Around them
// the zlib header (2), the padding of the last block (1) and the Adler-32 (4).
TIFF_HD size_t bound(size_t n) { return n + 6 * (n / (size_t)TOKCAP + n / STORED_MAX + 2) + 2 + 1 + 4 + 8; }

TIFF_HD bool make_geom(const lbdrn_tiffw_layout& W, tiff::Geom* g)
{
    lbdrn_tiff_layout L;
    L.C = W.C; L.H = W.H; L.W = W.W; L.bits = W.bits; L.big_endian = W.big_endian; L.planar = W.planar; L.seg_w = W.seg_w;
    L.seg_h = W.seg_h; L.tiled = W.tiled; L.compression = W.compression; L.predictor = W.predictor;
    if (W.big_endian != 0 || (W.compression != tiff::COMP_NONE && W.compression != tiff::COMP_DEFLATE)) return false;
    return tiff::make_geom(L, g);
}

// where segment s starts when nothing is compressed: only a plane's last strip is short
TIFF_HD int64_t plain_offset(const tiff::Geom& g, int64_t s)
{
    const int64_t plane_bytes = g.tiled ? g.per_plane * g.seg_bytes : g.row_bytes * g.H;
    return (s / g.per_plane) * plane_bytes + (s % g.per_plane) * g.seg_bytes;
}

// ---------------------------------------------------------------- what the lanes of a step hand to each other

struct WaveScan {      // exclusive prefix sum over the lanes of a step, and its total
    uint32_t acc;
    TIFF_HD void init() { acc = 0; }
    TIFF_HD uint32_t excl(uint32_t v, int l)
    {
#if defined(__HIP_DEVICE_COMPILE__)
        uint32_t x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(x, o, 64);
            if (l >= o) x += up;
        }
        acc = __shfl(x, 63, 64);
        return x - v;
#else
        (void)l;
        const uint32_t r = acc;
        acc += v;
        return r;
#endif
    }
    TIFF_HD uint32_t total() const { return acc; }
};

struct WavePrev {      // the value of the lane before, across steps
    uint32_t carry;
    TIFF_HD void init() { carry = 0; }
    TIFF_HD uint32_t get(uint32_t v, int l)
    {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t up = __shfl_up(v, 1, 64);
        const uint32_t r = l == 0 ? carry : up;
        carry = __shfl(v, 63, 64);
        return r;
#else
        (void)l;
        const uint32_t r = carry;
        carry = v;
        return r;
#endif
    }
};

// ---------------------------------------------------------------- gather: one row of one segment

// planes[C][H][W] -> row r of segment s at seg (the segment's first byte): little-endian samples, chunky or planar, columns
// and rows outside the image zero, predictor 2 per sample channel over the whole row.  A strip's rows outside the image do
// not exist.
template <typename T>
TIFF_HD void gather_row(const tiff::Geom& g, const T* planes, int64_t s, int r, uint8_t* seg, int lane)
{
    const int rows = tiff::seg_rows(g, s);
    if (r >= rows && !g.tiled) return;
    uint8_t* dst = seg + (size_t)r * (size_t)g.row_bytes;
    const int64_t t = s % g.per_plane;
    const int x0 = (int)(t % g.segs_x) * g.seg_w;
    const int y = (int)(t / g.segs_x) * g.seg_h + (r < rows ? r : 0);
    const int cols = r < rows ? (g.seg_w < g.W - x0 ? g.seg_w : g.W - x0) : 0;
    const uint32_t mask = sizeof(T) == 1 ? 0xFFu : 0xFFFFu;
    for (int ch = 0; ch < g.spp; ++ch) {
        const int c = g.spp == 1 ? (int)(s / g.per_plane) : ch;
        const T* src = planes + ((size_t)c * g.H + (size_t)y) * g.W + x0;
        WavePrev pv;
        pv.init();
        for (int xb = 0; xb < g.seg_w; xb += WAVE) {
            TW_FOR_LANES(l, lane) {
                const int x = xb + l;
                const uint32_t v = x < cols ? (uint32_t)src[x] : 0u;
                uint32_t d = v;
                if (g.predictor == 2) d = (v - pv.get(v, l)) & mask;
                if (x < g.seg_w) {
                    uint8_t* q = dst + ((size_t)x * g.spp + ch) * sizeof(T);
                    q[0] = (uint8_t)d;
                    if (sizeof(T) == 2) q[1] = (uint8_t)(d >> 8);
                }
            }
        }
    }
}

// ---------------------------------------------------------------- Deflate: state

struct DeflateState {
    uint32_t ring[RING / 4];        // in[p] at byte ring_at(p)
    uint32_t head[HASH_SIZE];       // 1 + the latest position with that hash, 0: none
    uint32_t tok[TOKCAP];           // match: length << 16 | distance; literal: byte << 16
    uint32_t obuf[OBUF_WORDS];      // bits on their way out; byte 0 is out[ob]
    uint32_t mm[WAVE];              // the step's matches, as tokens; 0: none
    uint32_t hsh[WAVE];             // the step's hashes; HASH_SIZE: none
    uint32_t freq[DOFF + 32];       // histogram: literal/length at 0, distance at DOFF
    uint32_t clfreq[NCL + 1];
    uint32_t sortv[DOFF];           // build_lengths: frequencies in ascending order, then the tree in place
    uint32_t blc[16], nextc[16];    // codes of each length
    uint32_t tmp[4];
    uint32_t stats[4];              // blocks, tokens, kinds of block used (1 stored, 2 fixed, 4 dynamic), stored blocks
    uint16_t sorts[DOFF];           // build_lengths: symbols in ascending order of frequency
    uint16_t code[DOFF + 32];       // codes, bit-reversed: ready for an LSB-first stream
    uint16_t clcode[NCL + 1];
    uint16_t clsym[DOFF + 32];      // the code-length stream: symbol | extra bits << 8
    uint8_t len[DOFF + 32];         // code lengths
    uint8_t cllen[NCL + 1];
};

// ---------------------------------------------------------------- length-limited Huffman code lengths

// len[0 .. n) from freq[0 .. n): 0 for unused symbols, a minimum-redundancy code where that stays within `limit` bits, else
// the same code with its deepest leaves moved up until it fits (Kraft sum exactly 1 for two or more symbols; one symbol
// gets one bit).  The lanes share the ranking; lane 0 walks the tree (Moffat and Katajainen's in-place construction).
TIFF_HD void build_lengths(const uint32_t* freq, int n, int limit, uint8_t* len, DeflateState* st, int lane, int nl)
{
    TIFF_WAVE_FENCE();
    int m = 0;
    _Pragma("unroll 1") for (int s = 0; s < n; ++s) m += freq[s] != 0;
    _Pragma("unroll 1") for (int s = lane; s < n; s += nl) {
        const uint32_t f = freq[s];
        len[s] = 0;
        if (!f) continue;
        int rank = 0;
        _Pragma("unroll 1") for (int t = 0; t < n; ++t) {
            const uint32_t ft = freq[t];
            rank += ft != 0 && (ft < f || (ft == f && t < s));
        }
        st->sortv[rank] = f;
        st->sorts[rank] = (uint16_t)s;
    }
    TIFF_WAVE_FENCE();
    if (m == 0) return;
    if (lane == 0) {
        uint32_t* A = st->sortv;
        if (m == 1) {
            len[st->sorts[0]] = 1;
        } else {
            A[0] += A[1];
            int root = 0, leaf = 2;
            _Pragma("unroll 1") for (int next = 1; next < m - 1; ++next) {
                if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; }
                else A[next] = A[leaf++];
                if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; }
                else A[next] += A[leaf++];
            }
            A[m - 2] = 0;
            _Pragma("unroll 1") for (int next = m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
            int avbl = 1, used = 0, dpth = 0;
            root = m - 2;
            int next = m - 1;
            while (avbl > 0) {
                while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
                while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
                avbl = 2 * used;
                ++dpth;
                used = 0;
            }
            // A[i]: the depth of the i-th symbol in ascending order of frequency
            _Pragma("unroll 1") for (int l = 0; l < 16; ++l) st->blc[l] = 0;
            _Pragma("unroll 1") for (int i = 0; i < m; ++i) st->blc[(int)A[i] < limit ? (int)A[i] : limit]++;
            uint32_t total = 0;
            _Pragma("unroll 1") for (int l = 1; l <= limit; ++l) total += st->blc[l] << (limit - l);
            while (total > (1u << limit)) {      // one leaf off the deepest level, and a shallower leaf split to take it in
                st->blc[limit]--;
                _Pragma("unroll 1") for (int l = limit - 1; l > 0; --l)
                    if (st->blc[l]) { st->blc[l]--; st->blc[l + 1] += 2; break; }
                --total;
            }
            int i = 0;
            _Pragma("unroll 1") for (int l = limit; l >= 1; --l) {
                _Pragma("unroll 1") for (uint32_t k = 0; k < st->blc[l]; ++k) len[st->sorts[i++]] = (uint8_t)l;
            }
        }
    }
    TIFF_WAVE_FENCE();
}

// canonical codes of len[0 .. n), bit-reversed
TIFF_HD void gen_codes(const uint8_t* len, int n, uint16_t* code, DeflateState* st, int lane)
{
    TIFF_WAVE_FENCE();
    if (lane == 0) {
        _Pragma("unroll 1") for (int l = 0; l < 16; ++l) st->blc[l] = 0;
        _Pragma("unroll 1") for (int s = 0; s < n; ++s) st->blc[len[s] & 15]++;
        uint32_t c = 0;
        st->blc[0] = 0;
        _Pragma("unroll 1") for (int l = 1; l < 16; ++l) {
            c = (c + st->blc[l - 1]) << 1;
            st->nextc[l] = c;
        }
        _Pragma("unroll 1") for (int s = 0; s < n; ++s) {
            const int l = len[s] & 15;
            code[s] = l ? (uint16_t)tiff::reverse_bits(st->nextc[l]++, l) : (uint16_t)0;
        }
    }
    TIFF_WAVE_FENCE();
}

// ---------------------------------------------------------------- symbols of a token

TIFF_HD void length_symbol(uint32_t len, uint32_t* sym, uint32_t* eb, uint32_t* ex)
{
    const uint32_t l = len - 3u;
    if (l < 8u) { *sym = 257u + l; *eb = 0; *ex = 0; }
    else if (len == 258u) { *sym = 285u; *eb = 0; *ex = 0; }
    else {
        const uint32_t e = (uint32_t)(31 - __builtin_clz(l)) - 2u;
        *sym = 257u + 4u * (e + 1u) + ((l >> e) & 3u);
        *eb = e;
        *ex = l & ((1u << e) - 1u);
    }
}
TIFF_HD void dist_symbol(uint32_t dist, uint32_t* sym, uint32_t* eb, uint32_t* ex)
{
    const uint32_t d = dist - 1u;
    if (d < 4u) { *sym = d; *eb = 0; *ex = 0; }
    else {
        const uint32_t e = (uint32_t)(31 - __builtin_clz(d)) - 1u;
        *sym = 2u * (e + 1u) + ((d >> e) & 1u);
        *eb = e;
        *ex = d & ((1u << e) - 1u);
    }
}
TIFF_HD uint32_t ll_extra_bits(int s) { return s >= 265 && s < 285 ? (uint32_t)(s - 261) >> 2 : 0u; }
TIFF_HD uint32_t d_extra_bits(int s) { return s >= 4 ? (uint32_t)(s >> 1) - 1u : 0u; }
TIFF_HD uint32_t fixed_ll_len(int s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }
// the order in which the code-length code's lengths are sent: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
TIFF_HD int cl_order(int i)
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                        5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)(i < 12 ? (lo >> (5 * i)) & 31u : (hi >> (5 * (i - 12))) & 31u);
}

// ---------------------------------------------------------------- bits out

// v (nb <= 48 bits) into the words at bit offset `at`; other lanes may write the same words
TIFF_HD void or_bits(uint32_t* words, uint32_t at, uint64_t v, uint32_t nb)
{
    if (!nb) return;
    const uint32_t w = at >> 5, sh = at & 31u;
    const uint32_t lo = (uint32_t)v << sh;
    const uint64_t rest = sh ? v >> (32u - sh) : v >> 32;
    const uint32_t mid = (uint32_t)rest, hi = (uint32_t)(rest >> 32);
    if (lo) TW_OR(&words[w], lo);
    if (mid) TW_OR(&words[w + 1], mid);
    if (hi) TW_OR(&words[w + 2], hi);
}

struct BitOut {
    uint8_t* out;
    size_t cap;
    uint32_t* obuf;
    uint64_t bp;       // bits written so far
    uint64_t ob;       // out[ob] is byte 0 of obuf; whole bytes before it are in out
    int lane, nl;
    TIFF_HD void init(uint8_t* o, size_t c, uint32_t* b, int lane_, int nl_)
    {
        out = o; cap = c; obuf = b; bp = 0; ob = 0; lane = lane_; nl = nl_;
        for (uint32_t k = (uint32_t)lane; k < OBUF_WORDS; k += (uint32_t)nl) obuf[k] = 0;
        TIFF_WAVE_FENCE();
    }
    TIFF_HD uint32_t rel() const { return (uint32_t)(bp - ob * 8u); }
    // whole bytes to out; the bits of a started byte stay
    TIFF_HD void flush()
    {
        TIFF_WAVE_FENCE();
        const uint32_t full = (uint32_t)((bp >> 3) - ob);
        for (uint32_t k = (uint32_t)lane; k < full; k += (uint32_t)nl)
            if (ob + k < cap) out[ob + k] = (uint8_t)(obuf[k >> 2] >> (8u * (k & 3u)));
        const uint32_t part = (bp & 7u) ? (obuf[full >> 2] >> (8u * (full & 3u))) & 0xFFu : 0u;
        TIFF_WAVE_FENCE();
        for (uint32_t k = (uint32_t)lane; k < OBUF_WORDS; k += (uint32_t)nl) obuf[k] = k ? 0u : part;
        TIFF_WAVE_FENCE();
        ob += full;
    }
    // wave-uniform: nb <= 32 bits, stored by lane 0
    TIFF_HD void put(uint32_t v, uint32_t nb)
    {
        if (rel() + 64u > OBUF_BITS) flush();
        if (lane == 0) or_bits(obuf, rel(), v, nb);
        bp += nb;
    }
    TIFF_HD void align() { bp = (bp + 7u) & ~(uint64_t)7u; }
};

// ---------------------------------------------------------------- one block

// the code-length stream of lens[0 .. nll) and lens[DOFF .. DOFF + nd): run-length coded with 16 / 17 / 18; lane 0
TIFF_HD uint32_t rle_lengths(const uint8_t* len, int nll, int nd, uint16_t* clsym)
{
    const int total = nll + nd;
    uint32_t out = 0;
    int i = 0;
    while (i < total) {
        const uint32_t v = len[i < nll ? i : DOFF + (i - nll)];
        int run = 1;
        while (i + run < total && len[i + run < nll ? i + run : DOFF + (i + run - nll)] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) { const int r = run < 138 ? run : 138; clsym[out++] = (uint16_t)(18u | (uint32_t)(r - 11) << 8); run -= r; }
            if (run >= 3) { clsym[out++] = (uint16_t)(17u | (uint32_t)(run - 3) << 8); run = 0; }
            while (run-- > 0) clsym[out++] = 0;
        } else {
            clsym[out++] = (uint16_t)v;
            --run;
            while (run >= 3) { const int r = run < 6 ? run : 6; clsym[out++] = (uint16_t)(16u | (uint32_t)(r - 3) << 8); run -= r; }
            while (run-- > 0) clsym[out++] = (uint16_t)v;
        }
    }
    return out;
}

// the ntok tokens of st->tok cover in[bstart .. bend): written as the cheapest of a dynamic block, a fixed block and stored
// blocks, by exact bit count
TIFF_HD void flush_block(DeflateState* st, BitOut* bo, const uint8_t* in, size_t bstart, size_t bend, uint32_t ntok, uint32_t final_,
                         int lane, int nl)
{
    TIFF_WAVE_FENCE();
    for (int k = lane; k < DOFF + 32; k += nl) { st->freq[k] = 0; st->len[k] = 0; }
    for (int k = lane; k < NCL + 1; k += nl) st->clfreq[k] = 0;
    TIFF_WAVE_FENCE();
    for (uint32_t i = (uint32_t)lane; i < ntok; i += (uint32_t)nl) {
        const uint32_t t = st->tok[i];
        if (t & 0xFFFFu) {
            uint32_t s, eb, ex;
            length_symbol(t >> 16, &s, &eb, &ex);
            TW_ADD(&st->freq[s], 1u);
            dist_symbol(t & 0xFFFFu, &s, &eb, &ex);
            TW_ADD(&st->freq[DOFF + s], 1u);
        } else {
            TW_ADD(&st->freq[t >> 16], 1u);
        }
    }
    if (lane == 0) TW_ADD(&st->freq[256], 1u);
    build_lengths(st->freq, NLL, LL_LIMIT, st->len, st, lane, nl);
    build_lengths(st->freq + DOFF, ND, LL_LIMIT, st->len + DOFF, st, lane, nl);
    int nll = 257, nd = 1;
    _Pragma("unroll 1") for (int s = 257; s < NLL; ++s) if (st->len[s]) nll = s + 1;
    _Pragma("unroll 1") for (int s = 1; s < ND; ++s) if (st->len[DOFF + s]) nd = s + 1;
    if (lane == 0) {
        const uint32_t ncl = rle_lengths(st->len, nll, nd, st->clsym);
        st->tmp[0] = ncl;
        int used = 0;
        _Pragma("unroll 1") for (uint32_t i = 0; i < ncl; ++i) used += st->clfreq[st->clsym[i] & 0xFFu]++ == 0;
        if (used < 2) st->clfreq[st->clfreq[0] ? 1 : 0]++;      // the code-length code must be complete: two codes of one bit
    }
    build_lengths(st->clfreq, NCL, CL_LIMIT, st->cllen, st, lane, nl);
    const uint32_t ncl = st->tmp[0];
    int hclen = 4;
    _Pragma("unroll 1") for (int k = NCL - 1; k >= 4; --k) if (st->cllen[cl_order(k)]) { hclen = k + 1; break; }

    // the three costs, in bits
    uint64_t dyn = 0, fix = 0;
    for (int s = lane; s < NLL; s += nl) {
        const uint64_t f = st->freq[s];
        dyn += f * (st->len[s] + ll_extra_bits(s));
        fix += f * (fixed_ll_len(s) + ll_extra_bits(s));
    }
    for (int s = lane; s < ND; s += nl) {
        const uint64_t f = st->freq[DOFF + s];
        dyn += f * (st->len[DOFF + s] + d_extra_bits(s));
        fix += f * (5u + d_extra_bits(s));
    }
    for (uint32_t i = (uint32_t)lane; i < ncl; i += (uint32_t)nl) {
        const uint32_t s = st->clsym[i] & 0xFFu;
        dyn += st->cllen[s] + (s == 16u ? 2u : s == 17u ? 3u : s == 18u ? 7u : 0u);
    }
    dyn = tiff::lane_sum(dyn, nl) + 3u + 14u + 3u * (uint32_t)hclen;
    fix = tiff::lane_sum(fix, nl) + 3u;
    const size_t blen = bend - bstart;
    const size_t chunks = blen ? (blen + STORED_MAX - 1) / STORED_MAX : 1;
    const uint64_t pad = (8u - ((bo->bp + 3u) & 7u)) & 7u;
    const uint64_t sto = 3u + pad + 32u + (uint64_t)(chunks - 1) * 40u + 8u * (uint64_t)blen;
    const int kind = sto < dyn && sto < fix ? 1 : fix <= dyn ? 2 : 4;
    if (lane == 0) {
        st->stats[0]++;
        st->stats[1] += ntok;
        st->stats[2] |= (uint32_t)kind;
        if (kind == 1) st->stats[3] += (uint32_t)chunks;
    }

    if (kind == 1) {
        size_t at = bstart;
        for (size_t c = 0; c < chunks; ++c) {
            const size_t take = bend - at < STORED_MAX ? bend - at : STORED_MAX;
            bo->put(final_ && c + 1 == chunks ? 1u : 0u, 1);
            bo->put(0u, 2);
            bo->align();
            bo->put((uint32_t)take, 16);
            bo->put((uint32_t)take ^ 0xFFFFu, 16);
            bo->flush();      // on a byte boundary now, nothing left in obuf
            for (size_t i = (size_t)lane; i < take; i += (size_t)nl)
                if (bo->ob + i < bo->cap) bo->out[bo->ob + i] = in[at + i];
            bo->ob += take;
            bo->bp += 8u * (uint64_t)take;
            at += take;
        }
        return;
    }

    bo->put(final_, 1);
    if (kind == 2) {
        bo->put(1u, 2);
        TIFF_WAVE_FENCE();
        for (int s = lane; s < DOFF; s += nl) st->len[s] = (uint8_t)fixed_ll_len(s);
        for (int s = lane; s < 32; s += nl) st->len[DOFF + s] = 5;
        gen_codes(st->len, DOFF, st->code, st, lane);
        gen_codes(st->len + DOFF, 32, st->code + DOFF, st, lane);
    } else {
        bo->put(2u, 2);
        gen_codes(st->len, NLL, st->code, st, lane);
        gen_codes(st->len + DOFF, ND, st->code + DOFF, st, lane);
        gen_codes(st->cllen, NCL, st->clcode, st, lane);
        bo->put((uint32_t)(nll - 257), 5);
        bo->put((uint32_t)(nd - 1), 5);
        bo->put((uint32_t)(hclen - 4), 4);
        for (int k = 0; k < hclen; ++k) bo->put(st->cllen[cl_order(k)], 3);
        for (uint32_t i = 0; i < ncl; ++i) {
            const uint32_t e = st->clsym[i], s = e & 0xFFu;
            bo->put(st->clcode[s], st->cllen[s]);
            if (s >= 16u) bo->put(e >> 8, s == 16u ? 2u : s == 17u ? 3u : 7u);
        }
    }
    bo->flush();
    // the tokens, 64 a step: each lane's bits, a prefix sum of their lengths, and every lane ORs its bits into place
    for (uint32_t base = 0; base < ntok; base += WAVE) {
        WaveScan sc;
        sc.init();
        const uint32_t rel = bo->rel();      // < 8 after a flush; 64 tokens of at most 48 bits fit behind it
        TW_FOR_LANES(l, lane) {
            const uint32_t i = base + (uint32_t)l;
            uint64_t bits = 0;
            uint32_t nb = 0;
            if (i < ntok) {
                const uint32_t t = st->tok[i];
                if (t & 0xFFFFu) {
                    uint32_t s, eb, ex;
                    length_symbol(t >> 16, &s, &eb, &ex);
                    bits = st->code[s]; nb = st->len[s];
                    bits |= (uint64_t)ex << nb; nb += eb;
                    dist_symbol(t & 0xFFFFu, &s, &eb, &ex);
                    bits |= (uint64_t)st->code[DOFF + s] << nb; nb += st->len[DOFF + s];
                    bits |= (uint64_t)ex << nb; nb += eb;
                } else {
                    bits = st->code[t >> 16]; nb = st->len[t >> 16];
                }
            }
            const uint32_t off = sc.excl(nb, l);
            or_bits(bo->obuf, rel + off, bits, nb);
        }
        bo->bp += sc.total();
        bo->flush();
    }
    bo->put(st->code[256], st->len[256]);
}

// ---------------------------------------------------------------- one segment

TIFF_HD uint32_t match_length(const uint8_t* rb, size_t a, size_t b, uint32_t maxl)
{
    uint32_t k = 0, ia = ring_at(a), ib = ring_at(b);
    while (k < maxl && rb[ia] == rb[ib]) {
        ++k;
        if (++ia == RING) ia = 0;
        if (++ib == RING) ib = 0;
    }
    return k;
}

// in[0 .. n), n >= 1 -> a zlib stream in out[0 .. cap); returns its size (at most bound(n))
TIFF_HD size_t deflate(const uint8_t* in, size_t n, uint8_t* out, size_t cap, DeflateState* st, int lane, int nl)
{
    for (int k = lane; k < HASH_SIZE; k += nl) st->head[k] = 0;
    if (lane == 0) st->stats[0] = st->stats[1] = st->stats[2] = st->stats[3] = 0;
    BitOut bo;
    bo.init(out, cap, st->obuf, lane, nl);
    bo.put(0x78u, 8);      // Deflate, 32 KiB window
    bo.put(0x01u, 8);      // no dictionary, fastest; 0x7801 is a multiple of 31
    const uint8_t* rb = (const uint8_t*)st->ring;
    size_t staged = 0, cur = 0, bstart = 0;
    uint32_t ntok = 0;
    for (size_t p0 = 0; p0 < n; p0 += WAVE) {
        // the segment passes through the ring a chunk at a time, whole words where the segment has them
        size_t need = p0 + WAVE + MAX_MATCH + 4;
        if (need > n) need = n;
        while (staged < need) {
            TIFF_WAVE_FENCE();
            for (uint32_t k = (uint32_t)lane; k < STAGE_CHUNK / 4; k += (uint32_t)nl) {
                const size_t at = staged + 4u * (size_t)k;
                if (at + 4 <= n) {
                    uint32_t w;
                    memcpy(&w, in + at, 4);
                    st->ring[ring_at(at) >> 2] = w;      // (at and RING are multiples of 4)
                } else {
                    for (size_t j = at; j < n; ++j) ((uint8_t*)st->ring)[ring_at(j)] = in[j];
                }
            }
            staged += STAGE_CHUNK;
            TIFF_WAVE_FENCE();
        }
        // the step's 64 positions: each lane hashes its own, looks up the latest earlier position with that hash (from
        // before this step) and the byte before it, and measures both matches
        const bool search = cur < p0 + WAVE;
        TW_FOR_LANES(l, lane) {
            const size_t p = p0 + (size_t)l;
            uint32_t h = HASH_SIZE, best = 0, bdist = 0;
            if (p + 3 <= n) {
                const uint32_t v = (uint32_t)rb[ring_at(p)] | (uint32_t)rb[ring_at(p + 1)] << 8 | (uint32_t)rb[ring_at(p + 2)] << 16;
                h = (v * 2654435761u) >> (32 - HASH_BITS);
                if (search && p >= cur) {
                    const uint32_t maxl = n - p < (size_t)MAX_MATCH ? (uint32_t)(n - p) : (uint32_t)MAX_MATCH;
                    const uint32_t c1 = st->head[h];
                    if (c1 && p - (size_t)(c1 - 1u) <= (size_t)MAX_DIST) {
                        best = match_length(rb, (size_t)(c1 - 1u), p, maxl);
                        bdist = (uint32_t)(p - (size_t)(c1 - 1u));
                    }
                    if (p >= 1) {
                        const uint32_t l1 = match_length(rb, p - 1, p, maxl);
                        if (l1 >= best) { best = l1; bdist = 1; }
                    }
                    if (best < (uint32_t)MIN_MATCH || (best == (uint32_t)MIN_MATCH && bdist > TOO_FAR)) best = 0;
                }
            }
            st->mm[l] = best ? (best << 16) | bdist : 0u;
            st->hsh[l] = h;
        }
        TIFF_WAVE_FENCE();
        TW_FOR_LANES(l, lane) {
            const uint32_t h = st->hsh[l];
            if (h < (uint32_t)HASH_SIZE) TW_MAX(&st->head[h], (uint32_t)(p0 + (size_t)l) + 1u);
        }
        TIFF_WAVE_FENCE();
        // greedy selection, wave-uniform
        const size_t end = p0 + WAVE < n ? p0 + WAVE : n;
        while (cur < end) {
            if (ntok == (uint32_t)TOKCAP) {
                flush_block(st, &bo, in, bstart, cur, ntok, 0u, lane, nl);
                ntok = 0;
                bstart = cur;
            }
            const uint32_t m = st->mm[cur - p0];
            const uint32_t t = m ? m : (uint32_t)rb[ring_at(cur)] << 16;
            if (lane == 0) st->tok[ntok] = t;
            ++ntok;
            cur += m ? (size_t)(m >> 16) : 1;
        }
    }
    flush_block(st, &bo, in, bstart, n, ntok, 1u, lane, nl);
    bo.align();
    const uint32_t check = tiff::adler32(in, n, lane, nl);
    bo.put(check >> 24, 8);
    bo.put((check >> 16) & 0xFFu, 8);
    bo.put((check >> 8) & 0xFFu, 8);
    bo.put(check & 0xFFu, 8);
    bo.flush();
    TIFF_WAVE_FENCE();
    return (size_t)(bo.bp >> 3);
}

}  // namespace tiffw
