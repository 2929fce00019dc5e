// The residual layer's format text ("LBR1", include/lbdrn_resid.h), written once for the device and the host: the
// quantiser, the per-row Rice coder and decoder, the bit gather that concatenates a block's rows, the header and the
// host-side validation of a body's tables.  csrc/resid.hip compiles it for the kernels, tests/resid_host_shim.cpp and
// tests/resid_damage_main.cpp compile the same text with a host compiler.  No state, no allocation, no I/O.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#if defined(__HIPCC__)
#define RESID_HD __host__ __device__ inline
#else
#define RESID_HD inline
#endif

namespace resid {

constexpr int BLOCK_ROWS = 64;       // rows of a block = lanes of the wave that codes it
constexpr int BLOCK_COLS = 256;
constexpr int K_BITS = 4;            // a non-empty row starts with its Rice parameter
constexpr int K_MAX = 15;
constexpr int ESC_Q = 24;            // a unary quotient of 24 ones announces the raw value
constexpr int RAW_BITS = 17;         // u <= 131071
constexpr int ESC_BITS = ESC_Q + RAW_BITS;
constexpr uint32_t U_LIMIT = (1u << RAW_BITS) - 1u;
constexpr int ROW_MAX_BITS = K_BITS + BLOCK_COLS * ESC_BITS;      // 10500: the format's bound (fits the u16 row length);
                                                                 // what a reader accepts and lbdrn_resid_bound counts
// What the coder can write is less: it takes the cheapest parameter, so no row costs more than it does under k = 15, where
// u >> 15 <= 3 and a sample is at most 3 + 1 + 15 bits.  The lanes' private streams are sized by that.
constexpr int ROW_CODED_MAX_BITS = K_BITS + BLOCK_COLS * ((int)(U_LIMIT >> K_MAX) + 1 + K_MAX);      // 4868
constexpr int ROW_WORDS = (ROW_CODED_MAX_BITS + 31) / 32;        // 153: a lane's private stream, 32-bit words
constexpr int HEADER_BYTES = 20;
constexpr int VERSION = 1;
constexpr int MAX_C = 65535, MAX_SIDE = 1 << 20;
constexpr int64_t MAX_BLOCKS = (int64_t)1 << 30;

static_assert(ROW_MAX_BITS < 65536, "a row's bit length is stored in 16 bits");
static_assert((U_LIMIT >> K_MAX) < (uint32_t)ESC_Q, "under k = 15 no sample escapes: ROW_CODED_MAX_BITS holds");

// ---------------------------------------------------------------- geometry

struct Geom {
    int C, H, W, nbx, nby;
    int64_t nblocks;
};

RESID_HD bool make_geom(int64_t C, int64_t H, int64_t W, Geom* g)
{
    if (C < 1 || H < 1 || W < 1 || C > MAX_C || H > MAX_SIDE || W > MAX_SIDE) return false;
    g->C = (int)C; g->H = (int)H; g->W = (int)W;
    g->nbx = (int)((W + BLOCK_COLS - 1) / BLOCK_COLS);
    g->nby = (int)((H + BLOCK_ROWS - 1) / BLOCK_ROWS);
    g->nblocks = C * g->nbx * g->nby;
    return g->nblocks <= MAX_BLOCKS;
}
RESID_HD int block_rows(const Geom& g, int by) { return g.H - by * BLOCK_ROWS < BLOCK_ROWS ? g.H - by * BLOCK_ROWS : BLOCK_ROWS; }
RESID_HD int block_cols(const Geom& g, int bx) { return g.W - bx * BLOCK_COLS < BLOCK_COLS ? g.W - bx * BLOCK_COLS : BLOCK_COLS; }
// the most bytes a block of this size can take: the row lengths, every sample escaped, padding
RESID_HD uint32_t block_bound(int rows, int cols)
{
    return 2u * (uint32_t)rows + ((uint32_t)rows * (uint32_t)(K_BITS + cols * ESC_BITS) + 7u) / 8u;
}
RESID_HD size_t body_bound(const Geom& g)
{
    size_t total = (size_t)HEADER_BYTES + 4 * (size_t)g.nblocks;
    const int ry[2] = {BLOCK_ROWS, g.H % BLOCK_ROWS}, rx[2] = {BLOCK_COLS, g.W % BLOCK_COLS};
    const size_t ny[2] = {(size_t)(g.H / BLOCK_ROWS), g.H % BLOCK_ROWS ? (size_t)1 : 0};
    const size_t nx[2] = {(size_t)(g.W / BLOCK_COLS), g.W % BLOCK_COLS ? (size_t)1 : 0};
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
            if (ny[i] && nx[j]) total += (size_t)g.C * ny[i] * nx[j] * block_bound(ry[i], rx[j]);
    return total;
}

// ---------------------------------------------------------------- quantiser (orig, recon in 0..65535; 0 <= tau <= 65535)

RESID_HD int32_t quantise(int32_t orig, int32_t recon, int32_t tau)
{
    const int32_t e = orig - recon, a = e < 0 ? -e : e;
    const int32_t q = (a + tau) / (2 * tau + 1);
    return e < 0 ? -q : q;
}
RESID_HD uint32_t fold(int32_t q) { return q >= 0 ? 2u * (uint32_t)q : 2u * (uint32_t)(-q) - 1u; }
RESID_HD int32_t unfold(uint32_t u) { return (u & 1u) ? -(int32_t)((u + 1u) >> 1) : (int32_t)(u >> 1); }
RESID_HD uint32_t max_symbol(int32_t tau) { return 2u * (uint32_t)((65535 + tau) / (2 * tau + 1)); }
RESID_HD uint16_t enhance(int32_t recon, int32_t q, int32_t tau)
{
    const int64_t v = (int64_t)recon + (int64_t)q * (2 * (int64_t)tau + 1);
    return (uint16_t)(v < 0 ? 0 : (v > 65535 ? 65535 : v));
}

// ---------------------------------------------------------------- the row coder

RESID_HD uint32_t symbol_bits(uint32_t u, int k)
{
    const uint32_t q = u >> k;
    return q >= (uint32_t)ESC_Q ? (uint32_t)ESC_BITS : q + 1u + (uint32_t)k;
}

struct RowCost {          // the bits of a row under each parameter, fed one sample at a time
    uint32_t c[K_MAX + 1];
    uint32_t any;
    RESID_HD void init()
    {
#pragma unroll
        for (int k = 0; k <= K_MAX; ++k) c[k] = 0;
        any = 0;
    }
    RESID_HD void add(uint32_t u)
    {
        any |= u;
#pragma unroll
        for (int k = 0; k <= K_MAX; ++k) c[k] += symbol_bits(u, k);
    }
    // the parameter with the fewest bits, the lowest on a tie; *bits = the row's length (0 for a row of zeros)
    RESID_HD int pick(uint32_t* bits) const
    {
        if (!any) { *bits = 0; return 0; }
        int best = 0;
        uint32_t lo = c[0];
#pragma unroll
        for (int k = 1; k <= K_MAX; ++k)
            if (c[k] < lo) { lo = c[k]; best = k; }
        *bits = (uint32_t)K_BITS + lo;
        return best;
    }
};

struct RowWriter {        // MSB-first into 32-bit words (bit 31 of word 0 is the stream's first bit)
    uint32_t* w;
    uint64_t acc;
    int nb, n;
    RESID_HD void init(uint32_t* words) { w = words; acc = 0; nb = 0; n = 0; }
    RESID_HD void put(uint32_t code, int len)      // len <= 24
    {
        acc = (acc << len) | code;
        nb += len;
        if (nb >= 32) {
            w[n++] = (uint32_t)(acc >> (nb - 32));
            nb -= 32;
        }
    }
    RESID_HD void symbol(uint32_t u, int k)
    {
        const uint32_t q = u >> k;
        if (q >= (uint32_t)ESC_Q) {
            put(0xFFFFFFu, ESC_Q);
            put(u & U_LIMIT, RAW_BITS);
        } else {
            put(((1u << q) - 1u) << 1, (int)q + 1);
            if (k) put(u & ((1u << k) - 1u), k);
        }
    }
    RESID_HD void finish()
    {
        if (nb) w[n++] = (uint32_t)(acc << (32 - nb));
        nb = 0;
    }
};

// n <= BLOCK_COLS samples u[0], u[stride], ... (each <= U_LIMIT) -> words (at most ROW_WORDS); returns the row's bits
RESID_HD uint32_t encode_row(const uint32_t* u, int n, int stride, uint32_t* words)
{
    RowCost rc;
    rc.init();
    for (int j = 0; j < n; ++j) rc.add(u[(size_t)j * stride]);
    uint32_t bits;
    const int k = rc.pick(&bits);
    if (!bits) return 0;
    RowWriter wr;
    wr.init(words);
    wr.put((uint32_t)k, K_BITS);
    for (int j = 0; j < n; ++j) wr.symbol(u[(size_t)j * stride], k);
    wr.finish();
    return bits;
}

struct RowReader {        // reads bits [start, start + len) of p[0 .. limit); whatever lies beyond reads as zero
    const uint8_t* p;
    uint64_t acc;
    uint32_t byte, endbyte;
    int nb;
    int64_t left;
    bool bad;
    RESID_HD void fill()
    {
        while (nb <= 56 && byte < endbyte) {
            acc |= (uint64_t)p[byte++] << (56 - nb);
            nb += 8;
        }
    }
    RESID_HD void take(int len)
    {
        acc <<= len;
        nb = nb > len ? nb - len : 0;
        left -= len;
        if (left < 0) bad = true;
    }
    RESID_HD void init(const uint8_t* data, uint32_t limit, uint64_t start, uint32_t len)
    {
        p = data; acc = 0; nb = 0; bad = false;
        const uint64_t last = (start + len + 7) >> 3;
        byte = (uint32_t)((start >> 3) < limit ? (start >> 3) : limit);
        endbyte = (uint32_t)(last < limit ? last : limit);
        left = (int64_t)len + (int64_t)(start & 7);
        fill();
        take((int)(start & 7));
    }
    RESID_HD int parameter()
    {
        fill();
        const int k = (int)(acc >> 60);
        take(K_BITS);
        return k;
    }
    RESID_HD uint32_t symbol(int k)
    {
        fill();
        const uint32_t inv = ~(uint32_t)(acc >> 32);
        const int ones = inv ? __builtin_clz(inv) : 32;
        if (ones >= ESC_Q) {
            const uint32_t u = (uint32_t)(acc >> (64 - ESC_BITS)) & U_LIMIT;
            take(ESC_BITS);
            return u;
        }
        const int len = ones + 1 + k;
        const uint32_t rem = k ? (uint32_t)(acc >> (64 - len)) & ((1u << k) - 1u) : 0u;
        take(len);
        return ((uint32_t)ones << k) | rem;
    }
};

// the inverse of encode_row on bits [start, start + len) of p[0 .. limit).  false: the row is damaged (its samples are
// then unspecified values <= U_LIMIT); nothing outside p[0 .. limit) is read, nothing outside the n samples written.
RESID_HD bool decode_row(const uint8_t* p, uint32_t limit, uint64_t start, uint32_t len, int n, uint32_t* u, int stride)
{
    if (len == 0) {
        for (int j = 0; j < n; ++j) u[(size_t)j * stride] = 0;
        return true;
    }
    RowReader rd;
    rd.init(p, limit, start, len);
    const int k = rd.parameter();
    for (int j = 0; j < n; ++j) u[(size_t)j * stride] = rd.symbol(k);
    return !rd.bad && rd.left == 0 && len > (uint32_t)K_BITS;
}

// ---------------------------------------------------------------- a block: row lengths, then the rows bit by bit

// Byte t of a block's concatenated rows.  start[r] is row r's first bit in the concatenation (start[rows] its length);
// row r's bits are the words priv[r * pitch ...] as RowWriter left them.
RESID_HD uint32_t gather_byte(const uint32_t* start, int rows, const uint32_t* priv, size_t pitch, uint32_t t)
{
    uint32_t pos = 8u * t;
    const uint32_t end = pos + 8u < start[rows] ? pos + 8u : start[rows];
    int lo = 0, hi = rows;                       // the last row that starts at or before pos
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= pos) lo = mid; else hi = mid;
    }
    int r = lo, got = 0;
    uint32_t out = 0;
    while (pos < end) {
        while (start[r + 1] <= pos) ++r;         // empty rows
        const uint32_t off = pos - start[r];
        const uint32_t n = (end < start[r + 1] ? end : start[r + 1]) - pos;      // 1..8
        const uint32_t* w = priv + (size_t)r * pitch;
        const uint32_t wi = off >> 5, bi = off & 31u;
        const uint64_t two = ((uint64_t)w[wi] << 32) | (bi + n > 32u ? (uint64_t)w[wi + 1] : 0u);
        out = (out << n) | ((uint32_t)(two >> (64u - bi - n)) & ((1u << n) - 1u));
        got += (int)n;
        pos += n;
    }
    return (out << (8 - got)) & 0xFFu;
}

// ---------------------------------------------------------------- header and tables

struct Header {
    uint32_t tau, C, H, W;
};

RESID_HD uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
RESID_HD uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

RESID_HD void write_header(uint8_t* p, uint32_t tau, uint32_t C, uint32_t H, uint32_t W)
{
    p[0] = 'L'; p[1] = 'B'; p[2] = 'R'; p[3] = '1';
    p[4] = (uint8_t)VERSION; p[5] = 0;
    p[6] = (uint8_t)tau; p[7] = (uint8_t)(tau >> 8);
    const uint32_t v[3] = {C, H, W};
    for (int i = 0; i < 3; ++i)
        for (int b = 0; b < 4; ++b) p[8 + 4 * i + b] = (uint8_t)(v[i] >> (8 * b));
}
RESID_HD bool read_header(const uint8_t* p, Header* h)      // p holds HEADER_BYTES
{
    if (p[0] != 'L' || p[1] != 'B' || p[2] != 'R' || p[3] != '1' || p[4] != VERSION || p[5] != 0) return false;
    h->tau = le16(p + 6); h->C = le32(p + 8); h->H = le32(p + 12); h->W = le32(p + 16);
    return true;
}

// A block's own table: the row lengths must add up to exactly the block's bytes.  start (optional): rows + 1 bit offsets
// from the block's first byte.
RESID_HD bool check_block(const uint8_t* blk, uint32_t blen, int rows, int cols, uint32_t* start)
{
    if (blen < 2u * (uint32_t)rows || blen > block_bound(rows, cols)) return false;
    uint32_t bits = 16u * (uint32_t)rows;
    for (int r = 0; r < rows; ++r) {
        const uint32_t len = le16(blk + 2 * r);
        if ((len && len <= (uint32_t)K_BITS) || len > (uint32_t)(K_BITS + cols * ESC_BITS)) return false;
        if (start) start[r] = bits;
        bits += len;
    }
    if (start) start[rows] = bits;
    return (bits + 7u) / 8u == blen;
}

// Host: the whole body's header, block table and every block's row lengths.  0, or -1 and a message.
inline int check_body(const uint8_t* body, size_t n, Header* h, char* msg, size_t cap)
{
    Geom g;
    if (n < (size_t)HEADER_BYTES || !read_header(body, h)) {
        snprintf(msg, cap, "not an LBR1 body (%zu bytes; magic, version or reserved byte)", n);
        return -1;
    }
    if (!make_geom(h->C, h->H, h->W, &g)) {
        snprintf(msg, cap, "LBR1 geometry %u x %u x %u is out of range", h->C, h->H, h->W);
        return -1;
    }
    if ((n - HEADER_BYTES) / 4 < (size_t)g.nblocks) {
        snprintf(msg, cap, "LBR1 body of %zu bytes cannot hold the table of %lld blocks", n, (long long)g.nblocks);
        return -1;
    }
    const uint8_t* table = body + HEADER_BYTES;
    const size_t data = n - HEADER_BYTES - 4 * (size_t)g.nblocks;
    size_t off = 0;
    int64_t b = 0;
    for (int c = 0; c < g.C; ++c)
        for (int by = 0; by < g.nby; ++by)
            for (int bx = 0; bx < g.nbx; ++bx, ++b) {
                const uint32_t blen = le32(table + 4 * b);
                if (blen > data - off || !check_block(table + 4 * (size_t)g.nblocks + off, blen, block_rows(g, by), block_cols(g, bx), nullptr)) {
                    snprintf(msg, cap, "LBR1 block %lld: %u bytes do not match its row lengths or overrun the body", (long long)b, blen);
                    return -1;
                }
                off += blen;
            }
    if (off != data) {
        snprintf(msg, cap, "LBR1 body has %zu bytes behind its last block", data - off);
        return -1;
    }
    return 0;
}

}  // namespace resid
