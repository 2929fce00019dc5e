/* JPEG 2000 Part 1 (ITU-T T.800) oracle for the GPU encoder of csrc/jp2k.hip: reversible 5/3 transform, tier-1 coder
 * and decoder, geometry, tier-2 writer and parser, whole files -- written from the standard in its textbook form and
 * sharing no text with csrc/.  TEST INFRASTRUCTURE: slow, plain, one sample at a time.
 *
 *   transform   sequential lifting on a line (extend, predict the odd samples, update the even ones, deinterleave),
 *               columns then rows, level by level (F.3 / F.4), for any parity of the line's first coordinate
 *   tier-1      one flag byte per sample inside a one-sample border, the scan of D.1 sample by sample, the contexts
 *               of Tables D.1 - D.4 as tables, the MQ coder of the Annex C flowcharts
 *   geometry    B.5 - B.7 with ceiling divisions of tile coordinates
 *   tier-2      B.10 packet headers (tag trees, Table B.4, Lblock, bit stuffing), A.4 - A.6 marker segments, I.5 boxes
 *
 * What the standard leaves to an encoder, and this one takes from the product (csrc/jp2k_t2.inc) so that
 * the two files can be compared byte for byte -- nothing else is shared:
 *   1. the coding parameters of csrc/jp2_shim.c: unsigned 8 / 16 bit components, tiles of 1024 x 1024 when a side
 *      exceeds 1024, LRCP, one layer, no component transform, 64 x 64 code blocks of style 0, 5/3, up to five
 *      decompositions (as many as keep one sample of the shorter side), one precinct per resolution, no
 *      quantisation (exponent = bits + gain), two guard bits
 *   2. no COM segment
 *   3. one tile-part per tile
 *   4. a packet without any included block is written as a single 0 bit
 *   5. Lblock grows by the fewest increments that make the length fit
 *   6. every block is one codeword segment over all passes from its first non-zero bit-plane, closed by the C.2.9
 *      flush, a trailing 0xFF dropped
 *   7. the JP2 boxes: signature, ftyp (brand and compatibility "jp2 "), jp2h with ihdr and an enumerated colr
 *      (sRGB for three components, greyscale for one, 0 otherwise), jp2c with its true length
 * The decoder and the parser accept more than the encoder writes (COM segments, non-included blocks inside non-empty
 * packets, SOP / EPH, other code-block sizes and resolution counts), since they also read OpenJPEG's and Pillow's files.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static char g_err[256];
const char *jo_last_error(void) { return g_err; }
#define FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

/* ------------------------------------------------------------------ counters: which rarely taken paths were taken */
enum {
    CNT_RL_EXIT0 = 0, /* .. 3: run-length mode left at row 0..3 */
    CNT_RL_ZERO = 4,  /* run-length mode, four zeros */
    CNT_PARTIAL_STRIPE = 5, CNT_NARROW_BLOCK = 6, CNT_PASSES_16BIT = 7, CNT_LBLOCK_INC = 8, CNT_HEADER_STUFF = 9,
    CNT_TREE_NOT_POW2 = 10, CNT_EMPTY_BAND_BESIDE_FULL = 11, CNT_EMPTY_PACKET = 12,
    CNT_PASS_ROW0 = 13, /* .. 17: rows of Table B.4 */
    CNT_EXCLUDED_IN_FULL_PACKET = 18, CNT_N = 24
};
static uint64_t g_cnt[CNT_N];
void jo_counters(uint64_t *out, int reset)
{
    if (out) memcpy(out, g_cnt, sizeof g_cnt);
    if (reset) memset(g_cnt, 0, sizeof g_cnt);
}

static int64_t cdiv(int64_t a, int64_t b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }
static int64_t fdiv(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
static int ilog2(uint32_t v) { int n = 0; while (v > 1) { v >>= 1; ++n; } return n; }

/* ================================================================== the 5/3 transform (Annex F) */

/* periodic symmetric extension of a line of n samples: the sample that stands at index i (F.3.7) */
static int pse(int i, int n)
{
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}

/* one line, analysis: x[0..n) with stride `step`, the first sample at coordinate i0; low-pass samples (even
 * coordinates) first, then the high-pass ones */
static void line_forward(int32_t *x, int n, int step, int i0, int32_t *tmp)
{
    if (n == 1) {
        if (i0 & 1) x[0] *= 2;
        return;
    }
    int32_t *e = tmp + 4;   /* e[k] is the sample at coordinate i0 + k, k in -4 .. n + 3 */
    for (int k = -4; k < n + 4; ++k) e[k] = x[(size_t)pse(k, n) * step];
    for (int k = -3; k < n + 3; ++k)          /* predict: odd coordinates */
        if ((i0 + k) & 1) e[k] -= (e[k - 1] + e[k + 1]) >> 1;
    for (int k = -2; k < n + 2; ++k)          /* update: even coordinates */
        if (!((i0 + k) & 1)) e[k] += (e[k - 1] + e[k + 1] + 2) >> 2;
    int at = 0;
    for (int k = 0; k < n; ++k) if (!((i0 + k) & 1)) x[(size_t)(at++) * step] = e[k];
    for (int k = 0; k < n; ++k) if ((i0 + k) & 1) x[(size_t)(at++) * step] = e[k];
}

static void line_inverse(int32_t *x, int n, int step, int i0, int32_t *tmp)
{
    if (n == 1) {
        if (i0 & 1) x[0] /= 2;
        return;
    }
    int32_t *e = tmp + 4, *il = tmp + 4 + n + 8 + 4;
    int lo = 0, hi = 0;
    for (int k = 0; k < n; ++k) if (!((i0 + k) & 1)) ++hi;   /* hi: where the high-pass samples start */
    for (int k = 0; k < n; ++k) il[k] = ((i0 + k) & 1) ? x[(size_t)(hi++) * step] : x[(size_t)(lo++) * step];
    for (int k = -4; k < n + 4; ++k) e[k] = il[pse(k, n)];
    for (int k = -3; k < n + 3; ++k)
        if (!((i0 + k) & 1)) e[k] -= (e[k - 1] + e[k + 1] + 2) >> 2;
    for (int k = -2; k < n + 2; ++k)
        if ((i0 + k) & 1) e[k] += (e[k - 1] + e[k + 1]) >> 1;
    for (int k = 0; k < n; ++k) x[(size_t)k * step] = e[k];
}

/* a: tile-component of w x h samples, rows `stride` apart, its first sample at (x0, y0) of the reference grid.
 * Mallat layout: after level l the LL band of that level is the top-left corner. */
int jo_dwt53(int32_t *a, int w, int h, int stride, int x0, int y0, int levels, int inverse)
{
    if (w < 1 || h < 1 || levels < 0 || levels > 32) FAIL(-1, "jo_dwt53: bad argument");
    const int m = w > h ? w : h;
    int32_t *tmp = (int32_t *)malloc(sizeof(int32_t) * (size_t)(2 * m + 32));
    if (!tmp) FAIL(-2, "out of memory");
    for (int s = 0; s < levels; ++s) {
        const int l = inverse ? levels - 1 - s : s;
        const int ux0 = (int)cdiv(x0, (int64_t)1 << l), ux1 = (int)cdiv((int64_t)x0 + w, (int64_t)1 << l);
        const int uy0 = (int)cdiv(y0, (int64_t)1 << l), uy1 = (int)cdiv((int64_t)y0 + h, (int64_t)1 << l);
        const int rw = ux1 - ux0, rh = uy1 - uy0;
        if (!inverse) {
            for (int x = 0; x < rw; ++x) line_forward(a + x, rh, stride, uy0, tmp);
            for (int y = 0; y < rh; ++y) line_forward(a + (size_t)y * stride, rw, 1, ux0, tmp);
        } else {
            for (int y = 0; y < rh; ++y) line_inverse(a + (size_t)y * stride, rw, 1, ux0, tmp);
            for (int x = 0; x < rw; ++x) line_inverse(a + x, rh, stride, uy0, tmp);
        }
    }
    free(tmp);
    return 0;
}

/* ================================================================== the MQ coder (Annex C) */

typedef struct { uint16_t qe; uint8_t nmps, nlps, sw; } qe_row;
static const qe_row QE[47] = {   /* Table C.2 */
    {0x5601, 1, 1, 1},   {0x3401, 2, 6, 0},   {0x1801, 3, 9, 0},   {0x0AC1, 4, 12, 0},  {0x0521, 5, 29, 0},  {0x0221, 38, 33, 0},
    {0x5601, 7, 6, 1},   {0x5401, 8, 14, 0},  {0x4801, 9, 14, 0},  {0x3801, 10, 14, 0}, {0x3001, 11, 17, 0}, {0x2401, 12, 18, 0},
    {0x1C01, 13, 20, 0}, {0x1601, 29, 21, 0}, {0x5601, 15, 14, 1}, {0x5401, 16, 14, 0}, {0x5101, 17, 15, 0}, {0x4801, 18, 16, 0},
    {0x3801, 19, 17, 0}, {0x3401, 20, 18, 0}, {0x3001, 21, 19, 0}, {0x2801, 22, 19, 0}, {0x2401, 23, 20, 0}, {0x2201, 24, 21, 0},
    {0x1C01, 25, 22, 0}, {0x1801, 26, 23, 0}, {0x1601, 27, 24, 0}, {0x1401, 28, 25, 0}, {0x1201, 29, 26, 0}, {0x1101, 30, 27, 0},
    {0x0AC1, 31, 28, 0}, {0x09C1, 32, 29, 0}, {0x08A1, 33, 30, 0}, {0x0521, 34, 31, 0}, {0x0441, 35, 32, 0}, {0x02A1, 36, 33, 0},
    {0x0221, 37, 34, 0}, {0x0141, 38, 35, 0}, {0x0111, 39, 36, 0}, {0x0085, 40, 37, 0}, {0x0049, 41, 38, 0}, {0x0025, 42, 39, 0},
    {0x0015, 43, 40, 0}, {0x0009, 44, 41, 0}, {0x0005, 45, 42, 0}, {0x0001, 45, 43, 0}, {0x5601, 46, 46, 0}};

enum { CX_ZC = 0, CX_SC = 9, CX_MR = 14, CX_RL = 17, CX_UNI = 18, CX_N = 19 };

typedef struct {
    int decoding;
    uint32_t A, C;
    int CT;
    uint8_t *bp, *start, *end;   /* encoder: bp points at the pending byte B; start[-1] exists */
    uint8_t I[CX_N], MPS[CX_N];
} mq_t;

static void mq_reset_contexts(mq_t *q)   /* Table D.7 */
{
    memset(q->I, 0, sizeof q->I);
    memset(q->MPS, 0, sizeof q->MPS);
    q->I[CX_ZC] = 4;
    q->I[CX_RL] = 3;
    q->I[CX_UNI] = 46;
}

/* ---- encoder: INITENC, BYTEOUT, RENORME, CODEMPS, CODELPS, FLUSH */
static void enc_init(mq_t *q, uint8_t *buf, size_t cap)
{
    q->decoding = 0;
    q->A = 0x8000; q->C = 0; q->CT = 12;
    buf[0] = 0;
    q->start = buf + 1; q->bp = buf; q->end = buf + cap;
    mq_reset_contexts(q);
}
static void enc_byteout(mq_t *q)
{
    if (*q->bp == 0xFF) goto stuffed;
    if (q->C < 0x8000000u) goto plain;
    ++*q->bp;                              /* the carry */
    if (*q->bp == 0xFF) { q->C &= 0x7FFFFFFu; goto stuffed; }
plain:
    ++q->bp; *q->bp = (uint8_t)(q->C >> 19); q->C &= 0x7FFFFu; q->CT = 8;
    return;
stuffed:
    ++q->bp; *q->bp = (uint8_t)(q->C >> 20); q->C &= 0xFFFFFu; q->CT = 7;
}
static void enc_renorm(mq_t *q)
{
    do {
        q->A <<= 1; q->C <<= 1;
        if (--q->CT == 0) enc_byteout(q);
    } while (!(q->A & 0x8000u));
}
static void enc_symbol(mq_t *q, int cx, int d)
{
    const qe_row r = QE[q->I[cx]];
    q->A -= r.qe;
    if (d == q->MPS[cx]) {                 /* CODEMPS */
        if (q->A & 0x8000u) { q->C += r.qe; return; }
        if (q->A < r.qe) q->A = r.qe; else q->C += r.qe;
        q->I[cx] = r.nmps;
    } else {                               /* CODELPS */
        if (q->A < r.qe) q->C += r.qe; else q->A = r.qe;
        if (r.sw) q->MPS[cx] ^= 1;
        q->I[cx] = r.nlps;
    }
    enc_renorm(q);
}
static int enc_flush(mq_t *q)              /* returns the segment's length */
{
    const uint32_t tempc = q->C + q->A;    /* SETBITS */
    q->C |= 0xFFFFu;
    if (q->C >= tempc) q->C -= 0x8000u;
    q->C <<= q->CT; enc_byteout(q);
    q->C <<= q->CT; enc_byteout(q);
    if (*q->bp != 0xFF) ++q->bp;           /* a last byte of 0xFF is discarded */
    return (int)(q->bp - q->start);
}

/* ---- decoder: INITDEC, BYTEIN, RENORMD, DECODE with the two exchanges */
static void dec_bytein(mq_t *q)
{
    if (*q->bp == 0xFF) {
        if (q->bp[1] > 0x8F) { q->C += 0xFF00u; q->CT = 8; }
        else { ++q->bp; q->C += (uint32_t)*q->bp << 9; q->CT = 7; }
    } else { ++q->bp; q->C += (uint32_t)*q->bp << 8; q->CT = 8; }
}
static void dec_init(mq_t *q, uint8_t *buf)   /* buf: the segment followed by 0xFF 0xFF */
{
    q->decoding = 1;
    q->bp = q->start = buf;
    q->C = (uint32_t)*q->bp << 16;
    dec_bytein(q);
    q->C <<= 7; q->CT -= 7; q->A = 0x8000;
    mq_reset_contexts(q);
}
static int dec_symbol(mq_t *q, int cx)
{
    const qe_row r = QE[q->I[cx]];
    int d;
    q->A -= r.qe;
    if ((q->C >> 16) < r.qe) {             /* LPS_EXCHANGE */
        if (q->A < r.qe) { d = q->MPS[cx]; q->I[cx] = r.nmps; }
        else { d = 1 - q->MPS[cx]; if (r.sw) q->MPS[cx] ^= 1; q->I[cx] = r.nlps; }
        q->A = r.qe;
    } else {
        q->C -= (uint32_t)r.qe << 16;
        if (q->A & 0x8000u) return q->MPS[cx];
        if (q->A < r.qe) { d = 1 - q->MPS[cx]; if (r.sw) q->MPS[cx] ^= 1; q->I[cx] = r.nlps; }   /* MPS_EXCHANGE */
        else { d = q->MPS[cx]; q->I[cx] = r.nmps; }
    }
    do {                                   /* RENORMD */
        if (q->CT == 0) dec_bytein(q);
        q->A <<= 1; q->C <<= 1; --q->CT;
    } while (!(q->A & 0x8000u));
    return d;
}
/* the decision d goes through the coder: written when encoding, read (d ignored) when decoding */
static int mq_io(mq_t *q, int cx, int d) { if (q->decoding) return dec_symbol(q, cx); enc_symbol(q, cx, d); return d; }

/* ================================================================== coefficient bit modelling (Annex D) */

/* Table D.1.  LL and LH: [sum H][sum V][sum D]; HL: H and V change places; HH: [sum H + sum V][sum D] */
static const uint8_t ZC_LL_LH[3][3][5] = {
    {{0, 1, 2, 2, 2}, {3, 3, 3, 3, 3}, {4, 4, 4, 4, 4}},
    {{5, 6, 6, 6, 6}, {7, 7, 7, 7, 7}, {7, 7, 7, 7, 7}},
    {{8, 8, 8, 8, 8}, {8, 8, 8, 8, 8}, {8, 8, 8, 8, 8}}};
static const uint8_t ZC_HH[5][5] = {   /* [H + V][D] */
    {0, 3, 6, 8, 8}, {1, 4, 7, 8, 8}, {2, 5, 7, 8, 8}, {2, 5, 7, 8, 8}, {2, 5, 7, 8, 8}};
/* Table D.2: the contribution of two neighbours, each insignificant (0), positive (1) or negative (2) */
static const int8_t CONTRIB[3][3] = {{0, 1, -1}, {1, 1, 0}, {-1, 0, -1}};
/* Table D.3: [H + 1][V + 1] -> context label, XOR bit */
static const uint8_t SC_CX[3][3] = {{13, 12, 11}, {10, 9, 10}, {11, 12, 13}};
static const uint8_t SC_XOR[3][3] = {{1, 1, 1}, {1, 0, 0}, {0, 0, 0}};

enum { F_SIG = 1, F_NEG = 2, F_VISITED = 4, F_REFINED = 8 };

typedef struct {
    mq_t mq;
    int w, h, orient, fw;     /* fw: flag words per row = w + 2 */
    uint8_t *flags;           /* (h + 2) * (w + 2) */
    uint32_t *mag;            /* h * w */
} t1_t;

static int sig(uint8_t f) { return f & F_SIG; }
static int sign_state(uint8_t f) { return !(f & F_SIG) ? 0 : ((f & F_NEG) ? 2 : 1); }

static int zero_coding_context(const t1_t *t, const uint8_t *f, int *any)
{
    const int fw = t->fw;
    const int h = sig(f[-1]) + sig(f[1]), v = sig(f[-fw]) + sig(f[fw]);
    const int d = sig(f[-fw - 1]) + sig(f[-fw + 1]) + sig(f[fw - 1]) + sig(f[fw + 1]);
    if (any) *any = h + v + d;
    if (t->orient == 3) return CX_ZC + ZC_HH[h + v][d];
    if (t->orient == 1) return CX_ZC + ZC_LL_LH[v][h][d];
    return CX_ZC + ZC_LL_LH[h][v][d];
}
/* sign coding of a sample that has just become significant; returns whether it is negative */
static int code_sign(t1_t *t, uint8_t *f, int negative)
{
    const int H = CONTRIB[sign_state(f[-1])][sign_state(f[1])], V = CONTRIB[sign_state(f[-t->fw])][sign_state(f[t->fw])];
    const int x = SC_XOR[H + 1][V + 1];
    return mq_io(&t->mq, SC_CX[H + 1][V + 1], negative ^ x) ^ x;
}
static void becomes_significant(t1_t *t, uint8_t *f, uint32_t *m, int p)
{
    const int neg = code_sign(t, f, (int)(*m >> 31));
    if (t->mq.decoding) *m |= (1u << p) | ((uint32_t)neg << 31);
    *f |= F_SIG | (neg ? F_NEG : 0);
}

static void significance_pass(t1_t *t, int p)
{
    for (int y0 = 0; y0 < t->h; y0 += 4)
        for (int x = 0; x < t->w; ++x)
            for (int y = y0; y < y0 + 4 && y < t->h; ++y) {
                uint8_t *f = t->flags + (size_t)(y + 1) * t->fw + x + 1;
                uint32_t *m = t->mag + (size_t)y * t->w + x;
                int any;
                if (*f & F_SIG) continue;
                const int cx = zero_coding_context(t, f, &any);
                if (!any) continue;
                *f |= F_VISITED;
                if (mq_io(&t->mq, cx, (int)((*m >> p) & 1u))) becomes_significant(t, f, m, p);
            }
}
static void refinement_pass(t1_t *t, int p)
{
    for (int y0 = 0; y0 < t->h; y0 += 4)
        for (int x = 0; x < t->w; ++x)
            for (int y = y0; y < y0 + 4 && y < t->h; ++y) {
                uint8_t *f = t->flags + (size_t)(y + 1) * t->fw + x + 1;
                uint32_t *m = t->mag + (size_t)y * t->w + x;
                int any;
                if ((*f & (F_SIG | F_VISITED)) != F_SIG) continue;
                zero_coding_context(t, f, &any);
                const int cx = (*f & F_REFINED) ? 16 : (any ? 15 : 14);      /* Table D.4 */
                const int bit = mq_io(&t->mq, cx, (int)((*m >> p) & 1u));
                if (t->mq.decoding) *m |= (uint32_t)bit << p;
                *f |= F_REFINED;
            }
}
static void cleanup_pass(t1_t *t, int p)
{
    for (int y0 = 0; y0 < t->h; y0 += 4)
        for (int x = 0; x < t->w; ++x) {
            int first = y0;
            int runlength = y0 + 4 <= t->h;
            for (int y = y0; runlength && y < y0 + 4; ++y) {
                const uint8_t *f = t->flags + (size_t)(y + 1) * t->fw + x + 1;
                int any;
                zero_coding_context(t, f, &any);
                if ((*f & (F_SIG | F_VISITED)) || any) runlength = 0;
            }
            if (runlength) {
                int r = 4;
                if (!t->mq.decoding)
                    for (r = 0; r < 4; ++r) if ((t->mag[(size_t)(y0 + r) * t->w + x] >> p) & 1u) break;
                if (!mq_io(&t->mq, CX_RL, r < 4)) { ++g_cnt[CNT_RL_ZERO]; continue; }
                const int hi = mq_io(&t->mq, CX_UNI, r >> 1), lo = mq_io(&t->mq, CX_UNI, r & 1);
                r = 2 * hi + lo;
                ++g_cnt[CNT_RL_EXIT0 + r];
                becomes_significant(t, t->flags + (size_t)(y0 + r + 1) * t->fw + x + 1, t->mag + (size_t)(y0 + r) * t->w + x, p);
                first = y0 + r + 1;
            }
            for (int y = first; y < y0 + 4 && y < t->h; ++y) {
                uint8_t *f = t->flags + (size_t)(y + 1) * t->fw + x + 1;
                uint32_t *m = t->mag + (size_t)y * t->w + x;
                if (*f & (F_SIG | F_VISITED)) continue;
                if (mq_io(&t->mq, zero_coding_context(t, f, NULL), (int)((*m >> p) & 1u))) becomes_significant(t, f, m, p);
            }
        }
    for (size_t k = 0; k < (size_t)(t->h + 2) * t->fw; ++k) t->flags[k] &= (uint8_t)~F_VISITED;
}

static int t1_open(t1_t *t, int w, int h, int orient)
{
    t->w = w; t->h = h; t->orient = orient; t->fw = w + 2;
    t->flags = (uint8_t *)calloc((size_t)(h + 2) * (w + 2), 1);
    t->mag = (uint32_t *)calloc((size_t)h * w, 4);
    if (!t->flags || !t->mag) { free(t->flags); free(t->mag); return -1; }
    return 0;
}
static void t1_close(t1_t *t) { free(t->flags); free(t->mag); }

static void run_passes(t1_t *t, int numbps, int passes)
{
    int done = 0;
    for (int p = numbps - 1; p >= 0 && done < passes; --p) {
        if (p != numbps - 1) {
            significance_pass(t, p);
            if (++done == passes) break;
            refinement_pass(t, p);
            if (++done == passes) break;
        }
        cleanup_pass(t, p);
        ++done;
    }
}

/* Codes a block of w x h coefficients (rows `stride` apart) of a subband of orientation 0 LL, 1 HL, 2 LH, 3 HH.
 * Returns the bytes of its codeword segment (all of them counted, the first `cap` written); *passes and *numbps as
 * the packet header announces them (0 and 0: nothing to code). */
int jo_t1_encode(const int32_t *coef, int stride, int w, int h, int orient, uint8_t *out, int cap, int32_t *passes, int32_t *numbps)
{
    *passes = 0; *numbps = 0;
    if (w < 1 || h < 1 || orient < 0 || orient > 3) FAIL(-1, "jo_t1_encode: bad argument");
    t1_t t;
    if (t1_open(&t, w, h, orient)) FAIL(-2, "out of memory");
    uint32_t all = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int32_t v = coef[(size_t)y * stride + x];
            const uint32_t m = v < 0 ? (uint32_t)(-(int64_t)v) : (uint32_t)v;
            t.mag[(size_t)y * w + x] = (m & 0x7FFFFFFFu) | (v < 0 ? 0x80000000u : 0);
            all |= m & 0x7FFFFFFFu;
        }
    int n = 0;
    if (all) {
        const int nb = ilog2(all) + 1;
        const size_t room = (size_t)w * h * nb / 2 + 4096;   /* (the coder spends about 1.1 bits per decision at worst) */
        uint8_t *buf = (uint8_t *)malloc(room);
        if (!buf) { t1_close(&t); FAIL(-2, "out of memory"); }
        enc_init(&t.mq, buf, room);
        run_passes(&t, nb, 3 * nb - 2);
        n = enc_flush(&t.mq);
        if (out && cap > 0) memcpy(out, buf + 1, (size_t)(n < cap ? n : cap));
        free(buf);
        *passes = 3 * nb - 2;
        *numbps = nb;
        if (h & 3) ++g_cnt[CNT_PARTIAL_STRIPE];
        if (w < 3) ++g_cnt[CNT_NARROW_BLOCK];
    }
    t1_close(&t);
    return n;
}

int jo_t1_decode(const uint8_t *data, int len, int w, int h, int orient, int numbps, int passes, int32_t *coef, int stride)
{
    if (w < 1 || h < 1 || orient < 0 || orient > 3 || numbps < 0 || numbps > 31 || len < 0) FAIL(-1, "jo_t1_decode: bad argument");
    t1_t t;
    if (t1_open(&t, w, h, orient)) FAIL(-2, "out of memory");
    if (passes > 0 && numbps > 0) {
        uint8_t *buf = (uint8_t *)malloc((size_t)len + 4);
        if (!buf) { t1_close(&t); FAIL(-2, "out of memory"); }
        if (len) memcpy(buf, data, (size_t)len);
        buf[len] = 0xFF; buf[len + 1] = 0xFF; buf[len + 2] = 0xFF; buf[len + 3] = 0xFF;
        dec_init(&t.mq, buf);
        run_passes(&t, numbps, passes);
        free(buf);
    }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint32_t m = t.mag[(size_t)y * w + x];
            const int32_t v = (int32_t)(m & 0x7FFFFFFFu);
            coef[(size_t)y * stride + x] = (m >> 31) ? -v : v;
        }
    t1_close(&t);
    return 0;
}

/* ================================================================== geometry (B.5 - B.7) */

typedef struct {
    int C, H, W, bits;
    int XT, YT;            /* tile size; the tile grid starts at (0, 0) like the image */
    int NL;                /* decompositions */
    int cbw, cbh;          /* code-block size */
    int guard;
    int eps[1 + 3 * 32];   /* exponents: LL, then HL LH HH of each resolution from the lowest */
    int prog, layers, mct, sop, eph;
} params_t;

/* the fields of a block record, int64 each: what jo_blocks and jo_parse return */
enum { R_TILE, R_COMP, R_RES, R_BAND, R_GX, R_GY, R_NUMBPS, R_PASSES, R_OFFSET, R_LENGTH, R_MB, R_X, R_Y, R_W, R_H, R_ORIENT, R_N };

typedef struct { int orient, x, y, w, h, gw, gh, mb; int64_t bx0, by0; } band_t;

static int ntiles_x(const params_t *p) { return (int)cdiv(p->W, p->XT); }
static int ntiles_y(const params_t *p) { return (int)cdiv(p->H, p->YT); }
static void tile_rect(const params_t *p, int t, int64_t *x0, int64_t *y0, int64_t *x1, int64_t *y1)
{
    const int tx = t % ntiles_x(p), ty = t / ntiles_x(p);
    *x0 = (int64_t)tx * p->XT; *y0 = (int64_t)ty * p->YT;
    *x1 = *x0 + p->XT < p->W ? *x0 + p->XT : p->W;
    *y1 = *y0 + p->YT < p->H ? *y0 + p->YT : p->H;
}
/* the bands of resolution r of tile t; returns their number (0: the resolution is empty and has no packet) */
static int bands_of(const params_t *p, int t, int r, band_t bd[3])
{
    int64_t x0, y0, x1, y1;
    tile_rect(p, t, &x0, &y0, &x1, &y1);
    const int64_t s = (int64_t)1 << (p->NL - r);
    const int64_t rx0 = cdiv(x0, s), rx1 = cdiv(x1, s), ry0 = cdiv(y0, s), ry1 = cdiv(y1, s);      /* (B-14) */
    if (rx1 <= rx0 || ry1 <= ry0) return 0;
    const int n = r == 0 ? 1 : 3;
    const int nb = r == 0 ? p->NL : p->NL - r + 1;
    const int64_t lx0 = cdiv(rx0, 2), lx1 = cdiv(rx1, 2), ly0 = cdiv(ry0, 2), ly1 = cdiv(ry1, 2);  /* the resolution below */
    for (int b = 0; b < n; ++b) {
        band_t *q = &bd[b];
        q->orient = r == 0 ? 0 : b + 1;
        const int xo = q->orient & 1, yo = q->orient >> 1;
        const int64_t half = nb ? (int64_t)1 << (nb - 1) : 0, full = (int64_t)1 << nb;
        const int64_t bx0 = cdiv(x0 - half * xo, full), bx1 = cdiv(x1 - half * xo, full);            /* (B-15) */
        const int64_t by0 = cdiv(y0 - half * yo, full), by1 = cdiv(y1 - half * yo, full);
        q->bx0 = bx0; q->by0 = by0;
        q->w = (int)(bx1 - bx0); q->h = (int)(by1 - by0);
        q->x = r == 0 ? 0 : (xo ? (int)(lx1 - lx0) : 0);
        q->y = r == 0 ? 0 : (yo ? (int)(ly1 - ly0) : 0);
        if (q->w <= 0 || q->h <= 0) { q->gw = q->gh = 0; }
        else {
            q->gw = (int)(cdiv(bx1, p->cbw) - fdiv(bx0, p->cbw));
            q->gh = (int)(cdiv(by1, p->cbh) - fdiv(by0, p->cbh));
        }
        q->mb = p->guard + p->eps[r == 0 ? 0 : 1 + 3 * (r - 1) + b] - 1;                              /* (E-2) */
    }
    return n;
}
static void block_rect(const params_t *p, const band_t *q, int gx, int gy, int *x, int *y, int *w, int *h)
{
    const int64_t cx0 = (fdiv(q->bx0, p->cbw) + gx) * p->cbw, cy0 = (fdiv(q->by0, p->cbh) + gy) * p->cbh;
    const int64_t ax0 = cx0 > q->bx0 ? cx0 : q->bx0, ay0 = cy0 > q->by0 ? cy0 : q->by0;
    const int64_t ax1 = cx0 + p->cbw < q->bx0 + q->w ? cx0 + p->cbw : q->bx0 + q->w;
    const int64_t ay1 = cy0 + p->cbh < q->by0 + q->h ? cy0 + p->cbh : q->by0 + q->h;
    *x = q->x + (int)(ax0 - q->bx0); *y = q->y + (int)(ay0 - q->by0);
    *w = (int)(ax1 - ax0); *h = (int)(ay1 - ay0);
}

static int own_params(params_t *p, int C, int H, int W, int bits)   /* choice 1 of the header comment */
{
    if (C < 1 || C > 16384 || H < 1 || W < 1 || H > 32768 || W > 32768 || (bits != 8 && bits != 16)) FAIL(-1, "bad geometry");
    memset(p, 0, sizeof *p);
    p->C = C; p->H = H; p->W = W; p->bits = bits;
    const int tiled = H > 1024 || W > 1024;
    p->XT = tiled ? 1024 : W; p->YT = tiled ? 1024 : H;
    const int m = H < W ? H : W;
    int R = 1;
    while ((m >> R) > 0 && R < 6) ++R;
    p->NL = R - 1;
    p->cbw = p->cbh = 64;
    p->guard = 2;
    p->eps[0] = bits;
    for (int r = 1; r <= p->NL; ++r) { p->eps[3 * r - 2] = bits + 1; p->eps[3 * r - 1] = bits + 1; p->eps[3 * r] = bits + 2; }
    p->prog = 0; p->layers = 1;
    return 0;
}

/* the blocks in the order the packets carry them: tile, resolution, component, band, raster.  rec may be NULL (count). */
static int64_t enumerate_blocks(const params_t *p, int64_t *rec, int64_t cap)
{
    int64_t n = 0;
    const int nt = ntiles_x(p) * ntiles_y(p);
    for (int t = 0; t < nt; ++t)
        for (int r = 0; r <= p->NL; ++r)
            for (int c = 0; c < p->C; ++c) {
                band_t bd[3];
                const int nbands = bands_of(p, t, r, bd);
                for (int b = 0; b < nbands; ++b)
                    for (int gy = 0; gy < bd[b].gh; ++gy)
                        for (int gx = 0; gx < bd[b].gw; ++gx, ++n) {
                            if (!rec || n >= cap) continue;
                            int64_t *q = rec + n * R_N;
                            int x, y, w, h;
                            block_rect(p, &bd[b], gx, gy, &x, &y, &w, &h);
                            memset(q, 0, sizeof(int64_t) * R_N);
                            q[R_TILE] = t; q[R_COMP] = c; q[R_RES] = r; q[R_BAND] = b; q[R_GX] = gx; q[R_GY] = gy;
                            q[R_OFFSET] = -1; q[R_MB] = bd[b].mb; q[R_X] = x; q[R_Y] = y; q[R_W] = w; q[R_H] = h;
                            q[R_ORIENT] = bd[b].orient;
                        }
            }
    return n;
}

/* the block table of the encoder's own geometry */
int64_t jo_blocks(int C, int H, int W, int bits, int64_t *rec, int64_t cap)
{
    params_t p;
    if (own_params(&p, C, H, W, bits)) return -1;
    return enumerate_blocks(&p, rec, cap);
}
/* {tiles across, tiles down, tile width, tile height, resolutions} of the encoder's own geometry */
int jo_layout(int C, int H, int W, int bits, int32_t out[5])
{
    params_t p;
    if (own_params(&p, C, H, W, bits)) return -1;
    out[0] = ntiles_x(&p); out[1] = ntiles_y(&p); out[2] = p.XT; out[3] = p.YT; out[4] = p.NL + 1;
    return 0;
}

/* ================================================================== tier-2: packet headers (B.10) */

typedef struct { uint8_t *p; size_t cap, n; } out_t;
static void o8(out_t *o, unsigned v) { if (o->n < o->cap) o->p[o->n] = (uint8_t)v; ++o->n; }
static void o16(out_t *o, unsigned v) { o8(o, v >> 8); o8(o, v & 0xFF); }
static void o32(out_t *o, uint32_t v) { o16(o, v >> 16); o16(o, v & 0xFFFF); }
static void otag(out_t *o, const char *s) { for (int k = 0; k < 4; ++k) o8(o, (unsigned char)s[k]); }
static void opatch32(out_t *o, size_t at, uint32_t v) { for (int k = 0; k < 4; ++k) if (at + k < o->cap) o->p[at + k] = (uint8_t)(v >> (24 - 8 * k)); }

/* bits of a packet header, either written or read: the byte after one of 0xFF holds seven, its top bit 0 (B.10.1) */
typedef struct {
    int reading;
    out_t *o;
    const uint8_t *in; size_t in_n, in_pos; int bad;
    unsigned cur, prev;
    int used, room;
} bits_t;
static void bits_begin_write(bits_t *b, out_t *o) { memset(b, 0, sizeof *b); b->o = o; b->room = 8; }
static void bits_begin_read(bits_t *b, const uint8_t *in, size_t n) { memset(b, 0, sizeof *b); b->reading = 1; b->in = in; b->in_n = n; }
static void put_bit(bits_t *b, int v)
{
    b->cur = (b->cur << 1) | (unsigned)(v & 1);
    if (++b->used == b->room) {
        o8(b->o, b->cur);
        if (b->cur == 0xFF) ++g_cnt[CNT_HEADER_STUFF];
        b->room = b->cur == 0xFF ? 7 : 8;
        b->prev = b->cur; b->cur = 0; b->used = 0;
    }
}
static int get_bit(bits_t *b)
{
    if (b->used == 0) {
        b->prev = b->cur;
        if (b->in_pos >= b->in_n) { b->bad = 1; return 0; }
        b->cur = b->in[b->in_pos++];
        b->used = b->prev == 0xFF ? 7 : 8;
    }
    return (int)((b->cur >> --b->used) & 1u);
}
static int io_bit(bits_t *b, int v) { if (b->reading) return get_bit(b); put_bit(b, v); return v & 1; }
static uint32_t io_bits(bits_t *b, uint32_t v, int n)
{
    uint32_t r = 0;
    for (int k = n - 1; k >= 0; --k) r = (r << 1) | (uint32_t)io_bit(b, (int)((v >> k) & 1u));
    return r;
}
static void bits_end(bits_t *b)
{
    if (b->reading) {
        b->used = 0;
        if (b->cur == 0xFF) ++b->in_pos;        /* the stuffed byte after a last 0xFF */
        return;
    }
    if (b->used) { b->cur <<= (b->room - b->used); o8(b->o, b->cur); b->prev = b->cur; }
    if (b->prev == 0xFF) o8(b->o, 0);
}

/* tag tree (B.10.2): a quad-tree of minima, each node's value told once, as zeros up to it and a one */
typedef struct { int parent, value, low, known; } tnode_t;
typedef struct { tnode_t *n; int leaves; } ttree_t;
#define TT_INF 0x3FFFFFFF
static int tt_build(ttree_t *t, int w, int h, const int *leaf_values)
{
    int total = 0, cw = w, ch = h, levels = 0, lw[20], lh[20], at[20];
    for (;;) {
        lw[levels] = cw; lh[levels] = ch; at[levels] = total;
        total += cw * ch; ++levels;
        if (cw * ch <= 1) break;
        cw = (cw + 1) / 2; ch = (ch + 1) / 2;
    }
    t->n = (tnode_t *)malloc(sizeof(tnode_t) * (size_t)total);
    if (!t->n) return -1;
    t->leaves = w * h;
    for (int k = 0; k < total; ++k) { t->n[k].parent = -1; t->n[k].value = TT_INF; t->n[k].low = 0; t->n[k].known = 0; }
    for (int l = 0; l + 1 < levels; ++l)
        for (int y = 0; y < lh[l]; ++y)
            for (int x = 0; x < lw[l]; ++x) t->n[at[l] + y * lw[l] + x].parent = at[l + 1] + (y / 2) * lw[l + 1] + x / 2;
    if (leaf_values) {
        for (int k = 0; k < w * h; ++k) t->n[k].value = leaf_values[k];
        for (int k = 0; k < total; ++k) {          /* children come before parents */
            const int up = t->n[k].parent;
            if (up >= 0 && t->n[k].value < t->n[up].value) t->n[up].value = t->n[k].value;
        }
    }
    if ((w & (w - 1)) || (h & (h - 1))) ++g_cnt[CNT_TREE_NOT_POW2];
    return 0;
}
/* tells (or learns) whether the node's value is below the threshold, root first; returns the node's lower bound */
static int tt_code(ttree_t *t, bits_t *b, int node, int threshold)
{
    tnode_t *nd = &t->n[node];
    int low = nd->parent >= 0 ? tt_code(t, b, nd->parent, threshold) : 0;
    if (low < nd->low) low = nd->low;
    while (low < threshold && !nd->known) {
        if (b->reading) {
            if (get_bit(b)) { nd->value = low; nd->known = 1; }
            else ++low;
            if (b->bad) break;
        } else {
            if (low >= nd->value) { put_bit(b, 1); nd->known = 1; }
            else { put_bit(b, 0); ++low; }
        }
    }
    if (nd->known && low < nd->value) low = nd->value;
    nd->low = low;
    return low;
}
static int tt_below(ttree_t *t, bits_t *b, int leaf, int threshold)
{
    tt_code(t, b, leaf, threshold);
    return t->n[leaf].known && t->n[leaf].value < threshold;
}

/* Table B.4: number of coding passes */
static int io_passes(bits_t *b, int n)
{
    static const struct { int first, last, prefix, prefix_bits, extra_bits; } ROWS[5] = {
        {1, 1, 0x0, 1, 0}, {2, 2, 0x2, 2, 0}, {3, 5, 0x3, 2, 2}, {6, 36, 0xF, 4, 5}, {37, 164, 0x1FF, 9, 7}};
    if (!b->reading) {
        for (int k = 0; k < 5; ++k)
            if (n >= ROWS[k].first && n <= ROWS[k].last) {
                io_bits(b, (uint32_t)ROWS[k].prefix, ROWS[k].prefix_bits);
                io_bits(b, (uint32_t)(n - ROWS[k].first), ROWS[k].extra_bits);
                ++g_cnt[CNT_PASS_ROW0 + k];
                if (k == 4) ++g_cnt[CNT_PASSES_16BIT];
            }
        return n;
    }
    if (!get_bit(b)) return 1;
    if (!get_bit(b)) return 2;
    uint32_t v = io_bits(b, 0, 2);
    if (v < 3) return 3 + (int)v;
    v = io_bits(b, 0, 5);
    if (v < 31) return 6 + (int)v;
    return 37 + (int)io_bits(b, 0, 7);
}

/* One packet header, written or parsed.  rec: per block of the packet (band by band, raster order) three values,
 * {passes (0: not included), numbps, bytes}.  The layer is the only one, so every Lblock is still 3. */
static int packet_header(bits_t *b, int nbands, const int32_t *gw, const int32_t *gh, const int32_t *mb, int32_t *rec)
{
    int64_t total = 0;
    int included = 0, empty_bands = 0, full_bands = 0;
    for (int k = 0; k < nbands; ++k) total += (int64_t)gw[k] * gh[k];
    if (!b->reading) for (int64_t k = 0; k < total; ++k) included += rec[3 * k] > 0;
    for (int k = 0; k < nbands; ++k) { if (gw[k] > 0 && gh[k] > 0) ++full_bands; else ++empty_bands; }
    if (!io_bit(b, included > 0)) {
        ++g_cnt[CNT_EMPTY_PACKET];
        if (b->reading) for (int64_t k = 0; k < total; ++k) rec[3 * k] = rec[3 * k + 1] = rec[3 * k + 2] = 0;
        bits_end(b);
        return 0;
    }
    if (empty_bands && full_bands) ++g_cnt[CNT_EMPTY_BAND_BESIDE_FULL];
    int32_t *r = rec;
    for (int k = 0; k < nbands; ++k) {
        const int n = gw[k] * gh[k];
        if (!n) continue;
        int *incl = (int *)malloc(sizeof(int) * 2 * (size_t)n), *zbp = incl ? incl + n : NULL;
        if (!incl) FAIL(-2, "out of memory");
        for (int i = 0; i < n; ++i) { incl[i] = r[3 * i] > 0 ? 0 : 1; zbp[i] = mb[k] - r[3 * i + 1]; }
        ttree_t ti, tz;
        if (tt_build(&ti, gw[k], gh[k], b->reading ? NULL : incl) || tt_build(&tz, gw[k], gh[k], b->reading ? NULL : zbp)) {
            free(incl);
            FAIL(-2, "out of memory");
        }
        for (int i = 0; i < n && !b->bad; ++i, r += 3) {
            if (!tt_below(&ti, b, i, 1)) {                   /* not in this (the only) layer */
                if (b->reading) r[0] = r[1] = r[2] = 0;
                ++g_cnt[CNT_EXCLUDED_IN_FULL_PACKET];
                continue;
            }
            int z;
            if (b->reading) { for (z = 1; !tt_below(&tz, b, i, z) && !b->bad && z < 64; ++z) {} --z; }
            else { z = zbp[i]; tt_below(&tz, b, i, z + 1); }
            const int passes = io_passes(b, (int)r[0]);
            int lblock = 3, more;
            if (b->reading) {
                while (get_bit(b) && !b->bad) ++lblock;
                r[0] = passes; r[1] = mb[k] - z;
                r[2] = (int32_t)io_bits(b, 0, lblock + ilog2((uint32_t)passes));
            } else {
                const int need = ilog2(r[2] > 0 ? (uint32_t)r[2] : 1u) + 1;
                more = need - (lblock + ilog2((uint32_t)passes));
                if (more > 0) ++g_cnt[CNT_LBLOCK_INC];
                for (int i2 = 0; i2 < more; ++i2) put_bit(b, 1);
                put_bit(b, 0);
                if (more > 0) lblock += more;
                io_bits(b, (uint32_t)r[2], lblock + ilog2((uint32_t)passes));
            }
        }
        free(ti.n); free(tz.n); free(incl);
    }
    bits_end(b);
    if (b->bad) FAIL(-3, "packet header runs beyond the data");
    return 0;
}

int64_t jo_packet_header_write(int nbands, const int32_t *gw, const int32_t *gh, const int32_t *mb, const int32_t *rec, uint8_t *out, size_t cap)
{
    out_t o = {out, cap, 0};
    bits_t b;
    bits_begin_write(&b, &o);
    if (packet_header(&b, nbands, gw, gh, mb, (int32_t *)rec)) return -1;
    return (int64_t)o.n;
}
/* returns the header's length */
int64_t jo_packet_header_parse(int nbands, const int32_t *gw, const int32_t *gh, const int32_t *mb, const uint8_t *in, size_t n, int32_t *rec)
{
    bits_t b;
    bits_begin_read(&b, in, n);
    if (packet_header(&b, nbands, gw, gh, mb, rec)) return -1;
    return (int64_t)b.in_pos;
}

/* ================================================================== whole files: writer */

static void level_shift_in(const uint16_t *planes, const params_t *p, int t, int c, int32_t *a)
{
    int64_t x0, y0, x1, y1;
    tile_rect(p, t, &x0, &y0, &x1, &y1);
    const int w = (int)(x1 - x0);
    for (int64_t y = y0; y < y1; ++y)
        for (int64_t x = x0; x < x1; ++x)
            a[(size_t)(y - y0) * w + (x - x0)] = (int32_t)planes[((size_t)c * p->H + y) * p->W + x] - (1 << (p->bits - 1));
}

/* the transformed coefficients of one tile-component (Mallat layout, rows of the tile's own width) */
int jo_coefficients(const uint16_t *planes, int C, int H, int W, int bits, int tile, int comp, int32_t *out)
{
    params_t p;
    if (own_params(&p, C, H, W, bits)) return -1;
    if (tile < 0 || tile >= ntiles_x(&p) * ntiles_y(&p) || comp < 0 || comp >= C) FAIL(-1, "jo_coefficients: no such tile-component");
    int64_t x0, y0, x1, y1;
    tile_rect(&p, tile, &x0, &y0, &x1, &y1);
    level_shift_in(planes, &p, tile, comp, out);
    return jo_dwt53(out, (int)(x1 - x0), (int)(y1 - y0), (int)(x1 - x0), (int)x0, (int)y0, p.NL, 0);
}

static void write_main_header(out_t *o, const params_t *p, size_t *jp2c_at)
{
    static const uint8_t signature[12] = {0, 0, 0, 12, 'j', 'P', ' ', ' ', 0x0D, 0x0A, 0x87, 0x0A};
    for (int k = 0; k < 12; ++k) o8(o, signature[k]);
    o32(o, 20); otag(o, "ftyp"); otag(o, "jp2 "); o32(o, 0); otag(o, "jp2 ");
    o32(o, 8 + 22 + 15); otag(o, "jp2h");
    o32(o, 22); otag(o, "ihdr"); o32(o, (uint32_t)p->H); o32(o, (uint32_t)p->W); o16(o, (unsigned)p->C);
    o8(o, (unsigned)p->bits - 1); o8(o, 7); o8(o, 0); o8(o, 0);
    o32(o, 15); otag(o, "colr"); o8(o, 1); o8(o, 0); o8(o, 0); o32(o, p->C == 3 ? 16u : (p->C == 1 ? 17u : 0u));
    *jp2c_at = o->n;
    o32(o, 0); otag(o, "jp2c");
    o16(o, 0xFF4F);                                                        /* SOC */
    o16(o, 0xFF51); o16(o, 38 + 3 * (unsigned)p->C); o16(o, 0);            /* SIZ */
    o32(o, (uint32_t)p->W); o32(o, (uint32_t)p->H); o32(o, 0); o32(o, 0);
    o32(o, (uint32_t)p->XT); o32(o, (uint32_t)p->YT); o32(o, 0); o32(o, 0);
    o16(o, (unsigned)p->C);
    for (int c = 0; c < p->C; ++c) { o8(o, (unsigned)p->bits - 1); o8(o, 1); o8(o, 1); }
    o16(o, 0xFF52); o16(o, 12); o8(o, 0);                                  /* COD */
    o8(o, (unsigned)p->prog); o16(o, (unsigned)p->layers); o8(o, 0);
    o8(o, (unsigned)p->NL); o8(o, (unsigned)ilog2((uint32_t)p->cbw) - 2); o8(o, (unsigned)ilog2((uint32_t)p->cbh) - 2); o8(o, 0); o8(o, 1);
    o16(o, 0xFF5C); o16(o, 4 + 3 * (unsigned)p->NL); o8(o, (unsigned)p->guard << 5);   /* QCD, no quantisation */
    for (int k = 0; k < 1 + 3 * p->NL; ++k) o8(o, (unsigned)p->eps[k] << 3);
}

int64_t jo_encode(const uint16_t *planes, int C, int H, int W, int bits, uint8_t *out, size_t cap)
{
    params_t p;
    if (own_params(&p, C, H, W, bits)) return -1;
    for (size_t k = 0; k < (size_t)C * H * W; ++k) if (planes[k] >> bits) FAIL(-1, "a value does not fit %d bits", bits);
    out_t o = {out, cap, 0};
    size_t jp2c;
    write_main_header(&o, &p, &jp2c);
    const int nt = ntiles_x(&p) * ntiles_y(&p);
    int rc = 0;
    for (int t = 0; t < nt && !rc; ++t) {
        int64_t x0, y0, x1, y1;
        tile_rect(&p, t, &x0, &y0, &x1, &y1);
        const int w = (int)(x1 - x0), h = (int)(y1 - y0);
        int32_t **coef = (int32_t **)calloc((size_t)C, sizeof *coef);
        if (!coef) FAIL(-2, "out of memory");
        for (int c = 0; c < C && !rc; ++c) {
            coef[c] = (int32_t *)malloc(sizeof(int32_t) * (size_t)w * h);
            if (!coef[c]) { rc = -2; break; }
            level_shift_in(planes, &p, t, c, coef[c]);
            rc = jo_dwt53(coef[c], w, h, w, (int)x0, (int)y0, p.NL, 0);
        }
        const size_t sot = o.n;
        o16(&o, 0xFF90); o16(&o, 10); o16(&o, (unsigned)t); o32(&o, 0); o8(&o, 0); o8(&o, 1);
        o16(&o, 0xFF93);
        for (int r = 0; r <= p.NL && !rc; ++r)
            for (int c = 0; c < C && !rc; ++c) {
                band_t bd[3];
                const int nbands = bands_of(&p, t, r, bd);
                if (!nbands) continue;
                int32_t gw[3], gh[3], mb[3];
                int64_t nblk = 0;
                for (int b = 0; b < nbands; ++b) { gw[b] = bd[b].gw; gh[b] = bd[b].gh; mb[b] = bd[b].mb; nblk += (int64_t)gw[b] * gh[b]; }
                int32_t *rec = (int32_t *)calloc((size_t)(nblk ? nblk : 1) * 3, sizeof(int32_t));
                uint8_t **bytes = (uint8_t **)calloc((size_t)(nblk ? nblk : 1), sizeof *bytes);
                if (!rec || !bytes) { free(rec); free(bytes); rc = -2; break; }
                int64_t k = 0;
                for (int b = 0; b < nbands && !rc; ++b)
                    for (int gy = 0; gy < bd[b].gh && !rc; ++gy)
                        for (int gx = 0; gx < bd[b].gw && !rc; ++gx, ++k) {
                            int bx, by, bw, bh;
                            block_rect(&p, &bd[b], gx, gy, &bx, &by, &bw, &bh);
                            const int room = bw * bh * 5 + 4096;
                            bytes[k] = (uint8_t *)malloc((size_t)room);
                            if (!bytes[k]) { rc = -2; break; }
                            const int n = jo_t1_encode(coef[c] + (size_t)by * w + bx, w, bw, bh, bd[b].orient, bytes[k], room, &rec[3 * k], &rec[3 * k + 1]);
                            if (n < 0 || n > room) { snprintf(g_err, sizeof g_err, "a block of %d bytes", n); rc = -3; break; }
                            if (rec[3 * k + 1] > mb[b]) { snprintf(g_err, sizeof g_err, "a block has %d bit-planes, its band announces %d", rec[3 * k + 1], mb[b]); rc = -3; break; }
                            rec[3 * k + 2] = n;
                        }
                if (!rc) {
                    bits_t bw_;
                    bits_begin_write(&bw_, &o);
                    rc = packet_header(&bw_, nbands, gw, gh, mb, rec);
                    for (int64_t i = 0; i < nblk && !rc; ++i) {
                        if (!rec[3 * i]) continue;
                        if (o.n + (size_t)rec[3 * i + 2] <= o.cap) memcpy(o.p + o.n, bytes[i], (size_t)rec[3 * i + 2]);
                        o.n += (size_t)rec[3 * i + 2];
                    }
                }
                for (int64_t i = 0; i < nblk; ++i) free(bytes[i]);
                free(bytes); free(rec);
            }
        opatch32(&o, sot + 6, (uint32_t)(o.n - sot));
        for (int c = 0; c < C; ++c) free(coef[c]);
        free(coef);
    }
    if (rc == -2) FAIL(-2, "out of memory");
    if (rc) return rc;
    o16(&o, 0xFFD9);
    opatch32(&o, jp2c, (uint32_t)(o.n - jp2c));
    return (int64_t)o.n;
}

/* ================================================================== whole files: parser and decoder */

static uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] << 8 | p[1]; }
static uint32_t rd32(const uint8_t *p) { return rd16(p) << 16 | rd16(p + 2); }

typedef struct { params_t p; size_t *tile_at, *tile_end; int ntiles; } stream_t;   /* tile_at: first byte behind SOD */

static void stream_free(stream_t *s) { free(s->tile_at); free(s->tile_end); }

static int read_headers(const uint8_t *f, size_t n, stream_t *s)
{
    memset(s, 0, sizeof *s);
    params_t *p = &s->p;
    size_t at = 0, end = n;
    if (n >= 12 && rd32(f) == 12 && !memcmp(f + 4, "jP  ", 4)) {             /* JP2: walk the boxes to jp2c */
        int found = 0;
        while (at + 8 <= n) {
            uint64_t len = rd32(f + at);
            size_t hdr = 8;
            if (len == 1) { if (at + 16 > n) break; len = (uint64_t)rd32(f + at + 8) << 32 | rd32(f + at + 12); hdr = 16; }
            else if (len == 0) len = n - at;
            if (len < hdr || at + len > n) FAIL(-3, "box at %zu runs beyond the file", at);
            if (!memcmp(f + at + 4, "jp2c", 4)) { end = at + (size_t)len; at += hdr; found = 1; break; }
            at += (size_t)len;
        }
        if (!found) FAIL(-3, "no jp2c box");
    }
    if (at + 4 > end || rd16(f + at) != 0xFF4F) FAIL(-3, "no SOC marker");
    at += 2;
    int have_siz = 0, have_cod = 0, have_qcd = 0;
    while (at + 4 <= end && rd16(f + at) != 0xFF90) {
        const uint32_t marker = rd16(f + at), len = rd16(f + at + 2);
        const uint8_t *q = f + at + 4;
        if (at + 2 + len > end || len < 2) FAIL(-3, "marker segment %04X runs beyond the stream", marker);
        if (marker == 0xFF51) {
            if (len < 41) FAIL(-3, "short SIZ");
            p->W = (int)rd32(q + 2); p->H = (int)rd32(q + 6);
            if (rd32(q + 10) || rd32(q + 14) || rd32(q + 26) || rd32(q + 30)) FAIL(-4, "image or tile offsets are not supported");
            p->XT = (int)rd32(q + 18); p->YT = (int)rd32(q + 22);
            p->C = (int)rd16(q + 34);
            if (len != 38 + 3u * (uint32_t)p->C || p->C < 1) FAIL(-3, "bad SIZ");
            for (int c = 0; c < p->C; ++c) {
                if (q[36 + 3 * c] != q[36] || q[37 + 3 * c] != 1 || q[38 + 3 * c] != 1) FAIL(-4, "components differ or are sub-sampled");
            }
            if (q[36] & 0x80) FAIL(-4, "signed components are not supported");
            p->bits = q[36] + 1;
            if (p->bits > 16 || p->W < 1 || p->H < 1 || p->XT < 1 || p->YT < 1) FAIL(-4, "unsupported SIZ");
            have_siz = 1;
        } else if (marker == 0xFF52) {
            if (len < 12) FAIL(-3, "short COD");
            if (q[0] & 1) FAIL(-4, "explicit precincts are not supported");
            p->sop = (q[0] >> 1) & 1; p->eph = (q[0] >> 2) & 1;
            p->prog = q[1]; p->layers = (int)rd16(q + 2); p->mct = q[4]; p->NL = q[5];
            p->cbw = 1 << (q[6] + 2); p->cbh = 1 << (q[7] + 2);
            if (q[8] != 0) FAIL(-4, "code-block style %u is not supported", q[8]);
            if (q[9] != 1) FAIL(-4, "only the reversible 5/3 transform is supported");
            if (p->layers != 1 || p->prog > 2 || p->mct || p->NL > 32) FAIL(-4, "layers %d, progression %d, component transform %d", p->layers, p->prog, p->mct);
            have_cod = 1;
        } else if (marker == 0xFF5C) {
            if ((q[0] & 31) != 0) FAIL(-4, "quantised streams are not supported");
            p->guard = q[0] >> 5;
            for (uint32_t k = 0; k + 3 < len && k < 97; ++k) p->eps[k] = q[1 + k] >> 3;
            have_qcd = (int)len - 3;
        } else if (marker == 0xFF53 || marker == 0xFF5D || marker == 0xFF5E || marker == 0xFF5F) {
            FAIL(-4, "marker %04X (COC / QCC / RGN / POC) is not supported", marker);
        }   /* COM and the pointer segments are skipped */
        at += 2 + len;
    }
    if (!have_siz || !have_cod || !have_qcd) FAIL(-3, "SIZ, COD or QCD missing");
    if (have_qcd < 1 + 3 * p->NL) FAIL(-3, "QCD has %d exponents, %d bands", have_qcd, 1 + 3 * p->NL);
    s->ntiles = ntiles_x(p) * ntiles_y(p);
    s->tile_at = (size_t *)calloc((size_t)s->ntiles, sizeof(size_t));
    s->tile_end = (size_t *)calloc((size_t)s->ntiles, sizeof(size_t));
    if (!s->tile_at || !s->tile_end) { stream_free(s); FAIL(-2, "out of memory"); }
    while (at + 12 <= end && rd16(f + at) == 0xFF90) {
        const uint32_t isot = rd16(f + at + 4), psot = rd32(f + at + 6);
        const size_t part_end = psot ? at + psot : end - 2;
        if ((int)isot >= s->ntiles || part_end > end || f[at + 10] != 0) { stream_free(s); FAIL(-4, "tile-part %u of tile %u: only one tile-part per tile is supported", f[at + 10], isot); }
        if (s->tile_at[isot]) { stream_free(s); FAIL(-4, "tile %u has several tile-parts", isot); }
        size_t q = at + 12;
        while (q + 4 <= part_end && rd16(f + q) != 0xFF93) {
            const uint32_t marker = rd16(f + q);
            if (marker != 0xFF64 && marker != 0xFF58 && marker != 0xFF61) { stream_free(s); FAIL(-4, "marker %04X in a tile-part header is not supported", marker); }
            q += 2 + rd16(f + q + 2);
        }
        if (q + 2 > part_end) { stream_free(s); FAIL(-3, "no SOD in tile-part of tile %u", isot); }
        s->tile_at[isot] = q + 2;
        s->tile_end[isot] = part_end;
        at = part_end;
    }
    if (at + 2 > end || rd16(f + at) != 0xFFD9) { stream_free(s); FAIL(-3, "no EOC where the tile-parts end (offset %zu)", at); }
    for (int t = 0; t < s->ntiles; ++t) if (!s->tile_at[t]) { stream_free(s); FAIL(-3, "tile %d is missing", t); }
    return 0;
}

/* {C, H, W, bits, tiles, blocks, resolutions, tile width, tile height} */
int jo_info(const uint8_t *f, size_t n, int64_t out[9])
{
    stream_t s;
    if (read_headers(f, n, &s)) return -1;
    out[0] = s.p.C; out[1] = s.p.H; out[2] = s.p.W; out[3] = s.p.bits; out[4] = s.ntiles;
    out[5] = enumerate_blocks(&s.p, NULL, 0); out[6] = s.p.NL + 1; out[7] = s.p.XT; out[8] = s.p.YT;
    stream_free(&s);
    return 0;
}

static int64_t parse_stream(const uint8_t *f, const stream_t *s, int64_t *rec, int64_t cap)
{
    const params_t *p = &s->p;
    const int64_t total = enumerate_blocks(p, rec, cap);
    if (total > cap) FAIL(-1, "%lld records, room for %lld", (long long)total, (long long)cap);
    int64_t k = 0;
    for (int t = 0; t < s->ntiles; ++t) {
        size_t at = s->tile_at[t];
        const size_t end = s->tile_end[t];
        for (int r = 0; r <= p->NL; ++r)
            for (int c = 0; c < p->C; ++c) {
                band_t bd[3];
                const int nbands = bands_of(p, t, r, bd);
                if (!nbands) continue;
                int32_t gw[3], gh[3], mb[3];
                int64_t nblk = 0;
                for (int b = 0; b < nbands; ++b) { gw[b] = bd[b].gw; gh[b] = bd[b].gh; mb[b] = bd[b].mb; nblk += (int64_t)gw[b] * gh[b]; }
                if (p->sop && at + 6 <= end && rd16(f + at) == 0xFF91) at += 6;
                int32_t *r3 = (int32_t *)calloc((size_t)(nblk ? nblk : 1) * 3, sizeof(int32_t));
                if (!r3) FAIL(-2, "out of memory");
                const int64_t used = jo_packet_header_parse(nbands, gw, gh, mb, f + at, end - at, r3);
                if (used < 0) { free(r3); return -3; }
                at += (size_t)used;
                if (p->eph) { if (at + 2 > end || rd16(f + at) != 0xFF92) { free(r3); FAIL(-3, "EPH missing"); } at += 2; }
                for (int64_t i = 0; i < nblk; ++i, ++k) {
                    int64_t *q = rec + k * R_N;
                    q[R_PASSES] = r3[3 * i]; q[R_NUMBPS] = r3[3 * i + 1]; q[R_LENGTH] = r3[3 * i + 2];
                    if (r3[3 * i]) { q[R_OFFSET] = (int64_t)at; at += (size_t)r3[3 * i + 2]; }
                    if (at > end) { free(r3); FAIL(-3, "tile %d: block data runs beyond the tile-part", t); }
                }
                free(r3);
            }
        if (at != end) FAIL(-3, "tile %d: %zu bytes of its tile-part are not accounted for", t, end - at);
    }
    return total;
}

/* rec: room for jo_info's block count * 16 int64.  Returns the number of records. */
int64_t jo_parse(const uint8_t *f, size_t n, int64_t *rec, int64_t cap)
{
    stream_t s;
    if (read_headers(f, n, &s)) return -1;
    const int64_t r = parse_stream(f, &s, rec, cap);
    stream_free(&s);
    return r;
}

/* planes: C * H * W uint16 */
int jo_decode(const uint8_t *f, size_t n, uint16_t *planes)
{
    stream_t s;
    if (read_headers(f, n, &s)) return -1;
    const params_t *p = &s.p;
    const int64_t total = enumerate_blocks(p, NULL, 0);
    int64_t *rec = (int64_t *)malloc(sizeof(int64_t) * R_N * (size_t)(total ? total : 1));
    if (!rec) { stream_free(&s); FAIL(-2, "out of memory"); }
    int rc = parse_stream(f, &s, rec, total) < 0 ? -3 : 0;
    for (int t = 0; t < s.ntiles && !rc; ++t) {
        int64_t x0, y0, x1, y1;
        tile_rect(p, t, &x0, &y0, &x1, &y1);
        const int w = (int)(x1 - x0), h = (int)(y1 - y0);
        int32_t *a = (int32_t *)malloc(sizeof(int32_t) * (size_t)w * h);
        if (!a) { rc = -2; break; }
        for (int c = 0; c < p->C && !rc; ++c) {
            memset(a, 0, sizeof(int32_t) * (size_t)w * h);
            for (int64_t k = 0; k < total && !rc; ++k) {
                const int64_t *q = rec + k * R_N;
                if (q[R_TILE] != t || q[R_COMP] != c || !q[R_PASSES]) continue;
                if (q[R_NUMBPS] < 0 || q[R_NUMBPS] > 31) { snprintf(g_err, sizeof g_err, "a block of %lld bit-planes", (long long)q[R_NUMBPS]); rc = -3; break; }
                rc = jo_t1_decode(f + q[R_OFFSET], (int)q[R_LENGTH], (int)q[R_W], (int)q[R_H], (int)q[R_ORIENT], (int)q[R_NUMBPS],
                                  (int)q[R_PASSES], a + (size_t)q[R_Y] * w + q[R_X], w);
            }
            if (!rc) rc = jo_dwt53(a, w, h, w, (int)x0, (int)y0, p->NL, 1);
            const int32_t half = 1 << (p->bits - 1), top = (1 << p->bits) - 1;
            for (int y = 0; y < h && !rc; ++y)
                for (int x = 0; x < w; ++x) {
                    int32_t v = a[(size_t)y * w + x] + half;
                    v = v < 0 ? 0 : (v > top ? top : v);
                    planes[((size_t)c * p->H + (size_t)(y0 + y)) * p->W + (size_t)(x0 + x)] = (uint16_t)v;
                }
        }
        free(a);
    }
    free(rec);
    stream_free(&s);
    return rc;
}
