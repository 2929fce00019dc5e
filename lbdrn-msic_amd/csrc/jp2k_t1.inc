// JPEG 2000 tier-1 (ITU-T T.800 Annex C: the MQ arithmetic coder; Annex D: coefficient bit modelling) for one code block
// of at most 64 x 64 coefficients, code-block style 0: every magnitude bit-plane from the first non-zero one, three
// passes per plane (significance propagation, magnitude refinement, clean-up with the run-length mode), 19 contexts, one
// codeword segment closed by the standard's flush.  Included by jp2k.hip (the coder, called from k_jp2k_blocks only) and,
// through jp2k_t1d.inc (the MQ decoder and the decoder's policy), by jp2k_dec.hip; every function is JP2K_HD (__host__
// __device__ under hipcc, nothing elsewhere), so a host compiler builds the same text and CPU tests judge both directions
// byte for byte against an independent codec without a GPU.
//
// The scan of Annex D exists once: t1_walk owns the plane / pass / stripe / column loops, the register windows, the flag
// words and every context choice.  t1_encode_block (here) and t1_decode_block (jp2k_t1d.inc) are its only callers; each
// hands it a policy (T1Coder, T1Decoder) that says where a decision comes from -- a bit of `mag` that is MQ-coded, or an
// MQ-decoded bit that is entered into `mag` -- and nothing else.
//
// State of a block, all of it in memory the CALLER provides (LDS in the kernels).  The caller fills the two tables
// (t1_fill_tables) and ZEROES `st`, and `mag` too before decoding; the entry points initialise `cx`:
//   mag[stripe][col][4]   sign (bit 31) and magnitude of the four samples of a stripe column: the coder reads a column it
//                         visits with one 128-bit read; the decoder enters a sample when it becomes significant and ORs
//                         its later bits in
//   st[(stripe+1)*66 + col+1]   16 flag bits of a stripe column: 0-3 significant, 4-7 negative, 8-11 coded in this
//                               plane's significance pass ("pi"), 12-15 refined before ("mu"); a border of zeros all round
//   cx[19]                the contexts' states: index into the 94-entry transition table below (2 * state + MPS)
// and A, C, CT, the pending byte and the position in registers.  A pass walks the stripes column by column with the
// significance / sign bits of the columns left, here and right in three 6-bit register windows (row -1 comes from the
// stripe above, row 4 from the one below); a column whose windows are empty is skipped without touching its samples.
// Every loop is bounded by the geometry: planes <= 31, passes <= 91, stripes <= 16, columns <= 64, rows <= 4.  The coder
// counts bytes beyond `cap` and never writes them; the decoder never reads beyond `len` (MqDec).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define JP2K_HD __host__ __device__ __forceinline__
#else
#define JP2K_HD inline
#endif

namespace jp2k {

constexpr int T1_CTX_ZC = 0, T1_CTX_SC = 9, T1_CTX_MAG = 14, T1_CTX_RL = 17, T1_CTX_UNI = 18, T1_NCTX = 19;
constexpr int T1_STW = 66;   // flag words per stripe row (64 columns + a border each side)
constexpr int T1_NST = 18;   // stripe rows (16 + a border above and below)

// T.800 Table C.2: Qe, NMPS, NLPS, SWITCH of the 47 states
struct MqRow { uint16_t qe; uint8_t nmps, nlps, sw; };
constexpr MqRow MQ_ROWS[47] = {
    {0x5601, 1, 1, 1},   {0x3401, 2, 6, 0},   {0x1801, 3, 9, 0},   {0x0AC1, 4, 12, 0},  {0x0521, 5, 29, 0},
    {0x0221, 38, 33, 0}, {0x5601, 7, 6, 1},   {0x5401, 8, 14, 0},  {0x4801, 9, 14, 0},  {0x3801, 10, 14, 0},
    {0x3001, 11, 17, 0}, {0x2401, 12, 18, 0}, {0x1C01, 13, 20, 0}, {0x1601, 29, 21, 0}, {0x5601, 15, 14, 1},
    {0x5401, 16, 14, 0}, {0x5101, 17, 15, 0}, {0x4801, 18, 16, 0}, {0x3801, 19, 17, 0}, {0x3401, 20, 18, 0},
    {0x3001, 21, 19, 0}, {0x2801, 22, 19, 0}, {0x2401, 23, 20, 0}, {0x2201, 24, 21, 0}, {0x1C01, 25, 22, 0},
    {0x1801, 26, 23, 0}, {0x1601, 27, 24, 0}, {0x1401, 28, 25, 0}, {0x1201, 29, 26, 0}, {0x1101, 30, 27, 0},
    {0x0AC1, 31, 28, 0}, {0x09C1, 32, 29, 0}, {0x08A1, 33, 30, 0}, {0x0521, 34, 31, 0}, {0x0441, 35, 32, 0},
    {0x02A1, 36, 33, 0}, {0x0221, 37, 34, 0}, {0x0141, 38, 35, 0}, {0x0111, 39, 36, 0}, {0x0085, 40, 37, 0},
    {0x0049, 41, 38, 0}, {0x0025, 42, 39, 0}, {0x0015, 43, 40, 0}, {0x0009, 44, 41, 0}, {0x0005, 45, 42, 0},
    {0x0001, 45, 43, 0}, {0x5601, 46, 46, 0}};

// entry 2 * state + MPS of the working table: Qe | next entry after an MPS << 16 | next entry after an LPS << 24
JP2K_HD uint32_t mq_entry(int e)
{
    const int s = e >> 1, mps = e & 1;
    const MqRow r = MQ_ROWS[s];
    return (uint32_t)r.qe | (uint32_t)(2 * r.nmps + mps) << 16 | (uint32_t)(2 * r.nlps + (mps ^ r.sw)) << 24;
}
constexpr int MQ_ENTRIES = 94;

// T.800 Table D.1: zero-coding context from the significant horizontal, vertical and diagonal neighbours.
// orient: 0 LL, 1 HL (horizontal high-pass), 2 LH, 3 HH.
JP2K_HD int zc_context(int h, int v, int d, int orient)
{
    if (orient == 3) {
        const int hv = h + v;
        if (d >= 3) return 8;
        if (d == 2) return hv >= 1 ? 7 : 6;
        if (d == 1) return hv >= 2 ? 5 : (hv == 1 ? 4 : 3);
        return hv >= 2 ? 2 : hv;
    }
    if (orient == 1) { const int t = h; h = v; v = t; }
    if (h == 2) return 8;
    if (h == 1) return v >= 1 ? 7 : (d >= 1 ? 6 : 5);
    if (v == 2) return 4;
    if (v == 1) return 3;
    return d >= 2 ? 2 : d;
}
// the 256-entry table the coder indexes: bits 0-2 the left column's rows r-1, r, r+1; 3-5 the right column's; 6 above; 7 below
JP2K_HD int zc_lut_entry(int idx, int orient)
{
    const int h = ((idx >> 1) & 1) + ((idx >> 4) & 1);
    const int v = ((idx >> 6) & 1) + ((idx >> 7) & 1);
    const int d = (idx & 1) + ((idx >> 2) & 1) + ((idx >> 3) & 1) + ((idx >> 5) & 1);
    return T1_CTX_ZC + zc_context(h, v, d, orient);
}
// mqtab[94] and zc[256] for a block of a subband of orientation `orient`, filled by `nlanes` callers of which this one is
// `lane` (the wave in the kernels; 0 of 1 on a host).  One loop on purpose: as two loops inlined into the kernels, hipcc
// 7.2 allocates k_jp2k_blocks and k_jp2k_unblocks 45 vector registers instead of 16 (DESIGN 7).
JP2K_HD void t1_fill_tables(uint32_t* mqtab, uint8_t* zc, int orient, int lane, int nlanes)
{
    for (int k = lane; k < 256; k += nlanes) {
        if (k < MQ_ENTRIES) mqtab[k] = mq_entry(k);
        zc[k] = (uint8_t)zc_lut_entry(k, orient);
    }
}

struct Mq {
    uint32_t A, C;
    int CT, B, pos;
    uint8_t* out;
    int cap;
    uint8_t* cx;            // [19] entries of the working table
    const uint32_t* tab;    // [94]

    JP2K_HD void init(uint8_t* out_, int cap_, uint8_t* cx_, const uint32_t* tab_)
    {
        A = 0x8000; C = 0; CT = 12; B = 0; pos = -1;
        out = out_; cap = cap_; cx = cx_; tab = tab_;
    }
    JP2K_HD void emit()
    {
        if (pos >= 0 && pos < cap) out[pos] = (uint8_t)B;
        ++pos;
    }
    JP2K_HD void byteout()
    {
        if (B != 0xFF && C >= 0x8000000u) {   // carry into the pending byte
            ++B;
            C &= 0x7FFFFFFu;
        }
        emit();
        if (B == 0xFF) { B = (int)(C >> 20); C &= 0xFFFFFu; CT = 7; }
        else { B = (int)(C >> 19); C &= 0x7FFFFu; CT = 8; }
    }
    JP2K_HD void renorm()
    {
        do {
            A <<= 1;
            C <<= 1;
            if (--CT == 0) byteout();
        } while (!(A & 0x8000u));
    }
    JP2K_HD void encode(int d, int ctx)
    {
        const int e = cx[ctx];
        const uint32_t t = tab[e];
        const uint32_t qe = t & 0xFFFFu;
        A -= qe;
        if (d == (e & 1)) {
            if (A & 0x8000u) { C += qe; return; }
            if (A < qe) A = qe; else C += qe;
            cx[ctx] = (uint8_t)((t >> 16) & 0xFF);
        } else {
            if (A < qe) C += qe; else A = qe;
            cx[ctx] = (uint8_t)(t >> 24);
        }
        renorm();
    }
    // T.800 C.2.9: FLUSH.  Returns the segment's length; a last byte of 0xFF is not part of it.
    JP2K_HD int flush()
    {
        const uint32_t temp = C + A;
        C |= 0xFFFFu;
        if (C >= temp) C -= 0x8000u;
        C <<= CT; byteout();
        C <<= CT; byteout();
        if (B != 0xFF) emit();
        return pos;
    }
};

// 6-bit windows (row -1 .. row 4) of one column's significance and sign bits, from the flag words of three stripes
JP2K_HD uint32_t t1_sig_window(uint32_t up, uint32_t cur, uint32_t dn) { return ((up >> 3) & 1u) | ((cur & 15u) << 1) | ((dn & 1u) << 5); }
JP2K_HD uint32_t t1_neg_window(uint32_t up, uint32_t cur, uint32_t dn) { return ((up >> 7) & 1u) | (((cur >> 4) & 15u) << 1) | (((dn >> 4) & 1u) << 5); }

// neighbour index of row r (0..3) for the zero-coding table
JP2K_HD int t1_nbr(uint32_t L, uint32_t M, uint32_t R, int r)
{
    return (int)(((L >> r) & 7u) | (((R >> r) & 7u) << 3) | (((M >> r) & 1u) << 6) | (((M >> (r + 2)) & 1u) << 7));
}
// T.800 Table D.3: the sign context of row r and, in x, the bit the sign is XORed with
JP2K_HD int t1_sign_ctx(uint32_t L, uint32_t M, uint32_t R, uint32_t Ln, uint32_t Mn, uint32_t Rn, int r, int& x)
{
    const int lp = (int)((L >> (r + 1)) & 1u), ln = (int)((Ln >> (r + 1)) & 1u);
    const int rp = (int)((R >> (r + 1)) & 1u), rn = (int)((Rn >> (r + 1)) & 1u);
    const int up = (int)((M >> r) & 1u), un = (int)((Mn >> r) & 1u);
    const int dp = (int)((M >> (r + 2)) & 1u), dn = (int)((Mn >> (r + 2)) & 1u);
    // (a neighbour's sign bit is only ever set together with its significance bit)
    const int hpos = (lp & ~ln) | (rp & ~rn), hneg = ln | rn;
    const int vpos = (up & ~un) | (dp & ~dn), vneg = un | dn;
    const int h = hpos - hneg, v = vpos - vneg;
    x = (h < 0 || (h == 0 && v < 0)) ? 1 : 0;
    return h != 0 ? 12 + h * v : (v != 0 ? 10 : 9);
}
// the sample at row r has just become significant in plane p: its sign, and its entry into the column's windows
template <class Io>
JP2K_HD void t1_found(Io& io, uint32_t L, uint32_t& M, uint32_t R, uint32_t Ln, uint32_t& Mn, uint32_t Rn, int r, int p)
{
    int x;
    const int ctx = t1_sign_ctx(L, M, R, Ln, Mn, Rn, r, x);
    const uint32_t neg = io.sign(r, p, ctx, x);
    M |= 2u << r;
    Mn |= neg << (r + 1);
}

// The coding passes of a w x h block (1..64 each) from bit-plane numbps - 1 (1..31) down, at most `max_passes` of them;
// returns how many were done.  st must be zero on entry; zc: the 256-entry zero-coding table of the block's subband.
// What Io supplies, all for the stripe column last named by column(s, c):
//   bit(r, p, ctx)        bit p of the sample at row r, coded or decoded in context ctx
//   refine(r, p, ctx)     the same for a sample that is significant already (the decoder enters the bit into `mag`)
//   sign(r, p, ctx, x)    the sign of the sample at row r that has become significant in plane p (1: negative), coded or
//                         decoded as sign ^ x in context ctx (the decoder enters the sample into `mag`)
//   run(p)                the run-length symbol of a column of four: -1 when none of them has bit p, else the first row
//                         that has (T1_CTX_RL, then the row's two bits in T1_CTX_UNI)
template <class Io>
JP2K_HD int t1_walk(Io& io, uint16_t* st, const uint8_t* zc, int w, int h, int numbps, int max_passes)
{
    const int nstripes = (h + 3) >> 2;
    int passes = 0;
    for (int p = numbps - 1; p >= 0 && passes < max_passes; --p) {
        for (int pass = p == numbps - 1 ? 2 : 0; pass < 3 && passes < max_passes; ++pass) {
            for (int s = 0; s < nstripes; ++s) {
                const int rows = h - 4 * s < 4 ? h - 4 * s : 4;
                uint16_t* up = st + s * T1_STW + 1;        // st row s is stripe s - 1
                uint16_t* cur = up + T1_STW;
                uint16_t* dn = cur + T1_STW;
                uint32_t L = 0, Ln = 0;
                uint32_t M = t1_sig_window(up[0], cur[0], dn[0]), Mn = t1_neg_window(up[0], cur[0], dn[0]);
                for (int c = 0; c < w; ++c) {
                    const uint32_t ru = up[c + 1], rc = cur[c + 1], rd = dn[c + 1];
                    const uint32_t R = t1_sig_window(ru, rc, rd), Rn = t1_neg_window(ru, rc, rd);
                    const uint32_t f = cur[c];
                    uint32_t pi = (f >> 8) & 15u, mu = (f >> 12) & 15u;
                    const uint32_t any = L | M | R;
                    if (pass == 0) {
                        if (any) {
                            io.column(s, c);
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                if (r < rows && !((M >> (r + 1)) & 1u)) {
                                    const int nb = t1_nbr(L, M, R, r);
                                    if (nb) {
                                        pi |= 1u << r;
                                        if (io.bit(r, p, zc[nb])) t1_found(io, L, M, R, Ln, Mn, Rn, r, p);
                                    }
                                }
                            }
                            cur[c] = (uint16_t)(((M >> 1) & 15u) | (((Mn >> 1) & 15u) << 4) | (pi << 8) | (mu << 12));
                        }
                    } else if (pass == 1) {
                        const uint32_t todo = ((M >> 1) & 15u) & ~pi;
                        if (todo) {
                            io.column(s, c);
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                if ((todo >> r) & 1u) io.refine(r, p, ((mu >> r) & 1u) ? 16 : (t1_nbr(L, M, R, r) ? 15 : 14));
                            }
                            mu |= todo;
                            cur[c] = (uint16_t)((f & 0x0FFFu) | (mu << 12));
                        }
                    } else {
                        io.column(s, c);
                        int r0 = 0;                // the first row that is coded sample by sample; -1: none is
                        if (rows == 4 && !any) {   // run-length mode: four insignificant samples without a significant neighbour
                            r0 = io.run(p);
                            if (r0 >= 0) {
                                t1_found(io, L, M, R, Ln, Mn, Rn, r0, p);
                                ++r0;
                            }
                        }
                        if (r0 >= 0) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                if (r >= r0 && r < rows && !((M >> (r + 1)) & 1u) && !((pi >> r) & 1u)) {
                                    if (io.bit(r, p, zc[t1_nbr(L, M, R, r)])) t1_found(io, L, M, R, Ln, Mn, Rn, r, p);
                                }
                            }
                            cur[c] = (uint16_t)(((M >> 1) & 15u) | (((Mn >> 1) & 15u) << 4) | (mu << 12));   // pi cleared for the next plane
                        }
                    }
                    L = M; Ln = Mn;
                    M = R; Mn = Rn;
                }
            }
            ++passes;
        }
    }
    return passes;
}

// What both entry points (t1_encode_block, t1_decode_block) do first.  False: there is nothing to code.  Otherwise the arguments are clamped to what the
// state holds and the contexts are in their initial states (T.800 Table D.7).
JP2K_HD bool t1_begin(uint8_t* cx, int& w, int& h, int& numbps)
{
    if (numbps <= 0 || w <= 0 || h <= 0) return false;
    if (numbps > 31) numbps = 31;
    if (w > 64) w = 64;
    if (h > 64) h = 64;
    for (int k = 0; k < T1_NCTX; ++k) cx[k] = 0;
    cx[T1_CTX_ZC] = 2 * 4;
    cx[T1_CTX_RL] = 2 * 3;
    cx[T1_CTX_UNI] = 2 * 46;
    return true;
}

struct T1Coder {           // a decision is a bit of `mag`, which is MQ-coded
    Mq mq;
    const uint32_t* mag;
    uint32_t m0, m1, m2, m3;

    JP2K_HD void column(int s, int c)
    {
        const uint32_t* mp = mag + ((size_t)s * 64 + c) * 4;
        m0 = mp[0]; m1 = mp[1]; m2 = mp[2]; m3 = mp[3];
    }
    JP2K_HD uint32_t sample(int r) const { return r == 0 ? m0 : (r == 1 ? m1 : (r == 2 ? m2 : m3)); }
    JP2K_HD int bit(int r, int p, int ctx)
    {
        const int d = (int)((sample(r) >> p) & 1u);
        mq.encode(d, ctx);
        return d;
    }
    JP2K_HD void refine(int r, int p, int ctx) { bit(r, p, ctx); }
    JP2K_HD uint32_t sign(int r, int, int ctx, int x)
    {
        const uint32_t neg = sample(r) >> 31;
        mq.encode((int)neg ^ x, ctx);
        return neg;
    }
    JP2K_HD int run(int p)
    {
        const uint32_t b = ((m0 >> p) & 1u) | (((m1 >> p) & 1u) << 1) | (((m2 >> p) & 1u) << 2) | (((m3 >> p) & 1u) << 3);
        mq.encode(b != 0, T1_CTX_RL);
        if (!b) return -1;
        const int r0 = (b & 1u) ? 0 : ((b & 2u) ? 1 : ((b & 4u) ? 2 : 3));
        mq.encode(r0 >> 1, T1_CTX_UNI);
        mq.encode(r0 & 1, T1_CTX_UNI);
        return r0;
    }
};

struct T1Result { int bytes, passes, numbps; };

// Codes the block.  w, h: its size; numbps: magnitude bits of its largest coefficient (0: nothing is coded);
// zc: the 256-entry zero-coding table of the block's subband; st must be zero on entry.
JP2K_HD T1Result t1_encode_block(const uint32_t* mag, uint16_t* st, uint8_t* cx, const uint32_t* mqtab, const uint8_t* zc,
                                 int w, int h, int numbps, uint8_t* out, int cap)
{
    T1Result res = {0, 0, numbps};
    if (!t1_begin(cx, w, h, numbps)) return res;
    T1Coder io;
    io.mag = mag;
    io.mq.init(out, cap, cx, mqtab);
    res.passes = t1_walk(io, st, zc, w, h, numbps, 3 * numbps - 2);   // every pass there is
    res.bytes = io.mq.flush();
    return res;
}

}  // namespace jp2k
