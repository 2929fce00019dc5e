// JPEG 2000 tier-1 DECODER (ITU-T T.800 Annex C.3: the MQ decoder -- INITDEC, DECODE, BYTEIN, RENORMD; Annex D: the three
// passes per bit-plane over the 19 contexts, in the scan of D.1) for one code block of at most 64 x 64 coefficients,
// code-block style 0, one codeword segment.  The counterpart of jp2k_t1.inc, whose MQ table, context tables, flag-word
// layout and register windows it uses; included by jp2k_dec.hip and called from k_jp2k_unblocks only.  Every function is
// JP2K_HD, so a host compiler builds the same text and a CPU test judges it against an independent decoder.
//
// State of a block, all of it in memory the caller provides (LDS in the kernel) and has ZEROED (mag and st):
//   mag[stripe][col][4]   receives sign (bit 31) and magnitude of the four samples of a stripe column
//   st[(stripe+1)*66 + col+1]   the 16 flag bits of a stripe column, as in the coder
//   cx[19]                the contexts' states (initialised here)
// The bytes are read from `data[0 .. len)`; beyond them the decoder is fed 0xFF, as C.3.4 has it for the end of the
// segment (0xFF 0xFF is a marker, which BYTEIN never steps over), so no position beyond `len` is ever read and a
// truncated or damaged segment decodes to SOME coefficients in bounded time: planes <= 31, passes <= 91, stripes <= 16,
// columns <= 64, rows <= 4.
#pragma once
#include "jp2k_t1.inc"

namespace jp2k {

struct MqDec {
    uint32_t A, C;
    int CT, pos, len;
    const uint8_t* in;
    uint8_t* cx;            // [19] entries of the working table
    const uint32_t* tab;    // [94]

    JP2K_HD uint32_t byte(int i) const { return i < len ? (uint32_t)in[i] : 0xFFu; }
    JP2K_HD void bytein()
    {
        if (byte(pos) == 0xFFu) {
            const uint32_t next = byte(pos + 1);
            if (next > 0x8Fu) { C += 0xFF00u; CT = 8; }          // a marker: the segment has ended, ones from here on
            else { ++pos; C += next << 9; CT = 7; }              // a stuffed bit
        } else {
            ++pos;
            C += byte(pos) << 8;
            CT = 8;
        }
    }
    JP2K_HD void init(const uint8_t* in_, int len_, uint8_t* cx_, const uint32_t* tab_)
    {
        in = in_; len = len_ < 0 ? 0 : len_; cx = cx_; tab = tab_;
        pos = 0;
        C = byte(0) << 16;
        bytein();
        C <<= 7;
        CT -= 7;
        A = 0x8000u;
    }
    JP2K_HD int decode(int ctx)
    {
        const int e = cx[ctx];
        const uint32_t t = tab[e];
        const uint32_t qe = t & 0xFFFFu;
        int d = e & 1;
        A -= qe;
        if ((C >> 16) < qe) {              // LPS_EXCHANGE
            if (A < qe) cx[ctx] = (uint8_t)((t >> 16) & 0xFF);
            else { d ^= 1; cx[ctx] = (uint8_t)(t >> 24); }
            A = qe;
        } else {
            C -= qe << 16;
            if (A & 0x8000u) return d;
            if (A < qe) { d ^= 1; cx[ctx] = (uint8_t)(t >> 24); }      // MPS_EXCHANGE
            else cx[ctx] = (uint8_t)((t >> 16) & 0xFF);
        }
        do {                               // RENORMD
            if (CT == 0) bytein();
            A <<= 1;
            C <<= 1;
            --CT;
        } while (!(A & 0x8000u));
        return d;
    }
};

// T.800 Table D.3 read backwards: the sign of the sample at row r that has just become significant
JP2K_HD int t1d_sign(MqDec& mq, uint32_t L, uint32_t M, uint32_t R, uint32_t Ln, uint32_t Mn, uint32_t Rn, int r)
{
    const int lp = (int)((L >> (r + 1)) & 1u), ln = (int)((Ln >> (r + 1)) & 1u);
    const int rp = (int)((R >> (r + 1)) & 1u), rn = (int)((Rn >> (r + 1)) & 1u);
    const int up = (int)((M >> r) & 1u), un = (int)((Mn >> r) & 1u);
    const int dp = (int)((M >> (r + 2)) & 1u), dn = (int)((Mn >> (r + 2)) & 1u);
    const int hpos = (lp & ~ln) | (rp & ~rn), hneg = ln | rn;
    const int vpos = (up & ~un) | (dp & ~dn), vneg = un | dn;
    const int h = hpos - hneg, v = vpos - vneg;
    const int ctx = h != 0 ? 12 + h * v : (v != 0 ? 10 : 9);
    const int x = (h < 0 || (h == 0 && v < 0)) ? 1 : 0;
    return mq.decode(ctx) ^ x;
}

// Decodes the first `passes` coding passes of a block whose first coded bit-plane is numbps - 1 (passes beyond
// 3 * numbps - 2 do not exist and are not run).  w, h: the block's size; zc: the 256-entry zero-coding table of its
// subband; mag and st must be zero on entry.
JP2K_HD void t1_decode_block(uint32_t* mag, uint16_t* st, uint8_t* cx, const uint32_t* mqtab, const uint8_t* zc, int w, int h,
                             int numbps, int passes, const uint8_t* data, int len)
{
    if (numbps <= 0 || passes <= 0 || w <= 0 || h <= 0) return;
    if (numbps > 31) numbps = 31;
    if (w > 64) w = 64;
    if (h > 64) h = 64;
    for (int k = 0; k < T1_NCTX; ++k) cx[k] = 0;
    cx[T1_CTX_ZC] = 2 * 4;
    cx[T1_CTX_RL] = 2 * 3;
    cx[T1_CTX_UNI] = 2 * 46;
    MqDec mq;
    mq.init(data, len, cx, mqtab);
    const int nstripes = (h + 3) >> 2;
    int done = 0;
    for (int p = numbps - 1; p >= 0 && done < passes; --p) {
        const int first = p == numbps - 1;
        const uint32_t one = 1u << p;
        for (int pass = first ? 2 : 0; pass < 3 && done < passes; ++pass) {
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
                    uint32_t* mp = mag + ((size_t)s * 64 + c) * 4;
                    if (pass == 0) {
                        if (any) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                if (r < rows && !((M >> (r + 1)) & 1u)) {
                                    const int nb = t1_nbr(L, M, R, r);
                                    if (nb) {
                                        pi |= 1u << r;
                                        if (mq.decode(zc[nb])) {
                                            const uint32_t neg = (uint32_t)t1d_sign(mq, L, M, R, Ln, Mn, Rn, r);
                                            M |= 2u << r;
                                            Mn |= neg << (r + 1);
                                            mp[r] = one | (neg << 31);
                                        }
                                    }
                                }
                            }
                            cur[c] = (uint16_t)(((M >> 1) & 15u) | (((Mn >> 1) & 15u) << 4) | (pi << 8) | (mu << 12));
                        }
                    } else if (pass == 1) {
                        const uint32_t todo = ((M >> 1) & 15u) & ~pi;
                        if (todo) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                if ((todo >> r) & 1u) {
                                    const int ctx = ((mu >> r) & 1u) ? 16 : (t1_nbr(L, M, R, r) ? 15 : 14);
                                    if (mq.decode(ctx)) mp[r] |= one;
                                }
                            }
                            mu |= todo;
                            cur[c] = (uint16_t)((f & 0x0FFFu) | (mu << 12));
                        }
                    } else {
                        int r0 = 0;
                        bool coded = true;
                        if (rows == 4 && !any) {   // run-length mode
                            if (!mq.decode(T1_CTX_RL)) coded = false;
                            else {
                                r0 = mq.decode(T1_CTX_UNI) << 1;
                                r0 |= mq.decode(T1_CTX_UNI);
                                const uint32_t neg = (uint32_t)t1d_sign(mq, L, M, R, Ln, Mn, Rn, r0);
                                M |= 2u << r0;
                                Mn |= neg << (r0 + 1);
                                mp[r0] = one | (neg << 31);
                                ++r0;
                            }
                        }
                        if (coded) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                if (r >= r0 && r < rows && !((M >> (r + 1)) & 1u) && !((pi >> r) & 1u)) {
                                    if (mq.decode(zc[t1_nbr(L, M, R, r)])) {
                                        const uint32_t neg = (uint32_t)t1d_sign(mq, L, M, R, Ln, Mn, Rn, r);
                                        M |= 2u << r;
                                        Mn |= neg << (r + 1);
                                        mp[r] = one | (neg << 31);
                                    }
                                }
                            }
                            cur[c] = (uint16_t)(((M >> 1) & 15u) | (((Mn >> 1) & 15u) << 4) | (mu << 12));   // pi cleared for the next plane
                        }
                    }
                    L = M; Ln = Mn;
                    M = R; Mn = Rn;
                }
            }
            ++done;
        }
    }
}

}  // namespace jp2k
