// JPEG 2000 tier-1 DECODER for one code block: the MQ decoder (ITU-T T.800 Annex C.3), the policy that makes t1_walk
// (jp2k_t1.inc, which owns the scan of Annex D, the tables, the flag words and the state layout) a decoder, and
// t1_decode_block.  Included by jp2k_dec.hip and called from k_jp2k_unblocks only.  Every function is JP2K_HD, so a host
// compiler builds the same text and a CPU test judges it against an independent decoder.  The caller provides the state,
// fills the tables (t1_fill_tables) and ZEROES mag and st.
#pragma once
#include "jp2k_t1.inc"

namespace jp2k {

// T.800 C.3: INITDEC, DECODE, BYTEIN, RENORMD.  The bytes are read from in[0 .. len); beyond them the decoder is fed 0xFF,
// as C.3.4 has it for the end of the segment (0xFF 0xFF is a marker, which BYTEIN never steps over), so no position
// beyond `len` is ever read and a truncated or damaged segment decodes to SOME coefficients in bounded time.
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

struct T1Decoder {         // a decision is MQ-decoded and entered into `mag`
    MqDec mq;
    uint32_t* mag;
    uint32_t* mp;

    JP2K_HD void column(int s, int c) { mp = mag + ((size_t)s * 64 + c) * 4; }
    JP2K_HD int bit(int, int, int ctx) { return mq.decode(ctx); }
    JP2K_HD void refine(int r, int p, int ctx)
    {
        if (mq.decode(ctx)) mp[r] |= 1u << p;
    }
    JP2K_HD uint32_t sign(int r, int p, int ctx, int x)
    {
        const uint32_t neg = (uint32_t)(mq.decode(ctx) ^ x);
        mp[r] = (1u << p) | (neg << 31);
        return neg;
    }
    JP2K_HD int run(int)
    {
        if (!mq.decode(T1_CTX_RL)) return -1;
        const int hi = mq.decode(T1_CTX_UNI);
        return hi << 1 | mq.decode(T1_CTX_UNI);
    }
};

// Decodes the first `passes` coding passes of a block whose first coded bit-plane is numbps - 1 (passes beyond
// 3 * numbps - 2 do not exist and are not run).  w, h: the block's size; zc: the 256-entry zero-coding table of its
// subband; mag and st must be zero on entry.
JP2K_HD void t1_decode_block(uint32_t* mag, uint16_t* st, uint8_t* cx, const uint32_t* mqtab, const uint8_t* zc, int w, int h,
                             int numbps, int passes, const uint8_t* data, int len)
{
    if (passes <= 0 || !t1_begin(cx, w, h, numbps)) return;
    T1Decoder io;
    io.mag = io.mp = mag;
    io.mq.init(data, len, cx, mqtab);
    t1_walk(io, st, zc, w, h, numbps, passes);
}

}  // namespace jp2k
