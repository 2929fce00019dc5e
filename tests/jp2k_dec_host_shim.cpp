// The decoder's host-compilable text (csrc/jp2k_t1d.inc: the tier-1 decoder; csrc/jp2k_t2d.inc: headers, geometry,
// packet headers, the block table) behind a C ABI, compiled by a host C++ compiler into a temporary directory by
// tests/test_jp2k_dec_host.py, which judges it against oracle/jp2k_oracle.c without a GPU.  TEST INFRASTRUCTURE.
//
// The only product text restated here is what k_jp2k_unblocks (csrc/jp2k_dec.hip) does around the decoder: zeroed
// state, the two tables, and the read-out mag[((y >> 2) * 64 + x) * 4 + (y & 3)] -> signed int32.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "jp2k_t1d.inc"
#include "jp2k_t2d.inc"

extern "C" {

int jp2kd_shim_t1_decode(const uint8_t* data, int len, int w, int h, int orient, int numbps, int passes, int32_t* coef, int stride)
{
    static thread_local uint32_t mag[16 * 64 * 4];
    static thread_local uint16_t st[jp2k::T1_NST * jp2k::T1_STW];
    uint32_t mqtab[jp2k::MQ_ENTRIES];
    uint8_t zc[256], cx[32];
    if (w < 1 || h < 1 || w > 64 || h > 64 || orient < 0 || orient > 3 || len < 0) return -1;
    memset(mag, 0, sizeof mag);
    memset(st, 0, sizeof st);
    jp2k::t1_fill_tables(mqtab, zc, orient, 0, 1);
    jp2k::t1_decode_block(mag, st, cx, mqtab, zc, w, h, numbps, passes, data, len);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const uint32_t m = mag[((y >> 2) * 64 + x) * 4 + (y & 3)];
            const int32_t v = (int32_t)(m & 0x7FFFFFFFu);
            coef[(size_t)y * stride + x] = (m >> 31) ? -v : v;
        }
    return 0;
}

// rec: three values per block (passes, numbps, bytes).  Returns the header's length, -1 for a header beyond `n`.
int64_t jp2kd_shim_packet_header(int nbands, const int32_t* gw, const int32_t* gh, const int32_t* mb, const uint8_t* in, size_t n,
                                 int32_t* rec)
{
    return jp2k::dec_packet_header(in, n, nbands, gw, gh, mb, rec);
}

static int copy_message(const jp2k::DecError& e, char* msg, size_t cap)
{
    if (msg && cap) snprintf(msg, cap, "%s", e.msg);
    return e.code;
}

// {C, H, W, bits, tiles, blocks, resolutions, tile width, tile height}; 0, or DEC_BAD / DEC_UNSUPPORTED and a message
int jp2kd_shim_info(const uint8_t* f, size_t n, int64_t out[9], char* msg, size_t cap)
{
    jp2k::DecStream s;
    jp2k::DecError e = {0, ""};
    if (jp2k::dec_read_headers(f, n, &s, &e)) return copy_message(e, msg, cap);
    const int64_t nb = jp2k::dec_count_blocks(s.p, &e);
    if (nb < 0) return copy_message(e, msg, cap);
    out[0] = s.p.C; out[1] = s.p.H; out[2] = s.p.W; out[3] = s.p.bits; out[4] = (int64_t)s.p.ntx * s.p.nty;
    out[5] = nb; out[6] = s.p.NL + 1; out[7] = s.p.XT; out[8] = s.p.YT;
    return 0;
}

// The block table, sixteen int64 per block in the order of oracle/jp2k.py FIELDS.  Returns the number of blocks (the first
// `cap` are written), or a negative code and a message.
int64_t jp2kd_shim_parse(const uint8_t* f, size_t n, int64_t* rec, int64_t cap, char* msg, size_t msgcap)
{
    jp2k::DecStream s;
    jp2k::DecError e = {0, ""};
    std::vector<jp2k::DecBlock> t;
    if (jp2k::dec_read_headers(f, n, &s, &e) || jp2k::dec_parse(f, n, s, &t, &e)) return copy_message(e, msg, msgcap);
    for (size_t k = 0; k < t.size() && (int64_t)k < cap; ++k) {
        const jp2k::DecBlock& b = t[k];
        int64_t* q = rec + 16 * k;
        q[0] = b.tile; q[1] = b.comp; q[2] = b.res; q[3] = b.band; q[4] = b.gx; q[5] = b.gy; q[6] = b.numbps; q[7] = b.passes;
        q[8] = b.offset; q[9] = b.length; q[10] = b.mb; q[11] = b.x; q[12] = b.y; q[13] = b.w; q[14] = b.h; q[15] = b.orient;
    }
    return (int64_t)t.size();
}

}  // extern "C"
