// JPEG 2000 on the host side of liblbdrn_hip's encoder: the geometry (tiles, resolutions, subbands, code blocks) and
// everything that is not tier-1 -- packet headers (T.800 Annex B.10: tag trees, pass counts, Lblock), tile-parts, the
// main header (Annex A) and the JP2 boxes (Annex I).  Plain C++ without any HIP, included by jp2k.hip.
//
// The coding parameters are those csrc/jp2_shim.c asks OpenJPEG for (what GDAL's JP2OpenJPEG driver does for
// QUALITY=100 REVERSIBLE=YES): unsigned components of 8 or 16 bits, tiles of 1024 x 1024 when the raster is larger than
// that, LRCP, one layer, no component transform, 64 x 64 code blocks of style 0, reversible 5/3 with up to five
// decompositions, default precincts (one per resolution), no quantisation, two guard bits.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

namespace jp2k {

constexpr int TILE = 1024, CBLK = 64, GUARD = 2, MAX_RES = 6;
constexpr int MAX_SIDE = 32768;   // beyond it a resolution has more than one default precinct

constexpr int ceil_shift(int a, int k) { return (int)(((int64_t)a + (1 << k) - 1) >> k); }
// whole-sample symmetric extension of a line of n >= 2 samples: the sample that index j in -2 .. n + 1 stands for
constexpr int mirror(int j, int n)
{
    if (j < 0) j = -j;
    if (j > n - 1) j = 2 * (n - 1) - j;
    return j < 0 ? -j : j;
}

struct Band {
    int orient;        // 0 LL, 1 HL, 2 LH, 3 HH
    int x, y, w, h;    // where it lies in the transformed tile-component (Mallat layout), and its size
    int bx0, by0;      // its origin in subband coordinates (the code-block grid is anchored at 0 there)
    int gw, gh;        // code blocks across and down
    int mb;            // magnitude bit-planes the quantisation step announces: guard + exponent - 1
    int64_t first;     // index of its first block in the block table
};
struct Packet {        // one resolution of one tile-component
    int nbands;
    Band band[3];
};
struct Block {         // what the device needs of a code block (32 bytes)
    uint64_t slot;     // offset of its slot in the staging buffer
    uint32_t cap;      // bytes of its slot
    uint32_t slab;     // tile-component index: the coefficients start at slab * (tile width * tile height)
    uint16_t x, y, w, h;
    uint8_t orient, mb, pad0, pad1;
    uint32_t pad2;
};
static_assert(sizeof(Block) == 32, "Block is copied to the device as it is");
struct BlockOut {      // what comes back (16 bytes)
    uint32_t bytes, passes, numbps, pad;
};

struct Geometry {
    int C, H, W, bits, R;
    int tw, th;        // nominal tile size (the raster itself when it is not tiled)
    int ntx, nty;
    int64_t nblocks;
    uint64_t staging;  // sum of the slots
    std::vector<Packet> packets;   // [tile][resolution][component] -- the order LRCP writes them in
    std::vector<Block> blocks;     // in packet order, band by band, raster order inside a band
};

inline int num_resolutions(int H, int W)
{
    const int m = H < W ? H : W;
    int r = 1;
    while ((m >> r) > 0 && r < MAX_RES) ++r;
    return r;
}
// bytes that hold any block of w x h coefficients with mb magnitude planes: every sample costs at most one magnitude
// decision per plane and one sign; the adaptive coder's worst sustained cost measured on incompressible planes is 1.07
// bits per decision, the slot allows 2 (a block that still outgrows it is reported, never written past its slot)
inline uint32_t block_slot(int w, int h, int mb) { return (uint32_t)(((int64_t)w * h * (mb + 2) + 3) / 4 + 64); }

// Builds the packet list; the block table too when `with_blocks`.  The tile origins are multiples of 1024 and there are at
// most five decompositions, so every resolution of every tile starts at an even coordinate (the low-pass sample comes
// first in every lifting step) and a 64-aligned cell of the subband grid is never cut by a tile's edge from the left.
inline bool make_geometry(int C, int H, int W, int bits, bool with_blocks, Geometry* g)
{
    if (C < 1 || C > 16384 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE || (bits != 8 && bits != 16)) return false;
    g->C = C; g->H = H; g->W = W; g->bits = bits;
    g->R = num_resolutions(H, W);
    const bool tiled = H > TILE || W > TILE;
    g->tw = tiled ? TILE : W;
    g->th = tiled ? TILE : H;
    g->ntx = (W + g->tw - 1) / g->tw;
    g->nty = (H + g->th - 1) / g->th;
    g->nblocks = 0;
    g->staging = 0;
    g->packets.clear();
    g->blocks.clear();
    const int R = g->R;
    for (int ty = 0; ty < g->nty; ++ty)
        for (int tx = 0; tx < g->ntx; ++tx) {
            const int x0 = tx * g->tw, y0 = ty * g->th;
            const int x1 = x0 + g->tw < W ? x0 + g->tw : W, y1 = y0 + g->th < H ? y0 + g->th : H;
            const int w = x1 - x0, h = y1 - y0;
            for (int r = 0; r < R; ++r)
                for (int c = 0; c < C; ++c) {
                    Packet pk;
                    pk.nbands = r == 0 ? 1 : 3;
                    const int nb = r == 0 ? R - 1 : R - r;   // decomposition level of the bands
                    const int rw = ceil_shift(w, R - 1 - r), rh = ceil_shift(h, R - 1 - r);   // this resolution
                    const int lw = (rw + 1) >> 1, lh = (rh + 1) >> 1;                           // the one below
                    for (int b = 0; b < pk.nbands; ++b) {
                        Band& bd = pk.band[b];
                        bd.orient = r == 0 ? 0 : b + 1;
                        const int xo = bd.orient & 1, yo = bd.orient >> 1;
                        if (r == 0) { bd.x = 0; bd.y = 0; bd.w = rw; bd.h = rh; }
                        else {
                            bd.x = xo ? lw : 0; bd.y = yo ? lh : 0;
                            bd.w = xo ? rw - lw : lw; bd.h = yo ? rh - lh : lh;
                        }
                        bd.bx0 = x0 >> nb;   // = ceil((x0 - xo * 2^(nb-1)) / 2^nb) for x0 a multiple of 2^nb
                        bd.by0 = y0 >> nb;
                        const bool empty = bd.w <= 0 || bd.h <= 0;
                        bd.gw = empty ? 0 : (bd.bx0 + bd.w + CBLK - 1) / CBLK - bd.bx0 / CBLK;
                        bd.gh = empty ? 0 : (bd.by0 + bd.h + CBLK - 1) / CBLK - bd.by0 / CBLK;
                        const int gain = (bd.orient == 0) ? 0 : (bd.orient == 3 ? 2 : 1);
                        bd.mb = GUARD + bits + gain - 1;
                        bd.first = g->nblocks;
                        g->nblocks += (int64_t)bd.gw * bd.gh;
                        if (!with_blocks) continue;
                        for (int gy = 0; gy < bd.gh; ++gy)
                            for (int gx = 0; gx < bd.gw; ++gx) {
                                // the cell of the anchored grid, clipped to the band, in band-local coordinates
                                const int cx0 = (bd.bx0 / CBLK + gx) * CBLK - bd.bx0, cy0 = (bd.by0 / CBLK + gy) * CBLK - bd.by0;
                                const int ax0 = cx0 < 0 ? 0 : cx0, ay0 = cy0 < 0 ? 0 : cy0;
                                const int ax1 = cx0 + CBLK < bd.w ? cx0 + CBLK : bd.w, ay1 = cy0 + CBLK < bd.h ? cy0 + CBLK : bd.h;
                                Block bl;
                                memset(&bl, 0, sizeof bl);
                                bl.slab = (uint32_t)((ty * g->ntx + tx) * C + c);
                                bl.x = (uint16_t)(bd.x + ax0); bl.y = (uint16_t)(bd.y + ay0);
                                bl.w = (uint16_t)(ax1 - ax0); bl.h = (uint16_t)(ay1 - ay0);
                                bl.orient = (uint8_t)bd.orient;
                                bl.mb = (uint8_t)bd.mb;
                                bl.cap = block_slot(bl.w, bl.h, bd.mb);
                                bl.slot = g->staging;
                                g->staging += bl.cap;
                                g->blocks.push_back(bl);
                            }
                    }
                    g->packets.push_back(pk);
                }
        }
    return true;
}

// ------------------------------------------------------------------ bytes

struct Writer {        // bounded: counts what it is given, writes what fits
    uint8_t* p;
    size_t cap, n;
    void u8(unsigned v) { if (n < cap) p[n] = (uint8_t)v; ++n; }
    void u16(unsigned v) { u8(v >> 8); u8(v); }
    void u32(uint32_t v) { u16(v >> 16); u16(v & 0xFFFFu); }
    void tag(const char* t) { for (int k = 0; k < 4; ++k) u8((unsigned char)t[k]); }
    void patch32(size_t at, uint32_t v) { for (int k = 0; k < 4; ++k) if (at + k < cap) p[at + k] = (uint8_t)(v >> (24 - 8 * k)); }
};

struct BitWriter {     // packet-header bits: after a byte of 0xFF the next byte carries seven
    Writer* w;
    unsigned acc;
    int nbits, room;
    unsigned last;
    void begin(Writer* w_) { w = w_; acc = 0; nbits = 0; room = 8; last = 0; }
    void put(unsigned bit)
    {
        acc = (acc << 1) | (bit & 1u);
        if (++nbits == room) out();
    }
    void out()
    {
        last = acc & 0xFFu;
        w->u8(last);
        acc = 0; nbits = 0;
        room = last == 0xFF ? 7 : 8;
    }
    void bits(uint32_t v, int n) { for (int k = n - 1; k >= 0; --k) put((v >> k) & 1u); }
    void end()
    {
        if (nbits) { acc <<= (room - nbits); nbits = room; out(); }
        if (last == 0xFF) w->u8(0);
    }
};

struct TagTree {       // T.800 B.10.2
    struct Node { int parent, value, low, known; };
    std::vector<Node> nodes;
    void build(int w, int h, const int* leaves)
    {
        nodes.clear();
        std::vector<int> lw, lh, first;
        int cw = w, ch = h, total = 0;
        for (;;) {
            lw.push_back(cw); lh.push_back(ch); first.push_back(total);
            total += cw * ch;
            if (cw * ch <= 1) break;
            cw = (cw + 1) / 2; ch = (ch + 1) / 2;
        }
        nodes.assign((size_t)total, Node{-1, 0x7FFFFFFF, 0, 0});
        for (int k = 0; k < w * h; ++k) nodes[(size_t)k].value = leaves[k];
        for (size_t l = 0; l + 1 < lw.size(); ++l)
            for (int y = 0; y < lh[l]; ++y)
                for (int x = 0; x < lw[l]; ++x) {
                    const int me = first[l] + y * lw[l] + x, up = first[l + 1] + (y / 2) * lw[l + 1] + x / 2;
                    nodes[(size_t)me].parent = up;
                    if (nodes[(size_t)me].value < nodes[(size_t)up].value) nodes[(size_t)up].value = nodes[(size_t)me].value;
                }
    }
    void encode(BitWriter& bw, int leaf, int threshold)
    {
        int stack[32], sp = 0, node = leaf;
        while (nodes[(size_t)node].parent >= 0 && sp < 32) { stack[sp++] = node; node = nodes[(size_t)node].parent; }
        int low = 0;
        for (;;) {
            Node& nd = nodes[(size_t)node];
            if (low > nd.low) nd.low = low; else low = nd.low;
            while (low < threshold) {
                if (low >= nd.value) {
                    if (!nd.known) { bw.put(1); nd.known = 1; }
                    break;
                }
                bw.put(0);
                ++low;
            }
            nd.low = low;
            if (!sp) break;
            node = stack[--sp];
        }
    }
};

inline int floor_log2(uint32_t v) { int n = 0; while (v > 1) { v >>= 1; ++n; } return n; }

inline void put_passes(BitWriter& bw, int n)   // T.800 Table B.4
{
    if (n == 1) bw.put(0);
    else if (n == 2) bw.bits(2, 2);
    else if (n <= 5) bw.bits(0xC | (uint32_t)(n - 3), 4);
    else if (n <= 36) bw.bits(0x1E0 | (uint32_t)(n - 6), 9);
    else bw.bits(0xFF80 | (uint32_t)(n - 37), 16);
}

// One packet's header.  res: the records of the block table; the packet's blocks are bd.first .. of each band.
inline void put_packet_header(Writer& w, const Packet& pk, const BlockOut* res)
{
    BitWriter bw;
    bw.begin(&w);
    bool any = false;
    for (int b = 0; b < pk.nbands; ++b) {
        const Band& bd = pk.band[b];
        for (int64_t k = 0; k < (int64_t)bd.gw * bd.gh; ++k) any = any || res[bd.first + k].passes > 0;
    }
    if (!any) {       // an empty packet
        bw.put(0);
        bw.end();
        return;
    }
    bw.put(1);
    std::vector<int> incl, zbp;
    TagTree ti, tz;
    for (int b = 0; b < pk.nbands; ++b) {
        const Band& bd = pk.band[b];
        const int n = bd.gw * bd.gh;
        if (!n) continue;
        incl.resize((size_t)n); zbp.resize((size_t)n);
        for (int k = 0; k < n; ++k) {
            const BlockOut& o = res[bd.first + k];
            incl[(size_t)k] = o.passes ? 0 : 1;            // the layer it is first included in (there is one)
            zbp[(size_t)k] = bd.mb - (int)o.numbps;        // missing most significant planes
        }
        ti.build(bd.gw, bd.gh, incl.data());
        tz.build(bd.gw, bd.gh, zbp.data());
        for (int k = 0; k < n; ++k) {
            const BlockOut& o = res[bd.first + k];
            ti.encode(bw, k, 1);
            if (!o.passes) continue;
            tz.encode(bw, k, 0x7FFFFFF0);
            put_passes(bw, (int)o.passes);
            const int base = 3 + floor_log2(o.passes);      // Lblock starts at 3
            const int need = floor_log2(o.bytes ? o.bytes : 1) + 1;
            const int inc = need > base ? need - base : 0;
            for (int i = 0; i < inc; ++i) bw.put(1);
            bw.put(0);
            bw.bits(o.bytes, base + inc);
        }
    }
    bw.end();
}

inline size_t main_header_bytes(const Geometry& g) { return 85 + 2 + (40 + 3 * (size_t)g.C) + 14 + (5 + 1 + 3 * (size_t)(g.R - 1)); }

// signature box .. QCD; returns the offset of the jp2c box's length field
inline size_t put_main_header(Writer& w, const Geometry& g)
{
    static const uint8_t sig[12] = {0, 0, 0, 12, 'j', 'P', ' ', ' ', 13, 10, 0x87, 10};
    for (int k = 0; k < 12; ++k) w.u8(sig[k]);
    w.u32(20); w.tag("ftyp"); w.tag("jp2 "); w.u32(0); w.tag("jp2 ");
    w.u32(8 + 22 + 15); w.tag("jp2h");
    w.u32(22); w.tag("ihdr"); w.u32((uint32_t)g.H); w.u32((uint32_t)g.W); w.u16((unsigned)g.C);
    w.u8((unsigned)g.bits - 1); w.u8(7); w.u8(0); w.u8(0);
    w.u32(15); w.tag("colr"); w.u8(1); w.u8(0); w.u8(0); w.u32(g.C == 3 ? 16u : (g.C == 1 ? 17u : 0u));
    const size_t at = w.n;
    w.u32(0); w.tag("jp2c");
    w.u16(0xFF4F);
    w.u16(0xFF51); w.u16(38 + 3 * (unsigned)g.C); w.u16(0);
    w.u32((uint32_t)g.W); w.u32((uint32_t)g.H); w.u32(0); w.u32(0);
    w.u32((uint32_t)g.tw); w.u32((uint32_t)g.th); w.u32(0); w.u32(0);
    w.u16((unsigned)g.C);
    for (int c = 0; c < g.C; ++c) { w.u8((unsigned)g.bits - 1); w.u8(1); w.u8(1); }
    w.u16(0xFF52); w.u16(12); w.u8(0); w.u8(0); w.u16(1); w.u8(0);
    w.u8((unsigned)g.R - 1); w.u8(4); w.u8(4); w.u8(0); w.u8(1);
    w.u16(0xFF5C); w.u16(4 + 3 * (unsigned)(g.R - 1)); w.u8(GUARD << 5);
    w.u8((unsigned)g.bits << 3);
    for (int r = 1; r < g.R; ++r) { w.u8((unsigned)(g.bits + 1) << 3); w.u8((unsigned)(g.bits + 1) << 3); w.u8((unsigned)(g.bits + 2) << 3); }
    return at;
}

// a bound on everything but the block bytes: headers, and per packet one bit plus per block the tag-tree bits (at most
// two trees of depth 5 and a value below 32), 16 bits of pass count, up to 24 of Lblock and 32 of length, stuffing included
inline size_t overhead_bound(const Geometry& g)
{
    return main_header_bytes(g) + 2 + (size_t)g.ntx * g.nty * 14 + g.packets.size() * 4 + (size_t)g.nblocks * 24;
}

// Assembles the file.  data: the block bytes packed back to back in block-table order (total bytes).  Returns the file's
// length; nothing is written beyond `cap` (the caller compares the two).
inline size_t assemble(const Geometry& g, const BlockOut* res, const uint8_t* data, uint64_t total, uint8_t* out, size_t cap)
{
    Writer w = {out, cap, 0};
    const size_t jp2c = put_main_header(w, g);
    const size_t per_tile = (size_t)g.R * g.C;
    uint64_t off = 0;
    for (int t = 0; t < g.ntx * g.nty; ++t) {
        const size_t sot = w.n;
        w.u16(0xFF90); w.u16(10); w.u16((unsigned)t); w.u32(0); w.u8(0); w.u8(1);
        w.u16(0xFF93);
        for (size_t k = 0; k < per_tile; ++k) {
            const Packet& pk = g.packets[(size_t)t * per_tile + k];
            put_packet_header(w, pk, res);
            for (int b = 0; b < pk.nbands; ++b) {
                const Band& bd = pk.band[b];
                for (int64_t i = 0; i < (int64_t)bd.gw * bd.gh; ++i) {
                    const uint32_t n = res[bd.first + i].bytes;
                    if (!res[bd.first + i].passes) continue;
                    if (w.n + n <= w.cap && off + n <= total) memmove(w.p + w.n, data + off, n);   // (data may be the tail of out)
                    w.n += n;
                    off += n;
                }
            }
        }
        w.patch32(sot + 6, (uint32_t)(w.n - sot));
    }
    w.u16(0xFFD9);
    w.patch32(jp2c, (uint32_t)(w.n - jp2c));
    return w.n;
}

}  // namespace jp2k
