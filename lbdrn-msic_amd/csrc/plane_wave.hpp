// What one 64-lane wave does around the lane coder (plane_lane.inc), the same in LBB2's kernels (plane_codec.hip) and LBB3's
// (plane3.hip): a lane's private bit stream, the 4 KB tile of a pass's symbol lengths, the encoder's replay of the
// decoder's word requests and the decoder's hand-out of a strip's or unit's words, a ballot + mbcnt per anti-diagonal
// step.  Device only.  Where a lane's coder state lives between passes, how many pixel windows there are and how the
// mode words are laid out is each kernel's own.
#pragma once
#include <hip/hip_runtime.h>

#include "plane_lane.inc"

namespace lbdrn {

constexpr int PW_T = plane_lane::T;

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int lanes_below(unsigned long long mask)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// A lane's private stream (encoder, phase A): whole 32-bit words go to priv as they fill, the rest with the tail.
struct BitWriter {
    unsigned long long acc = 0;
    int nb = 0;
    size_t pwords = 0;
    __device__ __forceinline__ void put(uint32_t* priv, uint32_t code, int len)
    {
        if (len) {
            acc = (acc << len) | code;
            nb += len;
            if (nb >= 32) {
                priv[pwords++] = (uint32_t)(acc >> (nb - 32));
                nb -= 32;
            }
        }
    }
    __device__ __forceinline__ void tail(uint32_t* priv) { priv[pwords++] = nb ? (uint32_t)(acc << (32 - nb)) : 0u; }  // zero padded
};

// the symbol lengths of one band of one pass, 64 x 64 bytes, between LDS and the workspace: coalesced, the whole wave
__device__ __forceinline__ void copy_lens_tile(uint8_t* dst, const uint8_t* src, int lane)
{
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (int idx = lane; idx < PW_T * PW_T / 4; idx += PW_T) d[idx] = s[idx];
}

// The encoder's phase B: the words of the lanes' private streams in the order the decoding wave asks for them.
struct Replay {
    uint32_t nw;        // words of wout written so far (the kernel writes head and mode words itself and counts them here)
    int fill = 0;       // bits the decoding lane would hold
    size_t taken = 0;   // words of the lane's private stream handed out
    // one band of one pass: glens its recorded symbol lengths, priv[0 .. pwords) the lane's private stream
    __device__ __forceinline__ void band(const uint8_t* glens, const uint32_t* priv, size_t pwords, int rows, int tw, int lane,
                                         uint8_t (*lensw)[PW_T], uint32_t (*pwin)[PW_T + 1], uint32_t* wout)
    {
        __syncthreads();
        copy_lens_tile(&lensw[0][0], glens, lane);
        const size_t taken0 = taken;
        for (int u = 0; u <= PW_T; ++u) pwin[lane][u] = taken0 + u < pwords ? priv[taken0 + u] : 0u;   // a symbol takes a word at the most
        __syncthreads();
        for (int d = 0; d < rows + tw - 1; ++d) {
            const int j = d - lane;
            const bool active = lane < rows && j >= 0 && j < tw;
            const bool need = active && fill < 32;
            const unsigned long long mask = __ballot(need);
            if (need) {
                wout[nw + lanes_below(mask)] = pwin[lane][taken - taken0];
                taken += 1;
                fill += 32;
            }
            nw += (uint32_t)__popcll(mask);
            if (active) fill -= lensw[lane][j];
        }
    }
};

// The decoder's hand-out of the words ws[0 .. nws) of a strip or unit: a lane's bit buffer and the wave's position.
struct WordReader {
    unsigned long long buf = 0;
    int nb = 0;
    uint32_t cur, cur0;     // the next word, and the first one of the staged window
    // the next `size` words into wwin, zeros beyond nws; the caller puts a barrier before and behind
    __device__ __forceinline__ void stage(uint32_t* wwin, uint32_t size, const uint32_t* ws, uint32_t nws, int lane)
    {
        cur0 = cur;
        for (uint32_t idx = lane; idx < size; idx += PW_T) wwin[idx] = (uint64_t)cur0 + idx < nws ? ws[cur0 + idx] : 0u;
    }
    // One step: the active lanes short of 32 bits take the next words in lane order.  False where a lane asks beyond nws.
    __device__ __forceinline__ bool refill(bool active, const uint32_t* wwin, uint32_t size, uint32_t nws)
    {
        bool ok = true;
        const bool need = active && nb < 32;
        const unsigned long long mask = __ballot(need);
        if (need) {
            const uint32_t idx = cur + (uint32_t)lanes_below(mask);
            if (idx >= nws) ok = false;
            buf |= (unsigned long long)wwin[min(idx - cur0, size - 1)] << (32 - nb);
            nb += 32;
        }
        cur += (uint32_t)__popcll(mask);
        return ok;
    }
    __device__ __forceinline__ uint32_t top() const { return (uint32_t)(buf >> 32); }
    __device__ __forceinline__ void drop(int len) { buf <<= len; nb -= len; }
};

}  // namespace lbdrn
