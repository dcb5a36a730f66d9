/*
 * crc_term_kernels.hpp -- CRC-aided early termination of the streaming decoders (ldpc_decoder_config::crc_kind /
 * crc_bits): the one launch a round gains between syndrome_kernel and state_kernel (flood_round.hpp).
 *
 * syndrome_kernel has left the round's fail word of every tile slice: bit l set = frame V*l+v of the tile has an odd
 * parity check.  crc_term_kernel clears the bits of the frames whose first `bits` hard bits leave remainder zero under
 * the decoder's CRC; state_kernel then freezes them exactly as it freezes frames with a clean syndrome, and polling,
 * running[] and the hand-overs follow without knowing of the CRC.  Frames stopped by the CRC alone (their fail bit was
 * set, they were still running) are counted into summary[3].
 *
 * The hard bits are bit-sliced, hard[tile][n][v] = one 64-frame word per column, and the CRC is linear: a frame's
 * remainder is the XOR of the weights w[n] (crc_term_host.hpp) of its set bits.  LANE = FRAME: a wave takes 64 columns
 * at a time -- one coalesced load of their 64 words and one of their 64 weights --, broadcasts word and weight of
 * column k to all lanes (v_readlane: both are wave-uniform from then on) and every lane XORs the weight into its
 * 32-bit accumulator where its own bit of the word is set.  No shift register, no dependence between columns.  The waves
 * of a block take the 64-column chunks round-robin and meet in LDS; one block per (tile, v), so nothing crosses blocks
 * and the result does not depend on any order.
 *
 * Measured at 4096 frames: 166 us per launch for 32400 columns, 286 us for 58320 -- 64 blocks keep
 * 64 of the 256 compute units busy, four waves to a SIMD, eleven instructions per column.  A few microseconds for the few
 * hundred columns of a short block.  The split over several blocks per tile (integer atomicXor into per-round slots and
 * a second small launch) is not built.
 */
#pragma once

#include "flood_common.hpp"

namespace ldpc {

constexpr int kCrcMaxWaves = 16;        /* 1024 threads: the largest workgroup */

struct CrcTermArgs {
    const uint64_t *__restrict__ hard;  /* [T][N][V] */
    uint64_t *__restrict__ fail;        /* [T][V] syndrome of this round: passing frames' bits are cleared */
    const uint64_t *__restrict__ done;  /* [T][V] */
    const uint32_t *__restrict__ w;     /* [bits] weight of every covered column */
    int32_t *__restrict__ stops;        /* [1] += running frames that pass the CRC although their syndrome is not clean */
    int32_t N;
    int32_t bits;                       /* the CRC covers hard bits [0, bits), bits <= N */
    TailRef tail;
};

/* waves of a block: one per 64-column chunk, at most kCrcMaxWaves */
inline int crc_term_waves(int32_t bits)
{
    const int chunks = (bits + 63) / 64;
    return chunks < kCrcMaxWaves ? (chunks > 0 ? chunks : 1) : kCrcMaxWaves;
}

/* column k of a chunk: its word (two halves) and its weight, broadcast from lane k, into this lane's accumulator */
__device__ __forceinline__ uint32_t crc_term_step(uint32_t acc, uint32_t lo, uint32_t hi, uint32_t wt, int k, bool upper, int sh)
{
    const uint32_t l = __builtin_amdgcn_readlane(lo, k), h = __builtin_amdgcn_readlane(hi, k);
    const uint32_t w = __builtin_amdgcn_readlane(wt, k);
    return acc ^ ((0u - (((upper ? h : l) >> sh) & 1u)) & w);
}

/* grid (tiles, V), block 64 * crc_term_waves(bits) */
template <int V> __global__ __launch_bounds__(64 * kCrcMaxWaves) void crc_term_kernel(const CrcTermArgs a)
{
    __shared__ uint32_t part[kCrcMaxWaves][64];
    const int tile = tile_select<V>(a.tail, a.done, (int)blockIdx.x);
    if (tile < 0) return;               /* finished, or not live after a hand-over: the whole block leaves */
    const int v = (int)blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = wave_id_in_block(), waves = (int)(blockDim.x >> 6);
    const uint64_t *h = a.hard + (size_t)tile * (size_t)a.N * V + v;
    const int sh = lane & 31;
    const bool upper = lane >= 32;
    uint32_t acc = 0;
    for (int n0 = wave * 64; n0 < a.bits; n0 += waves * 64) {
        const int m = min(64, a.bits - n0);
        const int mine = n0 + (lane < m ? lane : m - 1);
        const uint64_t word = h[(size_t)mine * V];
        const uint32_t wt = a.w[mine];
        const uint32_t lo = (uint32_t)word, hi = (uint32_t)(word >> 32);
        if (m == 64) {
#pragma unroll
            for (int k = 0; k < 64; ++k) {
                acc = crc_term_step(acc, lo, hi, wt, k, upper, sh);
            }
        } else {
            for (int k = 0; k < m; ++k) {
                acc = crc_term_step(acc, lo, hi, wt, k, upper, sh);
            }
        }
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave != 0) return;
    uint32_t x = 0;
    for (int i = 0; i < waves; ++i) x ^= part[i][lane];
    const uint64_t pass = __ballot(x == 0);
    if (lane == 0) {
        const size_t wi = (size_t)tile * V + v;
        const uint64_t before = a.fail[wi];
        a.fail[wi] = before & ~pass;
        const int n = __popcll(pass & before & ~a.done[wi]);
        if (n) atomicAdd(a.stops, n);
    }
}

}  // namespace ldpc
