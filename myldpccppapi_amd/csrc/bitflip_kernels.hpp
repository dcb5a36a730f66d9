/*
 * bitflip_kernels.hpp -- LDPC_ALGO_BITFLIP (include/ldpc_hip.h): hard-decision parallel bit flipping on bit-sliced frames.
 *
 * The whole state is bits.  Frames go in the bits of 64-bit words, one word per column and 64 frames (the layout of the
 * streaming decoders' hard bits at one frame per lane, hard[tile][n], which pack_kernel, crc_term_kernel and the debug
 * tap read as they are):
 *     x[tile][n]   the decoder's bits (ldpc_decoder::hard)       r[tile][n]   the received bits, kept
 *     s[tile][m]   the syndrome words of the round               fail[round][tile] = OR of s over m, done[tile]
 * so a tile of 64 frames is 8 (2 N + M) bytes of state and a round moves a few bits per edge and frame where the cheapest
 * soft decoder moves 6 bytes.
 *
 *   bitflip_init_kernel    y (float, fp16 or int8 rows; padding frames read 1) -> r = x = ballot(y < 0): the transpose of
 *                          the streaming init kernels, one ballot per 64 frames and column
 *   bitflip_check_kernel   one work-item per (tile, row): s = XOR of x over the row; the wave, then the block, OR their
 *                          words into the tile's fail word (syndrome_kernel's reduction)
 *   bitflip_state_kernel   frames whose fail bit is clear are done: done |= ~fail, iters = round - 1
 *   bitflip_vote_kernel    one work-item per (tile, column): the d syndrome words of the column and the word x ^ r are
 *                          counted into six bit planes (E <= 63: column degrees up to 62) with full adders -- three words
 *                          become a sum and a carry word, which ripple into the planes from bit 0 and bit 1 --, the planes
 *                          are compared with a constant bit by bit from the top, and the tile learns, per frame, whether
 *                          a column reaches T(d, round) and how large the largest E is (64 words: any[tile][.]).  T comes
 *                          from the degree and one launch argument (off): uniform integer work.
 *   bitflip_flip_kernel    the same count again (the syndrome words are in cache), the flip mask of the rule, without the
 *                          done frames, XORed into x.
 * A round is check -> (crc_term_kernel) -> state -> vote -> flip: small launches, every word of x and s written once.
 * Finished tiles leave at entry with early termination; without it they run and their frames stay frozen all the same.
 *
 * Every index is bounded by its launch: rows m < M, columns n < N, tiles < the tiles of the call (<= T of max_batch).
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "flood_round.hpp"
#include "crc_term_kernels.hpp"
#include "hip_host.hpp"
#include "llr_input.hpp"
#include "engines.hpp"

namespace ldpc {

constexpr int kBitflipMaxDegree = 62;       /* E = u + (x != r) <= 63: six bit planes */
constexpr int kBitflipThresholds = 16;      /* ldpc_decoder_config::bf_threshold */

/* off(i) of round i >= 1 (include/ldpc_hip.h): i - 1, or the caller's table */
inline int bitflip_offset(const int32_t *bf_threshold, int round)
{
    bool any = false;
    for (int j = 0; j < kBitflipThresholds; ++j) any = any || bf_threshold[j] != 0;
    if (!any) return round - 1;
    return bf_threshold[round - 1 < kBitflipThresholds ? round - 1 : kBitflipThresholds - 1];
}

/* The kernels are plain functions, not templates: only the translation unit that defines LDPC_ENGINE_BITFLIP
 * (engine_bitflip.hip) compiles them and the driver below; the other units see the plan and the run block. */
#ifdef LDPC_ENGINE_BITFLIP
struct BitflipInitArgs {
    const void *__restrict__ llr;       /* [frames][N], elements of the kernel's IN */
    uint64_t *__restrict__ x;           /* [T][N] */
    uint64_t *__restrict__ r;           /* [T][N] */
    int64_t frames;
    int32_t N;
    float llr_unit;
};

/* grid (ceil(N / kInitCols), tiles), block kBlock */
template <typename IN> __global__ __launch_bounds__(kBlock) void bitflip_init_kernel(const BitflipInitArgs a)
{
    constexpr int F = 64, LD = F + 1;
    __shared__ float patch[kInitCols * LD];
    const int tile = blockIdx.y;
    const int n0 = blockIdx.x * kInitCols;
    const IN *__restrict__ llr = static_cast<const IN *>(a.llr);
    if constexpr (!std::is_same<IN, float>::value) {
        llr_patch_fill<IN, F, LD, kInitCols, kBlock, false>(patch, llr, a.llr_unit, a.frames, a.N, tile, n0, 1.0f);
    } else {
        const int c = threadIdx.x & (kInitCols - 1);
        const int n = n0 + c;
        for (int f = threadIdx.x / kInitCols; f < F; f += kBlock / kInitCols) {
            const int64_t frame = (int64_t)tile * F + f;
            float y = 1.0f;
            if (frame < a.frames && n < a.N) y = llr[(size_t)frame * a.N + n];
            patch[c * LD + f] = y;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int c = threadIdx.x >> 6; c < kInitCols; c += kWavesPerBlock) {
        const int n = n0 + c;
        if (n >= a.N) break;
        const uint64_t w = __ballot(patch[c * LD + lane] < 0.0f);       /* NaN and -0 read 0 */
        if (lane == 0) {
            a.x[(size_t)tile * a.N + n] = w;
            a.r[(size_t)tile * a.N + n] = w;
        }
    }
}

struct BitflipCheckArgs {
    const int32_t *__restrict__ row_ptr;    /* [M + 1] */
    const int32_t *__restrict__ edge_col;   /* [E] */
    const uint64_t *__restrict__ x;         /* [T][N] */
    uint64_t *__restrict__ s;               /* [T][M] */
    uint64_t *__restrict__ fail;            /* [T], zeroed before the decode */
    const uint64_t *__restrict__ done;      /* [T] */
    int32_t M, N;
    int32_t skip_done;                      /* early_term */
};

/* grid (ceil(M / kBlock), tiles), block kBlock */
__global__ __launch_bounds__(kBlock) void bitflip_check_kernel(const BitflipCheckArgs a)
{
    const int tile = blockIdx.y;
    if (a.skip_done && tile_finished<1>(a.done, tile)) return;
    const int m = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    const uint64_t *xt = a.x + (size_t)tile * (size_t)a.N;
    uint64_t s = 0;
    if (m < a.M) {
        for (int p = a.row_ptr[m]; p < a.row_ptr[m + 1]; ++p) s ^= xt[a.edge_col[p]];
        a.s[(size_t)tile * (size_t)a.M + m] = s;
    }
    __shared__ uint64_t part[kWavesPerBlock];
    uint64_t o = s;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)o, off);
        const uint32_t hi = __shfl_xor((uint32_t)(o >> 32), off);
        o |= ((uint64_t)hi << 32) | lo;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = o;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t all = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) all |= part[w];
        if (all) atomicOr(reinterpret_cast<unsigned long long *>(&a.fail[tile]), (unsigned long long)all);
    }
}

/* round i: a frame whose fail bit is clear is done with iters = i - 1 (state_kernel of flood_round.hpp counts a round
 * later and starts at 1); it also clears the tile's vote words.  grid tiles, block 64 */
__global__ void bitflip_state_kernel(uint64_t *__restrict__ done, const uint64_t *__restrict__ fail, int32_t *__restrict__ iters,
                                     uint64_t *__restrict__ any, int32_t round)
{
    const int tile = blockIdx.x, lane = threadIdx.x;
    any[(size_t)tile * 64 + lane] = 0;          /* the round's votes (bitflip_vote_kernel) */
    const uint64_t old = done[tile];
    const uint64_t newly = ~fail[tile] & ~old;
    if ((newly >> lane) & 1ull) iters[(size_t)tile * 64 + lane] = round - 1;
    if (lane == 0 && newly) done[tile] = old | newly;
}

struct BitflipVarArgs {
    const int32_t *__restrict__ col_ptr;    /* [N + 1] */
    const int32_t *__restrict__ col_row;    /* [E] rows of every column, ascending */
    uint64_t *__restrict__ x;               /* [T][N] */
    const uint64_t *__restrict__ r;         /* [T][N] */
    const uint64_t *__restrict__ s;         /* [T][M] */
    const uint64_t *__restrict__ done;      /* [T] as bitflip_state_kernel left it for this round */
    uint64_t *__restrict__ any;             /* [T][64] votes of the round (kBitflipVoteHit, 2 .. 63), zeroed by bitflip_state_kernel */
    int32_t M, N;
    int32_t off;                            /* T(d) = max((d + 1) / 2 + 1, d + 1 - off) */
    int32_t skip_done;
};

/* planes += w at bit `from`: a ripple of half adders */
__device__ __forceinline__ void bitflip_add(uint64_t (&p)[6], uint64_t w, int from)
{
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (k < from) continue;
        const uint64_t c = p[k] & w;
        p[k] ^= w;
        w = c;
    }
}

/* E_n = u_n + (x_n != r_n) of column n in six bit planes; returns the column's degree */
__device__ __forceinline__ int bitflip_count(const BitflipVarArgs &a, int tile, int n, uint64_t x, uint64_t (&p)[6])
{
    const uint64_t *st = a.s + (size_t)tile * (size_t)a.M;
    const int p0 = a.col_ptr[n], p1 = a.col_ptr[n + 1];
    p[0] = x ^ a.r[(size_t)tile * (size_t)a.N + n];
#pragma unroll
    for (int b = 1; b < 6; ++b) p[b] = 0;
    int k = p0;
    for (; k + 3 <= p1; k += 3) {           /* a full adder: three words of weight 1 -> one of weight 1, one of weight 2 */
        const uint64_t u = st[a.col_row[k]], v = st[a.col_row[k + 1]], w = st[a.col_row[k + 2]];
        bitflip_add(p, u ^ v ^ w, 0);
        bitflip_add(p, (u & v) | (w & (u ^ v)), 1);
    }
    for (; k < p1; ++k) bitflip_add(p, st[a.col_row[k]], 0);
    return p1 - p0;
}

/* the frames with E >= t, 0 <= t <= 63: bit-serially from the top plane */
__device__ __forceinline__ uint64_t bitflip_ge(const uint64_t (&p)[6], int t)
{
    uint64_t gt = 0, eq = ~0ull;
#pragma unroll
    for (int b = 5; b >= 0; --b) {
        const uint64_t tb = ((t >> b) & 1) ? ~0ull : 0ull;
        gt |= eq & p[b] & ~tb;
        eq &= ~(p[b] ^ tb);
    }
    return gt | eq;
}

__device__ __forceinline__ int bitflip_threshold(int d, int off) { return max((d + 1) / 2 + 1, d + 1 - off); }

constexpr int kBitflipVoteHit = 0;          /* any[tile][0]: frames in which some column reaches its threshold */

/* First pass over the columns: any[tile][0] |= (E_n >= T_n), any[tile][t] |= (E_n >= t) for t = 2 .. d_n + 1 -- per frame
 * whether a column reaches its threshold, and the largest E as a thermometer.  Words meet in LDS, then one atomic per
 * block and non-zero word.  grid (ceil(N / kBlock), tiles), block kBlock */
__global__ __launch_bounds__(kBlock) void bitflip_vote_kernel(const BitflipVarArgs a)
{
    __shared__ unsigned long long votes[64];
    const int tile = blockIdx.y;
    if (a.skip_done && a.done[tile] == ~0ull) return;
    if (threadIdx.x < 64) votes[threadIdx.x] = 0;
    __syncthreads();
    const int n = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (n < a.N) {
        uint64_t p[6];
        const int d = bitflip_count(a, tile, n, a.x[(size_t)tile * (size_t)a.N + n], p);
        const uint64_t hit = bitflip_ge(p, bitflip_threshold(d, a.off));
        if (hit) atomicOr(&votes[kBitflipVoteHit], (unsigned long long)hit);
        for (int t = 2; t <= d + 1; ++t) {          /* d <= 62: t <= 63 */
            const uint64_t ge = bitflip_ge(p, t);
            if (!ge) break;                         /* E >= t + 1 implies E >= t */
            atomicOr(&votes[t], (unsigned long long)ge);
        }
    }
    __syncthreads();
    if (threadIdx.x < 64 && votes[threadIdx.x])
        atomicOr(reinterpret_cast<unsigned long long *>(&a.any[(size_t)tile * 64 + threadIdx.x]), votes[threadIdx.x]);
}

/* Second pass: a frame with a hit flips its hit columns; a frame without flips the columns whose E is the frame's largest,
 * if that is >= 2.  Done frames keep their bits.  grid (ceil(N / kBlock), tiles), block kBlock */
__global__ __launch_bounds__(kBlock) void bitflip_flip_kernel(const BitflipVarArgs a)
{
    const int tile = blockIdx.y;
    const uint64_t frozen = a.done[tile];
    if (a.skip_done && frozen == ~0ull) return;
    const int n = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (n >= a.N) return;
    const size_t xi = (size_t)tile * (size_t)a.N + n;
    const uint64_t x = a.x[xi];
    uint64_t p[6];
    const int d = bitflip_count(a, tile, n, x, p);
    const uint64_t *any = a.any + (size_t)tile * 64;
    const uint64_t with_hit = any[kBitflipVoteHit];
    uint64_t flip = bitflip_ge(p, bitflip_threshold(d, a.off)) & with_hit;
    uint64_t rest = ~with_hit & ~frozen;            /* frames that fall back to their largest E */
    for (int t = 2; t <= d + 1 && rest; ++t) {
        const uint64_t ge = bitflip_ge(p, t) & rest;
        if (!ge) break;
        const uint64_t above = t + 1 < 64 ? any[t + 1] : 0ull;      /* frames in which some column has E > t */
        flip |= ge & ~above;
    }
    flip &= ~frozen;
    if (flip) a.x[xi] = x ^ flip;
}

#endif  /* LDPC_ENGINE_BITFLIP */

/* ------------------------------------------------------------- host side */

struct BitflipPlan {
    int32_t M = 0, N = 0;
    int64_t E = 0;
    int T = 0;                          /* tiles of 64 frames at max_batch */
    int32_t thresholds[kBitflipThresholds] = {};
    DevBuf<int32_t> col_row;            /* [E] */
    DevBuf<uint64_t> r, s, any;         /* [T][N], [T][M], [T][64] */
};

/* rows: row of every edge (row-major order); col_edge: the edges of every column, ascending */
inline hipError_t bitflip_plan_create(BitflipPlan *pl, int32_t M, int32_t N, int64_t E, const std::vector<int32_t> &rows,
                                      const std::vector<int32_t> &col_edge, int T, const int32_t *bf_threshold)
{
    pl->M = M; pl->N = N; pl->E = E; pl->T = T;
    for (int j = 0; j < kBitflipThresholds; ++j) pl->thresholds[j] = bf_threshold[j];
    std::vector<int32_t> col_row((size_t)E);
    for (int64_t k = 0; k < E; ++k) col_row[(size_t)k] = rows[(size_t)col_edge[(size_t)k]];
    hipError_t e = pl->col_row.upload(col_row);
    if (e == hipSuccess) e = pl->r.alloc((size_t)T * N);
    if (e == hipSuccess) e = pl->s.alloc((size_t)T * M);
    if (e == hipSuccess) e = pl->any.alloc((size_t)T * 64);
    return e;
}

struct BitflipRun : StreamRun {     /* engines.hpp; hard is [T][N], failw [max_iter + 2][T], done [T] */
    const int32_t *col_ptr = nullptr;
};

/* which: 0 = the syndrome words of the last round run, [frame][M] as 0 / 1 */
inline hipError_t bitflip_dump_syndrome(BitflipPlan *pl, float *host_out, int64_t count, int64_t frames)
{
    if (count != frames * pl->M) return hipErrorInvalidValue;
    const int tiles = (int)((frames + 63) / 64);
    std::vector<uint64_t> w((size_t)tiles * pl->M);
    const hipError_t e = hipMemcpy(w.data(), pl->s.p, w.size() * sizeof(uint64_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (int64_t f = 0; f < frames; ++f)
        for (int32_t m = 0; m < pl->M; ++m)
            host_out[f * pl->M + m] = (float)((w[(size_t)(f / 64) * pl->M + m] >> (f % 64)) & 1ull);
    return hipSuccess;
}

#ifdef LDPC_ENGINE_BITFLIP
inline hipError_t bitflip_run(BitflipPlan *pl, const BitflipRun &r, hipStream_t s, int32_t *launched)
{
    const int tiles = (int)((r.frames + 63) / 64);
    const size_t slot = (size_t)pl->T;
    const int rounds = r.tap_iter ? (r.tap_iter < r.max_iter ? r.tap_iter : r.max_iter) : r.max_iter;
    hipError_t e;
    if ((e = hipMemsetAsync(r.failw, 0, (size_t)(r.max_iter + 2) * slot * sizeof(uint64_t), s))) return e;
    if ((e = hipMemsetAsync(r.summary, 0, 4 * sizeof(int32_t), s))) return e;
    if ((e = hipMemsetAsync(pl->s.p, 0, (size_t)tiles * pl->M * sizeof(uint64_t), s))) return e;
    {
        BitflipInitArgs ia{r.llr.p, r.hard, pl->r.p, r.frames, pl->N, r.llr.unit};
        const dim3 grid((unsigned)((pl->N + kInitCols - 1) / kInitCols), (unsigned)tiles);
        if (r.span_begin && (e = r.span_begin(r.span_ctx, s, 3, 0, r.frames * (int64_t)pl->N * (int64_t)llr_elem_size(r.llr.type)))) return e;
        dispatch_llr(r.llr.type, [&](auto in) { bitflip_init_kernel<decltype(in)><<<grid, kBlock, 0, s>>>(ia); });
        if (r.span_end && (e = r.span_end(r.span_ctx, s))) return e;
        StateArgs st{r.done, nullptr, r.iters, nullptr, r.frames, 0, r.max_iter, 1};      /* padding frames are born done */
        state_kernel<1><<<tiles, 64, 0, s>>>(st);
    }
    const dim3 cgrid((unsigned)((pl->M + kBlock - 1) / kBlock), (unsigned)tiles);
    const dim3 vgrid((unsigned)((pl->N + kBlock - 1) / kBlock), (unsigned)tiles);
    for (int it = 1; it <= rounds; ++it) {
        uint64_t *fw = r.failw + (size_t)it * slot;
        /* algorithmic bytes of a tile slice: the row gathers and the s word; the column gathers, x twice and r */
        BitflipCheckArgs ca{r.row_ptr, r.edge_col, r.hard, pl->s.p, fw, r.done, pl->M, pl->N, r.early_term};
        if (r.span_begin && (e = r.span_begin(r.span_ctx, s, 0, 0, (int64_t)tiles * 8 * (pl->E + pl->M)))) return e;
        bitflip_check_kernel<<<cgrid, kBlock, 0, s>>>(ca);
        if (r.span_end && (e = r.span_end(r.span_ctx, s))) return e;
        if (r.crc_bits) {       /* frames whose covered bits pass the CRC count as clean (crc_term_kernels.hpp) */
            CrcTermArgs ct{r.hard, fw, r.done, r.crc_w, r.summary + 3, pl->N, r.crc_bits, TailRef{nullptr, 0, 0}};
            crc_term_kernel<1><<<dim3((unsigned)tiles, 1), 64 * crc_term_waves(r.crc_bits), 0, s>>>(ct);
        }
        bitflip_state_kernel<<<tiles, 64, 0, s>>>(r.done, fw, r.iters, pl->any.p, it);
        BitflipVarArgs va{r.col_ptr, pl->col_row.p, r.hard, pl->r.p, pl->s.p, r.done, pl->any.p, pl->M, pl->N,
                          bitflip_offset(pl->thresholds, it), r.early_term};
        if (r.span_begin && (e = r.span_begin(r.span_ctx, s, 1, 1, (int64_t)tiles * 8 * (pl->E + 2 * (int64_t)pl->N)))) return e;
        bitflip_vote_kernel<<<vgrid, kBlock, 0, s>>>(va);
        if (r.span_end && (e = r.span_end(r.span_ctx, s))) return e;
        if (r.span_begin && (e = r.span_begin(r.span_ctx, s, 1, 2, (int64_t)tiles * 8 * (pl->E + 3 * (int64_t)pl->N)))) return e;
        bitflip_flip_kernel<<<vgrid, kBlock, 0, s>>>(va);
        if (r.span_end && (e = r.span_end(r.span_ctx, s))) return e;
    }
    *launched = rounds;
    PackArgs pa{r.hard, r.out_dev, r.iters, r.iters_dev, r.frames, r.out_bytes, pl->N, r.K, r.pack_mode};
    if (r.out_dev || r.iters_dev) {
        if (r.pack_mode == 0) {
            pack_kernel<1><<<pack_grid<1>(r.K, tiles), kBlock, 0, s>>>(pa);
        } else {
            const int64_t n = r.out_bytes > r.frames ? r.out_bytes : r.frames;
            pack_kernel<1><<<(unsigned)((n + kBlock - 1) / kBlock), kBlock, 0, s>>>(pa);
        }
    }
    layered_summary_kernel<1><<<(unsigned)((r.frames + 255) / 256), 256, 0, s>>>(r.iters, r.done, r.frames, r.summary);
    return hipGetLastError();
}
#endif  /* LDPC_ENGINE_BITFLIP */

}  // namespace ldpc
