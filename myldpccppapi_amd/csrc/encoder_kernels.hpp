/*
 * encoder_kernels.hpp -- systematic LDPC encoding of a batch of frames on gfx950 (wave64).
 *
 * The batch is BIT-SLICED: X[n][w] is one 64-bit word that holds code bit n of the 64 frames
 * 64 w .. 64 w + 63 (bit l = frame 64 w + l), n < N, w < W = ceil(frames / 64).  X[0 .. K) are the
 * information bits, X[K .. N) the parity bits.  Frames are the lanes' bits and consecutive words are
 * consecutive lanes, so a row or column index of H is the same for a whole wave (a scalar load, as the
 * decoders' index tables) and every XOR handles 64 frames.  One code path per parity structure:
 *
 *   enc_load_kernel     packed source bytes -> X[0 .. K)      (64 x 64 bit transposes by ballot)
 *   enc_rows_kernel     out[m] = XOR of X[col] over a row's listed edges (lambda = A s; extension rows)
 *   enc_dd_core_kernel  dual diagonal: p1 = P_b^-1 sum lambda_i, then the forward substitution --
 *                       circulant shifts are index arithmetic on rows, nothing is rotated
 *   enc_stair_*         staircase: p_m = p_{m-1} ^ lambda_m as a chunked prefix XOR over lambda (per chunk: local
 *                       prefix and total; exclusive scan of the totals; apply)
 *   enc_dense_kernel    dense: p = T lambda, a bit-sliced GF(2) matrix product by the method of the Four Russians
 *   enc_store_kernel    X -> packed bytes (N/8 per frame) or one byte per code bit (N per frame)
 *
 * GF(2) only: no floating point.  Every kernel guards its rows by the counts it is given and its words by W;
 * stores to the caller's buffer are guarded by `frames` and N.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ldpc {

constexpr int kEncBlock = 256;       /* 4 waves */
constexpr int kEncWaves = 4;
constexpr int kEncChunk = 64;        /* staircase: rows per chunk of the prefix XOR */
constexpr int kEncScanWaves = 16;    /* staircase: waves that share the scan of the chunk totals */

__device__ inline int enc_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

/* 64 x 64 bit transpose across a wave: lane l returns the word whose bit i is bit l of lane i's v.
 * All 64 lanes must be active. */
__device__ inline uint64_t enc_transpose64(uint64_t v, int lane)
{
    uint64_t mine = 0;
#pragma unroll
    for (int l = 0; l < 64; ++l) {
        const uint64_t m = __ballot((int)((v >> l) & 1ull));
        if (lane == l) mine = m;
    }
    return mine;
}

/* Frame first + f reads the K/8 whole bytes from byte ((first + f) K) / 8 of the caller's stream (Coder::encode);
 * `src` points at byte (first K) / 8 = `base` of that stream and holds src_bytes bytes: beyond them zero. */
__global__ __launch_bounds__(kEncBlock) void enc_load_kernel(const uint8_t *__restrict__ src, int64_t src_bytes, int64_t first,
                                                            int64_t base, int64_t frames, int32_t K,
                                                            uint64_t *__restrict__ X, int32_t W)
{
    const int lane = threadIdx.x & 63;
    const int64_t i0 = ((int64_t)blockIdx.x * kEncWaves + enc_wave()) * 64;
    if (i0 >= K) return;
    const int32_t w = blockIdx.y;
    const int64_t f = (int64_t)w * 64 + lane;
    const int32_t kb = K / 8;
    uint64_t v = 0;
    if (f < frames) {
        const int64_t start = (first + f) * (int64_t)K / 8 - base;
        const int64_t at = start + i0 / 8;                       /* the lane's 8 bytes: src[at .. at + 8) */
        const int sh = (int)(((uintptr_t)src + (uintptr_t)at) & 7);
        const int64_t lo = at - sh;                              /* the two aligned words that cover them */
        if (i0 / 8 + 8 <= kb && lo >= 0 && lo + 16 <= src_bytes) {
            const uint64_t a = *reinterpret_cast<const uint64_t *>(src + lo);
            const uint64_t b = *reinterpret_cast<const uint64_t *>(src + lo + 8);
            v = sh ? (a >> (8 * sh)) | (b << (64 - 8 * sh)) : a;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int64_t j = i0 / 8 + k;
                if (j < kb && at + k < src_bytes) v |= (uint64_t)src[at + k] << (8 * k);
            }
        }
    }
    const uint64_t word = enc_transpose64(v, lane);     /* lane = bit i0 + lane, bits = frames */
    if (i0 + lane < K) X[(size_t)(i0 + lane) * W + w] = word;
}

/* out[m][w] = XOR over e in [ptr[m], ptr[m+1]) of X[col[e]][w] for rows [row_lo, row_hi): one wave per row and
 * 64 words (grid.y tiles the words) */
__global__ __launch_bounds__(kEncBlock) void enc_rows_kernel(const uint64_t *__restrict__ X, const int32_t *__restrict__ ptr,
                                                            const int32_t *__restrict__ col, int32_t row_lo, int32_t row_hi,
                                                            uint64_t *__restrict__ out, int32_t W)
{
    const int32_t m = row_lo + (int32_t)blockIdx.x * kEncWaves + enc_wave();
    const int32_t w = (int32_t)blockIdx.y * 64 + (threadIdx.x & 63);
    if (m >= row_hi || w >= W) return;
    uint64_t acc = 0;
    const int32_t e1 = ptr[m + 1];
    for (int32_t e = ptr[m]; e < e1; ++e) acc ^= X[(size_t)col[e] * W + w];
    out[(size_t)m * W + w] = acc;
}

/* Core of the dual-diagonal structure, c block rows of z rows, lam[c z][W] = A s.  The first parity block column
 * has circulants of shift a, b, a in block rows 0, x, c-1 ((P_p v)[r] = v[(r + p) mod z]); parity block columns
 * 1 .. c-1 are the dual diagonal.  Adding all block rows leaves P_b p1 = sum_i lam_i =: S, so
 *     p1[(r + b) mod z] = S[r],   v1[r] = lam_0[r] ^ p1[(r + a) mod z] = lam_0[r] ^ S[(r + a - b) mod z],
 *     v_{i+1}[r] = lam_i[r] ^ v_i[r] ^ (i == x ? S[r] : 0),  i = 1 .. c-2.
 * One wave per r and 64 words; P = X + K W receives p1 | v1 | ... | v_{c-1}. */
__global__ __launch_bounds__(kEncBlock) void enc_dd_core_kernel(const uint64_t *__restrict__ lam, uint64_t *__restrict__ P, int32_t z,
                                                               int32_t c, int32_t x, int32_t a, int32_t b, int32_t W)
{
    const int32_t r = (int32_t)blockIdx.x * kEncWaves + enc_wave();
    const int32_t w = (int32_t)blockIdx.y * 64 + (threadIdx.x & 63);
    if (r >= z || w >= W) return;
    const int32_t r2 = (r + a - b + z) % z;
    uint64_t s = 0, t = 0;
    for (int32_t i = 0; i < c; ++i) {
        s ^= lam[((size_t)i * z + r) * W + w];
        t ^= lam[((size_t)i * z + r2) * W + w];
    }
    P[(size_t)((r + b) % z) * W + w] = s;
    uint64_t v = lam[(size_t)r * W + w] ^ t;
    P[((size_t)z + r) * W + w] = v;
    for (int32_t i = 1; i <= c - 2; ++i) {
        v ^= lam[((size_t)i * z + r) * W + w] ^ (i == x ? s : 0ull);
        P[((size_t)(i + 1) * z + r) * W + w] = v;
    }
}

/* Staircase, step 1 (after enc_rows_kernel has put lambda_m into P[m]): one wave per chunk of kEncChunk rows;
 * P[m] = XOR of lambda over the chunk's rows up to m, T[chunk] = the chunk's total.  The addresses do not depend on
 * the data, so the loads of a chunk are in flight together. */
__global__ __launch_bounds__(kEncBlock) void enc_stair_local_kernel(int32_t M, uint64_t *__restrict__ P, uint64_t *__restrict__ T, int32_t W)
{
    const int32_t ch = (int32_t)blockIdx.x * kEncWaves + enc_wave();
    const int32_t w = (int32_t)blockIdx.y * 64 + (threadIdx.x & 63);
    const int32_t m0 = ch * kEncChunk;
    if (m0 >= M || w >= W) return;
    uint64_t acc = 0;
    if (m0 + kEncChunk <= M) {
#pragma unroll 16
        for (int k = 0; k < kEncChunk; ++k) {
            acc ^= P[(size_t)(m0 + k) * W + w];
            P[(size_t)(m0 + k) * W + w] = acc;
        }
    } else {
        for (int32_t m = m0; m < M; ++m) {
            acc ^= P[(size_t)m * W + w];
            P[(size_t)m * W + w] = acc;
        }
    }
    T[(size_t)ch * W + w] = acc;
}

/* Staircase, step 2: T[chunk] becomes the XOR of the totals of all chunks before it.  One workgroup per 64 words;
 * its kEncScanWaves waves take contiguous runs of chunks (run total -> LDS, prefix over the runs, second pass). */
__global__ __launch_bounds__(64 * kEncScanWaves) void enc_stair_scan_kernel(uint64_t *__restrict__ T, int32_t chunks, int32_t W)
{
    __shared__ uint64_t run_total[kEncScanWaves][64];
    const int lane = threadIdx.x & 63;
    const int wave = enc_wave();
    const int32_t w = (int32_t)blockIdx.x * 64 + lane;
    const int32_t per = (chunks + kEncScanWaves - 1) / kEncScanWaves;
    const int32_t c0 = wave * per;
    const int32_t c1 = c0 + per < chunks ? c0 + per : chunks;
    uint64_t tot = 0;
    if (w < W)
        for (int32_t ch = c0; ch < c1; ++ch) tot ^= T[(size_t)ch * W + w];
    run_total[wave][lane] = tot;
    __syncthreads();
    if (w >= W) return;
    uint64_t run = 0;
    for (int k = 0; k < wave; ++k) run ^= run_total[k][lane];
    for (int32_t ch = c0; ch < c1; ++ch) {
        const uint64_t t = T[(size_t)ch * W + w];
        T[(size_t)ch * W + w] = run;
        run ^= t;
    }
}

/* Staircase, step 3: P[m] ^= T[chunk of m] */
__global__ __launch_bounds__(kEncBlock) void enc_stair_apply_kernel(uint64_t *__restrict__ P, const uint64_t *__restrict__ T, int32_t M,
                                                                   int32_t W)
{
    const int32_t m = kEncChunk + (int32_t)blockIdx.x * kEncWaves + enc_wave();     /* chunk 0 has nothing before it */
    const int32_t w = (int32_t)blockIdx.y * 64 + (threadIdx.x & 63);
    if (m >= M || w >= W) return;
    P[(size_t)m * W + w] ^= T[(size_t)(m / kEncChunk) * W + w];
}

/* Dense structure: P[r][w] = XOR over the columns j < M with bit j of T's row r set of lam[j][w], r < rho -- a GF(2)
 * matrix product whose right-hand side is bit-sliced (lam[M][W] = H_s u by enc_rows_kernel, T: rho rows of tw words).
 * Method of the Four Russians: a workgroup owns kDenseRows output rows and 64 words and walks the M columns in stages of
 * kDenseCols = 4 kDenseGroups columns.  Per stage it builds, per group of 4 lambda rows, the XOR of each of their 16
 * subsets in LDS (tab[group][entry][lane], one XOR per entry in Gray-code order: entry i ^ (i >> 1) differs from its
 * predecessor in bit ctz(i)); an output row then takes one 8-byte LDS read per 4 columns.  A stage lies inside one word of
 * T, and the row is the wave's, so that word is one scalar load and the entry index is wave-uniform: every LDS access is
 * base + 8 lane, free of bank conflicts.  The lambda rows of the next stage are loaded into registers before the current
 * stage's reads, so their latency hides behind them.  grid.z cuts the columns into slices (enc_dense_slices): each
 * slice adds its share into a zeroed P with a 64-bit atomic XOR.  Guards: rows by rho, words by W, lambda rows by M (T's tail bits
 * are zero, but no load relies on that). */
#ifndef LDPC_ENC_DENSE_ROWS
#define LDPC_ENC_DENSE_ROWS 64      /* measurement builds (tools/encoder_measure.py --dense) override these two */
#endif
#ifndef LDPC_ENC_DENSE_GROUPS
#define LDPC_ENC_DENSE_GROUPS 4
#endif
constexpr int kDenseRows = LDPC_ENC_DENSE_ROWS;        /* output rows per workgroup */
constexpr int kDenseGroups = LDPC_ENC_DENSE_GROUPS;    /* tables of 16 entries per stage: 4, 8 or 16 */
constexpr int kDenseCols = 4 * kDenseGroups;
constexpr size_t kDenseLds = (size_t)kDenseGroups * 16 * 64 * sizeof(uint64_t);     /* 8 KiB per group */
static_assert(kDenseRows % kEncWaves == 0 && kDenseGroups % kEncWaves == 0 && 64 % kDenseCols == 0, "dense encoder tile");

__global__ __launch_bounds__(kEncBlock, 2) void enc_dense_kernel(const uint64_t *__restrict__ T, int32_t tw, const uint64_t *__restrict__ lam,
                                                             int32_t M, int32_t rho, uint64_t *__restrict__ P, int32_t W, int32_t slice_cols)
{
    extern __shared__ uint64_t dense_tab[];     /* [kDenseGroups][16][64] */
    constexpr int GW = kDenseGroups / kEncWaves, RW = kDenseRows / kEncWaves;
    const int lane = threadIdx.x & 63;
    const int wave = enc_wave();
    const int32_t w = (int32_t)blockIdx.y * 64 + lane;
    const bool live = w < W;
    const int32_t wc = live ? w : 0;                                     /* every load is in bounds; a dead lane's is dropped */
    const int32_t r0 = (int32_t)blockIdx.x * kDenseRows + wave * RW;      /* this wave's rows r0 .. r0 + RW */
    uint64_t acc[RW], l[GW][4];
#pragma unroll
    for (int i = 0; i < RW; ++i) acc[i] = 0;
    /* this wave builds the tables of groups wave GW .. wave GW + GW - 1; a lambda row beyond M reads as zero */
    auto fetch = [&](int32_t j0) {
#pragma unroll
        for (int q = 0; q < GW; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int32_t j = j0 + 4 * (wave * GW + q) + i;
                const uint64_t v = lam[(size_t)(j < M ? j : M - 1) * W + wc];
                l[q][i] = live && j < M ? v : 0ull;
            }
    };
    /* grid.z cuts the columns into slices of slice_cols (a multiple of kDenseCols); uniform for the workgroup */
    const int32_t j_lo = (int32_t)blockIdx.z * slice_cols;
    const int32_t j_hi = j_lo + slice_cols < M ? j_lo + slice_cols : M;
    if (j_lo >= M) return;
    fetch(j_lo);
    const uint64_t *tl = dense_tab + lane;
    for (int32_t j0 = j_lo; j0 < j_hi; j0 += kDenseCols) {
#pragma unroll
        for (int q = 0; q < GW; ++q) {
            uint64_t *t = dense_tab + (size_t)(wave * GW + q) * 16 * 64 + lane;
            uint64_t cur = 0;
            t[0] = 0;
#pragma unroll
            for (int i = 1; i < 16; ++i) {
                cur ^= l[q][__builtin_ctz(i)];
                t[(i ^ (i >> 1)) * 64] = cur;
            }
        }
        __syncthreads();
        if (j0 + kDenseCols < j_hi) fetch(j0 + kDenseCols);
        const uint64_t *trow = T + (j0 >> 6);
        const int sh = j0 & 63;
#pragma unroll
        for (int i = 0; i < RW; ++i) {
            /* a row beyond rho reads row rho - 1 and is never stored */
            const int32_t r = r0 + i < rho ? r0 + i : rho - 1;
            const uint64_t bits = trow[(size_t)r * tw] >> sh;
#pragma unroll
            for (int g = 0; g < kDenseGroups; ++g)
                acc[i] ^= tl[(g * 16 + (int)((bits >> (4 * g)) & 15u)) * 64];
            /* four rows' reads (4 kDenseGroups) are issued together; without the fence all of a stage's reads and their
             * addresses are hoisted and the kernel spills */
            if (i % 4 == 3) __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
    }
    if (!live) return;
#pragma unroll
    for (int i = 0; i < RW; ++i)
        if (r0 + i < rho) {
            /* more than one slice: P was zeroed and every slice adds its share (XOR commutes: the bytes do not depend
             * on the order) */
            if (gridDim.z > 1) atomicXor(reinterpret_cast<unsigned long long *>(P + (size_t)(r0 + i) * W + w), (unsigned long long)acc[i]);
            else P[(size_t)(r0 + i) * W + w] = acc[i];
        }
}

/* Slices of columns for enc_dense_kernel: few output rows or few words leave the 256 CUs with less than a workgroup each,
 * and a workgroup's walk is a chain of dependent stages (load, build, read); cutting the columns gives kDenseTargetBlocks
 * workgroups to overlap those chains.  Returns the columns per slice; *slices = grid.z */
constexpr int kDenseTargetBlocks = 2048;
constexpr int kDenseMaxSlices = 32;
inline int32_t enc_dense_slices(int32_t M, int32_t rho, int32_t W, int32_t *slices)
{
    const int64_t blocks = (int64_t)((rho + kDenseRows - 1) / kDenseRows) * ((W + 63) / 64);
    const int32_t stages = (M + kDenseCols - 1) / kDenseCols;
    int64_t want = (kDenseTargetBlocks + blocks - 1) / blocks;
    if (want > kDenseMaxSlices) want = kDenseMaxSlices;
    if (want > stages) want = stages;
    const int32_t per = (int32_t)((stages + want - 1) / want);      /* stages per slice */
    *slices = (stages + per - 1) / per;
    return per * kDenseCols;
}

/* 4 bits -> 4 bytes of 0/1 (bit k to byte k): k + 7 j = 8 k' only for j = k = k', and no two products share a bit */
__device__ inline uint32_t enc_spread4(uint32_t nibble) { return (nibble * 0x00204081u) & 0x01010101u; }

/* X -> the caller's buffer.  A wave takes 64 code bits x 64 frames; after the transpose lane l holds bits
 * i0 .. i0 + 63 of frame 64 w + l: 8 consecutive bytes (packed, LSB first) or 64 consecutive bytes (bits) of that
 * frame.  `align`: width in bytes of the stores the buffer's address and N allow for every frame (packed: 4 or 1;
 * bits: 16, 4 or 1).  Bits with 16-byte stores -- the bulk of the traffic -- go through LDS so that one store
 * instruction writes whole 64-byte runs (4 lanes per frame, 16 frames) instead of 16 bytes in each of 64 frames. */
template <int BITS> __global__ __launch_bounds__(kEncBlock) void enc_store_kernel(const uint64_t *__restrict__ X, int32_t N, int32_t W,
                                                                                 int64_t frames, uint8_t *__restrict__ code, int32_t align)
{
    const int lane = threadIdx.x & 63;
    const int wave = enc_wave();
    const int64_t i0 = ((int64_t)blockIdx.x * kEncWaves + wave) * 64;
    const int32_t w = blockIdx.y;
    const uint64_t word = i0 + lane < N ? X[(size_t)(i0 + lane) * W + w] : 0ull;      /* a wave beyond N: all zero, stores nothing */
    const uint64_t v = enc_transpose64(word, lane);     /* lane = frame, bits = code bits i0 .. i0 + 63 */
    const int64_t f = (int64_t)w * 64 + lane;
    if (BITS) {
        const int n = i0 >= N ? 0 : N - i0 < 64 ? (int)(N - i0) : 64;
        if (align == 16) {
            __shared__ uint4 stage[kEncWaves][64][5];           /* rows of 64 + 16 bytes: no bank conflicts either way */
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t h = (uint32_t)(v >> (16 * g)) & 0xffffu;
                uint4 q;
                q.x = enc_spread4(h & 15u);
                q.y = enc_spread4((h >> 4) & 15u);
                q.z = enc_spread4((h >> 8) & 15u);
                q.w = enc_spread4(h >> 12);
                stage[wave][lane][g] = q;
            }
            __syncthreads();
            const int g = lane & 3;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int fr = 16 * k + (lane >> 2);
                const int64_t ff = (int64_t)w * 64 + fr;
                if (ff < frames && 16 * g + 16 <= n)
                    *reinterpret_cast<uint4 *>(code + ff * (int64_t)N + i0 + 16 * g) = stage[wave][fr][g];
            }
            return;
        }
        if (f >= frames) return;
        uint8_t *dst = code + f * (int64_t)N + i0;
        if (align == 4) {
#pragma unroll
            for (int g = 0; g < 16; ++g)
                if (4 * g + 4 <= n) *reinterpret_cast<uint32_t *>(dst + 4 * g) = enc_spread4((uint32_t)(v >> (4 * g)) & 15u);
        } else {
            for (int k = 0; k < n; ++k) dst[k] = (uint8_t)((v >> k) & 1ull);
        }
    } else {
        if (f >= frames || i0 >= N) return;
        const int64_t nb = N / 8;
        uint8_t *dst = code + f * nb + i0 / 8;
        const int n = nb - i0 / 8 < 8 ? (int)(nb - i0 / 8) : 8;
        if (align == 4) {
            if (n >= 4) *reinterpret_cast<uint32_t *>(dst) = (uint32_t)v;
            if (n >= 8) *reinterpret_cast<uint32_t *>(dst + 4) = (uint32_t)(v >> 32);
        } else {
            for (int k = 0; k < n; ++k) dst[k] = (uint8_t)(v >> (8 * k));
        }
    }
}

}  // namespace ldpc
