/*
 * flood_handover.hpp -- handing the last running frames over: tail compaction into a child decoder (compact_*)
 * and the device-side tail into the overflow tiles (tail_*).
 */
#pragma once

#include "flood_common.hpp"

namespace ldpc {

/* ---- tail compaction (early termination): when only a few frames of a large batch are still
 * running, their state moves into ONE 64-frame tile of a small child decoder, which finishes
 * them; the parent's tiles stop being launched.  Frames are independent, so nothing changes for
 * any frame except where its state lives.
 * compact_list_kernel: map[slot] = frame index of every running frame (slot order is arbitrary). */
template <int V> __global__ __launch_bounds__(kBlock) void compact_list_kernel(const uint64_t *__restrict__ done, int64_t frames,
                                                                               int32_t *__restrict__ map, int32_t *__restrict__ count,
                                                                               int32_t capacity)
{
    constexpr int F = 64 * V;
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= frames) return;
    const int64_t tile = f / F;
    const int fi = (int)(f % F);
    if ((done[tile * V + fi % V] >> (fi / V)) & 1ull) return;
    const int slot = atomicAdd(count, 1);
    if (slot < capacity) map[slot] = (int32_t)f;
}

/* The child's tiles hold cf = 64 * cv frames (cv = 1, or 4 for the 1024-frame child of large batches); slot j of the
 * hand-over is frame j % cf of child tile j / cf, i.e. element j % cf of a row's segment and bit (j % cf) / cv of mask
 * word (j % cf) % cv. */
__host__ __device__ inline size_t child_elem(int j, int cf, int64_t rows, int64_t i) { return ((size_t)(j / cf) * rows + i) * cf + (j % cf); }

/* dst[i][j] = src[tile(map[j])][i][position of map[j]] for j < count (0 beyond): the per-edge /
 * per-column values of the running frames, gathered into the child's tiles.  One wave per row i and 64 slots. */
template <int V, typename T>
__global__ __launch_bounds__(kBlock) void compact_gather_kernel(const T *__restrict__ src, T *__restrict__ dst,
                                                                const int32_t *__restrict__ map, int32_t count, int64_t rows, int cf,
                                                                const int32_t *__restrict__ src_row = nullptr,
                                                                const int32_t *__restrict__ dst_row = nullptr)
{
    /* src_row / dst_row: where row i lives in the parent's / the child's array (the Q arrays: CheckArgs::qpos of either
     * decoder -- their column-fused edges differ with the tile size); nullptr: row i */
    constexpr int F = 64 * V;
    const int j = threadIdx.x & 63, jg = blockIdx.y * 64 + j;               /* slot jg */
    const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + wave_id_in_block();
    if (i >= rows) return;
    const int64_t is = src_row ? src_row[i] : i, id = dst_row ? dst_row[i] : i;
    T val = (T)0;
    if (jg < count) {
        const int64_t f = map[jg];
        val = src[((f / F) * rows + is) * F + (f % F)];
    }
    dst[child_elem(jg, cf, rows, id)] = val;
}

/* The same gather for MANY frames (hundreds, sitting in every tile of the batch): one thread per element as
 * above touches a 64-byte sector for every 2- or 4-byte value, i.e. reads the whole array through the L2 in
 * sector-sized requests.  Here a block takes one row i, streams that row's segments of all `tiles` parent
 * tiles into LDS with coalesced 16-byte loads, chunk by chunk, and picks the running frames' values from
 * there.  HBM traffic = one pass over the parent array (a third of a round) however many frames move. */
constexpr int kGatherChunk = 4096;      /* elements staged at a time (16 KB of fp32) */
/* rows a block walks, the next one's loads in flight: 2-byte rows (8 KB for 4096 frames) left the memory pipe idle with one row
 * per block (3.6 -> 4.9 TB/s with eight); 4-byte rows have enough in flight with one row per block and LOSE with eight (650 -> 880 us
 * for the headline code's 3.7 GB: the block's serial stage / pick phases then stand in the way);
 * 1-byte rows (4 KB for 4096 frames) walk eight rows like the 2-byte ones (not measured on their own) */
template <typename T> constexpr int gather_rows_per_block() { return sizeof(T) < 4 ? 8 : 1; }
template <int V, typename T>
__global__ __launch_bounds__(kBlock) void compact_gather_rows_kernel(const T *__restrict__ src, T *__restrict__ dst,
                                                                     const int32_t *__restrict__ map, int32_t count,
                                                                     int64_t rows, int32_t tiles, int cf,
                                                                     const int32_t *__restrict__ src_row = nullptr,
                                                                     const int32_t *__restrict__ dst_row = nullptr)
{
    constexpr int F = 64 * V;
    constexpr int TPC = kGatherChunk / F;               /* parent tiles per chunk */
    constexpr int VEC = 16 / (int)sizeof(T);            /* 16 bytes per lane (a tile's row segment is F * sizeof(T) >= 64 bytes -- fp8 at V = 1 --, 16-byte aligned) */
    static_assert(F % VEC == 0 && kGatherChunk % (kBlock * VEC) == 0, "whole 16-byte vectors per segment and per pass");
    constexpr int NV = kGatherChunk / (kBlock * VEC);   /* 16-byte vectors a thread stages per chunk */
    __shared__ __attribute__((aligned(16))) T stage[kGatherChunk];
    const int cslots = ((count + cf - 1) / cf) * cf;    /* child slots in use (whole child tiles) */
    constexpr int RPB = gather_rows_per_block<T>();
    const int64_t r0 = (int64_t)blockIdx.x * RPB;
    const int64_t r1 = r0 + RPB < rows ? r0 + RPB : rows;
    if (tiles <= TPC) {
        /* the usual case, a row's segments of all tiles fit one chunk: the block walks its rows with the NEXT row's
         * loads in flight while this row's values are picked from LDS (one row per block left the memory pipe idle
         * during the pick: 3.6 TB/s on fp16 rows of 8 KB) */
        vf4 pre[NV];
        auto issue = [&](int64_t r) {
            const int64_t i = src_row ? src_row[r] : r;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int k = (v * kBlock + (int)threadIdx.x) * VEC;
                if (k < tiles * F) pre[v] = ld_stream(reinterpret_cast<const vf4 *>(src + ((size_t)(k / F) * rows + i) * F + (k % F)));
            }
        };
        if (r0 < r1) issue(r0);
        /* this thread's slots j = threadIdx.x + u * kBlock: where they come from and where they go is the same for every
         * row (child_elem's run-time divisions, per element, were a quarter of a millisecond of integer arithmetic) */
        constexpr int NS = (2 * kCompactCapacity + kBlock - 1) / kBlock;      /* slots per thread: 1024 frames at most */
        int from[NS];
        size_t to[NS];
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const int j = (int)threadIdx.x + u * kBlock;
            from[u] = j < count ? map[j] : -1;
            to[u] = j < cslots ? child_elem(j, cf, rows, 0) : 0;
        }
        for (int64_t r = r0; r < r1; ++r) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int k = (v * kBlock + (int)threadIdx.x) * VEC;
                if (k < tiles * F) *reinterpret_cast<vf4 *>(&stage[k]) = pre[v];
            }
            __syncthreads();
            if (r + 1 < r1) issue(r + 1);
            const int64_t id = dst_row ? dst_row[r] : r;
            T *drow = dst + (size_t)id * cf;                 /* child_elem(j, cf, rows, id) = child_elem(j, cf, rows, 0) + id * cf */
#pragma unroll
            for (int u = 0; u < NS; ++u)
                if ((int)threadIdx.x + u * kBlock < cslots) drow[to[u]] = from[u] >= 0 ? stage[from[u]] : (T)0;
            __syncthreads();
        }
        return;
    }
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t i = src_row ? src_row[r] : r;         /* the row in the parent ... */
        const int64_t id = dst_row ? dst_row[r] : r;        /* ... and in the child */
        for (int t0 = 0; t0 < tiles; t0 += TPC) {
            const int nt = min(TPC, tiles - t0);
            for (int k = threadIdx.x * VEC; k < nt * F; k += kBlock * VEC)
                *reinterpret_cast<vf4 *>(&stage[k]) =
                    ld_stream(reinterpret_cast<const vf4 *>(src + ((size_t)(t0 + k / F) * rows + i) * F + (k % F)));
            __syncthreads();
            for (int j = threadIdx.x; j < cslots; j += kBlock) {
                if (j < count) {
                    const int f = map[j] - t0 * F;
                    if (f >= 0 && f < nt * F) dst[child_elem(j, cf, rows, id)] = stage[f];
                } else if (t0 == 0) {
                    dst[child_elem(j, cf, rows, id)] = (T)0;
                }
            }
            __syncthreads();
        }
    }
}

/* hard bits, parent -> child (sum-product only: its decision rule can keep the previous bit): child bit of slot j <- parent
 * bit of frame map[j].  One wave per column n and group g of 64 slots.  With a child of cv frames per lane the group's slots
 * are frames (g % cv) * 64 ... + 63 of child tile g / cv, i.e. the 64 / cv-bit field number g % cv of each of its cv mask
 * words (bit l of word v = frame cv * l + v) -- written as that field alone, no atomics (compress_stride: the bits of the
 * lanes v, v + cv, ... of the ballot).  The way back is compact_hard_back_kernel. */
template <int V> __global__ __launch_bounds__(kBlock) void compact_hard_kernel(const uint64_t *__restrict__ parent, uint64_t *__restrict__ child,
                                                                               const int32_t *__restrict__ map, int32_t count, int32_t N,
                                                                               int cv)
{
    constexpr int F = 64 * V;
    const int j = threadIdx.x & 63, g = blockIdx.y, jg = g * 64 + j;
    const int64_t n = (int64_t)blockIdx.x * kWavesPerBlock + wave_id_in_block();
    if (n >= N) return;
    const int64_t f = jg < count ? map[jg] : 0;
    const int fi = (int)(f % F);
    const uint64_t word = parent[((f / F) * N + n) * V + fi % V];
    const bool bit = jg < count && ((word >> (fi / V)) & 1ull);
    const uint64_t b = __ballot(bit);
    uint64_t *cw = child + ((size_t)(g / cv) * N + n) * cv;              /* the cv words of child tile g / cv, column n */
    if (cv == 1) {
        if (j == 0) cw[0] = b;
    } else if (cv == 2) {
        if (j < 2) reinterpret_cast<uint32_t *>(cw + j)[g % 2] = (uint32_t)compress_stride<2>(b >> j);
    } else {
        if (j < 4) reinterpret_cast<uint16_t *>(cw + j)[g % 4] = (uint16_t)compress_stride<4>(b >> j);
    }
}

/* The same gather for parents of up to kGatherParentWords mask words per column (4096 frames at V = 4) and up to
 * 2 * kCompactCapacity slots: a block takes 64 columns, stages their parent words (contiguous per tile) and the decoded slot
 * table in LDS, and each thread assembles whole child words from there.  One wave per column and 64 slots (above) reads one
 * scattered 8-byte word per lane through the L2: 66 M requests, 150-200 us for the 1024-frame child of the headline code. */
constexpr int kGatherParentWords = 64;
template <int V> __global__ __launch_bounds__(kBlock) void compact_hard_lds_kernel(const uint64_t *__restrict__ parent, uint64_t *__restrict__ child,
                                                                                   const int32_t *__restrict__ map, int32_t count, int32_t N,
                                                                                   int cv, int ptiles, int cwords)
{
    constexpr int F = 64 * V;
    constexpr int COLS = 64, TPC = kBlock / COLS;           /* columns per block, threads per column (one wave each) */
    __shared__ uint64_t pw[kGatherParentWords][COLS];
    __shared__ int32_t sbit[2 * kCompactCapacity];          /* slot j -> (parent word of the column) << 8 | bit */
    const int n0 = blockIdx.x * COLS;
    for (int idx = threadIdx.x; idx < ptiles * COLS * V; idx += kBlock) {
        const int tile = idx / (COLS * V), rem = idx % (COLS * V), c = rem / V, v = rem % V;
        pw[tile * V + v][c] = n0 + c < N ? parent[((size_t)tile * N + n0) * V + rem] : 0ull;
    }
    for (int j = threadIdx.x; j < count; j += kBlock) {
        const int f = map[j], fi = f % F;
        sbit[j] = (((f / F) * V + fi % V) << 8) | (fi / V);
    }
    __syncthreads();
    const int c = threadIdx.x % COLS, q = threadIdx.x / COLS, n = n0 + c;
    if (n >= N) return;
    const int cf = 64 * cv;
    for (int cwd = q; cwd < cwords; cwd += TPC) {
        const int ctile = cwd / cv, cword = cwd % cv;       /* per child word, not per bit */
        uint64_t val = 0;
        for (int b = 0; b < 64; ++b) {
            const int j = ctile * cf + b * cv + cword;      /* the slot whose bit is bit b of this word */
            if (j >= count) break;
            const int sb = sbit[j];
            val |= ((pw[sb >> 8][c] >> (sb & 255)) & 1ull) << b;
        }
        child[((size_t)ctile * N + n) * cv + cword] = val;
    }
}

/* The way back (for any number of frames; one atomic per bit, as rounds 2 and early 3 did it, is 44 M device
 * atomics for 681 frames of the rate-9/10 code): every parent word is rewritten by ONE thread that looks up, for
 * the bits of its frames that were handed over, the child's bit: inv[frame] = where that bit sits in the child,
 * moved[(tile, v)] = which bits of that word moved (both filled by compact_inverse_kernel). */
template <int V> __global__ void compact_inverse_kernel(const int32_t *__restrict__ map, int32_t count, int32_t *__restrict__ inv,
                                                        unsigned long long *__restrict__ moved, int cv)
{
    /* inv[f] = where slot j's bit sits in the child, decoded once here: (child word of the column) << 8 | bit
     * (compact_hard_back_kernel did the four run-time divisions per moved frame and column: 79 us of integer arithmetic) */
    constexpr int F = 64 * V;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const int f = map[j], fi = f % F;
    const int cf = 64 * cv, cfi = j % cf;
    inv[f] = (((j / cf) * cv + cfi % cv) << 8) | (cfi / cv);
    atomicOr(&moved[(size_t)(f / F) * V + fi % V], 1ull << (fi / V));
}

constexpr int kBackWords = 16;          /* child mask words per column a block keeps: 1024 frames */
template <int V> __global__ __launch_bounds__(kBlock) void compact_hard_back_kernel(uint64_t *__restrict__ parent, const uint64_t *__restrict__ child,
                                                                                    const int32_t *__restrict__ inv,
                                                                                    const unsigned long long *__restrict__ moved, int32_t N,
                                                                                    int cv, int cwords)
{
    /* cwords = child tiles in use x cv <= kBackWords: the column's child words go to LDS once (thread-private
     * entries, read back by a run-time index) -- one load per moved frame instead read 8 of every 32 fetched bytes,
     * 1.4 GB through the L2 for 681 frames: 79 us */
    constexpr int F = 64 * V;
    __shared__ uint64_t cw[kBackWords][kBlock];
    __shared__ int32_t sinv[F];             /* the tile's slots: a global load per moved frame put its latency into every trip */
    const int n = blockIdx.x * kBlock + threadIdx.x;
    const int tile = blockIdx.y;
    bool any = false;
#pragma unroll
    for (int v = 0; v < V; ++v) any = any || moved[(size_t)tile * V + v] != 0;
    if (!any) return;                       /* block-uniform */
    for (int k = threadIdx.x; k < F; k += kBlock) sinv[k] = inv[tile * F + k];
    __syncthreads();
    if (n >= N) return;
    for (int w = 0; w < cwords; ++w) cw[w][threadIdx.x] = child[((size_t)(w / cv) * N + n) * cv + w % cv];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        uint64_t m = moved[(size_t)tile * V + v];
        if (!m) continue;
        uint64_t w = parent[((size_t)tile * N + n) * V + v];
        while (m) {
            const int l = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const int j = sinv[l * V + v];                  /* child word << 8 | bit (compact_inverse_kernel) */
            const uint64_t bit = (cw[j >> 8][threadIdx.x] >> (j & 255)) & 1ull;
            w = (w & ~(1ull << l)) | (bit << l);
        }
        parent[((size_t)tile * N + n) * V + v] = w;
    }
}

/* iteration counts and converged flags back; one thread per slot */
template <int V> __global__ void compact_finish_kernel(uint64_t *__restrict__ parent_done, int32_t *__restrict__ parent_iters,
                                                       const uint64_t *__restrict__ child_done, const int32_t *__restrict__ child_iters,
                                                       const int32_t *__restrict__ map, int32_t count, int cv)
{
    constexpr int F = 64 * V;
    const int cf = 64 * cv;
    const int jg = blockIdx.x * 64 + threadIdx.x;
    if (jg >= count) return;
    const int64_t f = map[jg];
    const int fi = (int)(f % F), cfi = jg % cf;
    parent_iters[f] = child_iters[jg];
    if ((child_done[(size_t)(jg / cf) * cv + cfi % cv] >> (cfi / cv)) & 1ull)
        atomicOr(reinterpret_cast<unsigned long long *>(parent_done) + (f / F) * V + fi % V, 1ull << (fi / V));
}

/* the child's bookkeeping when it takes over `count` running frames: slots beyond are padding.  One block of 64
 * lanes per child tile. */
template <int kUnused = 0>       /* a template only so that every translation unit may include this header */
__global__ void compact_child_state_kernel(uint64_t *__restrict__ done, int32_t *__restrict__ iters, int32_t count, int32_t max_iter, int cv)
{
    const int l = threadIdx.x, tile = blockIdx.x, cf = 64 * cv;
    for (int v = 0; v < cv; ++v) {
        const int slot = tile * cf + l * cv + v;
        iters[slot] = max_iter;
        const uint64_t pad = __ballot(slot >= count);
        if (l == 0) done[(size_t)tile * cv + v] = pad;
    }
}

/* ---- device-side tail: the same hand-over decided and carried out without the host ---------------
 * tail_gather_kernel runs after the state update of a round.  Every block reads the number of
 * frames still running after that round; unless 0 < running <= threshold (and at most a quarter
 * of the batch) nothing happens.  Otherwise each block lists the running frames (the same list in
 * every block: ascending mask word, ascending bit), and the blocks share the rows of Q, of the
 * channel array and of the hard-bit masks: the running frames' values go to consecutive slots of
 * the overflow tiles (same layout, same V).  The block that finishes last publishes the list,
 * marks every batch tile finished and the overflow slots in use, and sets state[0]: the next
 * launch's blocks follow it (tile_select).  tail_scatter_kernel brings bits, iteration counts and
 * converged flags back before packing. */
struct TailArgs {
    int32_t *state;                     /* [0] handed, [1] count, [2] round, [3] ticket */
    int32_t *map;                       /* [capacity] frame index of each overflow slot */
    const int32_t *running;             /* [max_iter + 2] frames still running after round i */
    uint64_t *done;                     /* [T + TO][V] */
    int32_t *iters;                     /* [T + TO][F] */
    void *Q;                            /* [T + TO][E][F] */
    void *chan;                         /* [T + TO][N][F] */
    uint64_t *hard;                     /* [T + TO][N][V] */
    int64_t E;
    int64_t frames;
    int32_t N;
    int32_t tiles;                      /* batch tiles in use by this call */
    int32_t base_tile;                  /* first overflow tile */
    int32_t capacity;                   /* overflow slots */
    int32_t threshold;
    int32_t iter;
    int32_t max_iter;
};

constexpr int kTailMaxWords = 4096;     /* mask words a block can list: 262144 frames */

template <int V, typename T>
__global__ __launch_bounds__(kBlock) void tail_gather_kernel(const TailArgs a)
{
    constexpr int F = 64 * V;
    __shared__ int32_t s_map[kCompactCapacity];
    __shared__ int32_t s_scan[kBlock];
    const int running = a.running[a.iter];
    if (a.state[0] || running <= 0 || running > a.threshold || (int64_t)running * 4 > a.frames) return;   /* uniform */
    const int words = a.tiles * V;
    /* list the running frames: thread t owns words t, t + 256, ... (ascending); exclusive scan of the
     * per-thread counts over consecutive word ranges keeps the order ascending in (word, bit) */
    const int per = (words + kBlock - 1) / kBlock;
    const int w0 = min((int)threadIdx.x * per, words), w1 = min(w0 + per, words);
    int mine = 0;
    for (int w = w0; w < w1; ++w) mine += __popcll(~a.done[w]);
    s_scan[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
        const int v = threadIdx.x >= off ? s_scan[threadIdx.x - off] : 0;
        __syncthreads();
        s_scan[threadIdx.x] += v;
        __syncthreads();
    }
    int slot = s_scan[threadIdx.x] - mine;
    const int count = s_scan[kBlock - 1];
    for (int w = w0; w < w1; ++w) {
        uint64_t m = ~a.done[w];
        const int tile = w / V, v = w % V;
        while (m) {
            const int l = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            if (slot < a.capacity) s_map[slot] = tile * F + l * V + v;      /* bit l of word v = frame V*l+v */
            ++slot;
        }
    }
    __syncthreads();
    if (count > a.capacity || count != running) return;      /* cannot happen: both come from the same masks */
    const int ctiles = (count + F - 1) / F;
    /* rows of Q (E), of the channel array (N) and of the hard masks (N), dealt over the blocks */
    const int64_t total_rows = a.E + 2 * (int64_t)a.N;
    for (int64_t row = blockIdx.x; row < total_rows; row += gridDim.x) {
        if (row < a.E + a.N) {
            const bool isq = row < a.E;
            const int64_t i = isq ? row : row - a.E, rows = isq ? a.E : a.N;
            T *arr = static_cast<T *>(isq ? a.Q : a.chan);
            for (int j = threadIdx.x; j < ctiles * F; j += kBlock) {
                T val = (T)0;
                if (j < count) {
                    const int64_t f = s_map[j];
                    val = arr[((f / F) * rows + i) * F + (f % F)];
                }
                arr[((size_t)(a.base_tile + j / F) * rows + i) * F + (j % F)] = val;
            }
        } else {
            const int64_t n = row - a.E - a.N;
            /* wave-wise: lane l of pass (ct, v) holds slot ct*F + V*l + v = bit l of word v */
            const int lane = threadIdx.x & 63;
            for (int unit = threadIdx.x >> 6; unit < ctiles * V; unit += kWavesPerBlock) {
                const int ct = unit / V, v = unit % V;
                const int j = ct * F + V * lane + v;
                bool bit = false;
                if (j < count) {
                    const int64_t f = s_map[j];
                    const int fi = (int)(f % F);
                    bit = (a.hard[((f / F) * a.N + n) * V + fi % V] >> (fi / V)) & 1ull;
                }
                const uint64_t w = __ballot(bit);
                if (lane == 0) a.hard[((size_t)(a.base_tile + ct) * a.N + n) * V + v] = w;
            }
        }
    }
    /* the last block to finish commits the hand-over */
    __threadfence();
    __shared__ int s_last;
    if (threadIdx.x == 0) s_last = (atomicAdd(&a.state[3], 1) == (int)gridDim.x - 1);
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    for (int j = threadIdx.x; j < count; j += kBlock) a.map[j] = s_map[j];
    for (int w = threadIdx.x; w < words; w += kBlock) a.done[w] = ~0ull;
    const int TOv = (a.capacity / F) * V;
    for (int w = threadIdx.x; w < TOv; w += kBlock) {
        /* overflow word (ct, v): bit l in use iff slot ct*F + V*l + v < count */
        const int ct = w / V, v = w % V;
        uint64_t used = 0;
        for (int l = 0; l < 64; ++l)
            if (ct * F + V * l + v < count) used |= 1ull << l;
        a.done[(size_t)a.base_tile * V + w] = ~used;
    }
    for (int j = threadIdx.x; j < a.capacity; j += kBlock) a.iters[(size_t)a.base_tile * F + j] = a.max_iter;
    __threadfence();
    if (threadIdx.x == 0) { a.state[1] = count; a.state[2] = a.iter; a.state[0] = 1; }
}

/* bits, iteration counts and converged flags of the handed-over frames back into the batch's tiles */
template <int V> __global__ __launch_bounds__(kBlock) void tail_scatter_kernel(const TailArgs a)
{
    constexpr int F = 64 * V;
    if (!a.state[0]) return;
    const int count = a.state[1];
    const int64_t n0 = (int64_t)blockIdx.x * kWavesPerBlock + wave_id_in_block();
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0) {
        for (int j = threadIdx.x; j < count; j += kBlock) {
            const int64_t f = a.map[j];
            const int fi = (int)(f % F), oj = j % F;
            a.iters[f] = a.iters[(size_t)a.base_tile * F + j];
            const bool conv = (a.done[(size_t)(a.base_tile + j / F) * V + oj % V] >> (oj / V)) & 1ull;
            /* the batch's word says "finished" for every frame since the hand-over: clear it for a
             * frame that never reached a clean syndrome */
            if (!conv) atomicAnd(reinterpret_cast<unsigned long long *>(a.done) + (f / F) * V + fi % V, ~(1ull << (fi / V)));
        }
    }
    for (int64_t n = n0; n < a.N; n += (int64_t)gridDim.x * kWavesPerBlock) {
        for (int j = lane; j < count; j += 64) {
            const int64_t f = a.map[j];
            const int fi = (int)(f % F), oj = j % F;
            const bool bit = (a.hard[((size_t)(a.base_tile + j / F) * a.N + n) * V + oj % V] >> (oj / V)) & 1ull;
            unsigned long long *word = reinterpret_cast<unsigned long long *>(a.hard) + ((f / F) * a.N + n) * V + fi % V;
            if (bit) atomicOr(word, 1ull << (fi / V));
            else atomicAnd(word, ~(1ull << (fi / V)));
        }
    }
}

}  // namespace ldpc
