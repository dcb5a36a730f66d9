/*
 * flood_round.hpp -- the kernels of a round that move no messages: input transpose and initialisation,
 * syndrome, frame state, output packing.
 */
#pragma once

#include "flood_common.hpp"
#include "ldpc_expf.h"
#include "llr_input.hpp"

namespace ldpc {

struct InitArgs {
    const void *__restrict__ llr;         /* [frames][N] frame-major (reference layout), elements of the kernel's IN */
    void *__restrict__ chan;              /* [T][N][F] (float or fp16) */
    void *__restrict__ Q;                 /* [T][E][F] */
    uint64_t *__restrict__ hard;          /* [T][N][V] */
    const int32_t *__restrict__ col_ptr;  /* [N+1] */
    const int32_t *__restrict__ col_edge; /* [E] */
    int64_t E;
    int64_t frames;
    int32_t N;
    float llr_scale;
    float llr_unit;                       /* narrow IN: y = (float)x * llr_unit (llr_input.hpp); unused for float */
};

/* decodeInit (decodeCL.c:3-22) / decodeInitMS (:113-124) + the transpose from the
 * reference's frame-major input to the tile layout.  One block = 32 columns x one
 * tile; the patch crosses LDS so both the read (along n) and the writes (along
 * frames) are contiguous.  Frames past `frames` are filled with y = +1.
 * IN: element type of the caller's buffer.  float is the kernel as it always was; int8_t and _Float16 read the
 * caller's rows directly (llr_patch_fill), cross LDS as floats and continue unchanged from patch[] on. */
constexpr int kInitCols = 32;

template <int ALGO, int V, typename T, typename IN = float>
__global__ __launch_bounds__(kBlock) void init_kernel(const InitArgs a)
{
    constexpr int F = 64 * V;
    constexpr int LD = F + 1;             /* +1 float: conflict-free column writes */
    __shared__ float patch[kInitCols * LD];
    const int tile = blockIdx.y;
    const int n0 = blockIdx.x * kInitCols;
    const IN *__restrict__ llr = static_cast<const IN *>(a.llr);
    if constexpr (!std::is_same<IN, float>::value) {
        llr_patch_fill<IN, F, LD, kInitCols, kBlock, false>(patch, llr, a.llr_unit, a.frames, a.N, tile, n0, 1.0f);
    } else if ((a.N & 3) == 0 && n0 + kInitCols <= a.N && (reinterpret_cast<uintptr_t>(llr) & 15) == 0) {
        /* 16-byte loads, all of a thread's F/32 requests in flight: 8 threads span the 32 columns
         * of a frame, 32 frames per pass */
        const int c4 = (threadIdx.x & 7) * 4, f0 = threadIdx.x >> 3;
        float4 vals[F / 32];
#pragma unroll
        for (int i = 0; i < F / 32; ++i) {
            const int64_t frame = (int64_t)tile * F + f0 + 32 * i;
            vals[i] = float4{1.0f, 1.0f, 1.0f, 1.0f};
            if (frame < a.frames) vals[i] = *reinterpret_cast<const float4 *>(llr + (size_t)frame * a.N + n0 + c4);
        }
#pragma unroll
        for (int i = 0; i < F / 32; ++i) {
            const int f = f0 + 32 * i;
            patch[(c4 + 0) * LD + f] = vals[i].x;
            patch[(c4 + 1) * LD + f] = vals[i].y;
            patch[(c4 + 2) * LD + f] = vals[i].z;
            patch[(c4 + 3) * LD + f] = vals[i].w;
        }
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
        float ch[V], q[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float y = patch[c * LD + lane * V + v];
            if (ALGO == kAlgoSP) {
                const float t = ldpc_expf(a.llr_scale * y);         /* decodeCL.c:9 */
                ch[v] = t;
                q[v] = t / (1.0f + t) - 1.0f / (1.0f + t);          /* :10-11, as q0-q1 */
            } else if (ALGO == kAlgoBP) {
                /* the LLR: one fp32 multiply; fp16 storage rounds the PRODUCT at the store.  The empty asm keeps the
                 * product a value of its own: folded into the conversion (v_fma_mixlo_f16) it is rounded once, from
                 * the exact product, and differs from the definition in the double-rounding cases */
                float t = a.llr_scale * y;
                asm volatile("" : "+v"(t));
                ch[v] = q[v] = t;
            } else {
                const float c = MsgChan<T>::of(y, a.llr_scale);     /* y; fixed point: llr_scale * y */
                ch[v] = c;                                          /* fp16 storage rounds it here */
                q[v] = c;                                           /* :121 */
            }
        }
        vstore<V>(static_cast<T *>(a.chan) + ((size_t)tile * a.N + n) * F + (size_t)lane * V, ch);
        if (a.Q) {      /* nullptr: round 1's check kernels read the channel values themselves (CheckArgs::first_chan) */
            /* the column's Q slots: one load by the wave's first lanes, a broadcast per store (a load per store
             * serialised the stores behind the index latency) */
            const int p0 = a.col_ptr[n], deg = a.col_ptr[n + 1] - p0;
            T *Qt = static_cast<T *>(a.Q) + (size_t)tile * (size_t)a.E * F + (size_t)lane * V;
            for (int k0 = 0; k0 < deg; k0 += 64) {
                const int m = min(64, deg - k0);
                const int mine = a.col_edge[p0 + k0 + (lane < m ? lane : m - 1)];
                for (int k = 0; k < m; ++k)
                    vstore<V>(Qt + (size_t)__builtin_amdgcn_readlane(mine, k) * F, q);
            }
        }
        if (lane < V) a.hard[((size_t)tile * a.N + n) * V + lane] = 0;
    }
}

/* checkResult, decodeCL.c:88-108, on the bit masks: one thread per row XORs the
 * 64-frame words of its columns (an L2-resident gather), a wave ORs its rows and
 * issues one atomic per word.  Runs after every variable-node round. */
struct SyndromeArgs {
    const int32_t *__restrict__ row_ptr;  /* [M+1] */
    const int32_t *__restrict__ edge_col; /* [E]   */
    const uint64_t *__restrict__ hard;    /* [T][N][V] */
    uint64_t *__restrict__ fail;          /* [T][V] */
    const uint64_t *__restrict__ done;    /* [T][V] */
    int32_t M, N;
    int32_t tiles;                        /* > 0: XCD-aware 1-D grid (see syndrome_kernel) */
    int32_t row_blocks;
    TailRef tail;
};

template <int V> __global__ __launch_bounds__(kBlock) void syndrome_kernel(const SyndromeArgs a)
{
    /* A tile's bit masks (N*V*8 B, 2 MB at V = 4) are re-read ~d_c times: keep them in ONE
     * XCD's L2.  Blocks are dealt round-robin over the 8 XCDs, so blocks with equal
     * blockIdx.x % 8 share an L2: block b serves tile (b % 8) + 8 * ((b / 8) / row_blocks).
     * (Speed only; any placement gives the same result.) */
    int tile, rb;
    if (a.tiles > 0) {
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        tile = xcd + 8 * (j / a.row_blocks);
        rb = j % a.row_blocks;
        if (tile >= a.tiles) return;
    } else {
        tile = blockIdx.y;
        rb = blockIdx.x;
    }
    tile = tile_select<V>(a.tail, a.done, tile);
    if (tile < 0) return;
    const int m = rb * kBlock + threadIdx.x;
    const uint64_t *hard_t = a.hard + (size_t)tile * (size_t)a.N * V;
    uint64_t s[V];
#pragma unroll
    for (int v = 0; v < V; ++v) s[v] = 0;
    if (m < a.M) {
        for (int p = a.row_ptr[m]; p < a.row_ptr[m + 1]; ++p) {
            const int c = a.edge_col[p];
#pragma unroll
            for (int v = 0; v < V; ++v) s[v] ^= hard_t[(size_t)c * V + v];
        }
    }
    /* OR over the wave, then over the block's 4 waves (LDS), then at most one atomic per
     * block and word -- and none when the bits are already set: every block of a tile ORs into
     * the same word, and same-address device atomics serialise chip-wide (this was 150 us per
     * round at B = 4096).  The plain pre-read may be stale; stale only costs a redundant atomic. */
    __shared__ uint64_t part[kWavesPerBlock][V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        uint64_t x = s[v];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const uint32_t lo = __shfl_xor((uint32_t)x, off);
            const uint32_t hi = __shfl_xor((uint32_t)(x >> 32), off);
            x |= ((uint64_t)hi << 32) | lo;
        }
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][v] = x;
    }
    __syncthreads();
    if (threadIdx.x < V) {
        uint64_t x = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) x |= part[w][threadIdx.x];
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(&a.fail[(size_t)tile * V + threadIdx.x]);
        const uint64_t seen = __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (x & ~seen) atomicOr(dst, (unsigned long long)x);
    }
}

struct StateArgs {
    uint64_t *__restrict__ done;        /* [T][V] */
    const uint64_t *__restrict__ fail;  /* [T][V] syndrome of round `iter` */
    int32_t *__restrict__ iters;        /* [T][F] */
    int32_t *__restrict__ active;       /* [1] += number of frames still running */
    int64_t frames;
    int32_t iter;                       /* round whose syndrome `fail` holds; 0 = initialise */
    int32_t max_iter;
    int32_t freeze;                     /* early_term */
    TailRef tail;
    int32_t *__restrict__ running;      /* [max_iter + 2] or nullptr: running[iter] += frames still running */
    int32_t *__restrict__ tile_rounds;  /* [1] or nullptr: += 1 per tile that still had a running frame when round `iter` began,
                                           i.e. whose kernels did not leave at entry (what the round's traffic is priced at) */
};

/* isDones bookkeeping (decodeCL.c:48-49, checkDones :296-300): a frame whose
 * syndrome is clean after round `iter` is frozen with iters = iter.
 * iter == 0 initialises: padding frames are born frozen, iters = max_iter. */
template <int V> __global__ void state_kernel(const StateArgs a)
{
    constexpr int F = 64 * V;
    int tile = blockIdx.x;
    if (a.tail.state && a.iter > 0 && a.tail.state[0]) {      /* handed over: only the overflow tiles live */
        if (tile >= a.tail.n_tiles) return;
        tile = a.tail.base_tile + tile;
    }
    const int lane = threadIdx.x;      /* 64 threads */
    int n_active = 0;
    bool worked = false;               /* some frame of the tile was running when this round began */
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int64_t frame = (int64_t)tile * F + (int64_t)lane * V + v;
        const bool valid = frame < a.frames;
        uint64_t d;
        if (a.iter == 0) {
            d = __ballot(!valid);
            a.iters[(size_t)tile * F + lane * V + v] = a.max_iter;
        } else {
            const uint64_t old = a.done[(size_t)tile * V + v];
            worked = worked || old != ~0ull;
            const uint64_t clean = ~a.fail[(size_t)tile * V + v];
            const uint64_t newly = clean & ~old;
            if ((newly >> lane) & 1ull) a.iters[(size_t)tile * F + lane * V + v] = a.iter;
            d = a.freeze ? (old | clean) : old;
        }
        if (lane == 0) a.done[(size_t)tile * V + v] = d;
        n_active += __popcll(~d);
    }
    if (lane == 0 && n_active && a.active) atomicAdd(a.active, n_active);
    if (lane == 0 && n_active && a.running) atomicAdd(&a.running[a.iter], n_active);
    if (lane == 0 && worked && a.tile_rounds) atomicAdd(a.tile_rounds, 1);
}

struct PackArgs {
    const uint64_t *__restrict__ hard;  /* [T][N][V] */
    uint8_t *__restrict__ out;          /* nullptr: no bytes are stored (iteration counts only) */
    const int32_t *__restrict__ iters_tile; /* [T][F] */
    int32_t *__restrict__ iters_out;    /* [frames] or nullptr */
    int64_t frames;
    int64_t out_bytes;
    int32_t N, K;
    int32_t pack_mode;
};

/* toChar, decodeCL.c:188-199: byte j of frame b = hard bits 8j..8j+7, LSB first,
 * at (b*K)/8 + j.  pack_mode 1 = decodeCPU's bit packing at bit b*K+i
 * (MyLdpc.cpp:765-774).
 * Bytes mode: a 64 x 64 bit transpose per wave.  One wave = 64 consecutive output bytes (lanes along
 * j) of the 64 frames of one tile slice v: each lane fetches its 8 hard words ONCE (64 frames' bits
 * of columns 8j..8j+7) and emits one byte per frame, 64 contiguous bytes per store.  (One thread
 * per output byte, the first version, re-read every hard word once per frame of the tile: 0.41 ms
 * for the 30 MB of a 4096-frame rate-9/10 batch.)  Grid: pack_grid<V>(). */
template <int V> inline dim3 pack_grid(int32_t K, int tiles)
{
    const int chunks = K / 8 > 0 ? (K / 8 + 63) / 64 : 1;
    return dim3((unsigned)((chunks * V + kWavesPerBlock - 1) / kWavesPerBlock), (unsigned)tiles);
}

template <int V> __global__ __launch_bounds__(kBlock) void pack_kernel(const PackArgs a)
{
    constexpr int F = 64 * V;
    if (a.pack_mode == 0) {
        const int tile = blockIdx.y;
        const int kb = a.K / 8;
        if (blockIdx.x == 0 && a.iters_out) {
            for (int f = threadIdx.x; f < F; f += kBlock) {
                const int64_t frame = (int64_t)tile * F + f;        /* tile-major index == frame index */
                if (frame < a.frames) a.iters_out[frame] = a.iters_tile[frame];
            }
        }
        if (!a.out) return;                 /* iteration counts only */
        const int unit = (int)blockIdx.x * kWavesPerBlock + wave_id_in_block();
        const int v = unit % V;
        const int j = (unit / V) * 64 + (threadIdx.x & 63);
        if (j >= kb) return;
        const uint64_t *h = a.hard + ((size_t)tile * a.N + (size_t)j * 8) * V + v;
        uint64_t w[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) w[b] = h[(size_t)b * V];
        for (int l = 0; l < 64; ++l) {
            const int64_t frame = (int64_t)tile * F + (int64_t)l * V + v;
            if (frame >= a.frames) break;
            unsigned byte = 0;
#pragma unroll
            for (int b = 0; b < 8; ++b) byte |= (unsigned)((w[b] >> l) & 1ull) << b;
            const int64_t off = frame * (int64_t)a.K / 8 + j;
            if (off < a.out_bytes) a.out[off] = (uint8_t)byte;
        }
    } else {
        const int64_t ob = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        if (ob < a.frames && a.iters_out) a.iters_out[ob] = a.iters_tile[ob];
        if (!a.out || ob >= a.out_bytes) return;
        unsigned byte = 0;
        for (int b = 0; b < 8; ++b) {
            const int64_t bit = ob * 8 + b;
            const int64_t frame = bit / a.K;
            if (frame >= a.frames) break;
            const int i = (int)(bit % a.K);
            const int64_t tile = frame / F;
            const int fi = (int)(frame % F);
            const uint64_t w = a.hard[((size_t)tile * a.N + i) * V + (fi % V)];
            byte |= (unsigned)((w >> (fi / V)) & 1ull) << b;
        }
        a.out[ob] = (uint8_t)byte;
    }
}

}  // namespace ldpc
