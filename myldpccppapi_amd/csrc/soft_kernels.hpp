/*
 * soft_kernels.hpp -- soft output of the streaming decoders (ldpc_decode_soft_device): the one launch a round gains
 * between the CRC test and state_kernel, and the small launches around it.
 *
 * The rule (include/ldpc_hip.h) is stated per frame: a frame's posterior is that of the round it froze in, the one its
 * output bits were decided from.  The streaming engines let a frozen frame's messages and posteriors keep evolving
 * unread, so the value is caught in that round and never recomputed at the end.  When soft_settle_kernel runs in round
 * i, `done` still holds the frames frozen BEFORE round i and `fail` this round's verdict (syndrome, then CRC): the
 * frames that settle now are ~done & ~fail -- in the last round that is launched, and without early termination, all of
 * ~done.  Every frame settles in exactly one round, so every value of the caller's buffer is written exactly once.
 *
 *   flooding min-sum : p = y + R_e1 + R_e2 + ..., fp32, one add at a time in ascending edge id along the column, y and R
 *                      widened from their storage first: the sum var_columns (flood_var.hpp) decided the bit from.  R_i
 *                      is still in place, the variable-node kernels only read it.
 *   layered          : p = P[n], the posterior after the round's last layer.
 *   extrinsic        : p - y, one fp32 subtraction; y as the decoder read it (flooding: the channel array, rounded to
 *                      fp16 with fp16 messages; layered: the caller's channel values).
 *
 * Loads are per-lane segments predicated on the settling mask, so only the 128-byte lines that hold a settling frame are
 * fetched.  The store is the mirror image of init_kernel's transpose: a patch of kInitCols columns x F frames crosses LDS
 * and leaves as runs of kInitCols consecutive floats per frame (4-byte stores N floats apart would make every value a
 * memory transaction of its own).  A tile without a settling frame leaves at kernel entry.
 */
#pragma once

#include "flood_round.hpp"

namespace ldpc {

struct SoftArgs {
    const void *__restrict__ chan;        /* flooding: [T][N][F] channel values (T); layered: P [T][N][F] (float) */
    const void *__restrict__ R;           /* flooding: [T][E][F] (T); layered: nullptr */
    const int32_t *__restrict__ col_ptr;  /* [N+1] */
    const int32_t *__restrict__ col_edge; /* [E] edge ids of every column, ascending */
    const uint64_t *__restrict__ done;    /* [T][V] frames frozen before this round */
    const uint64_t *__restrict__ fail;    /* [T][V] this round's verdict; nullptr: every running frame settles */
    float *__restrict__ soft;             /* [frames][N] the caller's buffer, frame-major */
    const void *__restrict__ llr;         /* layered, extrinsic: the caller's channel values [frames][N], elements of IN */
    const int32_t *__restrict__ fmap;     /* a hand-over child: slot -> frame of the caller's batch; nullptr: identity */
    const int32_t *__restrict__ tail_map; /* device-side tail: overflow slot -> frame (flood_handover.hpp) */
    int64_t E;
    int64_t frames;                       /* frames (slots) of this decoder's call */
    int32_t N;
    int32_t extrinsic;
    TailRef tail;
    float llr_unit;                       /* layered, extrinsic, narrow IN: y = (float)x * llr_unit (llr_input.hpp) */
};

/* grid (ceil(N / kInitCols), tiles), block kBlock.  T: storage type of the flooding messages; the layered form is
 * soft_settle_kernel<V, float> with R == nullptr.  IN: element type of the caller's channel values, which only the layered
 * extrinsic form reads: y is the product x * llr_unit of a narrow element, formed first. */
template <int V, typename T, typename IN = float>
__global__ __launch_bounds__(kBlock) void soft_settle_kernel(const SoftArgs a)
{
    constexpr int F = 64 * V;
    constexpr int LD = F + 1;
    __shared__ float patch[kInitCols * LD];
    const int tile = tile_select<V>(a.tail, a.done, (int)blockIdx.y);
    if (tile < 0) return;
    uint64_t settle[V];
    bool any = false;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        settle[v] = ~a.done[(size_t)tile * V + v];
        if (a.fail) settle[v] &= ~a.fail[(size_t)tile * V + v];
        any = any || settle[v] != 0ull;
    }
    if (!any) return;                   /* block-uniform */
    const int n0 = blockIdx.x * kInitCols;
    const int lane = threadIdx.x & 63;
    bool mine = false;                  /* one of this lane's V frames settles */
#pragma unroll
    for (int v = 0; v < V; ++v) mine = mine || ((settle[v] >> lane) & 1ull);
    const T *chan_t = static_cast<const T *>(a.chan) + (size_t)tile * (size_t)a.N * F + (size_t)lane * V;
    const T *Rt = static_cast<const T *>(a.R) + (size_t)tile * (size_t)a.E * F + (size_t)lane * V;
    for (int c = threadIdx.x >> 6; c < kInitCols; c += kWavesPerBlock) {
        const int n = n0 + c;
        if (n >= a.N) break;
        if (!mine) continue;
        float y[V], p[V];
        vload<V>(y, chan_t + (size_t)n * F);
#pragma unroll
        for (int v = 0; v < V; ++v) p[v] = y[v];
        if (a.R) {
            const int p0 = a.col_ptr[n], p1 = a.col_ptr[n + 1];
            for (int k = p0; k < p1; ++k) {
                const int e = __builtin_amdgcn_readfirstlane(a.col_edge[k]);
                float r[V];
                vload<V>(r, Rt + (size_t)e * F);
#pragma unroll
                for (int v = 0; v < V; ++v) p[v] += r[v];
            }
            if (a.extrinsic) {
#pragma unroll
                for (int v = 0; v < V; ++v) p[v] = p[v] - y[v];
            }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) patch[c * LD + lane * V + v] = p[v];
    }
    __syncthreads();
    /* frame f of the tile is bit f / V of word f % V; where it lives in the caller's batch */
    const bool over = a.tail.state && tile >= a.tail.base_tile;
    const int c = threadIdx.x & (kInitCols - 1);
    const int n = n0 + c;
    if (n >= a.N) return;
    for (int f = threadIdx.x / kInitCols; f < F; f += kBlock / kInitCols) {
        if (!((settle[f % V] >> (f / V)) & 1ull)) continue;
        int64_t frame = over ? (int64_t)(tile - a.tail.base_tile) * F + f : (int64_t)tile * F + f;
        if (frame >= (over ? (int64_t)a.tail.n_tiles * F : a.frames)) continue;
        if (over) frame = a.tail_map[frame];
        else if (a.fmap) frame = a.fmap[frame];
        float p = patch[c * LD + f];
        if (!a.R && a.extrinsic) p = p - llr_value<IN>(static_cast<const IN *>(a.llr)[(size_t)frame * a.N + n], a.llr_unit);
        a.soft[(size_t)frame * a.N + n] = p;
    }
}

/* one-launch kernels: they write the posterior of the round a frame stopped in themselves (FusedArgs / LdspArgs::dump_p);
 * the extrinsic value is one pass over the caller's two frame-major buffers afterwards */
template <int kUnused = 0>
__global__ __launch_bounds__(kBlock) void soft_extrinsic_kernel(float *__restrict__ soft, const float *__restrict__ llr, int64_t count)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < count) soft[i] = soft[i] - llr[i];
}

/* a hand-over child's slots in terms of the caller's frames: dst[j] = up ? up[cmap[j]] : cmap[j] */
template <int kUnused = 0>
__global__ __launch_bounds__(kBlock) void soft_map_kernel(int32_t *__restrict__ dst, const int32_t *__restrict__ cmap,
                                                          const int32_t *__restrict__ up, int32_t count)
{
    const int j = (int)blockIdx.x * kBlock + threadIdx.x;
    if (j >= count) return;
    const int32_t f = cmap[j];
    dst[j] = up ? up[f] : f;
}

}  // namespace ldpc
