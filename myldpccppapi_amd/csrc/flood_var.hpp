/*
 * flood_var.hpp -- the variable node of the streaming flooding decoders: var_sp, the unrolled column loop
 * (var_columns), var_kernel, the bucket launch (var_group_kernel) and the run-time-degree kernel.
 */
#pragma once

#include "flood_common.hpp"

namespace ldpc {

/* Sum-product variable node: hardDecision (decodeCL.c:72-82) and refreshQ
 * (:52-61) share the prefix products.  d[k] is the stored r0-r1 of edge k;
 * r0 = (1+d)/2, r1 = (1-d)/2 (:39-40; the halving is exact).  t = exp(scale*y),
 * priors t/(1+t) and 1/(1+t) (:9-11).  Returns q0-q1 per edge in outq and the
 * full products in full0/full1. */
template <int D, int V>
__device__ __forceinline__ void var_sp(const float (&t)[V], const float (&d)[D][V],
                                       float (&outq)[D][V], float (&full0)[V], float (&full1)[V])
{
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const float den = 1.0f + t[v];
        float pre0 = t[v] / den;
        float pre1 = 1.0f / den;
        float r0[D], r1[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            r0[k] = (1.0f + d[k][v]) * 0.5f;
            r1[k] = (1.0f - d[k][v]) * 0.5f;
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            float t0 = pre0, t1 = pre1;
#pragma unroll
            for (int j = k + 1; j < D; ++j) { t0 *= r0[j]; t1 *= r1[j]; }
            const float s = t0 + t1;
            const float q0 = t0 / s;
            const float q1 = t1 / s;
            outq[k][v] = q0 - q1;
            pre0 *= r0[k];
            pre1 *= r1[k];
        }
        full0[v] = pre0;
        full1[v] = pre1;
    }
}

/* The variable node keeps WIDE waves (V values per lane, whole 64*V-frame segments per
 * wave-instruction): narrow waves as in check_kernel were measured 10 % slower here
 * (1.69 vs 1.53 ms per round at B = 4096), 2 values per lane no faster (1.11 vs 1.12 ms) --
 * the gather prefers fewer, larger requests.  Segments twice as large would not help either:
 * tools/gather_probe.hip moves this exact traffic at 94-95 % of the box's copy rate with 1-, 2- and
 * 4-KiB segments alike (profiles/r02_gather_probe.txt). */
template <int ALGO, int D, int V, typename T>
__device__ __forceinline__ void var_columns(const T *Rt, T *Qt, const T *chan_t, uint64_t *hard_t, const uint64_t (&frozen)[V],
                                            const int32_t *__restrict__ cls_col, const int32_t *__restrict__ cls_edge,
                                            int c_begin, int c_end, int write_q, int lane, int64_t q_base, int n_cls)
{
    constexpr size_t F = 64 * V;
    for (int ci = c_begin; ci < c_end; ++ci) {
        const int n = cls_col[ci];
        int e[D];
#pragma unroll
        for (int k = 0; k < D; ++k) e[k] = cls_edge[(size_t)ci * D + k];
        float ch[V], r[D][V], q[D][V];
        vload<V>(ch, chan_t + (size_t)n * F);
#pragma unroll
        for (int k = 0; k < D; ++k) vload<V>(r[k], Rt + (size_t)e[k] * F);
        uint64_t old_w[V], new_w[V];
#pragma unroll
        for (int v = 0; v < V; ++v) old_w[v] = hard_t[(size_t)n * V + v];

        if (ALGO == kAlgoSP) {
            float f0[V], f1[V];
            var_sp<D, V>(ch, r, q, f0, f1);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                /* decodeCL.c:78-82: ties and NaN keep the previous bit.  The old bit is read unconditionally: a
                 * branch in place of this select cost var_kernel<sp, 8, 4> 17 instructions and 0.6 % of its time. */
                const bool oldb = (old_w[v] >> lane) & 1ull;
                const bool b = (f0[v] > f1[v]) ? false : ((f0[v] < f1[v]) ? true : oldb);
                new_w[v] = __ballot(b);
            }
        } else {
            /* refreshPostPMS decodeCL.c:157-166, refreshQMS :185 */
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float p = ch[v];
#pragma unroll
                for (int k = 0; k < D; ++k) p += r[k][v];
#pragma unroll
                for (int k = 0; k < D; ++k) q[k][v] = p - r[k][v];
                new_w[v] = __ballot(!(p > 0.0f));
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int v = 0; v < V; ++v)
                hard_t[(size_t)n * V + v] = (old_w[v] & frozen[v]) | (new_w[v] & ~frozen[v]);
        }
        if (write_q) {
            if (q_base >= 0) {
                T *Qc = Qt + ((size_t)q_base + (size_t)ci) * F;            /* this column's slot in stream 0 */
#pragma unroll
                for (int k = 0; k < D; ++k) vstore<V>(Qc + (size_t)k * (size_t)n_cls * F, q[k]);
            } else {
#pragma unroll
                for (int k = 0; k < D; ++k) vstore<V>(Qt + (size_t)e[k] * F, q[k]);
            }
        }
    }
}

/* The three kernels below open with the same tile prologue (this lane's V values of every R, Q and channel segment,
 * the tile's hard masks and frozen frames), written out in each: behind a helper the compiler schedules it
 * differently, and these are kernels the step time rests on. */

/* build-time experiment hook: -DLDPC_VAR_WAVES=n asks the compiler for n waves per SIMD */
#ifdef LDPC_VAR_WAVES
#define LDPC_VAR_ATTR __attribute__((amdgpu_waves_per_eu(LDPC_VAR_WAVES, LDPC_VAR_WAVES)))
#else
#define LDPC_VAR_ATTR
#endif
template <int ALGO, int D, int V, typename T>
__global__ __launch_bounds__(kBlock) LDPC_VAR_ATTR void var_kernel(const VarArgs a)
{
    constexpr size_t F = 64 * V;
    const int lane = threadIdx.x & 63;
    const GridPos gp = grid_pos(a.tiles_first);
    const int tile = tile_select<V>(a.tail, a.done, gp.row);
    if (tile < 0) return;
    const int wave = gp.block * kWavesPerBlock + wave_id_in_block();
    const int c_begin = wave * a.cols_per_wave;
    const int c_end = min(c_begin + a.cols_per_wave, a.n_cols);
    const T *Rt = static_cast<const T *>(a.R) + (size_t)tile * (size_t)a.E * F + (size_t)lane * V;
    T *Qt = static_cast<T *>(a.Q) + (size_t)tile * (size_t)a.E * F + (size_t)lane * V;
    const T *chan_t = static_cast<const T *>(a.chan) + (size_t)tile * (size_t)a.N * F + (size_t)lane * V;
    uint64_t *hard_t = a.hard + (size_t)tile * (size_t)a.N * V;
    uint64_t frozen[V];
#pragma unroll
    for (int v = 0; v < V; ++v) frozen[v] = a.done[(size_t)tile * V + v];
    var_columns<ALGO, D, V, T>(Rt, Qt, chan_t, hard_t, frozen, a.cls_col, a.cls_edge, c_begin, c_end, a.write_q, lane, a.q_base, a.n_cols);
}

template <int ALGO, int V, typename T, int D, int DLO> struct VarDispatch {
    static __device__ __forceinline__ void run(int deg, const T *Rt, T *Qt, const T *chan_t, uint64_t *hard_t,
                                               const uint64_t (&frozen)[V], const int32_t *col, const int32_t *edge,
                                               int cb, int ce, int write_q, int lane, int64_t q_base, int n_cls)
    {
        if (deg == D) var_columns<ALGO, D, V, T>(Rt, Qt, chan_t, hard_t, frozen, col, edge, cb, ce, write_q, lane, q_base, n_cls);
        else VarDispatch<ALGO, V, T, D - 1, DLO>::run(deg, Rt, Qt, chan_t, hard_t, frozen, col, edge, cb, ce, write_q, lane, q_base, n_cls);
    }
};
template <int ALGO, int V, typename T, int DLO> struct VarDispatch<ALGO, V, T, DLO, DLO> {
    static __device__ __forceinline__ void run(int, const T *Rt, T *Qt, const T *chan_t, uint64_t *hard_t,
                                               const uint64_t (&frozen)[V], const int32_t *col, const int32_t *edge,
                                               int cb, int ce, int write_q, int lane, int64_t q_base, int n_cls)
    {
        var_columns<ALGO, DLO, V, T>(Rt, Qt, chan_t, hard_t, frozen, col, edge, cb, ce, write_q, lane, q_base, n_cls);
    }
};

/* every column class of the degree bucket DLO..DHI in one launch (GroupClass table above) */
template <int ALGO, int V, typename T, int DLO, int DHI>
__global__ __launch_bounds__(kBlock) void var_group_kernel(const VarArgs a, const GroupClass *__restrict__ cls, int n_classes)
{
    constexpr size_t F = 64 * V;
    const int lane = threadIdx.x & 63;
    const GridPos gp = grid_pos(a.tiles_first);
    const int tile = tile_select<V>(a.tail, a.done, gp.row);
    if (tile < 0) return;
    int c = 0;
    while (c + 1 < n_classes && gp.block >= cls[c + 1].block_begin) ++c;
    const int wave = (gp.block - cls[c].block_begin) * kWavesPerBlock + wave_id_in_block();
    const int c_begin = wave * a.cols_per_wave;
    const int c_end = min(c_begin + a.cols_per_wave, cls[c].count);
    const T *Rt = static_cast<const T *>(a.R) + (size_t)tile * (size_t)a.E * F + (size_t)lane * V;
    T *Qt = static_cast<T *>(a.Q) + (size_t)tile * (size_t)a.E * F + (size_t)lane * V;
    const T *chan_t = static_cast<const T *>(a.chan) + (size_t)tile * (size_t)a.N * F + (size_t)lane * V;
    uint64_t *hard_t = a.hard + (size_t)tile * (size_t)a.N * V;
    uint64_t frozen[V];
#pragma unroll
    for (int v = 0; v < V; ++v) frozen[v] = a.done[(size_t)tile * V + v];
    VarDispatch<ALGO, V, T, DHI, DLO>::run(cls[c].degree, Rt, Qt, chan_t, hard_t, frozen, cls[c].ids, cls[c].edges,
                                           c_begin, c_end, a.write_q, lane, cls[c].q_base, cls[c].count);
}

template <int ALGO, int V, typename T>
__global__ __launch_bounds__(kBlock) void var_kernel_generic(const VarArgs a)
{
    constexpr size_t F = 64 * V;
    const int lane = threadIdx.x & 63;
    const GridPos gp = grid_pos(a.tiles_first);
    const int tile = tile_select<V>(a.tail, a.done, gp.row);
    if (tile < 0) return;
    const int wave = gp.block * kWavesPerBlock + wave_id_in_block();
    const int c_begin = wave * a.cols_per_wave;
    const int c_end = min(c_begin + a.cols_per_wave, a.n_cols);
    const int D = a.degree;
    const T *Rt = static_cast<const T *>(a.R) + (size_t)tile * (size_t)a.E * F + (size_t)lane * V;
    T *Qt = static_cast<T *>(a.Q) + (size_t)tile * (size_t)a.E * F + (size_t)lane * V;
    const T *chan_t = static_cast<const T *>(a.chan) + (size_t)tile * (size_t)a.N * F + (size_t)lane * V;
    uint64_t *hard_t = a.hard + (size_t)tile * (size_t)a.N * V;
    uint64_t frozen[V];
#pragma unroll
    for (int v = 0; v < V; ++v) frozen[v] = a.done[(size_t)tile * V + v];

    for (int ci = c_begin; ci < c_end; ++ci) {
        const int n = a.cls_col[ci];
        const int32_t *e = a.cls_edge + (size_t)ci * D;
        auto qs = [&](int k) -> size_t { return a.q_base >= 0 ? (size_t)a.q_base + (size_t)k * a.n_cols + ci : (size_t)e[k]; };
        float ch[V];
        vload<V>(ch, chan_t + (size_t)n * F);
        uint64_t old_w[V], new_w[V];
#pragma unroll
        for (int v = 0; v < V; ++v) old_w[v] = hard_t[(size_t)n * V + v];
        if (ALGO == kAlgoSP) {
            float p0[V], p1[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float den = 1.0f + ch[v];
                p0[v] = ch[v] / den;
                p1[v] = 1.0f / den;
            }
            for (int k = 0; k <= D; ++k) {     /* k == D: the full product (hard decision) */
                float t0[V], t1[V];
#pragma unroll
                for (int v = 0; v < V; ++v) { t0[v] = p0[v]; t1[v] = p1[v]; }
                for (int j = 0; j < D; ++j) {
                    if (j == k) continue;
                    float dj[V];
                    vload<V>(dj, Rt + (size_t)e[j] * F);
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        t0[v] *= (1.0f + dj[v]) * 0.5f;
                        t1[v] *= (1.0f - dj[v]) * 0.5f;
                    }
                }
                if (k < D) {
                    if (a.write_q) {
                        float o[V];
#pragma unroll
                        for (int v = 0; v < V; ++v) {
                            const float s = t0[v] + t1[v];
                            o[v] = t0[v] / s - t1[v] / s;
                        }
                        vstore<V>(Qt + qs(k) * F, o);
                    }
                } else {
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const bool oldb = (old_w[v] >> lane) & 1ull;
                        const bool b = (t0[v] > t1[v]) ? false : ((t0[v] < t1[v]) ? true : oldb);
                        new_w[v] = __ballot(b);
                    }
                }
            }
        } else {
            float p[V];
#pragma unroll
            for (int v = 0; v < V; ++v) p[v] = ch[v];
            for (int j = 0; j < D; ++j) {
                float rj[V];
                vload<V>(rj, Rt + (size_t)e[j] * F);
#pragma unroll
                for (int v = 0; v < V; ++v) p[v] += rj[v];
            }
#pragma unroll
            for (int v = 0; v < V; ++v) new_w[v] = __ballot(!(p[v] > 0.0f));
            if (a.write_q) {
                for (int j = 0; j < D; ++j) {
                    float rj[V], o[V];
                    vload<V>(rj, Rt + (size_t)e[j] * F);
#pragma unroll
                    for (int v = 0; v < V; ++v) o[v] = p[v] - rj[v];
                    vstore<V>(Qt + qs(j) * F, o);
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int v = 0; v < V; ++v)
                hard_t[(size_t)n * V + v] = (old_w[v] & frozen[v]) | (new_w[v] & ~frozen[v]);
        }
    }
}

}  // namespace ldpc
