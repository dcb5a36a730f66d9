/*
 * flood_check.hpp -- the check node of the streaming flooding decoders: check_sp / check_ms / check_bp, the unrolled row
 * loop (check_rows), check_kernel, the run-time-degree row and kernel, the bucket launch (check_group_kernel).
 */
#pragma once

#include "flood_common.hpp"

namespace ldpc {

/* Sum-product, decodeCL.c:32-40: out_k = prod_{j != k} x_j, multiplied left to
 * right in ascending j starting from 1.0f (1*x is exact, so the chain starts at
 * the first factor).  The prefix x_0..x_{k-1} is shared between outputs. */
template <int D, int V>
__device__ __forceinline__ void check_sp(const float (&x)[D][V], float (&out)[D][V])
{
#pragma unroll
    for (int v = 0; v < V; ++v) {
        if (D == 1) { out[0][v] = 1.0f; continue; }
        {
            float p = x[1][v];
#pragma unroll
            for (int j = 2; j < D; ++j) p *= x[j][v];
            out[0][v] = p;
        }
        float pre = x[0][v];
#pragma unroll
        for (int k = 1; k < D; ++k) {
            float p = pre;
#pragma unroll
            for (int j = k + 1; j < D; ++j) p *= x[j][v];
            out[k][v] = p;
            pre *= x[k][v];
        }
    }
}

/* Min-sum, decodeCL.c:132-146: sign = XOR of (x_j < 0) over j != k, magnitude =
 * fmin chain over |x_j| starting at 1000.  min is exact and order-free, so the
 * two-smallest form gives the same floats; NaNs are skipped as fmin skips them.
 * CORR: the candidates go through ms_corr<T> first; plain: through MsgStart<T> (fp8: the start value reads 448). */
template <int D, int V, bool CORR = false, typename T = float>
__device__ __forceinline__ void check_ms(const float (&x)[D][V], float (&out)[D][V], MsCorr c = MsCorr{1.0f, 0.0f})
{
#pragma unroll
    for (int v = 0; v < V; ++v) {
        float m1 = 1000.0f, m2 = 1000.0f;
        int idx = -1;
        unsigned par = 0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const float a = __builtin_fabsf(x[j][v]);
            par ^= (x[j][v] < 0.0f) ? 1u : 0u;
            if (a < m1) { m2 = m1; m1 = a; idx = j; }
            else if (a < m2) { m2 = a; }
        }
        if (CORR) { m1 = ms_corr<T>(m1, c); m2 = ms_corr<T>(m2, c); }
        else { m1 = MsgStart<T>::of(m1); m2 = MsgStart<T>::of(m2); }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const float b = (k == idx) ? m2 : m1;
            const unsigned s = par ^ ((x[k][v] < 0.0f) ? 1u : 0u);
            out[k][v] = s ? -b : b;
        }
    }
}

/* Log-domain sum-product (LDPC_ALGO_BP, include/ldpc_hip.h has the rule bit for bit): fp32, one operation at a time.
 * bp_clamp: a row's input as the row reads it -- |x| capped at min-sum's start value 1000, so NaN reads +1000 (fminf
 * drops it, its sign is +), -0 reads +0, +-inf read +-1000.  From there on every value is finite. */
__device__ __forceinline__ float bp_clamp(float x)
{
    const float a = fminf(__builtin_fabsf(x), 1000.0f);
    return (x < 0.0f) ? -a : a;
}
/* the linear stand-in for log1p(exp(-x)): ln 2 at 0, 0 from 4 ln 2 on.  0.25f * x is exact (a power of two; where it
 * underflows, x < 2^-124 and both forms give ln 2), so the fused multiply-add rounds the very number the definition's
 * multiply and subtract round: same bits, one instruction less -- the fp16 check kernels are bound by these (8k) */
__device__ __forceinline__ float bp_corr(float x) { return fmaxf(__builtin_fmaf(-0.25f, x, 0.6931472f), 0.0f); }
/* u [+] v = sign * max(min(|u|, |v|) + c(|u| + |v|) - c(||u| - |v||), 0): bitwise commutative, not associative */
__device__ __forceinline__ float bp_boxplus(float u, float v)
{
    const float au = __builtin_fabsf(u), av = __builtin_fabsf(v);
    const float m = fminf(au, av);
    const float s = au + av;
    const float d = __builtin_fabsf(au - av);
    const float g = fmaxf((m + bp_corr(s)) - bp_corr(d), 0.0f);
    return ((u < 0.0f) != (v < 0.0f)) ? -g : g;
}

/* A row of degree D: forward chain f_j = f_{j-1} [+] t_j from the left, backward chain b_j = t_j [+] b_{j+1} from the
 * right, out_k = f_{k-1} [+] b_{k+1} -- 3 (D - 2) box-plus operations.  The association is part of the definition.  The
 * backward values are kept (D registers per value next to the inputs), the forward value is carried.  The result is
 * rounded to the storage type here, where it is produced (MsgRound): the column-fused kernels keep some R in registers. */
template <int D, int W, typename T>
__device__ __forceinline__ void check_bp(const float (&x)[D][W], float (&out)[D][W])
{
#pragma unroll
    for (int w = 0; w < W; ++w) {
        float t[D];
#pragma unroll
        for (int j = 0; j < D; ++j) t[j] = bp_clamp(x[j][w]);
        if constexpr (D == 1) {
            out[0][w] = MsgRound<T>::of(1000.0f);
        } else if constexpr (D == 2) {
            out[0][w] = MsgRound<T>::of(t[1]);
            out[1][w] = MsgRound<T>::of(t[0]);
        } else {
            float b[D];
            b[D - 1] = t[D - 1];
#pragma unroll
            for (int j = D - 2; j >= 1; --j) b[j] = bp_boxplus(t[j], b[j + 1]);
            out[0][w] = MsgRound<T>::of(b[1]);
            float f = t[0];
#pragma unroll
            for (int k = 1; k <= D - 2; ++k) {
                out[k][w] = MsgRound<T>::of(bp_boxplus(f, b[k + 1]));
                f = bp_boxplus(f, t[k]);
            }
            out[D - 1][w] = MsgRound<T>::of(f);
        }
    }
}

/* the check node of one row in arithmetic ALGO: W values per lane, c = the min-sum correction (kAlgoMSC only) */
template <int ALGO, int D, int W, typename T>
__device__ __forceinline__ void check_node(const float (&x)[D][W], float (&out)[D][W], const MsCorr &c)
{
    if (ALGO == kAlgoSP) check_sp<D, W>(x, out);
    else if (ALGO == kAlgoBP) check_bp<D, W, T>(x, out);
    else if (ALGO == kAlgoMS) check_ms<D, W, false, T>(x, out);
    else check_ms<D, W, true, T>(x, out, c);
}

/* rows [r_begin, r_end) of the list e0s, degree D unrolled */
template <int ALGO, int D, int V, int W, typename T>
__device__ __forceinline__ void check_rows(const T *Qu, unsigned lane_off, T *Rt, const int32_t *__restrict__ e0s, int r_begin, int r_end,
                                           const T *Ct, const int32_t *__restrict__ edge_col,
                                           const int32_t *__restrict__ qpos, const MsCorr &c)
{
    const int lane = threadIdx.x & 63;
    constexpr size_t F = 64 * V;
    for (int r = r_begin; r < r_end; ++r) {
        const int e0 = e0s[r];
        float x[D][W], out[D][W];
        if (ALGO != kAlgoSP && Ct) {            /* round 1: q = y, by column (CheckArgs::first_chan) */
#pragma unroll
            for (int k = 0; k < D; ++k) vload<W>(x[k], Ct + (size_t)edge_col[e0 + k] * F);
        } else {
            int sl[D];
            row_slots<D>(qpos, e0, lane, sl);
#pragma unroll
            for (int k = 0; k < D; ++k) vload<W>(x[k], Qu + (size_t)sl[k] * F + lane_off);
        }
        check_node<ALGO, D, W, T>(x, out, c);
#pragma unroll
        for (int k = 0; k < D; ++k) vstore<W>(Rt + (size_t)(e0 + k) * F, out[k]);
    }
}

/* V = frames per lane of the LAYOUT (tile = 64*V frames); W <= V = floats per lane this
 * kernel moves: a row's 64*V-float segment is covered by V/W waves of 64*W floats each
 * (consecutive waves of a block).  Narrow waves (W = 1) need fewer registers and run at higher
 * occupancy: measured 6.0 TB/s against 5.5 TB/s for W = V = 4 on the degree-7 rows. */
template <int ALGO, int D, int V, int W, typename T>
__global__ __launch_bounds__(kBlock) void check_kernel(const CheckArgs a)
{
    constexpr size_t F = 64 * V;
    constexpr int SUB = V / W;
    const int lane = threadIdx.x & 63;
    const GridPos gp = grid_pos(a.tiles_first);
    const int tile = tile_select<V>(a.tail, a.done, gp.row);
    if (tile < 0) return;
    const int wave = gp.block * kWavesPerBlock + wave_id_in_block();
    const int sub = wave % SUB;
    const int r_begin = (wave / SUB) * a.rows_per_wave;
    const int r_end = min(r_begin + a.rows_per_wave, a.n_rows);
    const unsigned lane_off = (unsigned)sub * 64 * W + (unsigned)lane * W;
    const T *Qu = static_cast<const T *>(a.Q) + (size_t)tile * (size_t)a.E * F;      /* wave-uniform: + slot * F + lane_off */
    T *Rt = static_cast<T *>(a.R) + (size_t)tile * (size_t)a.E * F + lane_off;

    const T *Ct = (ALGO != kAlgoSP && a.first_chan)
                      ? static_cast<const T *>(a.first_chan) + (size_t)tile * (size_t)a.N * F + lane_off : nullptr;
    check_rows<ALGO, D, V, W, T>(Qu, lane_off, Rt, a.cls_e0, r_begin, r_end, Ct, a.edge_col, a.qpos, ms_corr_of(a));
}

/* One row of any degree with run-time loops (rows wider than the unrolled kernels, and the few
 * left-over rows a linked check launch takes along).  Min-sum: two passes over the row.  Sum-product:
 * the exact left-to-right product needs one pass per output, as the reference does (L1/L2 serve the
 * repeats).  Qt / Rt: this lane's V values of the tile. */
template <int ALGO, int V, typename T>
__device__ __forceinline__ void check_row_generic(const T *Qu, unsigned lane_off, T *Rt, int e0, int D,
                                                  const int32_t *__restrict__ qpos, const MsCorr &c)
{
    constexpr size_t F = 64 * V;
    if (ALGO == kAlgoBP) {
        /* check_bp's association with run-time loops: the forward value is carried in registers (never through T: fp16
         * would round it), b_{k+1} is rebuilt from the row's end for every output (L2 serves the re-reads) */
        auto load = [&](int j, float (&t)[V]) {
            vload<V>(t, Qu + (size_t)edge_slot(qpos, e0 + j) * F + lane_off);
#pragma unroll
            for (int v = 0; v < V; ++v) t[v] = bp_clamp(t[v]);
        };
        auto store = [&](int k, float (&o)[V]) {
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = MsgRound<T>::of(o[v]);
            vstore<V>(Rt + (size_t)(e0 + k) * F, o);
        };
        if (D <= 0) return;
        float f[V], b[V], t[V];
        if (D == 1) {
#pragma unroll
            for (int v = 0; v < V; ++v) b[v] = 1000.0f;
            store(0, b);
            return;
        }
        load(0, f);
        for (int k = 0; k < D - 1; ++k) {
            /* b = b_{k+1}; f = f_{k-1} (k >= 1) */
            load(D - 1, b);
            for (int j = D - 2; j > k; --j) {
                load(j, t);
#pragma unroll
                for (int v = 0; v < V; ++v) b[v] = bp_boxplus(t[v], b[v]);
            }
            if (k == 0) { store(0, b); continue; }
            float o[V];
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = bp_boxplus(f[v], b[v]);
            store(k, o);
            load(k, t);
#pragma unroll
            for (int v = 0; v < V; ++v) f[v] = bp_boxplus(f[v], t[v]);
        }
        store(D - 1, f);
        return;
    }
    if (ALGO != kAlgoSP) {
        /* two passes over the row instead of one per output: min1/min2/argmin and the sign
         * parity first, then each output from its own re-read value (L2 serves the re-read) */
        float m1[V], m2[V];
        int idx[V];
        unsigned par[V];
#pragma unroll
        for (int v = 0; v < V; ++v) { m1[v] = 1000.0f; m2[v] = 1000.0f; idx[v] = -1; par[v] = 0; }
        for (int j = 0; j < D; ++j) {
            float xj[V];
            vload<V>(xj, Qu + (size_t)edge_slot(qpos, e0 + j) * F + lane_off);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float m = __builtin_fabsf(xj[v]);
                par[v] ^= (xj[v] < 0.0f) ? 1u : 0u;
                if (m < m1[v]) { m2[v] = m1[v]; m1[v] = m; idx[v] = j; }
                else if (m < m2[v]) { m2[v] = m; }
            }
        }
        if (ALGO == kAlgoMSC) {
#pragma unroll
            for (int v = 0; v < V; ++v) { m1[v] = ms_corr<T>(m1[v], c); m2[v] = ms_corr<T>(m2[v], c); }
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) { m1[v] = MsgStart<T>::of(m1[v]); m2[v] = MsgStart<T>::of(m2[v]); }
        }
        for (int k = 0; k < D; ++k) {
            float xk[V], o[V];
            vload<V>(xk, Qu + (size_t)edge_slot(qpos, e0 + k) * F + lane_off);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float b = (k == idx[v]) ? m2[v] : m1[v];
                const unsigned sg = par[v] ^ ((xk[v] < 0.0f) ? 1u : 0u);
                o[v] = sg ? -b : b;
            }
            vstore<V>(Rt + (size_t)(e0 + k) * F, o);
        }
        return;
    }
    for (int k = 0; k < D; ++k) {
        float o[V];
        float p[V];
#pragma unroll
        for (int v = 0; v < V; ++v) p[v] = 1.0f;
        for (int j = 0; j < D; ++j) {
            if (j == k) continue;
            float xj[V];
            vload<V>(xj, Qu + (size_t)edge_slot(qpos, e0 + j) * F + lane_off);
#pragma unroll
            for (int v = 0; v < V; ++v) p[v] *= xj[v];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) o[v] = p[v];
        vstore<V>(Rt + (size_t)(e0 + k) * F, o);
    }
}

/* Any degree; only launched above the unrolled degrees. */
template <int ALGO, int V, typename T>
__global__ __launch_bounds__(kBlock) void check_kernel_generic(const CheckArgs a)
{
    constexpr size_t F = 64 * V;
    const int lane = threadIdx.x & 63;
    const GridPos gp = grid_pos(a.tiles_first);
    const int tile = tile_select<V>(a.tail, a.done, gp.row);
    if (tile < 0) return;
    const int wave = gp.block * kWavesPerBlock + wave_id_in_block();
    const int r_begin = wave * a.rows_per_wave;
    const int r_end = min(r_begin + a.rows_per_wave, a.n_rows);
    const T *Qu = static_cast<const T *>(a.Q) + (size_t)tile * (size_t)a.E * F;
    T *Rt = static_cast<T *>(a.R) + (size_t)tile * (size_t)a.E * F + (size_t)lane * V;
    for (int r = r_begin; r < r_end; ++r) check_row_generic<ALGO, V, T>(Qu, (unsigned)lane * V, Rt, a.cls_e0[r], a.degree, a.qpos, ms_corr_of(a));
}

template <int ALGO, int V, typename T, int D, int DLO, int W = 1> struct CheckDispatch {
    static __device__ __forceinline__ void run(int deg, const T *Qu, unsigned lane_off, T *Rt, const int32_t *e0s, int rb, int re,
                                               const T *Ct, const int32_t *edge_col, const int32_t *qpos, const MsCorr &c)
    {
        if (deg == D) check_rows<ALGO, D, V, W, T>(Qu, lane_off, Rt, e0s, rb, re, Ct, edge_col, qpos, c);
        else CheckDispatch<ALGO, V, T, D - 1, DLO, W>::run(deg, Qu, lane_off, Rt, e0s, rb, re, Ct, edge_col, qpos, c);
    }
};
template <int ALGO, int V, typename T, int DLO, int W> struct CheckDispatch<ALGO, V, T, DLO, DLO, W> {
    static __device__ __forceinline__ void run(int, const T *Qu, unsigned lane_off, T *Rt, const int32_t *e0s, int rb, int re,
                                               const T *Ct, const int32_t *edge_col, const int32_t *qpos, const MsCorr &c)
    {
        check_rows<ALGO, DLO, V, W, T>(Qu, lane_off, Rt, e0s, rb, re, Ct, edge_col, qpos, c);
    }
};

/* degrees DLO..DHI; W values per lane (V / W consecutive waves cover a row's segment).  W = 1: narrow waves,
 * the form of all fp32 kernels (256 B per wave-instruction).  fp16 messages at V = 4 use W = 2: with one
 * 2-byte value per lane a wave-instruction moves 128 B and the degree-30 rows of the rate-9/10 code ran at
 * 5.0 TB/s against 6.0 for the fp32 narrow form.  fp8 messages use W = V: a dword per lane at V = 4. */
template <int ALGO, int V, typename T, int DLO, int DHI, int W = 1>
__global__ __launch_bounds__(kBlock) void check_group_kernel(const CheckArgs a, const GroupClass *__restrict__ cls, int n_classes)
{
    constexpr size_t F = 64 * V;
    constexpr int SUB = V / W;
    const int lane = threadIdx.x & 63;
    const GridPos gp = grid_pos(a.tiles_first);
    const int tile = tile_select<V>(a.tail, a.done, gp.row);
    if (tile < 0) return;
    int c = 0;
    while (c + 1 < n_classes && gp.block >= cls[c + 1].block_begin) ++c;
    const int wave = (gp.block - cls[c].block_begin) * kWavesPerBlock + wave_id_in_block();
    const int sub = wave % SUB;
    const int r_begin = (wave / SUB) * a.rows_per_wave;
    const int r_end = min(r_begin + a.rows_per_wave, cls[c].count);
    const unsigned lane_off = (unsigned)sub * 64 * W + (unsigned)lane * W;
    const T *Qu = static_cast<const T *>(a.Q) + (size_t)tile * (size_t)a.E * F;
    T *Rt = static_cast<T *>(a.R) + (size_t)tile * (size_t)a.E * F + lane_off;
    const T *Ct = (ALGO != kAlgoSP && a.first_chan)
                      ? static_cast<const T *>(a.first_chan) + (size_t)tile * (size_t)a.N * F + lane_off : nullptr;
    CheckDispatch<ALGO, V, T, DHI, DLO, W>::run(cls[c].degree, Qu, lane_off, Rt, cls[c].ids, r_begin, r_end, Ct, a.edge_col, a.qpos, ms_corr_of(a));
}

}  // namespace ldpc
