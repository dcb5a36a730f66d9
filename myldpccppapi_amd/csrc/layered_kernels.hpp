/*
 * layered_kernels.hpp -- layered (TDMP) min-sum on gfx950.
 *
 * Semantic model: the reference's fused kernel decodeOnceTDMP
 * (decodeCL.c:307-426), generalised from its WiMAX-seed addressing to any edge
 * list whose rows come in layers of `layer_rows` rows with pairwise disjoint
 * columns.  (The reference's host-layered path, MyLdpc.cpp:889-976, mis-sizes its
 * layers -- :907,958 -- and is not followed.)
 *
 * Per frame: posteriors P[N] (start: channel values) and messages R[E] (start 0).
 * One pass over layer l, every row of the layer independently (decodeCL.c:345-383):
 *     q_k = P[col_k] - R_k ; a = prod q_k (fp32, ascending k) ; two smallest |q_k|
 *     R_k = sign(q_k) * (sign(a) * (k == argmin ? min2 : min1)) ; P[col_k] = q_k + R_k
 * After the last layer: bits = P < 0, syndrome, stop when clean or at max_iter
 * (:387-412).
 *
 * MI355X layout: frames are the lanes, P[tile][n][F] and R[tile][e][F] with
 * F = 64*V, as in flood_kernels.hpp.  One launch per layer (rows of a layer are
 * independent, layers are ordered); a row's R segments are consecutive, its P
 * segments are gathered.  16*E bytes per frame-iteration (R and P each read and
 * written once per edge).  Frozen frames keep their hard bits (bit masks), their
 * P/R keep evolving unread -- no per-lane predication in the hot loop.
 *
 * Structure.  A rule (LayerRule) is a row arithmetic; a storage (LayerStore) is the element types of P and R.  The four
 * float rules run on StoreF32; kLayerFx (LDPC_ALGO_LAYERED_FX) and kLayerBpFx (LDPC_ALGO_LAYERED_BP_FX) run on StoreFx, one-byte R
 * and int16 P.  Everything around the row arithmetic is written once over the storage:
 *   LayerArgs<S>, LayerWave<V, S>     the argument block of a layer launch and what one wave of it works on, set_bits
 *                                     included (LayerArgsFx adds L and LP behind the block, so the float kernarg has none)
 *   layer_kernel_generic<V, RULE>     rows of any degree, the rule's row as a function with run-time loops
 *   layered_init_kernel<V, IN, S, SCALED>, layered_extrinsic_kernel<IN, S>
 *                                     the start of P and the extrinsic pass, the value of a channel sample (layer_chan:
 *                                     y, llr_scale * y, or sq(llr_scale * y)) chosen at compile time
 *   layered_run_v<V, S>               the driver: one round loop, one kernel table per rule
 * The exception is the unrolled kernel, layer_kernel<D, V, RULE>: an overload per storage, and the float one writes the
 * wave's set-up and the hard-bit write out by hand (the reason stands above it).
 * The row arithmetics are not merged: layer_kernel's two float paths and its two fixed-point bodies, layer_row_generic,
 * layer_row_generic_bp, layer_row_generic_fx and layer_row_generic_bpfx each follow their own definition bit for bit.
 * engine_layered.hip instantiates the driver on StoreF32 and engine_layered_fx.hip on StoreFx, so the library's largest unit
 * builds beside the other; engine_layered_bpfx.hip instantiates kLayerBpFx's kernels and hands them to the StoreFx driver
 * as a table (layer_table_bpfx), a third unit beside the two.  The host driver calls engine_layered_run, which forwards by
 * LayeredPlan::rule.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <type_traits>
#include <utility>
#include <vector>

#include "flood_kernels.hpp"
#include "crc_term_kernels.hpp"
#include "soft_kernels.hpp"
#include "hip_host.hpp"
#include "engines.hpp"

namespace ldpc {

/* The row rules of the streaming layered kernels; the frame around them -- rows of a wave, loads, stores, hard bits --
 * is layer_kernel's (unrolled degrees) and layer_kernel_generic's (any degree). */
enum LayerRule {
    kLayerFused = 0,    /* the arithmetic of the fused kernel decodeOnceTDMP (above) */
    kLayerCorr,         /* the same with normalized / offset min-sum (LayeredPlan::ms_scale / ms_offset): the row's two
                           candidates b, c go through ms_corr (flood_common.hpp) before the sign and the per-edge selection
                           -- two operations per row, not per edge */
    kLayerHost,         /* the reference's host-layered path, Coder::decodeOnceTDMP (MyLdpc.cpp:889-976) over refreshQTDMP /
                           refreshRTDMP / refreshPostPTDMP (decodeCL.c:228-259, 283-290): q_k = P - R_k, the check node of
                           the MS kernel chain (sign = XOR of `< 0`, magnitude = fmin chain from 1000 == check_ms),
                           P = q_k + R_k; the hard decision is taken once per iteration by layered_hard_kernel */
    kLayerBp,           /* layered log-domain sum-product (LDPC_ALGO_LAYERED_BP, include/ldpc_hip.h has the rule bit for
                           bit): the row of LDPC_ALGO_BP (check_bp, flood_check.hpp) on x_k = q_k = P[col_k] - R_k:
                           R_k = out_k, P[col_k] = q_k + R_k.  The row's sign comes from (x < 0), never from a product of
                           messages, so an exact 0 does not kill a row */
    kLayerFx,           /* layered min-sum in fixed point (LDPC_ALGO_LAYERED_FX, include/ldpc_hip.h has the rule bit for
                           bit): the SUM path on one-byte R and int16 P with two clamps, the corrected row of LDPC_MSG_I8.
                           The overload of layer_kernel on LayerArgsFx and layer_row_generic_fx in layer_kernel_generic,
                           launched by the driver's instantiation in engine_layered_fx.hip */
    kLayerBpFx,         /* layered box-plus in fixed point (LDPC_ALGO_LAYERED_BP_FX, include/ldpc_hip.h has the rule bit for
                           bit): kLayerFx's schedule, storage and clamps with a row of min plus a correction read from a
                           table (layer_rows_bpfx, layer_row_generic_bpfx below).  Its kernels are instantiated in
                           engine_layered_bpfx.hip and handed to the driver as a table (layer_table_bpfx) */
};

/* ---- LDPC_ALGO_LAYERED_FX (kLayerFx): fixed-point layered min-sum, include/ldpc_hip.h has the rule bit for bit ----
 *
 * Storage: R [T][E][F] one byte per message (q8any: the loads and the store sequence of the flooding I8 kernels; the
 * values are in [-L, L] before they reach the store, so its clamp at 127 never acts), P [T][N][F] two bytes per value
 * (p16, below).  6 bytes per edge and frame-round instead of 16.  Arithmetic is fp32 on integers far below 2^24: exact.
 * L, LP and the correction are launch arguments; plain min-sum runs the corrected row with scale 1 and offset 0, which is
 * the identity on the integers of [0, L] and reads the start value 1000 as L, so there is one rule and not two. */

/* the posterior memory: a two's-complement int16 holding an integer in [-LP, LP], LP <= 32767 (the row clamps, the
 * store does not).  Per lane at V = 4 one dwordx2, at V = 2 one dword, at V = 1 one sign-extending short load.
 *   load,  V = 4: global_load_dwordx2; per value one v_cvt_f32_i32 with an SDWA word select and sign extension (or
 *                 v_bfe_i32 / v_ashrrev_i32 + v_cvt_f32_i32 where the backend prefers)
 *   store, V = 4: 4 v_cvt_i32_f32 (exact: the values are integers) + 2 v_perm_b32 gathering the low words
 *                 (selector 0x05040100) + global_store_dwordx2 = 1.5 VALU per value */
struct p16 {
    int16_t bits;
};
static_assert(sizeof(p16) == 2, "two bytes per posterior");
typedef int vi2 __attribute__((ext_vector_type(2)));

template <int V> __device__ __forceinline__ void vload(float (&d)[V], const p16 *p)
{
    static_assert(V == 1 || V == 2 || V == 4, "1, 2 or 4 posteriors per lane");
    if constexpr (V == 1) {
        d[0] = (float)(int)ld_stream(reinterpret_cast<const int16_t *>(p));
    } else if constexpr (V == 2) {
        const int w = ld_stream(reinterpret_cast<const int *>(p));
        d[0] = (float)(int)(int16_t)w; d[1] = (float)(w >> 16);
    } else {
        const vi2 w = ld_stream(reinterpret_cast<const vi2 *>(p));
        d[0] = (float)(int)(int16_t)w.x; d[1] = (float)(w.x >> 16);
        d[2] = (float)(int)(int16_t)w.y; d[3] = (float)(w.y >> 16);
    }
}
/* low words of two integers side by side: v_perm_b32, bytes 0..3 of the second operand, 4..7 of the first */
__device__ __forceinline__ int p16_pack2(float lo, float hi)
{
    return (int)__builtin_amdgcn_perm((uint32_t)(int)hi, (uint32_t)(int)lo, 0x05040100u);
}
template <int V> __device__ __forceinline__ void vstore(p16 *p, const float (&s)[V])
{
    static_assert(V == 1 || V == 2 || V == 4, "1, 2 or 4 posteriors per lane");
    if constexpr (V == 1) {
        st_stream(reinterpret_cast<int16_t *>(p), (int16_t)(int)s[0]);
    } else if constexpr (V == 2) {
        st_stream(reinterpret_cast<int *>(p), p16_pack2(s[0], s[1]));
    } else {
        vi2 t; t.x = p16_pack2(s[0], s[1]); t.y = p16_pack2(s[2], s[3]);
        st_stream(reinterpret_cast<vi2 *>(p), t);
    }
}

template <class S> struct LayerArgs;
struct LayerArgsFx;

/* A storage: the element types of the posterior and the message array, the argument block a layer kernel on it takes,
 * and the byte counts the timing hooks report. */
template <typename PT, typename RT> struct LayerStore {
    typedef PT P;
    typedef RT R;
    static constexpr bool kFixed = !std::is_same<PT, float>::value;
    typedef std::conditional_t<kFixed, LayerArgsFx, LayerArgs<LayerStore>> Args;
    static constexpr int64_t kEdgeBytes = 2 * sizeof(RT) + 2 * sizeof(PT);      /* R and P, each read and written */
    static constexpr int64_t kSettleBytes = sizeof(PT) + sizeof(float);         /* soft settle: P read, a float written */
};
typedef LayerStore<float, float> StoreF32;      /* kLayerFused, kLayerCorr, kLayerHost, kLayerBp */
typedef LayerStore<p16, q8any> StoreFx;         /* kLayerFx, kLayerBpFx */
/* the storage of a rule (a struct and not a conditional, so that the kernels' symbols stay readable) */
template <int RULE> struct RuleOn { typedef StoreF32 Store; };
template <> struct RuleOn<kLayerFx> { typedef StoreFx Store; };
template <> struct RuleOn<kLayerBpFx> { typedef StoreFx Store; };
template <int RULE> using RuleStore = typename RuleOn<RULE>::Store;

template <class S> struct LayerArgs {
    typename S::P *__restrict__ P;        /* [T][N][F] */
    typename S::R *__restrict__ R;        /* [T][E][F] */
    const int32_t *__restrict__ cls_e0;   /* rows of this (layer, degree) group: first edge id */
    const int32_t *__restrict__ edge_col; /* [E] */
    uint64_t *hard;                       /* [T][N][V] */
    const uint64_t *__restrict__ done;    /* [T][V] */
    int64_t E;
    int32_t N;
    int32_t n_rows;
    int32_t rows_per_wave;
    int32_t degree;
};
struct LayerArgsFx : LayerArgs<StoreFx> {
    float L;                              /* 2^(q-1) - 1: messages */
    float LP;                             /* 2^(p-1) - 1: posterior memory */
};

/* OpenCL sign(): +-1, +-0 for +-0, 0 for NaN. */
__device__ __forceinline__ float cl_sign(float x)
{
    return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : (x == 0.0f ? x : 0.0f));
}

/* a candidate of the fixed-point row as its message: fminf(truncf(fmaxf(m - offset, 0) * scale), L), fp32, in this order */
__device__ __forceinline__ float fx_corr(float m, const MsCorr &c, float L)
{
    return fminf(truncf(fmaxf(m - c.offset, 0.0f) * c.scale), L);
}

/* What one wave of a layer launch works on: its rows, its lanes' part of the tile's P and R, the tile's hard bits. */
template <int V, class S> struct LayerWave {
    static constexpr size_t F = 64 * V;
    int lane, r_begin, r_end;
    typename S::P *Pt;
    typename S::R *Rt;
    uint64_t *hard_t;
    uint64_t frozen[V];
    __device__ __forceinline__ explicit LayerWave(const LayerArgs<S> &a)
    {
        lane = threadIdx.x & 63;
        const int tile = blockIdx.y;
        const int wave = (int)blockIdx.x * kWavesPerBlock + wave_id_in_block();
        r_begin = wave * a.rows_per_wave;
        r_end = min(r_begin + a.rows_per_wave, a.n_rows);
        Pt = a.P + (size_t)tile * (size_t)a.N * F + (size_t)lane * V;
        Rt = a.R + (size_t)tile * (size_t)a.E * F + (size_t)lane * V;
        hard_t = a.hard + (size_t)tile * (size_t)a.N * V;
#pragma unroll
        for (int v = 0; v < V; ++v) frozen[v] = a.done[(size_t)tile * V + v];
    }
    /* bits = P < 0 (decodeCL.c:388-389), kept current per write; frozen frames keep theirs */
    __device__ __forceinline__ void set_bits(int col, const float (&p)[V]) const
    {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const uint64_t w = __ballot(p[v] < 0.0f);
            if (lane == 0) {
                const uint64_t old = hard_t[(size_t)col * V + v];
                hard_t[(size_t)col * V + v] = (old & frozen[v]) | (w & ~frozen[v]);
            }
        }
    }
};

/* Rows of degree D on StoreF32: one load and one store of R and of P per edge.  Every instantiation takes the MsCorr, so
 * that one table of one pointer type launches all four rules; only kLayerCorr reads it.  The wave's set-up and its hard-bit
 * write are written out here and not taken from LayerWave: with the struct, all 288 instantiations move by a few
 * instructions and four of the kLayerBp ones spill one to three more SGPRs. */
template <int D, int V, int RULE>
__global__ __launch_bounds__(kBlock) void layer_kernel(const LayerArgs<StoreF32> a, const MsCorr corr)
{
    static_assert(RULE != kLayerFx, "the fixed-point rule has the overload on LayerArgsFx");
    constexpr size_t F = 64 * V;
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.y;
    if (tile_finished<V>(a.done, tile)) return;
    const int wave = (int)blockIdx.x * kWavesPerBlock + wave_id_in_block();
    const int r_begin = wave * a.rows_per_wave;
    const int r_end = min(r_begin + a.rows_per_wave, a.n_rows);
    float *Pt = a.P + (size_t)tile * (size_t)a.N * F + (size_t)lane * V;
    float *Rt = a.R + (size_t)tile * (size_t)a.E * F + (size_t)lane * V;
    uint64_t *hard_t = a.hard + (size_t)tile * (size_t)a.N * V;
    uint64_t frozen[V];
#pragma unroll
    for (int v = 0; v < V; ++v) frozen[v] = a.done[(size_t)tile * V + v];
    for (int r = r_begin; r < r_end; ++r) {
        const int e0 = a.cls_e0[r];
        int col[D];
#pragma unroll
        for (int k = 0; k < D; ++k) col[k] = a.edge_col[e0 + k];
        float p[D][V], m[D][V];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            vload<V>(m[k], Rt + (size_t)(e0 + k) * F);
            vload<V>(p[k], Pt + (size_t)col[k] * F);
        }
        constexpr bool SUM = RULE == kLayerHost || RULE == kLayerBp;   /* the row is a function of the q_k: check_ms, check_bp */
        if constexpr (SUM) {
#pragma unroll
            for (int k = 0; k < D; ++k)
#pragma unroll
                for (int v = 0; v < V; ++v) p[k][v] = p[k][v] - m[k][v];      /* q_k (refreshQTDMP) */
            if constexpr (RULE == kLayerHost) check_ms<D, V>(p, m);               /* refreshRTDMP */
            else check_bp<D, V, float>(p, m);                                     /* R_k = out_k */
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float prod = 1.0f, b = 1000.0f, c = 1001.0f;   /* decodeCL.c:346-348 */
                int bind = -1;
                float sg[D];
#pragma unroll
                for (int k = 0; k < D; ++k) {                  /* :350-367 */
                    const float q = p[k][v] - m[k][v];
                    sg[k] = cl_sign(q);
                    prod *= q;
                    p[k][v] = q;
                    const float mag = __builtin_fabsf(q);
                    if (mag <= b) { c = b; b = mag; bind = k; }
                    else if (mag > b && mag <= c) { c = mag; }
                }
                if (RULE == kLayerCorr) { b = ms_corr<float>(b, corr); c = ms_corr<float>(c, corr); }   /* once per row */
                const float sa = cl_sign(prod);                /* :369 */
                const float ab = sa * b, ac = sa * c;
#pragma unroll
                for (int k = 0; k < D; ++k) {                  /* :371-383 */
                    const float rn = sg[k] * ((k == bind) ? ac : ab);
                    m[k][v] = rn;
                    p[k][v] = p[k][v] + rn;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if constexpr (SUM) {
#pragma unroll
                for (int v = 0; v < V; ++v) p[k][v] = p[k][v] + m[k][v];      /* P = q_k + R_k (refreshPostPTDMP) */
            }
            vstore<V>(Rt + (size_t)(e0 + k) * F, m[k]);
            vstore<V>(Pt + (size_t)col[k] * F, p[k]);
            if (RULE != kLayerHost) {
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const uint64_t w = __ballot(p[k][v] < 0.0f);
                    if (lane == 0) {
                        const uint64_t old = hard_t[(size_t)col[k] * V + v];
                        hard_t[(size_t)col[k] * V + v] = (old & frozen[v]) | (w & ~frozen[v]);
                    }
                }
            }
        }
    }
}

/* ---- LDPC_ALGO_LAYERED_BP_FX (kLayerBpFx): box-plus rows in fixed point, include/ldpc_hip.h has the rule bit for bit ----
 *
 * The table.  T_f has at most 57 entries (f = 4), each at most 11.  The host pads it with zeros to kBpFxTable = 256 bytes, so
 * that an index |a| + |b| <= 2 * 127 needs no clamp, and every block copies it into LDS once (64 lanes, one dword each).
 * A look-up is one ds_read_u8: two per box-plus, no memory round trip.  Bytes 0 .. 127 are 32 dwords in 32 banks and equal
 * addresses broadcast, so look-ups below 128 never conflict; one at 128 or above (q = 8 only, where it reads a zero) can
 * share a bank with one below.  The alternatives were weighed for <19, 4>, 51 box-plus per frame and row: a table held
 * wave-uniform in SGPRs needs a per-lane select over 15 dwords per look-up, a compare chain needs up to 11 compares per
 * look-up at f = 4 (T is a step function with T[0] steps) and is short only for f <= 1; the LDS copy costs two DS
 * instructions beside six VALU instructions per box-plus and no registers.
 *
 * Signs.  a [+] b = 0 whenever a or b is 0 (m = 0 and |a| + |b| = ||a| - |b||), so a zero stays a zero through every further
 * box-plus and the sign the definition gives it ("a zero counts as positive") never reaches a result that is not itself 0.
 * For every non-zero result the sign is the XOR of the signs of the inputs that went into it.  So the kernels split the
 * row as min-sum does: the sign of R_k is the row's parity XOR (x_k < 0), and the forward / backward association runs on
 * magnitudes alone -- min, sum, difference, two look-ups, subtract, add, max: six VALU instructions. */
constexpr int kBpFxTable = 256;
constexpr int kBpFxMaxFracBits = 4;

/* T_f[d] = floor(2^f log(1 + exp(-d / 2^f)) + 0.5) in double, d = 0, 1, ... up to and including the first 0: the number of
 * entries written (57 at f = 4, so cap = kBpFxTable always holds it).  Host code; ldpc_bp_fx_table hands it out. */
inline int bp_fx_table_build(int f, int32_t *out, int cap)
{
    const double s = (double)(1 << f);
    int n = 0;
    while (n < cap) {
        const int32_t v = (int32_t)std::floor(s * std::log(1.0 + std::exp(-(double)n / s)) + 0.5);
        out[n++] = v;
        if (v == 0) break;
    }
    return n;
}

/* |a [+] b| from |a| and |b|, both in [0, L]: max(0, m + T[|a| + |b|] - T[||a| - |b||]), where ||a| - |b|| = sum - 2 m */
__device__ __forceinline__ int bpfx_box(int ma, int mb, const uint8_t *T)
{
    const int m = min(ma, mb), sum = ma + mb;
    return max(m + (int)T[sum] - (int)T[sum - 2 * m], 0);
}

/* The table's address travels in the second argument of the launch.  Every layer kernel takes a MsCorr so that one table of
 * one pointer type launches all rules; kLayerBpFx has no correction (ms_scale / ms_offset are refused), and its eight bytes
 * carry the address instead, so that LayerArgsFx and with it every kLayerFx kernel stay as they were. */
static_assert(sizeof(MsCorr) == sizeof(const uint8_t *), "the table's address takes the place of the correction");
inline MsCorr bpfx_table_arg(const uint8_t *table)
{
    MsCorr c;
    __builtin_memcpy(&c, &table, sizeof c);
    return c;
}
__device__ __forceinline__ const uint8_t *bpfx_table_of(const MsCorr &c)
{
    const uint8_t *table;
    __builtin_memcpy(&table, &c, sizeof table);
    return table;
}

/* the block's copy of the table; every thread of the block comes here (a finished tile has left before, as a block) */
__device__ __forceinline__ void bpfx_table_fill(uint8_t *T, const uint8_t *__restrict__ src)
{
    static_assert(kBpFxTable == 4 * 64, "one dword per lane of the first wave");
    if (threadIdx.x < 64) reinterpret_cast<uint32_t *>(T)[threadIdx.x] = reinterpret_cast<const uint32_t *>(src)[threadIdx.x];
    __syncthreads();
}

/* Rows of degree D under kLayerBpFx: the loads, clamps and stores of the kLayerFx kernel below; between them the magnitudes
 * F_0 .. F_{D-2} forward, then B backward in one register while the messages come out: 3 (D - 2) box-plus per frame. */
template <int D, int V>
__device__ __forceinline__ void layer_rows_bpfx(const LayerArgsFx &a, const uint8_t *__restrict__ table)
{
    constexpr size_t F = 64 * V;
    __shared__ __attribute__((aligned(16))) uint8_t T[kBpFxTable];
    bpfx_table_fill(T, table);
    const LayerWave<V, StoreFx> w(a);
    const float L = a.L, LP = a.LP;
    for (int r = w.r_begin; r < w.r_end; ++r) {
        const int e0 = a.cls_e0[r];
        int col[D];
#pragma unroll
        for (int k = 0; k < D; ++k) col[k] = a.edge_col[e0 + k];
        float t[D][V], m[D][V];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            vload<V>(m[k], w.Rt + (size_t)(e0 + k) * F);
            vload<V>(t[k], w.Pt + (size_t)col[k] * F);
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            int mag[D];
            unsigned par = 0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                t[k][v] = t[k][v] - m[k][v];                                       /* t_k: exact, not clamped */
                const float x = __builtin_amdgcn_fmed3f(t[k][v], -L, L);           /* the variable->check message */
                mag[k] = (int)__builtin_fabsf(x);
                par ^= (x < 0.0f) ? 1u : 0u;
            }
            /* R_k = +-g, negative iff the parity XOR (x_k < 0); t_k < 0 says what x_k < 0 says, the clamp keeps the sign */
            auto emit = [&](int k, int g) {
                const float gf = (float)g;
                const float rn = (par ^ ((t[k][v] < 0.0f) ? 1u : 0u)) ? -gf : gf;
                m[k][v] = rn;
                t[k][v] = __builtin_amdgcn_fmed3f(t[k][v] + rn, -LP, LP);          /* only the posterior memory saturates */
            };
            if constexpr (D == 1) {
                emit(0, (int)L);                    /* LDPC_ALGO_LAYERED_BP's degree-1 row gives +1000, which reads L */
            } else if constexpr (D == 2) {
                emit(0, mag[1]); emit(1, mag[0]);
            } else {
                int fw[D - 1];
                fw[0] = mag[0];
#pragma unroll
                for (int k = 1; k <= D - 2; ++k) fw[k] = bpfx_box(fw[k - 1], mag[k], T);        /* F_k */
                emit(D - 1, fw[D - 2]);
                int b = mag[D - 1];                                                              /* B_{D-1} */
#pragma unroll
                for (int k = D - 2; k >= 1; --k) {
                    emit(k, bpfx_box(fw[k - 1], b, T));                                          /* F_{k-1} [+] B_{k+1} */
                    b = bpfx_box(mag[k], b, T);                                                  /* B_k */
                }
                emit(0, b);                                                                      /* B_1 */
            }
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            vstore<V>(w.Rt + (size_t)(e0 + k) * F, m[k]);
            vstore<V>(w.Pt + (size_t)col[k] * F, t[k]);
            w.set_bits(col[k], t[k]);
        }
    }
}

/* Rows of degree D in fixed point.  The SUM path of the float kernel (q = P - R, the check row, P = q + R) with the two
 * clamps: the row reads x = clamp(t, -L, L), the posterior memory takes clamp(t + R, -LP, LP) from the unclamped t.
 * kLayerBpFx has the same frame and another row (layer_rows_bpfx above). */
template <int D, int V, int RULE>
__global__ __launch_bounds__(kBlock) void layer_kernel(const LayerArgsFx a, const MsCorr corr)
{
    static_assert(RULE == kLayerFx || RULE == kLayerBpFx, "the fixed-point argument block belongs to kLayerFx and kLayerBpFx");
    constexpr size_t F = 64 * V;
    if (tile_finished<V>(a.done, blockIdx.y)) return;
    if constexpr (RULE == kLayerBpFx) {
        layer_rows_bpfx<D, V>(a, bpfx_table_of(corr));
        return;
    }
    const LayerWave<V, StoreFx> w(a);
    const float L = a.L, LP = a.LP;
    for (int r = w.r_begin; r < w.r_end; ++r) {
        const int e0 = a.cls_e0[r];
        int col[D];
#pragma unroll
        for (int k = 0; k < D; ++k) col[k] = a.edge_col[e0 + k];
        float t[D][V], m[D][V];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            vload<V>(m[k], w.Rt + (size_t)(e0 + k) * F);
            vload<V>(t[k], w.Pt + (size_t)col[k] * F);
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float m1 = 1000.0f, m2 = 1000.0f;   /* min-sum's start value, a candidate like any other: fx_corr makes it L */
            int idx = -1;
            unsigned par = 0;
            unsigned neg[D];
#pragma unroll
            for (int k = 0; k < D; ++k) {
                t[k][v] = t[k][v] - m[k][v];                                       /* t_k: exact, not clamped */
                const float x = __builtin_amdgcn_fmed3f(t[k][v], -L, L);           /* the variable->check message */
                const float mag = __builtin_fabsf(x);
                neg[k] = (x < 0.0f) ? 1u : 0u;
                par ^= neg[k];
                if (mag < m1) { m2 = m1; m1 = mag; idx = k; }
                else if (mag < m2) { m2 = mag; }
            }
            m1 = fx_corr(m1, corr, L); m2 = fx_corr(m2, corr, L);                  /* once per row */
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const float b = (k == idx) ? m2 : m1;
                const float rn = (par ^ neg[k]) ? -b : b;
                m[k][v] = rn;
                t[k][v] = __builtin_amdgcn_fmed3f(t[k][v] + rn, -LP, LP);          /* only the posterior memory saturates */
            }
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            vstore<V>(w.Rt + (size_t)(e0 + k) * F, m[k]);
            vstore<V>(w.Pt + (size_t)col[k] * F, t[k]);
            w.set_bits(col[k], t[k]);
        }
    }
}

/* A min-sum row of any degree: the same arithmetic with run-time loops, values re-read. */
template <int V, bool CORR>
__device__ __forceinline__ void layer_row_generic(const LayerArgs<StoreF32> &a, const LayerWave<V, StoreF32> &w, int e0,
                                                  const MsCorr corr)
{
    constexpr size_t F = 64 * V;
    const int D = a.degree;
    float prod[V], b[V], c[V], sa[V];
    int bind[V];
#pragma unroll
    for (int v = 0; v < V; ++v) { prod[v] = 1.0f; b[v] = 1000.0f; c[v] = 1001.0f; bind[v] = -1; }
    for (int k = 0; k < D; ++k) {
        const int col = a.edge_col[e0 + k];
        float m[V], p[V];
        vload<V>(m, w.Rt + (size_t)(e0 + k) * F);
        vload<V>(p, w.Pt + (size_t)col * F);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float q = p[v] - m[v];
            prod[v] *= q;
            p[v] = q;
            const float mag = __builtin_fabsf(q);
            if (mag <= b[v]) { c[v] = b[v]; b[v] = mag; bind[v] = k; }
            else if (mag > b[v] && mag <= c[v]) { c[v] = mag; }
        }
        vstore<V>(w.Pt + (size_t)col * F, p);          /* q parked in P, as decodeCL.c:357 */
    }
    if (CORR) {
#pragma unroll
        for (int v = 0; v < V; ++v) { b[v] = ms_corr<float>(b[v], corr); c[v] = ms_corr<float>(c[v], corr); }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) sa[v] = cl_sign(prod[v]);
    for (int k = 0; k < D; ++k) {
        const int col = a.edge_col[e0 + k];
        float q[V], rn[V];
        vload<V>(q, w.Pt + (size_t)col * F);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            rn[v] = cl_sign(q[v]) * ((k == bind[v]) ? sa[v] * c[v] : sa[v] * b[v]);
            q[v] = q[v] + rn[v];
        }
        vstore<V>(w.Rt + (size_t)(e0 + k) * F, rn);
        vstore<V>(w.Pt + (size_t)col * F, q);
        w.set_bits(col, q);
    }
}

/* A box-plus row of any degree: check_bp's association with run-time loops over a row that is updated in place, so the
 * order matters: k ascends, the forward value f_{k-1} is carried in registers, and b_{k+1} is rebuilt from the row's end
 * out of q_j = P[col_j] - R_j for j > k.
 *
 * Invariant: when step k begins, edges 0 .. k-1 of the row hold their new R and P, edges k .. D-1 their old ones.  Step k
 * reads q_j = P[col_j] - R_j only for j >= k -- q_k itself and, for b_{k+1}, the j > k -- and takes everything it needs
 * of the j < k from f = f_{k-1}, carried in registers and formed from q_{k-1} BEFORE step k-1 stored.  A row's columns
 * are distinct (edges ascend strictly within a row) and rows of a layer share no column (layered_plan_create), so what
 * step k stores at R_k and P[col_k] is read by no other edge of this row and by no other row of this launch. */
template <int V>
__device__ __forceinline__ void layer_row_generic_bp(const LayerArgs<StoreF32> &a, const LayerWave<V, StoreF32> &w, int e0)
{
    constexpr size_t F = 64 * V;
    const int D = a.degree;
    /* t_j = bp_clamp(q_j) of an edge that still holds its old values */
    auto load_t = [&](int j, float (&t)[V]) {
        float pj[V], mj[V];
        vload<V>(mj, w.Rt + (size_t)(e0 + j) * F);
        vload<V>(pj, w.Pt + (size_t)a.edge_col[e0 + j] * F);
#pragma unroll
        for (int v = 0; v < V; ++v) t[v] = bp_clamp(pj[v] - mj[v]);
    };
    float f[V];
#pragma unroll
    for (int v = 0; v < V; ++v) f[v] = 0.0f;
    for (int k = 0; k < D; ++k) {
        const int col = a.edge_col[e0 + k];
        float q[V], o[V];
        {
            float mk[V];
            vload<V>(mk, w.Rt + (size_t)(e0 + k) * F);
            vload<V>(q, w.Pt + (size_t)col * F);
#pragma unroll
            for (int v = 0; v < V; ++v) q[v] = q[v] - mk[v];
        }
        if (D == 1) {
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = 1000.0f;
        } else if (k == D - 1) {
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = f[v];                       /* f_{D-2} */
        } else {
            float b[V], t[V];
            load_t(D - 1, b);
            for (int j = D - 2; j > k; --j) {
                load_t(j, t);
#pragma unroll
                for (int v = 0; v < V; ++v) b[v] = bp_boxplus(t[v], b[v]);   /* b_j = t_j [+] b_{j+1} */
            }
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = (k == 0) ? b[v] : bp_boxplus(f[v], b[v]);
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {                   /* f_k from q_k, before edge k is stored */
            const float tk = bp_clamp(q[v]);
            f[v] = (k == 0) ? tk : bp_boxplus(f[v], tk);
            q[v] = q[v] + o[v];
        }
        vstore<V>(w.Rt + (size_t)(e0 + k) * F, o);
        vstore<V>(w.Pt + (size_t)col * F, q);
        w.set_bits(col, q);
    }
}

/* A fixed-point row of any degree: two passes with run-time loops.  The first stores nothing (t_k may need 17 bits and
 * cannot be parked in P as the float row parks q), the second forms t_k again from the edge's own old R and P: a row's
 * columns are distinct and rows of a layer share none, so step k reads nothing an earlier step of this launch wrote. */
template <int V>
__device__ __forceinline__ void layer_row_generic_fx(const LayerArgsFx &a, const LayerWave<V, StoreFx> &w, int e0,
                                                     const MsCorr corr)
{
    constexpr size_t F = 64 * V;
    const float L = a.L, LP = a.LP;
    const int D = a.degree;
    float m1[V], m2[V];
    int idx[V];
    unsigned par[V];
#pragma unroll
    for (int v = 0; v < V; ++v) { m1[v] = 1000.0f; m2[v] = 1000.0f; idx[v] = -1; par[v] = 0; }
    for (int k = 0; k < D; ++k) {
        float m[V], p[V];
        vload<V>(m, w.Rt + (size_t)(e0 + k) * F);
        vload<V>(p, w.Pt + (size_t)a.edge_col[e0 + k] * F);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float x = __builtin_amdgcn_fmed3f(p[v] - m[v], -L, L);
            const float mag = __builtin_fabsf(x);
            par[v] ^= (x < 0.0f) ? 1u : 0u;
            if (mag < m1[v]) { m2[v] = m1[v]; m1[v] = mag; idx[v] = k; }
            else if (mag < m2[v]) { m2[v] = mag; }
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) { m1[v] = fx_corr(m1[v], corr, L); m2[v] = fx_corr(m2[v], corr, L); }
    for (int k = 0; k < D; ++k) {
        const int col = a.edge_col[e0 + k];
        float m[V], p[V];
        vload<V>(m, w.Rt + (size_t)(e0 + k) * F);
        vload<V>(p, w.Pt + (size_t)col * F);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float t = p[v] - m[v];
            const float b = (k == idx[v]) ? m2[v] : m1[v];
            const unsigned s = par[v] ^ ((__builtin_amdgcn_fmed3f(t, -L, L) < 0.0f) ? 1u : 0u);
            m[v] = s ? -b : b;
            p[v] = __builtin_amdgcn_fmed3f(t + m[v], -LP, LP);
        }
        vstore<V>(w.Rt + (size_t)(e0 + k) * F, m);
        vstore<V>(w.Pt + (size_t)col * F, p);
        w.set_bits(col, p);
    }
}

/* A fixed-point box-plus row of any degree.  It keeps layer_row_generic_fx's premise -- nothing is parked in P, every t_j
 * is formed again from the edge's own old R and P -- and takes layer_row_generic_bp's order for the rest: k ascends, the
 * forward magnitude F_{k-1} and the parity of x_0 .. x_{k-1} are carried in registers, and B_{k+1} with the parity of the
 * x_j, j > k, is rebuilt from the row's end out of edges that still hold their old values (the invariant stated at
 * layer_row_generic_bp holds word for word).  So the forward values take neither a pass of their own nor scratch memory:
 * the price is D (D - 1) / 2 box-plus and re-reads per row instead of 3 (D - 2), paid only by rows wider than
 * kMaxUnrolledLayerDegree, and the register count does not depend on D. */
template <int V>
__device__ __forceinline__ void layer_row_generic_bpfx(const LayerArgsFx &a, const LayerWave<V, StoreFx> &w, int e0,
                                                       const uint8_t *T)
{
    constexpr size_t F = 64 * V;
    const float L = a.L, LP = a.LP;
    const int D = a.degree;
    /* t_j of an edge that still holds its old values, and |x_j|, (x_j < 0) of x_j = clamp(t_j, -L, L) */
    auto load_t = [&](int j, float (&t)[V], int (&mag)[V], unsigned (&neg)[V]) {
        float pj[V], mj[V];
        vload<V>(mj, w.Rt + (size_t)(e0 + j) * F);
        vload<V>(pj, w.Pt + (size_t)a.edge_col[e0 + j] * F);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            t[v] = pj[v] - mj[v];
            const float x = __builtin_amdgcn_fmed3f(t[v], -L, L);
            mag[v] = (int)__builtin_fabsf(x);
            neg[v] = (x < 0.0f) ? 1u : 0u;
        }
    };
    int f[V];
    unsigned pf[V];
#pragma unroll
    for (int v = 0; v < V; ++v) { f[v] = 0; pf[v] = 0; }
    for (int k = 0; k < D; ++k) {
        const int col = a.edge_col[e0 + k];
        float t[V], tj[V];
        int mk[V], mj[V], o[V];
        unsigned nk[V], nj[V], pb[V];
        load_t(k, t, mk, nk);
#pragma unroll
        for (int v = 0; v < V; ++v) pb[v] = 0;
        if (D == 1) {
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = (int)L;                      /* as the unrolled kernel */
        } else if (k == D - 1) {
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = f[v];                        /* F_{D-2} */
        } else {
            int b[V];
            load_t(D - 1, tj, b, pb);
            for (int j = D - 2; j > k; --j) {
                load_t(j, tj, mj, nj);
#pragma unroll
                for (int v = 0; v < V; ++v) { b[v] = bpfx_box(mj[v], b[v], T); pb[v] ^= nj[v]; }   /* B_j = x_j [+] B_{j+1} */
            }
#pragma unroll
            for (int v = 0; v < V; ++v) o[v] = (k == 0) ? b[v] : bpfx_box(f[v], b[v], T);
        }
        float rn[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {                   /* F_k and the parity up to k, before edge k is stored */
            const float g = (float)o[v];
            rn[v] = (pf[v] ^ pb[v]) ? -g : g;
            f[v] = (k == 0) ? mk[v] : bpfx_box(f[v], mk[v], T);
            pf[v] ^= nk[v];
            t[v] = __builtin_amdgcn_fmed3f(t[v] + rn[v], -LP, LP);
        }
        vstore<V>(w.Rt + (size_t)(e0 + k) * F, rn);
        vstore<V>(w.Pt + (size_t)col * F, t);
        w.set_bits(col, t);
    }
}

/* Rows of any degree (LayerArgs::degree); the host arithmetic has unrolled degrees only. */
template <int V, int RULE>
__global__ __launch_bounds__(kBlock) void layer_kernel_generic(const typename RuleStore<RULE>::Args a, const MsCorr corr)
{
    static_assert(RULE != kLayerHost, "no generic row with the host arithmetic");
    if (tile_finished<V>(a.done, blockIdx.y)) return;
    if constexpr (RULE == kLayerBpFx) {
        __shared__ __attribute__((aligned(16))) uint8_t T[kBpFxTable];
        bpfx_table_fill(T, bpfx_table_of(corr));
        const LayerWave<V, StoreFx> w(a);
        for (int r = w.r_begin; r < w.r_end; ++r) layer_row_generic_bpfx<V>(a, w, a.cls_e0[r], T);
        return;
    }
    const LayerWave<V, RuleStore<RULE>> w(a);
    for (int r = w.r_begin; r < w.r_end; ++r) {
        if constexpr (RULE == kLayerBp) layer_row_generic_bp<V>(a, w, a.cls_e0[r]);
        else if constexpr (RULE == kLayerFx) layer_row_generic_fx<V>(a, w, a.cls_e0[r], corr);
        else if constexpr (RULE != kLayerBpFx) layer_row_generic<V, RULE == kLayerCorr>(a, w, a.cls_e0[r], corr);
    }
}

/* hardDecisionTDMP, decodeCL.c:261-280, after the last layer of an iteration: P > 0 -> 0, P < 0 -> 1,
 * otherwise (0, NaN) the bit stays; frozen frames keep theirs.  One wave per column. */
template <int V>
__global__ __launch_bounds__(kBlock) void layered_hard_kernel(const float *__restrict__ P, uint64_t *hard,
                                                              const uint64_t *__restrict__ done, int32_t N)
{
    constexpr size_t F = 64 * V;
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.y;
    if (tile_finished<V>(done, tile)) return;
    const int n = (int)blockIdx.x * kWavesPerBlock + wave_id_in_block();
    if (n >= N) return;
    float p[V];
    vload<V>(p, P + ((size_t)tile * N + n) * F + (size_t)lane * V);
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const uint64_t old = hard[((size_t)tile * N + n) * V + v];
        const bool oldb = (old >> lane) & 1ull;
        const bool b = (p[v] > 0.0f) ? false : ((p[v] < 0.0f) ? true : oldb);
        const uint64_t w = __ballot(b);
        const uint64_t frozen = done[(size_t)tile * V + v];
        if (lane == 0) hard[((size_t)tile * N + n) * V + v] = (old & frozen) | (w & ~frozen);
    }
}

/* The value a rule starts P[n] with, and subtracts again for an extrinsic soft output, as a function of the channel
 * sample y:
 *   StoreF32          y (lP = postCode, decodeCL.c:331-334)
 *   StoreF32, SCALED  LDPC_ALGO_LAYERED_BP: chan = llr_scale * y, one fp32 multiply, padding frames included
 *   StoreFx           LDPC_ALGO_LAYERED_FX: sq(llr_scale * y): one fp32 multiply, NaN -> 0 (MsgChan, once per channel value),
 *                     the clamp, then the rounding to nearest even -- on a value in [-L, L], where rounding and clamping
 *                     commute.  SCALED is false. */
template <class S, bool SCALED> __device__ __forceinline__ float layer_chan(float y, float llr_scale, float L)
{
    static_assert(!(S::kFixed && SCALED), "the fixed-point storage has one form");
    if constexpr (S::kFixed) return __builtin_rintf(__builtin_amdgcn_fmed3f(MsgChan<q8any>::of(y, llr_scale), -L, L));
    else if constexpr (SCALED) return llr_scale * y;
    else return y;
}

template <class S> struct LayeredInitArgs {
    const void *__restrict__ llr;       /* [frames][N], elements of the kernel's IN */
    typename S::P *__restrict__ P;      /* [T][N][F] */
    uint64_t *__restrict__ hard;        /* [T][N][V] */
    int64_t frames;
    int32_t N;
    int32_t zero_bits;                  /* host-layered path: bits start at 0 (the reference: undefined) */
    float llr_unit;                     /* narrow IN: y = (float)x * llr_unit (llr_input.hpp); unused for float */
    float llr_scale, L;                 /* layer_chan's; the plain form reads neither */
};

/* P = layer_chan(y), transposed into the tile layout; bits = P < 0.  The patch holds y: padding frames read y = 1.  IN:
 * element type of the caller's buffer; a narrow one goes through llr_patch_fill (llr_input.hpp), float through the loop
 * below. */
template <int V, typename IN, class S, bool SCALED>
__global__ __launch_bounds__(kBlock) void layered_init_kernel(const LayeredInitArgs<S> a)
{
    constexpr int F = 64 * V;
    constexpr int LD = F + 1;
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
        float y[V];
#pragma unroll
        for (int v = 0; v < V; ++v) y[v] = layer_chan<S, SCALED>(patch[c * LD + lane * V + v], a.llr_scale, a.L);
        vstore<V>(a.P + ((size_t)tile * a.N + n) * F + (size_t)lane * V, y);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const uint64_t w = __ballot(y[v] < 0.0f);
            if (lane == 0) a.hard[((size_t)tile * a.N + n) * V + v] = a.zero_bits ? 0ull : w;
        }
    }
}

/* Extrinsic soft output of a rule whose P does not start at y (LAYERED_BP, LAYERED_FX): soft_settle_kernel leaves the
 * posterior of every frame's stop round in the caller's buffer (each value written once); this one pass afterwards
 * subtracts layer_chan(y), formed first, then one subtraction.  The empty asm keeps the scaled form's product a value of
 * its own: contracted into an fma the difference would be rounded once, from the exact product (the fixed-point value is an
 * integer and loses nothing by it).  IN: element type of the caller's buffer; y is the product x * unit of a narrow element,
 * formed first (llr_value). */
template <typename IN, class S>
__global__ __launch_bounds__(kBlock) void layered_extrinsic_kernel(float *__restrict__ soft, const IN *__restrict__ llr,
                                                                   float llr_scale, float L, int64_t count, float unit)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    float chan = layer_chan<S, !S::kFixed>(llr_value<IN>(llr[i], unit), llr_scale, L);
    asm volatile("" : "+v"(chan));
    soft[i] = soft[i] - chan;
}

/* summary[0] = the largest iteration count, summary[1] = the number of frames that stopped clean */
template <int V> __global__ void layered_summary_kernel(const int32_t *iters, const uint64_t *done,
                                                        int64_t frames, int32_t *summary)
{
    constexpr int F = 64 * V;
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= frames) return;
    const int64_t tile = f / F;
    const int fi = (int)(f % F);
    atomicMax(&summary[0], iters[f]);
    if ((done[tile * V + fi % V] >> (fi / V)) & 1ull) atomicAdd(&summary[1], 1);
}

/* ------------------------------------------------------------- host side */

constexpr int kMaxUnrolledLayerDegree = 24;

struct LayerGroup {
    int layer = 0, degree = 0, count = 0;
    DevBuf<int32_t> e0;
};

struct LayeredPlan {
    int32_t M = 0, N = 0, layer_rows = 0;
    int64_t E = 0;
    int T = 0, V = 1;
    LayerRule rule = kLayerFused;   /* the one row arithmetic of this decoder; kLayerFx and kLayerBpFx run on StoreFx, the
                                       others on StoreF32 */
    bool fixed() const { return rule == kLayerFx || rule == kLayerBpFx; }
    float ms_scale = 1.0f, ms_offset = 0.0f;    /* kLayerCorr, kLayerFx (1 / 0 = plain): normalized / offset min-sum */
    float llr_scale = 1.0f;         /* kLayerBp: chan = llr_scale * y; kLayerFx, kLayerBpFx: LSBs per unit of channel value */
    float L = 127.0f, LP = 32767.0f;    /* kLayerFx, kLayerBpFx: the limits of a message and of the posterior memory */
    DevBuf<uint8_t> bp_table;       /* kLayerBpFx: T_f padded with zeros to kBpFxTable bytes (ldpc_decoder_create) */
    DevBuf<float> P, R;             /* StoreF32: [T][N][F], [T][E][F]; only the rule's storage is allocated */
    DevBuf<p16> Pfx;                /* StoreFx: [T][N][F] int16 */
    DevBuf<q8any> Rfx;              /* StoreFx: [T][E][F] bytes */
    template <class S> DevBuf<typename S::P> &post() { if constexpr (S::kFixed) return Pfx; else return P; }
    template <class S> DevBuf<typename S::R> &msgs() { if constexpr (S::kFixed) return Rfx; else return R; }
    std::vector<LayerGroup> groups; /* ordered by layer */
};

/* returns 0, -1 for an invalid layering, -2 for a HIP failure */
inline int layered_plan_create(LayeredPlan *pl, int32_t M, int32_t N, int64_t E,
                               const std::vector<int32_t> &row_ptr, const std::vector<int32_t> &cols,
                               int32_t layer_rows, int T, int V)
{
    if (layer_rows <= 0 || M % layer_rows) return -1;
    pl->M = M; pl->N = N; pl->E = E; pl->layer_rows = layer_rows; pl->T = T; pl->V = V;
    std::vector<int32_t> seen((size_t)N, -1);
    const int layers = M / layer_rows;
    for (int l = 0; l < layers; ++l) {
        std::map<int, std::vector<int32_t>> by_deg;
        for (int32_t m = l * layer_rows; m < (l + 1) * layer_rows; ++m) {
            for (int32_t p = row_ptr[m]; p < row_ptr[m + 1]; ++p) {
                if (seen[cols[p]] == l) return -1;  /* two rows of one layer share a column */
                seen[cols[p]] = l;
            }
            const int deg = row_ptr[m + 1] - row_ptr[m];
            if (deg > 0) by_deg[deg].push_back(row_ptr[m]);
        }
        for (auto &kv : by_deg) {
            LayerGroup g;
            g.layer = l; g.degree = kv.first; g.count = (int)kv.second.size();
            if (g.e0.upload(kv.second) != hipSuccess) return -2;
            pl->groups.push_back(std::move(g));
        }
    }
    const size_t TF = (size_t)T * 64 * V;
    const bool ok = pl->fixed()
                        ? pl->Pfx.alloc(TF * N) == hipSuccess && pl->Rfx.alloc(TF * (size_t)E) == hipSuccess
                        : pl->P.alloc(TF * N) == hipSuccess && pl->R.alloc(TF * (size_t)E) == hipSuccess;
    return ok ? 0 : -2;
}

struct LayeredRun : StreamRun {     /* engines.hpp */
    /* soft output (ldpc_decode_soft_device): the caller's [frames][N] buffer, nullptr = a plain call; extrinsic: P - y */
    float *soft = nullptr;
    int32_t soft_extrinsic = 0;
};

/* The launching code instantiates the kernels above: only the translation units that define LDPC_ENGINE_LAYERED compile
 * it, engine_layered.hip for StoreF32, engine_layered_fx.hip for StoreFx and engine_layered_bpfx.hip for the kernel table of
 * kLayerBpFx; the host driver calls engine_layered_run. */
#ifdef LDPC_ENGINE_LAYERED
template <class S> using LayerFn = void (*)(const typename S::Args, const MsCorr);
/* t[D] = the kernel of the rule for rows of degree D = 1 .. kMaxUnrolledLayerDegree, t[0] = the one for wider rows */
template <int V, int RULE, int... D0>
inline void layer_table_fill(LayerFn<RuleStore<RULE>> *t, std::integer_sequence<int, D0...>)
{
    if constexpr (RULE == kLayerHost) t[0] = nullptr;
    else t[0] = layer_kernel_generic<V, RULE>;
    ((t[D0 + 1] = layer_kernel<D0 + 1, V, RULE>), ...);
}

/* the kernels of kLayerBpFx at V frames per lane, instantiated in engine_layered_bpfx.hip so that they build beside the
 * other two units; the driver that launches them is engine_layered_fx.hip's */
void layer_table_bpfx(int V, LayerFn<StoreFx> *t);

template <int V, class S>
inline hipError_t layered_run_v(LayeredPlan *pl, const LayeredRun &r, hipStream_t s, int32_t *launched)
{
    constexpr int F = 64 * V;
    const LayerRule rule = pl->rule;
    const bool has_chan = S::kFixed || rule == kLayerBp;    /* P does not start at y (layer_chan) */
    typename S::P *const P = pl->template post<S>().p;
    typename S::R *const R = pl->template msgs<S>().p;
    const int tiles = (int)((r.frames + F - 1) / F);
    const size_t slot = (size_t)pl->T * V;
    LayerFn<S> table[kMaxUnrolledLayerDegree + 1];
    const std::make_integer_sequence<int, kMaxUnrolledLayerDegree> degrees;
    if constexpr (S::kFixed) {
        if (rule == kLayerBpFx) layer_table_bpfx(V, table);
        else layer_table_fill<V, kLayerFx>(table, degrees);
    }
    else if (rule == kLayerCorr) layer_table_fill<V, kLayerCorr>(table, degrees);
    else if (rule == kLayerBp) layer_table_fill<V, kLayerBp>(table, degrees);
    else if (rule == kLayerHost) layer_table_fill<V, kLayerHost>(table, degrees);
    else layer_table_fill<V, kLayerFused>(table, degrees);
    MsCorr corr{pl->ms_scale, pl->ms_offset};
    if constexpr (S::kFixed) {
        if (rule == kLayerBpFx) corr = bpfx_table_arg(pl->bp_table.p);
    }
    const int rounds = r.tap_iter ? (r.tap_iter < r.max_iter ? r.tap_iter : r.max_iter) : r.max_iter;
    hipError_t e;
    if ((e = hipMemsetAsync(r.failw, 0, (size_t)(r.max_iter + 2) * slot * sizeof(uint64_t), s))) return e;
    if ((e = hipMemsetAsync(r.summary, 0, (r.crc_bits ? 4 : 2) * sizeof(int32_t), s))) return e;
    if ((e = hipMemsetAsync(R, 0, (size_t)tiles * F * (size_t)pl->E * sizeof(typename S::R), s))) return e;
    {
        LayeredInitArgs<S> ia{r.llr.p, P, r.hard, r.frames, pl->N, rule == kLayerHost, r.llr.unit, pl->llr_scale, pl->L};
        dim3 grid((pl->N + kInitCols - 1) / kInitCols, tiles);
        dispatch_llr(r.llr.type, [&](auto in) {
            using IN = decltype(in);
            auto init = layered_init_kernel<V, IN, S, false>;
            if constexpr (!S::kFixed) {
                if (rule == kLayerBp) init = layered_init_kernel<V, IN, S, true>;
            }
            init<<<grid, kBlock, 0, s>>>(ia);
        });
        StateArgs st{r.done, nullptr, r.iters, nullptr, r.frames, 0, r.max_iter, 1};
        state_kernel<V><<<tiles, 64, 0, s>>>(st);
    }
    int it = 0;
    for (it = 1; it <= rounds; ++it) {
        for (auto &g : pl->groups) {
            typename S::Args a{};
            static_cast<LayerArgs<S> &>(a) = LayerArgs<S>{P, R, g.e0.p, r.edge_col, r.hard, r.done, pl->E, pl->N, g.count,
                                                         4, g.degree};
            if constexpr (S::kFixed) { a.L = pl->L; a.LP = pl->LP; }
            const int waves = (g.count + a.rows_per_wave - 1) / a.rows_per_wave;
            dim3 grid((waves + kWavesPerBlock - 1) / kWavesPerBlock, tiles);
            const int k = g.degree <= kMaxUnrolledLayerDegree ? g.degree : 0;
            if (!table[k]) return hipErrorInvalidValue;      /* host arithmetic: unrolled degrees only */
            if (r.span_begin && (e = r.span_begin(r.span_ctx, s, 2, g.degree,
                                                  S::kEdgeBytes * g.degree * g.count * r.frames))) return e;
            table[k]<<<grid, kBlock, 0, s>>>(a, corr);
            if (r.span_end && (e = r.span_end(r.span_ctx, s))) return e;
        }
        if constexpr (!S::kFixed) {
            if (rule == kLayerHost) {
                dim3 hgrid((pl->N + kWavesPerBlock - 1) / kWavesPerBlock, tiles);
                layered_hard_kernel<V><<<hgrid, kBlock, 0, s>>>(P, r.hard, r.done, pl->N);
            }
        }
        /* syndrome of this round's bits, freeze (decodeCL.c:393-410) */
        if (!r.early_term && it != rounds) continue;
        uint64_t *fw = r.failw + (size_t)it * slot;
        SyndromeArgs sa{r.row_ptr, r.edge_col, r.hard, fw, r.done, pl->M, pl->N, 0, 0};
        dim3 sgrid((pl->M + kBlock - 1) / kBlock, tiles);
        syndrome_kernel<V><<<sgrid, kBlock, 0, s>>>(sa);
        if (r.crc_bits) {       /* frames whose information bits pass the CRC count as clean (crc_term_kernels.hpp) */
            CrcTermArgs ca{r.hard, fw, r.done, r.crc_w, r.summary + 3, pl->N, r.crc_bits, TailRef{nullptr, 0, 0}};
            crc_term_kernel<V><<<dim3((unsigned)tiles, V), 64 * crc_term_waves(r.crc_bits), 0, s>>>(ca);
        }
        if (r.soft) {
            /* soft_i (soft_kernels.hpp): `done` still holds the frames frozen before this round and fw this round's
             * verdict; the frames that settle now leave P -- the posterior after the round's last layer, which later
             * rounds overwrite -- in the caller's buffer, as floats.  In the last round launched every running frame
             * settles.  A rule with a chan of its own gets its extrinsic values in one pass at the end. */
            SoftArgs so{P, nullptr, nullptr, nullptr, r.done, (r.early_term && it < rounds) ? fw : nullptr, r.soft,
                        r.llr.p, nullptr, nullptr, pl->E, r.frames, pl->N, has_chan ? 0 : r.soft_extrinsic, TailRef{nullptr, 0, 0}, r.llr.unit};
            const dim3 grid((unsigned)((pl->N + kInitCols - 1) / kInitCols), (unsigned)tiles);
            if (r.span_begin && (e = r.span_begin(r.span_ctx, s, /*soft_settle_kernel*/ 7, 0, S::kSettleBytes * pl->N * r.frames))) return e;
            if constexpr (S::kFixed) {
                soft_settle_kernel<V, p16, float><<<grid, kBlock, 0, s>>>(so);       /* reads no llr: extrinsic is 0 */
            } else {
                dispatch_llr(r.llr.type, [&](auto in) { soft_settle_kernel<V, float, decltype(in)><<<grid, kBlock, 0, s>>>(so); });
            }
            if (r.span_end && (e = r.span_end(r.span_ctx, s))) return e;
        }
        StateArgs st{r.done, fw, r.iters, nullptr, r.frames, it, r.max_iter, 1};
        state_kernel<V><<<tiles, 64, 0, s>>>(st);
    }
    if (has_chan && r.soft && r.soft_extrinsic) {       /* posterior - chan (layered_extrinsic_kernel) */
        const int64_t count = r.frames * (int64_t)pl->N;
        dispatch_llr(r.llr.type, [&](auto in) {
            using IN = decltype(in);
            layered_extrinsic_kernel<IN, S><<<(unsigned)((count + kBlock - 1) / kBlock), kBlock, 0, s>>>(
                r.soft, static_cast<const IN *>(r.llr.p), pl->llr_scale, pl->L, count, r.llr.unit);
        });
    }
    *launched = rounds;
    PackArgs pa{r.hard, r.out_dev, r.iters, r.iters_dev, r.frames, r.out_bytes, pl->N, r.K, r.pack_mode};
    if (r.out_dev || r.iters_dev) {     /* the pack launch carries the iteration counts too (out_dev NULL: out_bytes is 0) */
        if (r.pack_mode == 0) {
            pack_kernel<V><<<pack_grid<V>(r.K, tiles), kBlock, 0, s>>>(pa);
        } else {
            const int64_t n = r.out_bytes > r.frames ? r.out_bytes : r.frames;
            pack_kernel<V><<<(unsigned)((n + kBlock - 1) / kBlock), kBlock, 0, s>>>(pa);
        }
    }
    layered_summary_kernel<V><<<(unsigned)((r.frames + 255) / 256), 256, 0, s>>>(r.iters, r.done, r.frames,
                                                                                 r.summary);
    return hipGetLastError();
}

template <class S>
inline hipError_t layered_run(LayeredPlan *pl, const LayeredRun &r, hipStream_t s, int32_t *launched)
{
    if (pl->V == 1) return layered_run_v<1, S>(pl, r, s, launched);
    if (pl->V == 2) return layered_run_v<2, S>(pl, r, s, launched);
    return layered_run_v<4, S>(pl, r, s, launched);
}
#endif  /* LDPC_ENGINE_LAYERED */

/* one tile of `count` elements of T from the device, widened to float */
template <typename T> inline hipError_t layered_tile_to_host(std::vector<float> &tile, const void *dev)
{
    std::vector<T> raw(tile.size());
    const hipError_t e = hipMemcpy(raw.data(), dev, raw.size() * sizeof(T), hipMemcpyDeviceToHost);
    std::copy(raw.begin(), raw.end(), tile.begin());
    return e;
}

/* which: 0 = R [frame][E], 2 = P [frame][N], 3 = bits [frame][N] */
inline hipError_t layered_dump(LayeredPlan *pl, int which, float *host_out, int64_t count, int64_t frames,
                               const uint64_t *hard_dev, const int32_t *)
{
    const int V = pl->V, F = 64 * V;
    const int tiles = (int)((frames + F - 1) / F);
    if (which == 0 || which == 2) {
        const int64_t per = which == 0 ? pl->E : pl->N;
        if (count != frames * per) return hipErrorInvalidValue;
        const bool fx = pl->fixed();                /* R bytes and P int16, widened */
        std::vector<float> tile((size_t)per * F);
        for (int t = 0; t < tiles; ++t) {
            const size_t at = (size_t)t * per * F;
            const hipError_t e = which == 0 ? (fx ? layered_tile_to_host<int8_t>(tile, pl->Rfx.p + at)
                                                  : layered_tile_to_host<float>(tile, pl->R.p + at))
                                            : (fx ? layered_tile_to_host<int16_t>(tile, pl->Pfx.p + at)
                                                  : layered_tile_to_host<float>(tile, pl->P.p + at));
            if (e != hipSuccess) return e;
            for (int fi = 0; fi < F; ++fi) {
                const int64_t f = (int64_t)t * F + fi;
                if (f >= frames) break;
                for (int64_t i = 0; i < per; ++i) host_out[f * per + i] = tile[(size_t)i * F + fi];
            }
        }
        return hipSuccess;
    }
    if (which == 3) {
        if (count != frames * pl->N) return hipErrorInvalidValue;
        std::vector<uint64_t> w((size_t)tiles * pl->N * V);
        hipError_t e = hipMemcpy(w.data(), hard_dev, w.size() * sizeof(uint64_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        for (int64_t f = 0; f < frames; ++f) {
            const int64_t t = f / F;
            const int fi = (int)(f % F);
            for (int32_t n = 0; n < pl->N; ++n)
                host_out[f * pl->N + n] = (float)((w[((size_t)t * pl->N + n) * V + fi % V] >> (fi / V)) & 1ull);
        }
        return hipSuccess;
    }
    return hipErrorInvalidValue;
}

}  // namespace ldpc
