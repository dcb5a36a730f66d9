/*
 * flood_common.hpp -- what every streaming flooding kernel shares: the V-wide stream loads and stores, the
 * tile a block works on (tile_finished / tile_select / GridPos), the argument blocks of the message kernels
 * (CheckArgs, VarArgs, GroupClass), the Q slots of a row, the min-sum correction and the bit-field helper of the
 * hard masks.  Layout and design: flood_kernels.hpp.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ldpc {

constexpr int kAlgoSP = 0;
constexpr int kAlgoMS = 1;
constexpr int kAlgoMSC = 2;   /* min-sum with the normalized / offset correction (check_ms, MsCorr) */
constexpr int kAlgoBP = 3;    /* log-domain sum-product: min-sum's variable node, box-plus check node (check_bp) */
constexpr int kCompactCapacity = 512;   /* frames a child decoder takes over (8 tiles of 64) */
constexpr int kLastCapacity = 64;       /* ... and the last decoder of the chain: one tile */
constexpr int kBlock = 256;          /* 4 waves */
constexpr int kWavesPerBlock = 4;
constexpr int kMaxUnrolledDegree = 16;       /* variable-node kernels, sum-product check kernels */
constexpr int kMaxUnrolledCheckDegreeMS = 32; /* min-sum check rows: O(D) registers in narrow waves */

/* ---- V-wide per-lane vectors --------------------------------------------- */
/* Message streams are touched once per kernel (7.4 GB per launch at B = 4096):
 * LDPC_NT_LOAD / LDPC_NT_STORE = 1 mark them non-temporal (measured on MI355X: both on
 * -4.3 % step time, loads only +2.8 %, stores only -1.6 %). */
#ifndef LDPC_NT_LOAD
#define LDPC_NT_LOAD 1
#endif
#ifndef LDPC_NT_STORE
#define LDPC_NT_STORE 1
#endif
typedef float vf2 __attribute__((ext_vector_type(2)));
typedef float vf4 __attribute__((ext_vector_type(4)));

template <typename T> __device__ __forceinline__ T ld_stream(const T *p)
{
#if LDPC_NT_LOAD
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
template <typename T> __device__ __forceinline__ void st_stream(T *p, T v)
{
#if LDPC_NT_STORE
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

template <int V> __device__ __forceinline__ void vload(float (&d)[V], const float *p);
template <> __device__ __forceinline__ void vload<1>(float (&d)[1], const float *p) { d[0] = ld_stream(p); }
template <> __device__ __forceinline__ void vload<2>(float (&d)[2], const float *p)
{
    const vf2 t = ld_stream(reinterpret_cast<const vf2 *>(p));
    d[0] = t.x; d[1] = t.y;
}
template <> __device__ __forceinline__ void vload<4>(float (&d)[4], const float *p)
{
    const vf4 t = ld_stream(reinterpret_cast<const vf4 *>(p));
    d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
}
template <int V> __device__ __forceinline__ void vstore(float *p, const float (&s)[V]);
template <> __device__ __forceinline__ void vstore<1>(float *p, const float (&s)[1]) { st_stream(p, s[0]); }
template <> __device__ __forceinline__ void vstore<2>(float *p, const float (&s)[2])
{
    vf2 t; t.x = s[0]; t.y = s[1];
    st_stream(reinterpret_cast<vf2 *>(p), t);
}
template <> __device__ __forceinline__ void vstore<4>(float *p, const float (&s)[4])
{
    vf4 t; t.x = s[0]; t.y = s[1]; t.z = s[2]; t.w = s[3];
    st_stream(reinterpret_cast<vf4 *>(p), t);
}

/* fp16 message storage (msg_dtype = LDPC_MSG_F16): 2 bytes per message, arithmetic in fp32.
 * Loads widen exactly; stores round to nearest even. */
typedef _Float16 hf;
typedef _Float16 vh2 __attribute__((ext_vector_type(2)));
typedef _Float16 vh4 __attribute__((ext_vector_type(4)));

template <int V> __device__ __forceinline__ void vload(float (&d)[V], const hf *p);
template <> __device__ __forceinline__ void vload<1>(float (&d)[1], const hf *p) { d[0] = (float)ld_stream(p); }
template <> __device__ __forceinline__ void vload<2>(float (&d)[2], const hf *p)
{
    const vh2 t = ld_stream(reinterpret_cast<const vh2 *>(p));
    d[0] = (float)t.x; d[1] = (float)t.y;
}
template <> __device__ __forceinline__ void vload<4>(float (&d)[4], const hf *p)
{
    const vh4 t = ld_stream(reinterpret_cast<const vh4 *>(p));
    d[0] = (float)t.x; d[1] = (float)t.y; d[2] = (float)t.z; d[3] = (float)t.w;
}
template <int V> __device__ __forceinline__ void vstore(hf *p, const float (&s)[V]);
template <> __device__ __forceinline__ void vstore<1>(hf *p, const float (&s)[1]) { st_stream(p, (hf)s[0]); }
template <> __device__ __forceinline__ void vstore<2>(hf *p, const float (&s)[2])
{
    vh2 t; t.x = (hf)s[0]; t.y = (hf)s[1];
    st_stream(reinterpret_cast<vh2 *>(p), t);
}
template <> __device__ __forceinline__ void vstore<4>(hf *p, const float (&s)[4])
{
    vh4 t; t.x = (hf)s[0]; t.y = (hf)s[1]; t.z = (hf)s[2]; t.w = (hf)s[3];
    st_stream(reinterpret_cast<vh4 *>(p), t);
}

/* fp8 message storage (msg_dtype = LDPC_MSG_F8): one OCP E4M3 byte per message (1-4-3, bias 7, subnormals down to
 * 2^-9, no infinities), arithmetic in fp32.  Loads widen exactly.  Stores apply s8 (include/ldpc_hip.h): NaN stays
 * NaN, everything else is clamped to [-448, 448] and rounded to nearest, ties to even, the sign of zero kept.  The
 * clamp is ours, in fp32, in front of the conversion instruction: what v_cvt_pk_fp8_f32 does out of range depends
 * on the wave's mode bits and is not relied on.  fminf / fmaxf drop a NaN, hence the select behind the clamp.
 * A struct, so that the overloads below are told apart from plain bytes; (f8)0 is the byte 0x00 = +0, which is what the
 * hand-over kernels (flood_handover.hpp) fill unused slots with. */
struct f8 {
    uint8_t bits;
    f8() = default;
    __host__ __device__ constexpr explicit f8(int) : bits(0) {}
};
static_assert(sizeof(f8) == 1, "one byte per message");

constexpr float kF8Max = 448.0f;
__device__ __forceinline__ float f8_clamp(float x)
{
    const float c = fminf(fmaxf(x, -kF8Max), kF8Max);
    return x != x ? x : c;
}
/* two values as E4M3 into the low (hi = false) or high half of a dword, the other half kept from `old` */
__device__ __forceinline__ int f8_pack2(float a, float b, int old, bool hi)
{
    return hi ? __builtin_amdgcn_cvt_pk_fp8_f32(f8_clamp(a), f8_clamp(b), old, true)
              : __builtin_amdgcn_cvt_pk_fp8_f32(f8_clamp(a), f8_clamp(b), old, false);
}
/* s8 as a float: the value a message has once it is stored */
__device__ __forceinline__ float f8_round(float x)
{
    return __builtin_amdgcn_cvt_f32_fp8(f8_pack2(x, x, 0, false), 0);
}

template <int V> __device__ __forceinline__ void vload(float (&d)[V], const f8 *p);
template <> __device__ __forceinline__ void vload<1>(float (&d)[1], const f8 *p)
{
    d[0] = __builtin_amdgcn_cvt_f32_fp8((int)ld_stream(reinterpret_cast<const uint8_t *>(p)), 0);
}
template <> __device__ __forceinline__ void vload<2>(float (&d)[2], const f8 *p)
{
    const int w = (int)ld_stream(reinterpret_cast<const uint16_t *>(p));
    d[0] = __builtin_amdgcn_cvt_f32_fp8(w, 0); d[1] = __builtin_amdgcn_cvt_f32_fp8(w, 1);
}
template <> __device__ __forceinline__ void vload<4>(float (&d)[4], const f8 *p)
{
    const int w = (int)ld_stream(reinterpret_cast<const uint32_t *>(p));
    d[0] = __builtin_amdgcn_cvt_f32_fp8(w, 0); d[1] = __builtin_amdgcn_cvt_f32_fp8(w, 1);
    d[2] = __builtin_amdgcn_cvt_f32_fp8(w, 2); d[3] = __builtin_amdgcn_cvt_f32_fp8(w, 3);
}
template <int V> __device__ __forceinline__ void vstore(f8 *p, const float (&s)[V]);
template <> __device__ __forceinline__ void vstore<1>(f8 *p, const float (&s)[1])
{
    st_stream(reinterpret_cast<uint8_t *>(p), (uint8_t)f8_pack2(s[0], s[0], 0, false));
}
template <> __device__ __forceinline__ void vstore<2>(f8 *p, const float (&s)[2])
{
    st_stream(reinterpret_cast<uint16_t *>(p), (uint16_t)f8_pack2(s[0], s[1], 0, false));
}
template <> __device__ __forceinline__ void vstore<4>(f8 *p, const float (&s)[4])
{
    const int lo = f8_pack2(s[0], s[1], 0, false);
    st_stream(reinterpret_cast<uint32_t *>(p), (uint32_t)f8_pack2(s[2], s[3], lo, true));
}

/* fixed-point message storage (msg_dtype = LDPC_MSG_I8, msg_bits = q): one two's-complement byte per message holding
 * an integer in [-L, L], L = 2^(q-1) - 1 a compile-time parameter; arithmetic in fp32, which is exact integer arithmetic
 * here (every sum stays far below 2^24).  Loads sign-extend and widen exactly.  Stores apply sq (include/ldpc_hip.h):
 * clamp to [-L, L] in fp32 (one v_med3_f32; nothing out of range ever reaches a conversion), then ONE add of
 * 1.5 * 2^23: in [2^23, 2^24) the fp32 grid is the integers, so the add itself rounds to nearest, ties to even, and the
 * low byte of the sum's bit pattern (0x4B400000 + n) is n in two's complement -- no v_rndne_f32, no v_cvt_i32_f32, no
 * mask.  v_perm_b32 gathers the low bytes: 4 messages are 4 med3 + 4 add + 2 perm + 1 or = 2.75 VALU instructions per
 * message (the fp8 store: 3.5), a load one v_cvt_f32_i32 with an SDWA byte select and sign extension per message.  -0 gives the byte 0; the code -128
 * is never produced.  sq's NaN case can only come from the caller's channel values -- a stored message is never NaN or
 * infinite -- and is settled there, once per channel value (MsgChan), not in every store; a NaN that did reach a store
 * would leave v_med3_f32 as -L, in range.  (T)0 is the byte 0x00, the zero message of the hand-over kernels. */
template <int L> struct q8 {
    int8_t bits;
    q8() = default;
    __host__ __device__ constexpr explicit q8(int) : bits(0) {}
};
static_assert(sizeof(q8<127>) == 1, "one byte per message");

constexpr float kQ8Magic = 12582912.0f;     /* 1.5 * 2^23 */
/* sq(x) as a dword whose LOW BYTE is the code (the upper bytes are the magic number's and are dropped by the pack) */
template <int L> __device__ __forceinline__ uint32_t q8_code(float x)
{
    return __float_as_uint(__builtin_amdgcn_fmed3f(x, -(float)L, (float)L) + kQ8Magic);
}

template <int V, int L> __device__ __forceinline__ void vload(float (&d)[V], const q8<L> *p)
{
    static_assert(V == 1 || V == 2 || V == 4, "1, 2 or 4 messages per lane");
    if constexpr (V == 1) {
        d[0] = (float)(int)ld_stream(reinterpret_cast<const int8_t *>(p));
    } else if constexpr (V == 2) {
        const int w = (int)ld_stream(reinterpret_cast<const int16_t *>(p));     /* sign-extended: the high byte is ready */
        d[0] = (float)(int)(int8_t)w; d[1] = (float)(w >> 8);
    } else {
        const int w = (int)ld_stream(reinterpret_cast<const uint32_t *>(p));
        d[0] = (float)(int)(int8_t)w; d[1] = (float)(int)(int8_t)(w >> 8);
        d[2] = (float)(int)(int8_t)(w >> 16); d[3] = (float)(w >> 24);
    }
}
template <int V, int L> __device__ __forceinline__ void vstore(q8<L> *p, const float (&s)[V])
{
    static_assert(V == 1 || V == 2 || V == 4, "1, 2 or 4 messages per lane");
    /* v_perm_b32 selectors: 0..3 bytes of the second operand, 4..7 of the first, 0x0c the constant 0 */
    if constexpr (V == 1) {
        st_stream(reinterpret_cast<uint8_t *>(p), (uint8_t)q8_code<L>(s[0]));
    } else if constexpr (V == 2) {
        st_stream(reinterpret_cast<uint16_t *>(p), (uint16_t)__builtin_amdgcn_perm(q8_code<L>(s[1]), q8_code<L>(s[0]), 0x0c0c0400u));
    } else {
        const uint32_t lo = __builtin_amdgcn_perm(q8_code<L>(s[1]), q8_code<L>(s[0]), 0x0c0c0400u);
        const uint32_t hi = __builtin_amdgcn_perm(q8_code<L>(s[3]), q8_code<L>(s[2]), 0x04000c0cu);
        st_stream(reinterpret_cast<uint32_t *>(p), lo | hi);
    }
}

/* a check->variable magnitude as its storage type holds it, applied where the message is produced: the column-fused
 * kernels keep some R in registers without ever storing them.  Fixed point: the corrected magnitude is truncated, as
 * hardware does it ((3m) >> 2 for ms_scale = 0.75), and saturates at L */
template <typename T> struct MsgRound;
template <> struct MsgRound<float> { static __device__ __forceinline__ float of(float r) { return r; } };
template <> struct MsgRound<hf> { static __device__ __forceinline__ float of(float r) { return (float)(hf)r; } };
template <> struct MsgRound<f8> { static __device__ __forceinline__ float of(float r) { return f8_round(r); } };
template <int L> struct MsgRound<q8<L>> { static __device__ __forceinline__ float of(float r) { return fminf(truncf(r), (float)L); } };
/* plain min-sum: a row's magnitude candidates are |q| of stored messages -- values of T already -- or the start value
 * 1000, which no E4M3 value reaches: it reads 448; fixed point: L */
template <typename T> struct MsgStart { static __device__ __forceinline__ float of(float m) { return m; } };
template <> struct MsgStart<f8> { static __device__ __forceinline__ float of(float m) { return fminf(m, kF8Max); } };
template <int L> struct MsgStart<q8<L>> { static __device__ __forceinline__ float of(float m) { return fminf(m, (float)L); } };
/* the min-sum channel value in front of its store: y as it is for the floating-point types; fixed point: llr_scale * y,
 * one fp32 multiply, the number of LSBs, with sq's NaN -> 0 (the store does the rest of sq) */
template <typename T> struct MsgChan { static __device__ __forceinline__ float of(float y, float) { return y; } };
template <int L> struct MsgChan<q8<L>> {
    static __device__ __forceinline__ float of(float y, float llr_scale)
    {
        const float t = llr_scale * y;
        return t != t ? 0.0f : t;
    }
};
/* message kinds whose one-byte elements only differ in how a STORE converts: kernels that load, copy and zero-fill
 * (hand-over, soft output) are instantiated once, for q8<127> */
typedef q8<127> q8any;

__device__ __forceinline__ int wave_id_in_block()
{
    return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

template <int V> __device__ __forceinline__ bool tile_finished(const uint64_t *done, int tile)
{
    bool all = true;
#pragma unroll
    for (int v = 0; v < V; ++v) all = all && (done[(size_t)tile * V + v] == ~0ull);
    return all;
}

/* ---- device-side tail (early termination without host polling) --------------------------------
 * An asynchronous caller has all max_iter rounds enqueued up front.  When only a few frames of a
 * large batch are still running, tail_gather_kernel (below) moves their state into `n_tiles`
 * OVERFLOW tiles that follow the batch's own tiles in every array and flips state[0]; from then on
 * the blocks of the first n_tiles grid rows of every launch work on the overflow tiles and all
 * other blocks leave at once -- the decision is taken on the device, no launch is added per round
 * except the (empty) gather attempt.  state == nullptr: feature off. */
struct TailRef {
    const int32_t *state;   /* [0] handed over, [1] frames handed over, [2] round of the hand-over */
    int32_t base_tile;      /* index of the first overflow tile = tiles of max_batch */
    int32_t n_tiles;        /* overflow tiles */
};

/* The tile a block with grid row `row` works on, or -1 if it has nothing to do. */
template <int V> __device__ __forceinline__ int tile_select(const TailRef &t, const uint64_t *done, int row)
{
    int tile = row;
    if (t.state && __builtin_amdgcn_readfirstlane(t.state[0])) {
        if (row >= t.n_tiles) return -1;
        tile = t.base_tile + row;
    }
    return tile_finished<V>(done, tile) ? -1 : tile;
}

struct CheckArgs {
    const void *__restrict__ Q;          /* [T][E][F] variable->check (float, fp16 or fp8) */
    void *__restrict__ R;                /* [T][E][F] check->variable          */
    const int32_t *__restrict__ cls_e0;  /* [n_rows] first edge id of each row of this degree class */
    const uint64_t *__restrict__ done;   /* [T][V] frozen frames                */
    int64_t E;
    int32_t n_rows;
    int32_t rows_per_wave;
    int32_t degree;                      /* generic kernel only */
    float ms_scale = 1.0f;               /* kAlgoMSC only: alpha (fills what was padding before `tail`) */
    TailRef tail;
    int32_t tiles_first = 0;             /* grid is (tiles, blocks) instead of (blocks, tiles): grid_pos() */
    float ms_offset = 0.0f;              /* kAlgoMSC only: beta (fills what was padding before `first_chan`) */
    /* min-sum, round 1 only: the variable->check messages of round 0 are the channel values (decodeInitMS,
     * decodeCL.c:121: q = y), so they are read from the channel array by column instead of from Q, which the input
     * transpose then does not have to write at all (a third of its traffic).  nullptr: read Q. */
    const void *__restrict__ first_chan = nullptr;     /* [T][N][F] */
    /* [E] column of every edge; like qpos never null in a launch, also where first_chan is: the side of check_rows'
     * choice that is not taken may still issue its wave-uniform (scalar) index load under an empty exec mask */
    const int32_t *__restrict__ edge_col = nullptr;
    int32_t N = 0;
    /* Where the variable->check message of edge e lives in Q: slot qpos[e] (nullptr: slot e).  Q is stored in the
     * order its WRITERS produce it -- the variable-node kernels column by column, then the column-fused check
     * kernel's own edges row by row -- so that every store of a round streams; the check kernels, which read Q,
     * gather instead (tools/gather_probe.hip: random 1-KiB reads cost nothing, random writes 9-15 %). */
    const int32_t *__restrict__ qpos = nullptr;        /* [E]; never null in a launch (the identity where Q is in edge order) */
};

/* Q slots (CheckArgs::qpos) of the D edges e0 ... of a row: ONE load by the wave's first D lanes and a broadcast each.
 * The values are wave-uniform, so a message's address is a scalar row address plus the lane's 32-bit offset (the
 * slots of a row are unrelated: one 64-bit vector address each would cost two registers per message in flight). */
template <int D> __device__ __forceinline__ void row_slots(const int32_t *__restrict__ qpos, int e0, int lane, int (&slot)[D])
{
    static_assert(D <= 64, "one lane per edge");
    const int mine = qpos[e0 + (lane < D ? lane : D - 1)];
#pragma unroll
    for (int k = 0; k < D; ++k) slot[k] = __builtin_amdgcn_readlane(mine, k);
}
/* slot of one edge */
__device__ __forceinline__ int edge_slot(const int32_t *__restrict__ qpos, int e)
{
    return __builtin_amdgcn_readfirstlane(qpos[e]);
}

/* Where a block stands in the launch.  Blocks are dispatched with blockIdx.x varying fastest: a grid of
 * (tiles, blocks) therefore has the blocks in flight at any moment spread over ALL tiles of the batch --
 * sixteen regions 58 MB apart instead of one moving window -- which the memory system rewards (the
 * column-fused check kernel: 1.39 -> 1.27 ms, profiles/r02_ab_tile_fastest_grid.txt).  The host asks for it
 * whenever the block count fits gridDim.y. */
struct GridPos { int row, block; };
__device__ __forceinline__ GridPos grid_pos(int tiles_first)
{
    return tiles_first ? GridPos{(int)blockIdx.x, (int)blockIdx.y} : GridPos{(int)blockIdx.y, (int)blockIdx.x};
}

/* Normalized / offset min-sum (LDPC_ALGO_MS / LAYERED with ms_scale or ms_offset set): each of a row's
 * two magnitude candidates m becomes fmaxf(m - beta, 0) * alpha, fp32, once per row and frame, before the
 * per-edge selection and sign.  With fp16 or fp8 messages the result is rounded to the storage type right here,
 * where R is produced (MsgRound): alpha * m is generally no binary16 / E4M3 value (+-min always was), and the
 * column-fused kernels keep some R in registers without ever storing them. */
struct MsCorr {
    float scale, offset;
};
template <typename T> __device__ __forceinline__ float ms_corr(float m, const MsCorr &c)
{
    const float r = fmaxf(m - c.offset, 0.0f) * c.scale;
    return MsgRound<T>::of(r);
}

__device__ __forceinline__ MsCorr ms_corr_of(const CheckArgs &a) { return MsCorr{a.ms_scale, a.ms_offset}; }

struct VarArgs {
    const void *__restrict__ R;           /* [T][E][F] (float, fp16 or fp8) */
    void *__restrict__ Q;                 /* [T][E][F] */
    const void *__restrict__ chan;        /* [T][N][F] SP: exp(scale*y); MS: y; BP: scale*y */
    uint64_t *hard;                       /* [T][N][V] read-modify-write */
    const uint64_t *__restrict__ done;    /* [T][V] */
    const int32_t *__restrict__ cls_col;  /* [n_cols] column ids of this degree class */
    const int32_t *__restrict__ cls_edge; /* [n_cols][D] edge ids, ascending */
    int64_t E;
    int32_t N;
    int32_t n_cols;
    int32_t cols_per_wave;
    int32_t write_q;                      /* 0 on the last round (MyLdpc.cpp:1035-1040) */
    int32_t degree;                       /* generic kernel only */
    TailRef tail;
    int32_t tiles_first = 0;              /* grid is (tiles, blocks): grid_pos() */
    /* first Q slot of this class (CheckArgs::qpos: Q is stored in the order its writers produce it): the class owns D
     * streams of n_cols slots, column ci writes message k to slot q_base + k * n_cols + ci -- the waves at work at any
     * moment write D moving fronts (tools/gather_probe.hip: 6079 GB/s, against 5540 with one 8-KiB run per column and
     * 5065 with the messages scattered to their edge ids).  -1: slot = edge id. */
    int64_t q_base = -1;
};

/* ---- several degree classes in ONE launch -------------------------------------------------
 * A round used to cost one launch per row / column degree class (DVB-S2 rate 1/2: 2 + 4, two of
 * them a single row / column).  A group launch covers every class of a degree bucket: the table
 * says which block range belongs to which class, the block's (wave-uniform) degree picks the
 * unrolled body.  Same bodies, same operation order, same bits; registers are those of the
 * bucket's widest degree, hence the buckets. */
struct GroupClass {
    int32_t block_begin;        /* first blockIdx.x of this class */
    int32_t degree;
    int32_t count;              /* rows / columns */
    int32_t pad;
    const int32_t *ids;         /* rows: first edge ids; columns: column ids */
    const int32_t *edges;       /* columns: [count][degree] edge ids */
    int64_t q_base;             /* columns: first Q slot of the class's D streams (VarArgs::q_base), -1: slot = edge id */
};

/* Bits of x at positions 0, V, 2V, ... gathered into the low 64/V bits (V = 1, 2, 4). */
template <int V> __device__ __forceinline__ uint64_t compress_stride(uint64_t x)
{
    if (V == 1) return x;
    if (V == 2) {
        x &= 0x5555555555555555ull;
        x = (x | (x >> 1)) & 0x3333333333333333ull;
        x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
        x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull;
        x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
        x = (x | (x >> 16)) & 0x00000000ffffffffull;
        return x;
    }
    x &= 0x1111111111111111ull;
    x = (x | (x >> 3)) & 0x0303030303030303ull;
    x = (x | (x >> 6)) & 0x000f000f000f000full;
    x = (x | (x >> 12)) & 0x000000ff000000ffull;
    x = (x | (x >> 24)) & 0x000000000000ffffull;
    return x;
}

}  // namespace ldpc
