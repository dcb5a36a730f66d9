/*
 * llr_input.hpp -- channel values that arrive narrower than fp32 (include/ldpc_hip.h: enum ldpc_llr_type): what the
 * driver hands an engine in place of a float pointer (LlrIn), the one rule that turns an element into the value the
 * decoders read (llr_value), the tile-patch loader the streaming init kernels share (llr_patch_fill), and the two small
 * kernels around it: llr_widen_kernel (typed -> float, for the one-launch and record kernels, which read `llr` deep
 * inside large kernels and stay as they are) and llr_quantize_kernel (the sender's side: float -> typed).
 *
 * The rule: y = (float)x * llr_unit, one fp32 multiply; the widening is exact.  y is a value of its own: whatever a
 * decoder does next (llr_scale * y, exp, the rounding to fp16 / E4M3 where it is stored) starts from the rounded
 * product.  The library is built without contraction; the empty asm behind the multiply says the same to the backend,
 * which would otherwise be free to fold a following conversion to fp16 into the multiply (v_fma_mixlo_f16), as
 * init_kernel's BP branch notes.  A float element is passed through untouched: no multiply by 1.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace ldpc {

/* enum ldpc_llr_type, for the headers that do not see the C ABI (ldpc_hip.hip asserts the equality) */
constexpr int kLlrF32 = 0, kLlrF16 = 1, kLlrI8 = 2;

/* the caller's channel buffer as the engines get it */
struct LlrIn {
    const void *p = nullptr;    /* [frames][N] elements of `type`, frame-major */
    int32_t type = kLlrF32;
    float unit = 1.0f;          /* exactly 1 for kLlrF32 */
};
inline LlrIn llr_in_float(const float *p) { return LlrIn{p, kLlrF32, 1.0f}; }
inline size_t llr_elem_size(int type) { return type == kLlrI8 ? 1 : type == kLlrF16 ? 2 : 4; }

/* the run-time element type as a type: fn(float{}), fn(_Float16{}) or fn(int8_t{}) */
template <typename Fn> inline void dispatch_llr(int type, Fn &&fn)
{
    if (type == kLlrI8) fn(int8_t{}); else if (type == kLlrF16) fn(_Float16{}); else fn(float{});
}

template <typename IN> __device__ __forceinline__ float llr_value(IN x, float unit)
{
    if constexpr (std::is_same<IN, float>::value) {
        return x;
    } else {
        float y = (float)x * unit;          /* int8 and binary16 widen exactly (inf and NaN as they are) */
        asm volatile("" : "+v"(y));
        return y;
    }
}

/* 16 bytes of narrow elements from a 16-byte aligned address */
template <typename IN> __device__ __forceinline__ void llr_load16(float (&y)[16 / sizeof(IN)], const IN *p, float unit)
{
    static_assert(sizeof(IN) == 1 || sizeof(IN) == 2, "narrow element types only");
    const uint4 raw = *reinterpret_cast<const uint4 *>(p);
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
    if constexpr (sizeof(IN) == 1) {
#pragma unroll
        for (int j = 0; j < 16; ++j) y[j] = llr_value<int8_t>((int8_t)(w[j >> 2] >> (8 * (j & 3))), unit);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint16_t h = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
            y[j] = llr_value<_Float16>(__builtin_bit_cast(_Float16, h), unit);
        }
    }
}

/* The input side of the streaming init kernels for a narrow element type: the COLS columns from n0 of the F frames of
 * `tile` into patch[column * LD + frame], as y (SCALED: as scale * y, a second multiply); frames past `frames` and
 * columns past N read y = +1.0f exactly.  Block of BLOCK threads.
 *   16-byte path: 16 int8 or 8 fp16 values per load, the lanes of a frame side by side -- only where the address, the
 *     row stride N * sizeof(IN) and the patch (all COLS columns inside N) allow it.  Rows of 648 int8 values do not: they
 *     start at every residue of 8 mod 16.
 *   otherwise one element per lane and pass, COLS consecutive elements of a frame per COLS lanes: byte and short loads
 *     that the memory pipeline merges per wave like the float kernel's dwords. */
template <typename IN, int F, int LD, int COLS, int BLOCK, bool SCALED>
__device__ __forceinline__ void llr_patch_fill(float *patch, const IN *__restrict__ llr, float unit, int64_t frames, int32_t N,
                                               int tile, int n0, float scale)
{
    constexpr int PER = 16 / (int)sizeof(IN);       /* elements per 16-byte load */
    constexpr int LPF = COLS / PER;                 /* lanes per frame */
    constexpr int FPP = BLOCK / LPF;                /* frames per pass */
    static_assert(COLS % PER == 0 && BLOCK % LPF == 0, "patch width is a whole number of 16-byte loads");
    const bool wide = ((size_t)N * sizeof(IN)) % 16 == 0 && n0 + COLS <= N && (reinterpret_cast<uintptr_t>(llr) & 15) == 0;
    if (wide) {
        const int c0 = ((int)threadIdx.x % LPF) * PER;
        for (int f = (int)threadIdx.x / LPF; f < F; f += FPP) {
            const int64_t frame = (int64_t)tile * F + f;
            float y[PER];
#pragma unroll
            for (int j = 0; j < PER; ++j) y[j] = 1.0f;
            if (frame < frames) llr_load16<IN>(y, llr + (size_t)frame * N + n0 + c0, unit);
#pragma unroll
            for (int j = 0; j < PER; ++j) patch[(c0 + j) * LD + f] = SCALED ? scale * y[j] : y[j];
        }
    } else {
        const int c = threadIdx.x & (COLS - 1);
        const int n = n0 + c;
        for (int f = threadIdx.x / COLS; f < F; f += BLOCK / COLS) {
            const int64_t frame = (int64_t)tile * F + f;
            float y = 1.0f;
            if (frame < frames && n < N) y = llr_value<IN>(llr[(size_t)frame * N + n], unit);
            if (SCALED) y = scale * y;
            patch[c * LD + f] = y;
        }
    }
}

/* y[i] = x[i] * unit for the one-launch and record kernels: one pass into a float buffer the handle owns */
template <typename IN>
__global__ __launch_bounds__(256) void llr_widen_kernel(const IN *__restrict__ x, float unit, float *__restrict__ y, int64_t count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) y[i] = llr_value<IN>(x[i], unit);
}

/* The sender's side (ldpc_llr_quantize_device): t = y / unit, one IEEE fp32 divide.
 *   int8:     NaN -> 0, else rintf(t) (ties to even) clamped to [-127, 127]; -128 is never produced.
 *   binary16: NaN stays NaN, else t clamped to +-65504 and rounded to nearest even. */
template <typename OUT>
__global__ __launch_bounds__(256) void llr_quantize_kernel(const float *__restrict__ y, float unit, OUT *__restrict__ out, int64_t count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float t = y[i] / unit;
    if constexpr (std::is_same<OUT, int8_t>::value) {
        const float r = fminf(fmaxf(rintf(t), -127.0f), 127.0f);
        out[i] = t != t ? (int8_t)0 : (int8_t)(int)r;
    } else {
        const float c = fminf(fmaxf(t, -65504.0f), 65504.0f);
        out[i] = (_Float16)(t != t ? t : c);
    }
}

}  // namespace ldpc
