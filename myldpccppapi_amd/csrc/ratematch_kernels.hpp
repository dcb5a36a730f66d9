/*
 * ratematch_kernels.hpp -- rate matching of a batch of frames on gfx950 (wave64): the two streaming kernels behind
 * ldpc_rate_match_device and ldpc_rate_recover_device (include/ldpc_hip.h, "rate matching").
 *
 * The index map is closed-form, so neither kernel reads a table.  With Ncb = N - P buffer positions, F = hi - lo
 * fillers at buffer positions [g, g + F), g = lo - P, and L = Ncb - F transmittable bits:
 *     rank(e)  = (r0 + e) mod L                       r0 = k0 minus the fillers before k0, reduced mod L by the host
 *     index(e) = P + rank + (rank >= g ? F : 0)
 * and, the other way round, code bit n (not punctured, no filler) has rank r = n - P - (n >= hi ? F : 0) and receives
 * the transmitted positions e = (r - r0) mod L, + L, + 2L, ... below E.
 *
 *   rate_match_kernel    lanes along e: one output dword per lane (4 code bits as bytes, or 32 packed); a frame's
 *                        row of tx starts at any byte, so a lane owns one ALIGNED dword of the buffer and the two
 *                        partial dwords at a row's ends leave as bytes (a neighbouring row writes the other bytes)
 *   rate_recover_kernel  lanes along n: a gather -- every code bit sums its own received values in ascending e (fp32,
 *                        the order is part of the contract), so there is no atomic and no scatter; consecutive lanes
 *                        read consecutive floats of rx except at the wrap and at the filler gap
 *
 * Bounds: every load of code / rx is guarded by N / E of the frame's own row, every store by the row's extent;
 * frames are guarded by `frames`; all element offsets are 64-bit.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ldpc {

constexpr int kRateBlock = 256;      /* 4 waves */
constexpr int kRateUnroll = 4;       /* recover: code bits per lane, kRateBlock apart (loads of all four in flight) */

struct RateMap {
    int32_t N, E;
    int32_t P;          /* punctured prefix                                   */
    int32_t lo, hi;     /* fillers as code bits [lo, hi) (lo = hi = P: none)  */
    int32_t L;          /* transmittable bits                                 */
    uint32_t r0;        /* rank at which the transmission starts, < L         */
    float fill_llr, erasure_llr;
};

__device__ inline int32_t rate_index(const RateMap &m, uint32_t e)
{
    const uint32_t rank = (m.r0 + e) % (uint32_t)m.L;
    return m.P + (int32_t)rank + ((int32_t)rank >= m.lo - m.P ? m.hi - m.lo : 0);
}

/* 4 bits -> 4 bytes of 0/1 (bit k to byte k), as enc_spread4 of the encoder */
__device__ inline uint32_t rate_spread4(uint32_t nibble) { return (nibble * 0x00204081u) & 0x01010101u; }

template <int IN_PACKED> __device__ inline uint32_t rate_code_bit(const uint8_t *__restrict__ row, int32_t n)
{
    return IN_PACKED ? (uint32_t)(row[n >> 3] >> (n & 7)) & 1u : (uint32_t)row[n] & 1u;
}

/* tx[f][e] = code[f][index(e)].  grid.x tiles the dwords of a row, grid.y strides over the frames.
 * IN_PACKED: code is N/8 bytes per frame (N % 8 == 0), else N bytes of 0/1.  OUT_PACKED: tx is E/8 bytes per frame
 * (E % 8 == 0), else E bytes of 0/1.  `code_bytes_total` = bytes of the whole code buffer (bounds of the wide loads). */
template <int IN_PACKED, int OUT_PACKED>
__global__ __launch_bounds__(kRateBlock) void rate_match_kernel(RateMap m, const uint8_t *__restrict__ code, int64_t code_bytes_total,
                                                               int64_t frames, uint8_t *__restrict__ tx)
{
    const int64_t in_row = IN_PACKED ? m.N / 8 : m.N;
    const int64_t out_row = OUT_PACKED ? m.E / 8 : m.E;
    const int64_t j = (int64_t)blockIdx.x * kRateBlock + threadIdx.x;       /* dword of the row's aligned cover */
    for (int64_t f = blockIdx.y; f < frames; f += gridDim.y) {
        uint8_t *row_out = tx + f * out_row;
        const int64_t head = (int64_t)((uintptr_t)row_out & 3);              /* bytes of the first dword before the row */
        const int64_t b0 = 4 * j - head;                                     /* the lane's bytes: row bytes [b0, b0 + 4) */
        if (b0 >= out_row) continue;
        const uint8_t *row_in = code + f * in_row;
        uint32_t word = 0;
        const int64_t lo = b0 < 0 ? 0 : b0, hi = b0 + 4 < out_row ? b0 + 4 : out_row;
        if (!OUT_PACKED) {
            /* output bytes lo .. hi-1 = transmitted bits e = lo .. hi-1 */
            const int32_t i0 = rate_index(m, (uint32_t)lo);
            const int32_t i3 = rate_index(m, (uint32_t)(hi - 1));
            bool done = false;
            if (!IN_PACKED && hi - lo == 4 && i3 == i0 + 3) {
                /* four consecutive code bytes: two aligned dwords that cover them, inside the buffer */
                const uintptr_t at = (uintptr_t)(row_in + i0);
                const int sh = (int)(at & 3);
                const uint8_t *base = row_in + i0 - sh;
                if (base >= code && base + (sh ? 8 : 4) <= code + code_bytes_total) {
                    const uint32_t a = *reinterpret_cast<const uint32_t *>(base);
                    const uint32_t b = sh ? *reinterpret_cast<const uint32_t *>(base + 4) : 0u;
                    word = (sh ? (a >> (8 * sh)) | (b << (32 - 8 * sh)) : a) & 0x01010101u;
                    done = true;
                }
            }
            if (!done)
                for (int64_t b = lo; b < hi; ++b)
                    word |= rate_code_bit<IN_PACKED>(row_in, rate_index(m, (uint32_t)b)) << (8 * (int)(b - b0));
        } else {
            for (int64_t b = lo; b < hi; ++b) {
                uint32_t byte = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) byte |= rate_code_bit<IN_PACKED>(row_in, rate_index(m, (uint32_t)(8 * b + k))) << k;
                word |= byte << (8 * (int)(b - b0));
            }
        }
        if (hi - lo == 4) {
            *reinterpret_cast<uint32_t *>(row_out + b0) = word;
        } else {
            for (int64_t b = lo; b < hi; ++b) row_out[b] = (uint8_t)(word >> (8 * (int)(b - b0)));
        }
    }
}

/* For every frame f < frames and code bit n < N (include/ldpc_hip.h states the contract):
 *     s = accumulate ? soft[f][n] : 0;  s += rx[f][e] for every e with index(e) = n, ascending;  fillers: s = 0
 *     soft[f][n] = s (if soft);  y[f][n] = filler ? fill_llr : s != 0 ? s : erasure value of n (if y)
 * grid.x tiles n in runs of kRateBlock * kRateUnroll, grid.y strides over the frames. */
__global__ __launch_bounds__(kRateBlock) void rate_recover_kernel(RateMap m, const float *__restrict__ rx, int64_t frames,
                                                                 float *soft, int32_t accumulate, float *__restrict__ y)
{
    const int32_t n0 = (int32_t)blockIdx.x * (kRateBlock * kRateUnroll) + (int32_t)threadIdx.x;
    const uint32_t L = (uint32_t)m.L, E = (uint32_t)m.E;
    const int32_t F = m.hi - m.lo;
    /* per lane and code bit: first transmitted position (E: none), whether it is a filler, its erasure value */
    uint32_t e0[kRateUnroll];
    bool filler[kRateUnroll];
    float erased[kRateUnroll];
#pragma unroll
    for (int k = 0; k < kRateUnroll; ++k) {
        const int32_t n = n0 + k * kRateBlock;
        filler[k] = n >= m.lo && n < m.hi;
        e0[k] = E;
        if (n < m.N && n >= m.P && !filler[k]) {
            const uint32_t r = (uint32_t)(n - m.P - (n >= m.hi ? F : 0));
            e0[k] = r >= m.r0 ? r - m.r0 : r + L - m.r0;
        }
        erased[k] = m.erasure_llr > 0.0f ? m.erasure_llr * (1.0f + (float)n / (float)m.N) : 0.0f;
    }
    for (int64_t f = blockIdx.y; f < frames; f += gridDim.y) {
        const float *row = rx + f * (int64_t)m.E;
        const int64_t out = f * (int64_t)m.N;
        float s[kRateUnroll];
#pragma unroll
        for (int k = 0; k < kRateUnroll; ++k) {
            const int32_t n = n0 + k * kRateBlock;
            s[k] = (accumulate && n < m.N && !filler[k]) ? soft[out + n] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < kRateUnroll; ++k) {
            if (e0[k] < E) s[k] += row[e0[k]];                               /* E <= L: at most this one */
        }
        if (E > L) {
#pragma unroll
            for (int k = 0; k < kRateUnroll; ++k)
                for (uint64_t e = (uint64_t)e0[k] + L; e < E; e += L) s[k] += row[e];
        }
#pragma unroll
        for (int k = 0; k < kRateUnroll; ++k) {
            const int32_t n = n0 + k * kRateBlock;
            if (n >= m.N) continue;
            if (soft) soft[out + n] = s[k];
            if (y) y[out + n] = filler[k] ? m.fill_llr : s[k] != 0.0f ? s[k] : erased[k];
        }
    }
}

}  // namespace ldpc
