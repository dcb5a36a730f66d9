/*
 * modem_kernels.hpp -- the modem stage of a batch of frames on gfx950 (wave64): the two streaming kernels behind
 * ldpc_modem_transmit_device and ldpc_modem_demap_device (include/ldpc_hip.h, "modem").
 *
 * Everything is closed-form, so neither kernel reads a table.  With Qm bits per symbol, m = Qm / 2 bits per axis,
 * S = E / Qm symbols per frame:
 *     e(i, j) = interleave ? i * S + j : j * Qm + i        tx / rx position of bit i of symbol j
 *     amp(c0 .. c(m-1)):  a = 0;  for k = 1 .. m:  a = (1 - 2 c(m-k)) * (2^(k-1) - a)      Gray, odd integers
 *     x = (float)amp * A                                    A = 1 / sqrt(2, 10, 42, 170), rounded once to float
 * The I axis of symbol j takes bits i = 0, 2, ..., the Q axis i = 1, 3, ...; a frame's row of symbols holds
 * I0 Q0 I1 Q1 ... (2 S floats), or E real samples for Qm = 1 (x = 1 - 2 b, the reference's BPSK).
 *
 *   modem_tx_kernel     one lane = one Philox group = real samples 4g .. 4g+3 of a frame = two symbols (four bits for
 *                       Qm = 1): the lane collects its 2 Qm bits -- with the interleaver from Qm streams that are each
 *                       contiguous across the lanes, without it from 2 Qm consecutive bytes --, maps them, adds
 *                       sd * z in double as ldpc_ch_sample does, and stores 16 bytes where the address allows
 *   modem_demap_kernel  lanes along symbols: 8 bytes in, the 2^m squared distances of each axis, the minima per bit
 *                       value, and Qm dwords out at e(i, j) -- Qm streams contiguous across the lanes with the
 *                       interleaver, Qm consecutive floats per lane without it
 *
 * Bounds: every load of tx is a bit e < E of the frame's own row, every load and store of sym a float n < row of the
 * frame's own row, every store of rx a position e < E; frames are guarded by `frames`; all element offsets are 64-bit.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ldpc_channel.h"

namespace ldpc {

constexpr int kModemBlock = 256;     /* 4 waves */

struct ModemMap {
    int32_t Qm, E;
    int32_t S;            /* symbols per frame, E / Qm                          */
    int32_t interleave;
    int32_t row;          /* floats of a frame's row of symbols: E or 2 S       */
    float A;              /* the constellation's scale (1 for Qm = 1)           */
};

/* integer level of the axis label whose bit k (c0 first) is bit m-1-k of `label` */
__host__ __device__ constexpr int modem_amp(int m, uint32_t label)
{
    int a = 0;
    for (int k = 1; k <= m; ++k) a = (1 - 2 * (int)((label >> (k - 1)) & 1u)) * ((1 << (k - 1)) - a);
    return a;
}

__device__ inline uint32_t modem_position(const ModemMap &m, int32_t i, int32_t j)
{
    return m.interleave ? (uint32_t)i * (uint32_t)m.S + (uint32_t)j : (uint32_t)j * (uint32_t)m.Qm + (uint32_t)i;
}

template <int PACKED> __device__ inline uint32_t modem_tx_bit(const uint8_t *__restrict__ row, uint32_t e)
{
    return PACKED ? (uint32_t)(row[e >> 3] >> (e & 7)) & 1u : (uint32_t)row[e] & 1u;
}

/* sym[f][n] = x(f, n) + sd * z(seed, first_frame + f, n).  grid.x tiles the Philox groups of a row, grid.y strides
 * over the frames.  PACKED: tx is E/8 bytes per frame (E % 8 == 0), else E bytes of 0/1. */
template <int PACKED>
__global__ __launch_bounds__(kModemBlock) void modem_tx_kernel(ModemMap m, const uint8_t *__restrict__ tx, int64_t frames, float sd,
                                                              uint64_t seed, int64_t first_frame, float *__restrict__ sym)
{
    const int64_t g = (int64_t)blockIdx.x * kModemBlock + threadIdx.x;      /* Philox group of the row */
    const int64_t n0 = 4 * g;
    if (n0 >= m.row) return;
    const int64_t in_row = PACKED ? m.E / 8 : m.E;
    const int half = m.Qm / 2;
    for (int64_t f = blockIdx.y; f < frames; f += gridDim.y) {
        const uint8_t *row_in = tx + f * in_row;
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t n = n0 + k;
            x[k] = 0.0f;
            if (n >= m.row) continue;
            if (m.Qm == 1) {
                x[k] = modem_tx_bit<PACKED>(row_in, (uint32_t)n) ? -1.0f : 1.0f;
            } else {
                const int32_t j = (int32_t)(n >> 1), axis = (int32_t)(n & 1);
                int a = 0;
                for (int b = half - 1; b >= 0; --b) {                           /* last axis bit first */
                    const uint32_t c = modem_tx_bit<PACKED>(row_in, modem_position(m, 2 * b + axis, j));
                    a = (1 - 2 * (int)c) * ((1 << (half - 1 - b)) - a);
                }
                x[k] = (float)a * m.A;
            }
        }
        if (sd != 0.0f) {
            double z[4];
            ldpc_ch_normal4(seed, (uint64_t)(first_frame + f), (uint32_t)g, z);
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = (float)((double)x[k] + (double)sd * z[k]);
        }
        float *out = sym + f * (int64_t)m.row + n0;
        if (n0 + 4 <= m.row && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
            *reinterpret_cast<float4 *>(out) = float4{x[0], x[1], x[2], x[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (n0 + k < m.row) out[k] = x[k];
        }
    }
}

/* one axis: y[k] = (D1 - D0) * 0.25f for the axis bits k < M, D_b = the smallest (r - x)^2 over the levels whose bit k is b */
template <int M> __device__ inline void modem_demap_axis(float r, float A, float y[M])
{
    float d[1 << M];
#pragma unroll
    for (uint32_t v = 0; v < (1u << M); ++v) {
        /* label v holds c0 as its top bit; modem_amp wants c(m-k) as bit k-1, which is the same thing */
        const float x = (float)modem_amp(M, v) * A;
        const float t = r - x;
        d[v] = t * t;
    }
#pragma unroll
    for (int k = 0; k < M; ++k) {
        float d0 = 0.0f, d1 = 0.0f;
        bool have0 = false, have1 = false;
#pragma unroll
        for (uint32_t v = 0; v < (1u << M); ++v) {
            if ((v >> (M - 1 - k)) & 1u) { d1 = have1 ? fminf(d1, d[v]) : d[v]; have1 = true; }
            else { d0 = have0 ? fminf(d0, d[v]) : d[v]; have0 = true; }
        }
        y[k] = (d1 - d0) * 0.25f;
    }
}

/* rx[f][e(i, j)] = max-log value of bit i of symbol j.  grid.x tiles the symbols of a row, grid.y strides over the
 * frames.  QM = 1: rx[f][e] = sym[f][e]. */
template <int QM>
__global__ __launch_bounds__(kModemBlock) void modem_demap_kernel(ModemMap m, const float *__restrict__ sym, int64_t frames,
                                                                 float *__restrict__ rx)
{
    const int64_t j = (int64_t)blockIdx.x * kModemBlock + threadIdx.x;      /* symbol of the row */
    if (j >= m.S) return;
    for (int64_t f = blockIdx.y; f < frames; f += gridDim.y) {
        const float *in = sym + f * (int64_t)m.row;
        float *out = rx + f * (int64_t)m.E;
        if constexpr (QM == 1) {
            out[j] = in[j];
        } else {
            constexpr int M = QM / 2;
            float y[2][M];
            modem_demap_axis<M>(in[2 * j], m.A, y[0]);
            modem_demap_axis<M>(in[2 * j + 1], m.A, y[1]);
#pragma unroll
            for (int i = 0; i < QM; ++i) out[modem_position(m, i, (int32_t)j)] = y[i & 1][i >> 1];
        }
    }
}

}  // namespace ldpc
