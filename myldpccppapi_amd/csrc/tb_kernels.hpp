/*
 * tb_kernels.hpp -- the transport-block stage of a batch on gfx950 (wave64): the kernels behind ldpc_tb_attach_device,
 * ldpc_tb_check_device and ldpc_tb_tally_device (include/ldpc_hip.h, "transport block").  tb_host.hpp has the algebra and
 * the plan; this file has the walk.
 *
 * One workgroup of W = min(C, 4) waves owns one transport block at a time (grid.y strides over them), one wave one code
 * block at a time (c = wave, wave + W, ...).  A wave walks the nb bytes of its block in 64 contiguous runs, lane l the
 * bytes [l R, (l + 1) R), R = ceil(nb / 64): every byte advances two reflected registers -- CRC24B for the code block,
 * CRC24A / CRC16 for the transport block -- through byte tables in LDS that are built at kernel entry.  A lane's
 * dependent chain is R table steps; its partial remainder, back in normal form, is multiplied by the plan's
 * x^(bits behind the run) and the wave XOR-reduces the 64 products with shuffles (the combine identity of tb_host.hpp).
 * Code blocks start at stream bit c S, in the middle of a byte when that is no multiple of 8: bytes cross between the
 * transport block's stream and the frames through a two-byte funnel.
 *
 *   tb_attach_kernel   source = payload row, sink = frame.  The walk treats the stream bits behind the payload (where
 *                      the transport block's parity will stand) as zeros and writes only the frame bytes that hold
 *                      payload bits alone.  A code block in front of the parity then finishes at once: last data bits,
 *                      CRC24B parity and zero fillers in closed form per byte.  The last code blocks -- those that hold
 *                      parity bits, at most ceil(24 / S) + 1 -- park their remainder in LDS until the waves' folded
 *                      segment remainders have met (plan: stepA, finA); the parity's own contribution to CRC24B is the
 *                      CRC of those few bits (linearity), and the same closed form writes the rest of the frame.
 *   tb_check_kernel    source = frame, sinks = payload row (whole bytes inside the code block; a byte that straddles
 *                      two code blocks is gathered bit by bit by the wave in front of the boundary), cb_ok, tb_ok.
 *                      Both remainders are only tested for zero, so no padding is undone.
 *   tb_tally_kernel    one workgroup per transport block, strided: any differing byte, then four atomic counters.
 *
 * Bounds: a source byte is loaded only below its row's length (bytes behind it read as zero), 16 bytes at a time only
 * where all 16 lie in the row; a sink stores 16 bytes only where all 16 belong to the lane's own run; rows are reached
 * through 64-bit offsets; transport blocks are guarded by `tbs`.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tb_host.hpp"
#include "row_io.hpp"

namespace ldpc {

constexpr int kTbParked = 32;        /* code blocks that can hold transport-block parity bits: at most 25 */

/* the bits of byte j that lie below bit `lim` of the row */
__device__ inline uint32_t tb_mask(int32_t j, int32_t lim)
{
    const int64_t rem = (int64_t)lim - 8 * (int64_t)j;
    return rem >= 8 ? 0xffu : rem <= 0 ? 0u : (1u << rem) - 1u;
}

/* the eight bits of a register (bit 0 first) that fall into a byte which begins `rel` bits behind the register's bit 0 */
__device__ inline uint32_t tb_align(uint32_t r, int64_t rel)
{
    if (rel <= -8 || rel >= 32) return 0;
    return (rel < 0 ? r << (-rel) : r >> rel) & 0xffu;
}

__device__ inline void tb_build_tables(const TbPlan &p, uint32_t *tA, uint32_t *tB)
{
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) {
        tB[i] = tb_table_entry(i, kG24B, 24);
        tA[i] = p.gA ? tb_table_entry(i, p.gA, p.LA) : 0u;
    }
    __syncthreads();
}

/* sum over the waves' folded segment remainders: the remainder of the whole stream */
__device__ inline uint32_t tb_meet(const TbPlan &p, const uint32_t *acc)
{
    uint32_t tot = 0;
    for (int w = 0; w < p.W; ++w) {
        const int32_t last = w + ((p.C - 1 - w) / p.W) * p.W;
        tot ^= gf2_mulmod(acc[w], p.finA[p.C - 1 - last], p.gA, p.LA);
    }
    return tot;
}

/* frame bytes [from, K/8) of code block c, one lane per byte: payload bits below bit min(S, A - c S), the transport
 * block's parity (register rrTb, p_0 = bit 0, standing at stream bit A) up to bit S, the code block's parity (rrB) from
 * bit S, zeros behind it */
__device__ inline void tb_attach_tail(const TbPlan &p, const uint8_t *__restrict__ pay, uint8_t *__restrict__ frame, int64_t s0,
                                      int32_t from, uint32_t rrTb, uint32_t rrB, int lane)
{
    const int64_t prow = p.A / 8;
    const int32_t frow = p.K / 8;
    const int sh = (int)(s0 & 7);
    for (int32_t j = from + lane; j < frow; j += 64) {
        uint32_t v = 0;
        if ((int64_t)8 * j < p.S) {
            const int64_t i = (s0 >> 3) + j;
            const uint32_t b0 = i < prow ? pay[i] : 0u;
            const uint32_t b1 = (sh && i + 1 < prow) ? pay[i + 1] : 0u;
            v = ((b0 | (b1 << 8)) >> sh) & 0xffu;
            if (p.gA) v |= tb_align(rrTb, (int64_t)8 * j - ((int64_t)p.A - s0));
            v &= tb_mask(j, p.S);
        }
        if (p.cb_crc) v |= tb_align(rrB, (int64_t)8 * j - p.S);
        frame[j] = (uint8_t)v;
    }
}

__global__ __launch_bounds__(64 * kTbMaxWaves) void tb_attach_kernel(TbPlan p, const uint8_t *__restrict__ payload, int64_t tbs,
                                                                    uint8_t *__restrict__ src)
{
    __shared__ uint32_t s_tA[256], s_tB[256];
    __shared__ uint32_t s_acc[kTbMaxWaves];
    __shared__ uint32_t s_rb[kTbParked];
    tb_build_tables(p, s_tA, s_tB);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t wA = p.wA[lane], wB = p.wB[lane];
    const int64_t prow = p.A / 8, frow = p.K / 8;
    const int32_t j0 = min(lane * p.R, p.nb), j1 = min(j0 + p.R, p.nb);
    for (int64_t t = blockIdx.y; t < tbs; t += gridDim.y) {
        const uint8_t *pay = payload + t * prow;
        uint32_t acc = 0;
        for (int32_t c = wave; c < p.C; c += p.W) {
            uint8_t *frame = src + (t * p.C + c) * frow;
            const int64_t s0 = (int64_t)c * p.S;
            const int sh = (int)(s0 & 7);
            const int32_t o0 = (int32_t)min((int64_t)p.S, max((int64_t)p.A - s0, (int64_t)0));   /* payload bits of the block */
            const int32_t jsafe = o0 >> 3;
            uint32_t rrA = 0, rrB = 0;
            if (j1 > j0) {
                TbSource in(pay, (s0 >> 3) + j0, prow);
                TbSink out(frame, j0, min(j1, jsafe));
                uint32_t prev = in.next();
                for (int32_t j = j0; j < j1; ++j) {
                    const uint32_t nx = in.next();
                    uint32_t v = ((prev | (nx << 8)) >> sh) & 0xffu;
                    if (8 * (int64_t)j + 8 > p.S) v &= tb_mask(j, p.S);
                    if (j < jsafe) out.push(v);
                    rrB = (rrB >> 8) ^ s_tB[(rrB ^ v) & 0xffu];
                    if (p.gA) rrA = (rrA >> 8) ^ s_tA[(rrA ^ v) & 0xffu];
                    prev = nx;
                }
            }
            const uint32_t rB = tb_wave_xor(gf2_mulmod(__brev(rrB) >> 8, wB, kG24B, 24));
            if (p.gA) {
                const uint32_t rA = tb_wave_xor(gf2_mulmod(__brev(rrA) >> (32 - p.LA), wA, p.gA, p.LA));
                acc = gf2_mulmod(acc, p.stepA, p.gA, p.LA) ^ rA;
            }
            if (c < p.cA) tb_attach_tail(p, pay, frame, s0, jsafe, 0u, __brev(rB) >> 8, lane);
            else if (lane == 0) s_rb[c - p.cA] = rB;
        }
        if (p.gA) {
            if (lane == 0) s_acc[wave] = acc;
            __syncthreads();
            const uint32_t tot = tb_meet(p, s_acc);
            const uint32_t rrTb = __brev(tot) >> (32 - p.LA);
            for (int32_t c = p.cA + wave; c < p.C; c += p.W) {
                const int64_t s0 = (int64_t)c * p.S;
                const int32_t i0 = (int32_t)max(s0 - p.A, (int64_t)0), i1 = (int32_t)(s0 + p.S - p.A);
                uint32_t d = 0;                      /* CRC24B of the parity bits that stand in this code block */
                for (int32_t i = i0; i < i1; ++i) d = tb_crc_step(d, rrTb >> i, kG24B, 24);
                const int32_t o0 = (int32_t)min((int64_t)p.S, max((int64_t)p.A - s0, (int64_t)0));
                tb_attach_tail(p, pay, src + (t * p.C + c) * frow, s0, o0 >> 3, rrTb, __brev(s_rb[c - p.cA] ^ d) >> 8, lane);
            }
            __syncthreads();                          /* s_acc and s_rb serve the next transport block */
        }
    }
}

__global__ __launch_bounds__(64 * kTbMaxWaves) void tb_check_kernel(TbPlan p, const uint8_t *__restrict__ dec, int64_t tbs,
                                                                   uint8_t *__restrict__ payload, uint8_t *__restrict__ cb_ok,
                                                                   uint8_t *__restrict__ tb_ok)
{
    __shared__ uint32_t s_tA[256], s_tB[256];
    __shared__ uint32_t s_acc[kTbMaxWaves], s_ok[kTbMaxWaves];
    tb_build_tables(p, s_tA, s_tB);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t wA = p.wA[lane], wB = p.wB[lane];
    const int64_t prow = p.A / 8, frow = p.K / 8;
    const int32_t j0 = min(lane * p.R, p.nb), j1 = min(j0 + p.R, p.nb);
    for (int64_t t = blockIdx.y; t < tbs; t += gridDim.y) {
        uint8_t *pay = payload ? payload + t * prow : nullptr;
        const uint8_t *frames = dec + t * p.C * frow;
        uint32_t acc = 0, ok = 1;
        for (int32_t c = wave; c < p.C; c += p.W) {
            const uint8_t *frame = frames + c * frow;
            const int64_t s0 = (int64_t)c * p.S;
            const int d = (int)((8 - (s0 & 7)) & 7);                  /* frame bit of the first whole payload byte */
            const int32_t limc = (int32_t)min((int64_t)p.S, max((int64_t)p.A - s0, (int64_t)0));
            uint32_t rrA = 0, rrB = 0;
            if (j1 > j0) {
                const int32_t jv = limc - 8 - d >= 0 ? (limc - 8 - d) >> 3 : -1;   /* last byte that starts a whole payload byte */
                const int32_t jend = pay ? min(j1, jv + 1) : j0;
                const int64_t pb = (s0 + 8 * (int64_t)j0 + d) >> 3;
                TbSource in(frame, j0, frow);
                TbSink out(pay, pb, pb + max(jend - j0, 0));
                uint32_t prev = in.next();
                for (int32_t j = j0; j < j1; ++j) {
                    const uint32_t nx = in.next();
                    const uint32_t vB = prev & tb_mask(j, p.Kp), vA = prev & tb_mask(j, p.S);
                    rrB = (rrB >> 8) ^ s_tB[(rrB ^ vB) & 0xffu];
                    if (p.gA) rrA = (rrA >> 8) ^ s_tA[(rrA ^ vA) & 0xffu];
                    if (j < jend) out.push(((prev | (nx << 8)) >> d) & 0xffu);
                    prev = nx;
                }
            }
            const uint32_t rB = tb_wave_xor(gf2_mulmod(__brev(rrB) >> 8, wB, kG24B, 24));
            const uint32_t okc = (p.cb_crc == 0 || rB == 0) ? 1u : 0u;
            if (cb_ok && lane == 0) cb_ok[t * p.C + c] = (uint8_t)okc;
            ok &= okc;
            if (p.gA) {
                const uint32_t rA = tb_wave_xor(gf2_mulmod(__brev(rrA) >> (32 - p.LA), wA, p.gA, p.LA));
                acc = gf2_mulmod(acc, p.stepA, p.gA, p.LA) ^ rA;
            }
            /* the payload byte that straddles the boundary behind this code block: gathered bit by bit, by the first
             * boundary that falls into the byte (S < 8 puts several there) */
            const int64_t bnd = s0 + p.S;
            if (pay && lane == 0 && c + 1 < p.C && (bnd & 7) && (bnd >> 3) < prow && ((s0 >> 3) != (bnd >> 3) || (s0 & 7) == 0)) {
                uint32_t v = 0;
                for (int q = 0; q < 8; ++q) {
                    const int64_t s = (bnd & ~(int64_t)7) + q;
                    const int64_t cc = s / p.S, i = s - cc * p.S;
                    v |= (uint32_t)((frames[cc * frow + (i >> 3)] >> (i & 7)) & 1) << q;
                }
                pay[bnd >> 3] = (uint8_t)v;
            }
        }
        if (tb_ok) {
            if (lane == 0) { s_acc[wave] = acc; s_ok[wave] = ok; }
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t all = 1;
                for (int w = 0; w < p.W; ++w) all &= s_ok[w];
                if (p.gA && tb_meet(p, s_acc) != 0) all = 0;
                tb_ok[t] = (uint8_t)all;
            }
            __syncthreads();
        }
    }
}

/* counts[0] += tb_ok == 0, [1] += payload != ref, [2] += differs although ok, [3] += not ok although equal */
__global__ __launch_bounds__(256) void tb_tally_kernel(const uint8_t *__restrict__ tb_ok, const uint8_t *__restrict__ payload,
                                                       const uint8_t *__restrict__ ref, int64_t tbs, int64_t bytes_per_tb,
                                                       unsigned long long *__restrict__ counts)
{
    for (int64_t t = blockIdx.x; t < tbs; t += gridDim.x) {
        unsigned diff = 0;
        for (int64_t j = threadIdx.x; j < bytes_per_tb; j += blockDim.x) {
            const int64_t i = t * bytes_per_tb + j;
            diff |= (unsigned)(payload[i] ^ (ref ? ref[i] : (uint8_t)0));
        }
        const int differs = __syncthreads_or(diff != 0);
        if (threadIdx.x == 0) {
            const bool ok = tb_ok[t] != 0;
            if (!ok) atomicAdd(&counts[0], 1ull);
            if (differs) atomicAdd(&counts[1], 1ull);
            if (differs && ok) atomicAdd(&counts[2], 1ull);
            if (!differs && !ok) atomicAdd(&counts[3], 1ull);
        }
    }
}

}  // namespace ldpc
