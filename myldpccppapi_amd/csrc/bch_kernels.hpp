/*
 * bch_kernels.hpp -- the outer-code stage of a batch on gfx950 (wave64): the kernels behind ldpc_bch_encode_device,
 * ldpc_bch_decode_device and ldpc_bch_tally_device (include/ldpc_hip.h, "outer code").  bch_host.hpp has the algebra and
 * the plan; this file has the walk, the key equation and the root search.
 *
 * One wave owns one frame at a time (a workgroup of four waves strides over the batch; after the tables are built the
 * waves never meet again, so a wave that has a dirty frame delays nobody).  The wave walks the row's bytes in 64
 * contiguous runs, lane l the bytes [l R, (l + 1) R), as the transport-block kernels do (TbSource / TbSink of
 * row_io.hpp carry the bytes): every byte advances one 16-bit register per distinct minimal polynomial through a
 * byte table in LDS.  A lane's partial remainders are multiplied by the plan's x^(bits behind the run) and the wave
 * XOR-reduces the products with shuffles.  TT is the number of registers a lane keeps, t rounded up to 4, 8 or 12:
 * everything indexed by a register number is unrolled, so that nothing lives in scratch.
 *
 *   bch_encode_kernel  source = payload row, sink = frame bytes [0, k / 8).  The reduced remainders u_i = x^r a mod m_i
 *                      become the parity by the Chinese remainder theorem: lane i forms ((u_i c_i) mod m_i) G_i, the
 *                      wave XORs the nmin products, lane q writes parity byte q; zeros behind bit n.
 *   bch_decode_kernel  source = frame, sink = payload row (copied during the walk, whatever the frame turns out to be).
 *                      Lane j - 1 evaluates S_j; a frame whose 2t syndromes are zero is done (status 0).  Otherwise, in
 *                      the same wave: inversion-free Berlekamp-Massey with lane i holding coefficient i of both
 *                      polynomials; Chien search with lane l over the positions [l P, (l + 1) P), term j stepped by the
 *                      constant alpha^j through two 256-entry tables in LDS; the roots are handed to lanes 0 .. L - 1 by
 *                      ballot.  The frame is corrected only if deg sigma = L <= t, exactly L roots lie in [0, n), and
 *                      the power sums of the L locators equal all 2t syndromes -- which is the definition of the
 *                      decoder's result, checked rather than argued.  A lane then rewrites the payload byte of its
 *                      root from the input byte (roots that share a byte are merged by the first of them).
 *   bch_tally_kernel   one workgroup per frame, strided: any differing byte, then six atomic counters.
 *
 * Bounds: the walk reads the bytes [0, nb) of a row and nothing else (TbSource), a sink stores only its own run; a root
 * position is below n by construction and a payload byte is rewritten only below k / 8; rows are reached through 64-bit
 * offsets; frames are guarded by `frames`.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bch_host.hpp"
#include "row_io.hpp"

namespace ldpc {

constexpr int kBchWaves = 4;

template <int TT> __device__ inline void bch_build_walk_tables(const BchPlan &p, uint16_t (*T)[256])
{
    for (uint32_t idx = threadIdx.x; idx < TT * 256u; idx += blockDim.x) {
        const int i = (int)(idx >> 8);
        T[i][idx & 255u] = i < p.nmin ? (uint16_t)bch_table_entry(idx & 255u, p.M[i]) : (uint16_t)0;
    }
}

/* lane l of a wave takes its run of the row's first p.nb bytes through the registers; bytes below `copy_to` also go to
 * `out`.  Returns with reg[i] = v mod M_i of the whole row (times x^r for the encoder's plan) in every lane. */
template <int TT> __device__ inline void bch_walk(const BchPlan &p, const uint16_t (*T)[256], const uint8_t *__restrict__ row,
                                                  uint8_t *__restrict__ out, int32_t copy_to, int lane, uint32_t (&reg)[TT])
{
    const int32_t j0 = min(lane * p.R, p.nb), j1 = min(j0 + p.R, p.nb);
#pragma unroll
    for (int i = 0; i < TT; ++i) reg[i] = 0;
    if (j1 > j0) {
        const int32_t jend = out ? max(min(j1, copy_to), j0) : j0;
        TbSource in(row, j0, p.nb);
        TbSink sink(out, j0, jend);
        for (int32_t j = j0; j < j1; ++j) {
            const uint32_t b = in.next();
            if (j < jend) sink.push(b);
            const uint32_t v = __brev(b) >> 24;
#pragma unroll
            for (int i = 0; i < TT; ++i) reg[i] = ((reg[i] & 0xffu) << 8) ^ T[i][reg[i] >> 8] ^ v;
        }
    }
#pragma unroll
    for (int i = 0; i < TT; ++i) {
        uint32_t v = 0;
        if (i < p.nmin) v = bch_mulmod(reg[i], p.w[i][lane], p.M[i], 16);
        reg[i] = tb_wave_xor(v);
    }
}

template <int TT>
__global__ __launch_bounds__(64 * kBchWaves) void bch_encode_kernel(BchPlan p, const uint8_t *__restrict__ payload, int64_t frames,
                                                                   uint8_t *__restrict__ src)
{
    __shared__ uint16_t s_T[TT][256];
    bch_build_walk_tables<TT>(p, s_T);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t kb = p.k / 8, nbytes = p.n / 8;
    for (int64_t f = (int64_t)blockIdx.x * kBchWaves + wave; f < frames; f += (int64_t)gridDim.x * kBchWaves) {
        uint8_t *row = src + f * p.row_bytes;
        uint32_t reg[TT];
        bch_walk<TT>(p, s_T, payload + f * kb, row, p.nb, lane, reg);
        /* lane i: z = (u_i c_i) mod m_i, then z G_i */
        uint32_t mine = 0;
#pragma unroll
        for (int i = 0; i < TT; ++i) mine = lane == i ? reg[i] : mine;
        uint64_t acc[kBchWords] = {0, 0, 0, 0};
        if (lane < p.nmin) {
            const int d = p.deg[lane];
            const uint32_t z = bch_mulmod(bch_reduce16(mine, p.mp[lane], d), p.c[lane], p.mp[lane], d);
            uint64_t G[kBchWords];
#pragma unroll
            for (int w = 0; w < kBchWords; ++w) G[w] = p.G[lane][w];
            for (int s = 0; s < 16; ++s) {
                if (!((z >> s) & 1u)) continue;
#pragma unroll
                for (int w = 0; w < kBchWords; ++w) {
                    acc[w] ^= G[w] << s;
                    if (s && w) acc[w] ^= G[w - 1] >> (64 - s);
                }
            }
        }
#pragma unroll
        for (int w = 0; w < kBchWords; ++w) {
            const uint32_t lo = tb_wave_xor((uint32_t)acc[w]), hi = tb_wave_xor((uint32_t)(acc[w] >> 32));
            acc[w] = (uint64_t)lo | ((uint64_t)hi << 32);
        }
        /* parity byte q holds p_(8q) .. p_(8q+7) = the coefficients of x^(r-1-8q) .. x^(r-8-8q), bit 0 first */
        for (int32_t q = lane; q < p.r / 8; q += 64) {
            const int32_t lowest = p.r - 8 - 8 * q;
            const int wsel = lowest >> 6;
            const uint64_t word = wsel == 0 ? acc[0] : wsel == 1 ? acc[1] : wsel == 2 ? acc[2] : acc[3];
            row[kb + q] = (uint8_t)(__brev((uint32_t)((word >> (lowest & 63)) & 0xffu)) >> 24);
        }
        for (int64_t j = nbytes + lane; j < p.row_bytes; j += 64) row[j] = 0;
    }
}

__device__ inline uint32_t bch_shfl(uint32_t v, int src)
{
    return (uint32_t)__shfl((int)v, src & 63);
}

template <int TT>
__global__ __launch_bounds__(64 * kBchWaves) void bch_decode_kernel(BchPlan p, const uint8_t *__restrict__ dec, int64_t frames,
                                                                   uint8_t *__restrict__ payload, int32_t *__restrict__ status)
{
    __shared__ uint16_t s_T[TT][256];
    __shared__ uint16_t s_lo[TT][256], s_hi[TT][256];     /* x -> x alpha^j and (x << 8) alpha^j, j = index + 1 */
    bch_build_walk_tables<TT>(p, s_T);
    for (uint32_t idx = threadIdx.x; idx < TT * 256u; idx += blockDim.x) {
        const int j = (int)(idx >> 8);
        const uint32_t x = idx & 255u, lo = x & ((1u << p.m) - 1u), hi = x << 8;
        const bool used = j < p.t;
        s_lo[j][x] = used ? (uint16_t)bch_mulmod(lo, p.aj[j], p.prim, p.m) : (uint16_t)0;
        s_hi[j][x] = used && (hi >> p.m) == 0 ? (uint16_t)bch_mulmod(hi, p.aj[j], p.prim, p.m) : (uint16_t)0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t kb = p.k / 8;
    const int two_t = 2 * p.t;
    for (int64_t f = (int64_t)blockIdx.x * kBchWaves + wave; f < frames; f += (int64_t)gridDim.x * kBchWaves) {
        const uint8_t *row = dec + f * p.row_bytes;
        uint8_t *pay = payload ? payload + f * kb : nullptr;
        uint32_t reg[TT];
        bch_walk<TT>(p, s_T, row, pay, (int32_t)kb, lane, reg);
        /* lane j - 1: S_j = u_c(alpha^j) */
        uint32_t S = 0;
        if (lane < two_t) {
            const int c = p.cls[lane];
            uint32_t u = 0;
#pragma unroll
            for (int i = 0; i < TT; ++i) u = c == i ? reg[i] : u;
#pragma unroll
            for (int b = 0; b < 16; ++b) S ^= ((u >> b) & 1u) ? (uint32_t)p.E[lane][b] : 0u;
        }
        if (__ballot(S != 0) == 0) {
            if (status && lane == 0) status[f] = 0;
            continue;
        }
        /* Berlekamp-Massey without inversions: C <- b C + d x^shift B; lane i holds C_i and B_i */
        uint32_t C = lane == 0 ? 1u : 0u, B = C, bb = 1;
        int L = 0, shift = 1;
        for (int n = 0; n < two_t; ++n) {
            const uint32_t Sv = bch_shfl(S, n - lane);
            const uint32_t d = tb_wave_xor(lane <= L && lane <= n ? bch_mulmod(C, Sv, p.prim, p.m) : 0u);
            if (d == 0) {
                ++shift;
                continue;
            }
            const uint32_t Bdown = bch_shfl(B, lane - shift);
            const uint32_t Bs = lane >= shift ? Bdown : 0u;
            const uint32_t Cn = bch_mulmod(C, bb, p.prim, p.m) ^ bch_mulmod(Bs, d, p.prim, p.m);
            if (2 * L <= n) {
                B = C;
                bb = d;
                L = n + 1 - L;
                shift = 1;
            } else {
                ++shift;
            }
            C = Cn;
        }
        int32_t result = -1;
        if (L <= p.t) {
            /* Chien search: term j = sigma_j X^-j at the lane's position, stepped by alpha^j per position */
            const uint32_t base = p.chien[lane], sigma0 = bch_shfl(C, 0);
            uint32_t term[TT], pw = base;
#pragma unroll
            for (int j = 0; j < TT; ++j) {
                term[j] = 0;
                if (j < L) {
                    term[j] = bch_mulmod(bch_shfl(C, j + 1), pw, p.prim, p.m);
                    pw = bch_mulmod(pw, base, p.prim, p.m);
                }
            }
            int found = 0;
            int32_t root = -1;
            for (int32_t s = 0; s < p.P; ++s) {
                const int32_t pos = lane * p.P + s;
                uint32_t sum = sigma0;
#pragma unroll
                for (int j = 0; j < TT; ++j) sum ^= term[j];
                unsigned long long hits = __ballot(pos < p.n && sum == 0);
                while (hits) {
                    const int srcl = __ffsll(hits) - 1;
                    const int32_t at = __shfl(pos, srcl);
                    if (lane == found) root = at;
                    ++found;
                    hits &= hits - 1;
                }
#pragma unroll
                for (int j = 0; j < TT; ++j)
                    if (j < L) term[j] = (uint32_t)s_lo[j][term[j] & 0xffu] ^ (uint32_t)s_hi[j][term[j] >> 8];
            }
            if (found == L) {
                /* the locators X = alpha^(n - 1 - root) of lanes 0 .. L - 1 and their power sums against S_1 .. S_2t */
                uint32_t X = 0;
                if (lane < L) X = bch_powmod(2u, (uint64_t)(p.n - 1 - root), p.prim, p.m);
                uint32_t xp = X;
                bool same = true;
                for (int j = 1; j <= two_t; ++j) {
                    const uint32_t sum = tb_wave_xor(xp), want = bch_shfl(S, j - 1);
                    same &= sum == want;
                    xp = bch_mulmod(xp, X, p.prim, p.m);
                }
                if (same) {
                    result = L;
                    if (pay) {
                        __threadfence();                 /* the walk's stores of this row are behind us */
                        uint32_t mask = 0;
                        bool first = true;
#pragma unroll
                        for (int q = 0; q < TT; ++q) {
                            const int32_t other = __shfl(root, q);
                            if (q < L && lane < L && (other >> 3) == (root >> 3)) {
                                mask ^= 1u << (other & 7);
                                if (q < lane) first = false;
                            }
                        }
                        if (lane < L && first && (root >> 3) < kb) pay[root >> 3] = (uint8_t)(row[root >> 3] ^ mask);
                    }
                }
            }
        }
        if (status && lane == 0) status[f] = result;
    }
}

/* counts[0] += status < 0, [1] += payload != ref, [2] += differs although status >= 0, [3] += status > 0,
 * [4] += max(status, 0), [5] += status < 0 although equal */
__global__ __launch_bounds__(256) void bch_tally_kernel(const int32_t *__restrict__ status, const uint8_t *__restrict__ payload,
                                                        const uint8_t *__restrict__ ref, int64_t frames, int64_t bytes_per_frame,
                                                        unsigned long long *__restrict__ counts)
{
    for (int64_t f = blockIdx.x; f < frames; f += gridDim.x) {
        unsigned diff = 0;
        for (int64_t j = threadIdx.x; j < bytes_per_frame; j += blockDim.x) {
            const int64_t i = f * bytes_per_frame + j;
            diff |= (unsigned)(payload[i] ^ (ref ? ref[i] : (uint8_t)0));
        }
        const int differs = __syncthreads_or(diff != 0);
        if (threadIdx.x == 0) {
            const int32_t st = status[f];
            if (st < 0) atomicAdd(&counts[0], 1ull);
            if (differs) atomicAdd(&counts[1], 1ull);
            if (differs && st >= 0) atomicAdd(&counts[2], 1ull);
            if (st > 0) atomicAdd(&counts[3], 1ull);
            if (st > 0) atomicAdd(&counts[4], (unsigned long long)st);
            if (!differs && st < 0) atomicAdd(&counts[5], 1ull);
        }
    }
}

}  // namespace ldpc
