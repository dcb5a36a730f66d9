/*
 * osd_kernels.hpp -- ordered-statistics decoding of the frames a decoder left with a dirty syndrome (the rule:
 * include/ldpc_hip.h, "ordered-statistics post-processing").
 *
 *   osd_flag_kernel   every frame: hard bits h = (p < 0), syndrome from the sparse graph, flag[f] = dirty; a clean frame's
 *                     outputs are written here.
 *   osd_kernel        one workgroup of 256 .. 1024 lanes (osd_block) per frame, gone at once when the frame is clean.
 *                     A dirty frame: the keys (w << 12) | n are sorted in LDS (bitonic), H is copied into LDS as R rows of W words, and the
 *                     columns are walked in key order.  A column whose bit survives in a row that has no pivot yet becomes
 *                     that row's pivot and is cleared from every other row (full reduction), so that at the end row i reads
 *                     c[p_i] = XOR of its free columns' bits.  With that,
 *                         mism_i = parity(row_i & h)                       (c0 differs from h at p_i)
 *                         D0     = sum_i w[p_i] mism_i
 *                         D_j    = D0 + w_j + sum_{i : A[i][j]} s_i,   s_i = mism_i ? -w[p_i] : +w[p_i]
 *                     and order 1 is a minimum over the free j of (D_j - D0, j) among the negative ones: on a tie c0 wins,
 *                     then the smallest j.  All sums are integers, so no order of summation shows.
 * Plain loads and vector stores, LDS atomics for the counters; no scratch.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osd_host.hpp"

namespace ldpc {

constexpr int kOsdFlagBlock = 256;
constexpr uint32_t kOsdNoRow = 0xFFFFFFFFu;
constexpr uint32_t kOsdUnused = 0xFFFFu;
/* ctl words: [0],[1] / [2],[3] = (count, pivot row) of even / odd columns; [4] = D0; [6..7] = the best flip (64 bits) */
constexpr int kOsdCtlD0 = 4, kOsdCtlBest = 6;

struct OsdOut {
    uint8_t *out, *code;        /* K / 8 and N bytes per frame; each may be null */
    int32_t *status, *metric;
    int32_t N, K;
};

struct OsdFlagArgs {
    const float *soft;
    int64_t frames;
    const int32_t *row_ptr, *cols;      /* the graph's rows, CSR */
    int32_t M;
    uint8_t *flag;
    OsdOut o;
};

struct OsdArgs {
    const float *soft;
    const uint32_t *image;      /* [R][W] */
    const uint8_t *flag;
    OsdLayout lay;
    int32_t order;
    float scale;
    OsdOut o;
};

/* the weight of the rule: integers, so that every sum is exact */
__device__ inline uint32_t osd_weight(float p, float scale)
{
    const float t = fabsf(p) * scale;
    return (p != p) ? 0u : (uint32_t)(int32_t)floorf(fminf(t, (float)kOsdMaxWeight));
}

/* a frame's outputs from the bitmap of its codeword */
__device__ inline void osd_store(const OsdOut &o, int64_t f, const uint32_t *cw, int32_t status, int32_t metric, int t, int T)
{
    if (o.code) {
        uint8_t *row = o.code + f * (int64_t)o.N;
        for (int n = t; n < o.N; n += T) row[n] = (uint8_t)((cw[n >> 5] >> (n & 31)) & 1u);
    }
    if (o.out) {
        const int nb = o.K / 8;
        uint8_t *row = o.out + f * (int64_t)nb;
        for (int b = t; b < nb; b += T) row[b] = (uint8_t)(cw[b >> 2] >> ((b & 3) * 8));
    }
    if (t == 0) {
        if (o.status) o.status[f] = status;
        if (o.metric) o.metric[f] = metric;
    }
}

/* the hard bit of position n; positions behind the row's end read as 0 */
__device__ inline bool osd_negative(const float *p, int n, int N) { return n < N && p[n] < 0.0f; }

__global__ __launch_bounds__(kOsdFlagBlock) void osd_flag_kernel(const OsdFlagArgs a)
{
    __shared__ uint32_t hb[kOsdMaxN / 32];
    const int t = (int)threadIdx.x, T = kOsdFlagBlock;
    const int N = a.o.N, W32 = 32 * ((N + 31) / 32);
    for (int64_t f = blockIdx.x; f < a.frames; f += gridDim.x) {
        const float *p = a.soft + f * (int64_t)N;
        for (int base = 0; base < W32; base += T) {
            const int n = base + t;
            const uint64_t b = __ballot(osd_negative(p, n, N));
            if ((t & 63) == 0 && n < W32) {
                hb[n >> 5] = (uint32_t)b;
                if (n + 32 < W32) hb[(n >> 5) + 1] = (uint32_t)(b >> 32);
            }
        }
        __syncthreads();
        uint32_t bad = 0;                                   /* any of this lane's rows with odd parity */
        for (int m = t; m < a.M; m += T) {
            uint32_t par = 0;                               /* per row: two failed rows of one lane must not cancel */
            for (int k = a.row_ptr[m]; k < a.row_ptr[m + 1]; ++k) {
                const int c = a.cols[k];
                par ^= (hb[c >> 5] >> (c & 31)) & 1u;
            }
            bad |= par;
        }
        const int dirty = __syncthreads_or((int)bad);
        if (t == 0) a.flag[f] = (uint8_t)(dirty != 0);
        if (!dirty) osd_store(a.o, f, hb, 0, 0, t, T);
        __syncthreads();
    }
}

__global__ __launch_bounds__(kOsdMaxBlock) void osd_kernel(const OsdArgs a)
{
    extern __shared__ uint32_t osd_lds[];
    const int64_t f = blockIdx.x;
    if (!a.flag[f]) return;
    const int t = (int)threadIdx.x, T = (int)blockDim.x;
    const int N = a.lay.N, R = a.lay.R, W = a.lay.W, P = a.lay.P;
    uint32_t *A = osd_lds + a.lay.A, *keys = osd_lds + a.lay.keys, *hb = osd_lds + a.lay.hb, *pm = osd_lds + a.lay.pm;
    uint32_t *cw = osd_lds + a.lay.cw, *ctl = osd_lds + a.lay.ctl;
    uint16_t *wt = reinterpret_cast<uint16_t *>(osd_lds + a.lay.wt);
    uint16_t *rowcol = reinterpret_cast<uint16_t *>(osd_lds + a.lay.rowcol);
    uint16_t *list = reinterpret_cast<uint16_t *>(osd_lds + a.lay.list);
    int32_t *s = reinterpret_cast<int32_t *>(osd_lds + a.lay.s);
    const float *p = a.soft + f * (int64_t)N;

    /* ---- keys, weights, hard bits, the image of H ---- */
    const int W32 = 32 * W, bound = P > W32 ? P : W32;
    for (int base = 0; base < bound; base += T) {
        const int n = base + t;
        const float v = n < N ? p[n] : 0.0f;
        if (n < P) {
            const uint32_t w = osd_weight(v, a.scale);
            if (n < N) wt[n] = (uint16_t)w;
            keys[n] = n < N ? (w << 12) | (uint32_t)n : 0xFFFFFFFFu;
        }
        const uint64_t b = __ballot(n < N && v < 0.0f);
        if ((t & 63) == 0 && n < W32) {
            hb[n >> 5] = (uint32_t)b;
            if (n + 32 < W32) hb[(n >> 5) + 1] = (uint32_t)(b >> 32);
        }
    }
    for (int i = t; i < R * W; i += T) A[i] = a.image[i];
    for (int r = t; r < R; r += T) rowcol[r] = (uint16_t)kOsdUnused;
    for (int w = t; w < W; w += T) pm[w] = 0;
    if (t < (int)kOsdCtlWords) ctl[t] = (t == 1 || t == 3 || t == kOsdCtlBest || t == kOsdCtlBest + 1) ? kOsdNoRow : 0u;
    __syncthreads();

    /* ---- order: bitonic sort of the P keys, the least reliable first, ties to the index ---- */
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += T) {
                const int x = i ^ j;
                if (x > i) {
                    const uint32_t u = keys[i], v = keys[x];
                    if ((u > v) == ((i & k) == 0)) { keys[i] = v; keys[x] = u; }
                }
            }
            __syncthreads();
        }

    /* ---- least reliable basis: walk the columns in key order, fully reduce on every pivot ---- */
    const int wl = t & (a.lay.G - 1), grp = t >> a.lay.logG, groups = T >> a.lay.logG;
    int rank = 0;
    for (int idx = 0; idx < N && rank < R; ++idx) {
        const int slot = (idx & 1) * 2;
        const int c = (int)(keys[idx] & 4095u), cword = c >> 5, cbit = c & 31;
        for (int r = t; r < R; r += T)
            if ((A[r * W + cword] >> cbit) & 1u) {
                list[atomicAdd(&ctl[slot], 1u)] = (uint16_t)r;
                if (rowcol[r] == kOsdUnused) atomicMin(&ctl[slot + 1], (uint32_t)r);
            }
        __syncthreads();
        const int hits = (int)ctl[slot];
        const uint32_t piv = ctl[slot + 1];
        if (t == 0) { ctl[slot ^ 2] = 0; ctl[(slot ^ 2) + 1] = kOsdNoRow; }     /* the next column's pair: nobody reads it now */
        if (piv != kOsdNoRow) {
            ++rank;
            if (t == 0) { rowcol[piv] = (uint16_t)c; pm[cword] |= 1u << cbit; }
            if (wl < W) {
                const uint32_t pw = A[piv * W + wl];
                if (pw)
                    for (int e = grp; e < hits; e += groups) {
                        const uint32_t r = list[e];
                        if (r != piv) A[r * W + wl] ^= pw;
                    }
            }
        }
        __syncthreads();
    }

    /* ---- order 0: the mismatch bit of every pivot, D0 ---- */
    int32_t d0 = 0;
    for (int r = t; r < R; r += T) {
        const uint32_t rc = rowcol[r];
        int32_t sv = 0;
        if (rc != kOsdUnused) {
            uint32_t par = 0;
            for (int w = 0; w < W; ++w) par ^= A[r * W + w] & hb[w];
            const int32_t wp = (int32_t)wt[rc];
            if (__popc(par) & 1) { rowcol[r] = (uint16_t)(rc | 0x8000u); d0 += wp; sv = -wp; }
            else sv = wp;
        }
        s[r] = sv;
    }
    if (d0) atomicAdd(&ctl[kOsdCtlD0], (uint32_t)d0);
    for (int w = t; w < W; w += T) cw[w] = hb[w];
    __syncthreads();

    /* ---- order 1: one lane per free position ---- */
    unsigned long long *best = reinterpret_cast<unsigned long long *>(ctl + kOsdCtlBest);
    if (a.order >= 1) {
        for (int j = t; j < N; j += T) {
            const int jw = j >> 5, jb = j & 31;
            if ((pm[jw] >> jb) & 1u) continue;
            int32_t delta = (int32_t)wt[j];
            for (int r = 0; r < R; ++r)
                if ((A[r * W + jw] >> jb) & 1u) delta += s[r];
            if (delta < 0) atomicMin(best, ((unsigned long long)((uint32_t)delta ^ 0x80000000u) << 32) | (uint32_t)j);
        }
        __syncthreads();
    }
    const unsigned long long chosen = *best;
    const bool flip = chosen != ~0ull;
    const int jf = (int)(uint32_t)chosen;
    const int32_t dflip = flip ? (int32_t)((uint32_t)(chosen >> 32) ^ 0x80000000u) : 0;

    /* ---- the codeword: h on the free positions (but jf), the pivots follow ---- */
    for (int r = t; r < R; r += T) {
        const uint32_t rc = rowcol[r];
        if (rc == kOsdUnused) continue;
        uint32_t m = rc >> 15;
        if (flip) m ^= (A[r * W + (jf >> 5)] >> (jf & 31)) & 1u;
        const uint32_t col = rc & 4095u;
        if (m) atomicXor(&cw[col >> 5], 1u << (col & 31));
    }
    if (t == 0 && flip) atomicXor(&cw[jf >> 5], 1u << (jf & 31));
    __syncthreads();
    osd_store(a.o, f, cw, flip ? 2 : 1, (int32_t)ctl[kOsdCtlD0] + dflip, t, T);
}

}  // namespace ldpc
