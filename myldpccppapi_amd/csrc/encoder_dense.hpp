/*
 * encoder_dense.hpp -- host analysis behind LDPC_PARITY_DENSE (include/ldpc_hip.h, "encoder"): the solve matrix T of
 * H_p p = H_s u for any parity part of full column rank, and the systematic column order of any H.  Bit-packed
 * Gaussian elimination in 64-bit words, GF(2) only; no device is touched here.
 */
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/ldpc_hip.h"
#include "graph.hpp"
#include "hip_host.hpp"

namespace ldpc {

constexpr int32_t kDenseMaxRows = 16384;              /* T is at most 16384 x 16384 bits = 32 MiB            */
constexpr int64_t kOrderMaxBits = (int64_t)1 << 27;   /* ldpc_graph_systematic_order eliminates M x N bits */

struct DenseSolve {
    int32_t rho = 0, rank_hp = 0, M = 0, tw = 0;
    std::vector<uint64_t> T;      /* [rho][tw]: T H_p = I_rho, row c solves parity bit c; tail bits zero */
};

inline void xor_words(uint64_t *__restrict__ d, const uint64_t *__restrict__ s, int32_t n)
{
    for (int32_t k = 0; k < n; ++k) d[k] ^= s[k];
}

/* Arguments and the M cap; then Gauss-Jordan on [H_p | I_M] with row swaps.  After column c has found its pivot, row c
 * of the array is the only row with a one in column c, so on a parity part of full column rank the array ends as
 * [I_rho; 0 | R] and T is the identity half of rows 0 .. rho-1.  A pivot row is zero left of its column in every pivot
 * column, and columns are visited once, so the H_p half is combined from word c / 64 on only.  Rows rho .. M-1 of R are
 * the combinations of H's rows whose parity part vanishes: rank(H) = rho iff their information part vanishes too, which
 * is checked on the sparse H_s.  out (optional) is filled as far as the analysis came; want_T = false leaves out->T empty. */
inline int dense_analyse(const ldpc_graph *g, int32_t K, bool want_T, DenseSolve *out)
{
    if (!g) return set_error(LDPC_ERR_ARG, "graph is NULL");
    const int32_t M = g->M, N = g->N;
    if (K <= 0 || K < N - M || K >= N)
        return set_error(LDPC_ERR_ARG, "K = %d outside [max(1, N - M), N) = [%d, %d)", K, std::max(1, N - M), N);
    const int32_t rho = N - K, tw = (M + 63) / 64, pw = (rho + 63) / 64, rw = pw + tw;
    if (out) { out->rho = rho; out->M = M; out->tw = tw; }
    if (M > kDenseMaxRows)
        return set_error(LDPC_ERR_UNSUPPORTED, "dense encoder: M = %d rows, the limit is %d (the solve matrix would exceed 32 MiB)", M, kDenseMaxRows);
    std::vector<uint64_t> a((size_t)M * rw, 0);
    for (int64_t e = 0; e < g->E; ++e)
        if (g->cols[e] >= K) {
            const int32_t q = g->cols[e] - K;
            a[(size_t)g->rows[e] * rw + (q >> 6)] |= 1ull << (q & 63);
        }
    for (int32_t m = 0; m < M; ++m) a[(size_t)m * rw + pw + (m >> 6)] |= 1ull << (m & 63);
    int32_t rank = 0;
    for (int32_t c = 0; c < rho; ++c) {
        const int32_t cw = c >> 6;
        const uint64_t bit = 1ull << (c & 63);
        int32_t piv = rank;
        while (piv < M && !(a[(size_t)piv * rw + cw] & bit)) ++piv;
        if (piv == M) continue;                         /* dependent on the columns before it */
        if (piv != rank) std::swap_ranges(a.begin() + (size_t)piv * rw, a.begin() + (size_t)(piv + 1) * rw, a.begin() + (size_t)rank * rw);
        const uint64_t *src = &a[(size_t)rank * rw + cw];
        for (int32_t m = 0; m < M; ++m)
            if (m != rank && (a[(size_t)m * rw + cw] & bit)) xor_words(&a[(size_t)m * rw + cw], src, rw - cw);
        ++rank;
    }
    if (out) out->rank_hp = rank;
    if (rank < rho)
        return set_error(LDPC_ERR_UNSUPPORTED, "parity part is singular: rank %d of %d (columns %d .. %d of H; ldpc_graph_systematic_order "
                         "gives a column order that is encodable)", rank, rho, K, N - 1);
    /* rows rho .. M-1: zero parity part; their information part must be zero as well */
    std::vector<uint8_t> par((size_t)K);
    for (int32_t q = rho; q < M; ++q) {
        std::fill(par.begin(), par.end(), 0);
        const uint64_t *r = &a[(size_t)q * rw + pw];
        for (int32_t m = 0; m < M; ++m)
            if (r[m >> 6] >> (m & 63) & 1ull)
                for (int32_t k = g->row_ptr[m]; k < g->row_ptr[m + 1]; ++k)
                    if (g->cols[k] < K) par[(size_t)g->cols[k]] ^= 1;
        for (int32_t n = 0; n < K; ++n)
            if (par[(size_t)n])
                return set_error(LDPC_ERR_UNSUPPORTED, "information bits are not free: rank(H) > rho = N - K = %d (a combination of rows has an empty "
                                 "parity part and information column %d)", rho, n);
    }
    if (out && want_T) {
        out->T.resize((size_t)rho * tw);
        for (int32_t c = 0; c < rho; ++c) std::copy_n(&a[(size_t)c * rw + pw], tw, &out->T[(size_t)c * tw]);
    }
    return LDPC_OK;
}

/* Columns N-1 .. 0: a column is a pivot iff it is independent of the pivots found so far.  Forward elimination on
 * bit-packed rows: a row that has served as a pivot row is left alone, every other row is kept reduced against the pivots
 * so far, so "some unused row has a one in column c" is the independence test.  Only words 0 .. c / 64 matter any more. */
inline int systematic_order(const ldpc_graph *g, int32_t *perm, int32_t *rank_out)
{
    if (!g) return set_error(LDPC_ERR_ARG, "graph is NULL");
    if (!perm || !rank_out) return set_error(LDPC_ERR_ARG, "perm/rank is NULL");
    const int32_t M = g->M, N = g->N;
    if ((int64_t)M * N > kOrderMaxBits)
        return set_error(LDPC_ERR_UNSUPPORTED, "systematic order: M N = %d x %d = %lld bits, the limit is 2^27 = %lld", M, N,
                         (long long)((int64_t)M * N), (long long)kOrderMaxBits);
    const int32_t nw = (N + 63) / 64;
    std::vector<uint64_t> a((size_t)M * nw, 0);
    for (int64_t e = 0; e < g->E; ++e) a[(size_t)g->rows[e] * nw + (g->cols[e] >> 6)] |= 1ull << (g->cols[e] & 63);
    std::vector<uint8_t> pivot((size_t)N, 0);
    int32_t rank = 0;           /* rows 0 .. rank-1 have served as pivot rows */
    for (int32_t c = N - 1; c >= 0 && rank < M; --c) {
        const int32_t cw = c >> 6;
        const uint64_t bit = 1ull << (c & 63);
        int32_t piv = rank;
        while (piv < M && !(a[(size_t)piv * nw + cw] & bit)) ++piv;
        if (piv == M) continue;
        if (piv != rank) std::swap_ranges(a.begin() + (size_t)piv * nw, a.begin() + (size_t)piv * nw + cw + 1, a.begin() + (size_t)rank * nw);
        const uint64_t *src = &a[(size_t)rank * nw];
        for (int32_t m = piv + 1; m < M; ++m)
            if (a[(size_t)m * nw + cw] & bit) xor_words(&a[(size_t)m * nw], src, cw + 1);
        pivot[(size_t)c] = 1;
        ++rank;
    }
    int32_t lo = 0, hi = N - rank;
    for (int32_t n = 0; n < N; ++n) perm[pivot[(size_t)n] ? hi++ : lo++] = n;
    *rank_out = rank;
    return LDPC_OK;
}

}  // namespace ldpc
