/*
 * osd_host.hpp -- the host-only part of the ordered-statistics stage (include/ldpc_hip.h, "ordered-statistics
 * post-processing"): the eligibility arithmetic, the dense bit image of H that a workgroup copies into LDS, and the LDS
 * layout of osd_kernels.hpp.  No HIP: tests/cpp/osd_host_test.cpp compiles this file alone under the host sanitizers.
 */
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <vector>

namespace ldpc {

constexpr int32_t kOsdMaxN = 4096;              /* a position fits the 12 low bits of a sort key                    */
constexpr int64_t kOsdMaxWords = 28672;         /* M * ceil(N / 32): 112 KiB of the 160 KiB a workgroup can have    */
constexpr int32_t kOsdMaxWeight = 65535;
constexpr int32_t kOsdMaxBlock = 1024;          /* most threads of the workgroup that owns a dirty frame            */
constexpr size_t kOsdMaxLds = 160 * 1024 - 512; /* one workgroup's dynamic LDS                                      */

inline int32_t osd_words(int32_t N) { return (N + 31) / 32; }

/* 0: the code fits.  1: it does not; msg states both numbers of the rule. */
inline int osd_eligible(int32_t M, int32_t N, char *msg, size_t cap)
{
    const int64_t words = (int64_t)M * osd_words(N);
    if (N <= kOsdMaxN && words <= kOsdMaxWords) return 0;
    snprintf(msg, cap,
             "ordered-statistics decoding needs N <= %d and M * ceil(N / 32) <= %lld words of LDS: this graph has N = %d and "
             "M * ceil(N / 32) = %d * %d = %lld",
             kOsdMaxN, (long long)kOsdMaxWords, N, M, osd_words(N), (long long)words);
    return 1;
}

/* The dense image: R rows of W = ceil(N / 32) words, bit n of a row = bit n % 32 of word n / 32; bits N .. 32 W - 1 are
 * zero.  R = M rows in the graph's order when M <= N.  A graph with more rows than columns has dependent rows; then the
 * image keeps the first maximal independent subset of them (R = rank <= N), which spans the same row space and so
 * defines the same code -- the per-row bookkeeping of the kernel is sized for R <= N.
 * row_ptr: [M + 1], cols: [E], the graph's CSR form. */
struct OsdImage {
    int32_t R = 0, W = 0;
    std::vector<uint32_t> bits;    /* [R][W] */
};

inline void osd_dense_image(int32_t M, int32_t N, const int32_t *row_ptr, const int32_t *cols, OsdImage *out)
{
    const int32_t W = osd_words(N);
    out->W = W;
    out->bits.clear();
    std::vector<uint32_t> row((size_t)W);
    auto fill = [&](int32_t m) {
        for (int32_t w = 0; w < W; ++w) row[(size_t)w] = 0;
        for (int32_t k = row_ptr[m]; k < row_ptr[m + 1]; ++k) row[(size_t)(cols[k] >> 5)] ^= 1u << (cols[k] & 31);
    };
    if (M <= N) {
        out->R = M;
        out->bits.reserve((size_t)M * W);
        for (int32_t m = 0; m < M; ++m) {
            fill(m);
            out->bits.insert(out->bits.end(), row.begin(), row.end());
        }
        return;
    }
    /* greedy independent subset: basis[c] is a reduced vector whose lowest set bit is column c */
    std::vector<std::vector<uint32_t>> basis((size_t)N);
    std::vector<uint32_t> v((size_t)W);
    int32_t R = 0;
    for (int32_t m = 0; m < M && R < N; ++m) {
        fill(m);
        v = row;
        for (;;) {
            int32_t lead = -1;
            for (int32_t w = 0; w < W && lead < 0; ++w)
                if (v[(size_t)w]) lead = 32 * w + __builtin_ctz(v[(size_t)w]);
            if (lead < 0) break;                      /* dependent on the rows kept so far */
            if (basis[(size_t)lead].empty()) {
                basis[(size_t)lead] = v;
                out->bits.insert(out->bits.end(), row.begin(), row.end());
                ++R;
                break;
            }
            for (int32_t w = 0; w < W; ++w) v[(size_t)w] ^= basis[(size_t)lead][(size_t)w];
        }
    }
    if (R == 0) {                                     /* H = 0 (cannot happen: a graph has an edge); keep one zero row */
        out->bits.assign((size_t)W, 0u);
        R = 1;
    }
    out->R = R;
}

/* The workgroup's LDS, offsets in 32-bit words.  A: the image, [R][W].  keys: the sort keys (w << 12) | n, padded to a
 * power of two P.  wt: the weights as uint16, [N].  hb / pm / cw: bitmaps of W words -- the hard bits, the pivot
 * columns, the chosen codeword.  rowcol: uint16 per row, the row's pivot column (bit 15: its mismatch bit), 0xFFFF while
 * unused.  s: int32 per row, the signed weight of its pivot.  list: uint16 per row, the rows that have the current
 * column.  ctl: counters, the pivot of the current column, reduction scratch. */
struct OsdLayout {
    int32_t R = 0, N = 0, W = 0, P = 0, G = 0, logG = 0;
    uint32_t A = 0, keys = 0, wt = 0, hb = 0, pm = 0, cw = 0, rowcol = 0, s = 0, list = 0, ctl = 0, total_words = 0;
    size_t bytes() const { return (size_t)total_words * 4; }
};
constexpr uint32_t kOsdCtlWords = 48;

/* threads of the workgroup that owns a dirty frame: sixteen groups of G = 2^ceil(log2 W) lanes, each group one row of the
 * XOR phase, within [256, 1024].  Measured: (576, 288), G = 32, is fastest at 512 lanes -- more lanes only make
 * its barriers dearer -- and (1152, 576), G = 64, at 1024. */
inline int32_t osd_block(int32_t W)
{
    int32_t G = 1;
    while (G < W) G *= 2;
    const int32_t T = 16 * G;
    return T < 256 ? 256 : T > kOsdMaxBlock ? kOsdMaxBlock : T;
}

inline OsdLayout osd_layout(int32_t R, int32_t N)
{
    OsdLayout l;
    l.R = R; l.N = N; l.W = osd_words(N);
    l.P = 2;
    while (l.P < N) l.P *= 2;
    /* lanes that share one row in the XOR phase: the power of two that holds a row's words */
    l.G = 1; l.logG = 0;
    while (l.G < l.W) { l.G *= 2; ++l.logG; }
    uint32_t at = 0;
    auto take = [&](uint32_t words) { const uint32_t a = at; at += words; return a; };
    l.A = take((uint32_t)R * (uint32_t)l.W);
    l.keys = take((uint32_t)l.P);
    l.wt = take(((uint32_t)N + 1) / 2);
    l.hb = take((uint32_t)l.W);
    l.pm = take((uint32_t)l.W);
    l.cw = take((uint32_t)l.W);
    l.rowcol = take(((uint32_t)R + 1) / 2);
    l.s = take((uint32_t)R);
    l.list = take(((uint32_t)R + 1) / 2);
    at = (at + 1) & ~1u;                              /* ctl holds a 64-bit word */
    l.ctl = take(kOsdCtlWords);
    l.total_words = at;
    return l;
}

}  // namespace ldpc
