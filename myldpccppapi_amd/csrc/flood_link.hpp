/*
 * flood_link.hpp -- the column-fused check kernels (column-local fusion of the staircase columns): wide,
 * narrow / half and deep forms.
 */
#pragma once

#include "flood_check.hpp"
#include "flood_var.hpp"

namespace ldpc {

/* ---- column-local fusion ------------------------------------------------------------
 * A degree-2 column whose two checks are CONSECUTIVE rows handled by the same wave (the
 * staircase parity columns of an IRA / DVB-S2 code: column K+m sits in rows m and m+1) never
 * needs its check->variable messages in HBM: the wave that has just produced both of them
 * holds everything the variable node needs.  It applies the variable-node update right there
 * (same fp32 operations in the same order as var_kernel, so results stay bit-identical),
 * writes the two NEW variable->check messages into the slots whose old values it has already
 * consumed (only these two rows ever read them), and sets the column's hard bit.  Per such
 * column this saves one 4-byte write and one 4-byte read per edge and frame
 * (DVB-S2 1/2, 16 rows per wave: 12.5 % of all traffic; measured -13.5 % step time).  Columns on a wave's chunk
 * boundary, and all other columns, go through var_kernel as before.
 *
 * The three forms below repeat one row pipeline on purpose.  Moving it into a shared body, or its selection chains,
 * mask handling and variable node into helpers, computes the same values but changes the compiler's schedule: of the
 * 750 instantiations some 270 then need 1 to 10 more VGPRs and nine lose a wave per SIMD, even when the shared
 * body is nothing but one form's own text behind a call.  A change to one form is made in all three by hand. */
struct LinkArgs {
    const int32_t *__restrict__ link_col;  /* [n_rows] column linking list row i and i+1, or -1 */
    const int32_t *__restrict__ link_pos;  /* [n_rows] ka | kb << 8: edge position in row i / row i+1 */
    const void *__restrict__ chan;         /* [T][N][F] */
    void *Qw;                              /* = Q, for the in-place writes */
    uint64_t *hard;                        /* [T][N][V] */
    int32_t N;
    int32_t write_q;
    int32_t store_all;                     /* debug taps: also store the fused columns' R */
    /* the few rows of OTHER degrees that are not worth a launch of their own (an IRA code's first row):
     * blocks from link_blocks on take one each per wave, run-time loops */
    const int32_t *__restrict__ extra_e0;  /* [n_extra] first edge id */
    const int32_t *__restrict__ extra_deg; /* [n_extra] */
    int32_t n_extra;
    int32_t link_blocks;                   /* blocks of the linked rows proper */
    /* guided chunks: the first n_big row chunks of a tile hold rows_per_wave rows, the rest small_rows.
     * With a grid of (tiles, blocks) -- grid_pos() -- the launch ENDS with the short
     * chunks of all tiles and its last waves are short ones -- with equal chunks the CUs drain over a whole
     * chunk's time (16 rows: 176 us of a 1.39 ms launch, half of it lost). */
    int32_t n_big, small_rows;
};

/* rows [*rb, *re) of chunk c of a class of n_rows rows (host: fusion lists, grid size; device: the kernels) */
__host__ __device__ inline void link_chunk_rows(int c, int rows_per_wave, int n_big, int small_rows, int n_rows,
                                               int *rb, int *re)
{
    int b, e;
    if (c < n_big) { b = c * rows_per_wave; e = b + rows_per_wave; }
    else { b = n_big * rows_per_wave + (c - n_big) * small_rows; e = b + small_rows; }
    *rb = b < n_rows ? b : n_rows;
    *re = e < n_rows ? e : n_rows;
}
/* number of chunks */
__host__ __device__ inline int link_chunk_count(int rows_per_wave, int n_big, int small_rows, int n_rows)
{
    const int rest = n_rows - n_big * rows_per_wave;
    return n_big + (rest > 0 ? (rest + small_rows - 1) / small_rows : 0);
}

/* the trailing blocks of a linked check launch: one left-over row per wave, V values per lane */
template <int ALGO, int V, typename T>
__device__ __forceinline__ void link_extra_rows(const CheckArgs &a, const LinkArgs &g, int tile, int block)
{
    constexpr size_t F = 64 * V;
    const int lane = threadIdx.x & 63;
    const int w = (block - g.link_blocks) * kWavesPerBlock + wave_id_in_block();
    if (w >= g.n_extra) return;
    const T *Qu = static_cast<const T *>(a.Q) + (size_t)tile * (size_t)a.E * F;
    T *Rt = static_cast<T *>(a.R) + (size_t)tile * (size_t)a.E * F + (size_t)lane * V;
    check_row_generic<ALGO, V, T>(Qu, (unsigned)lane * V, Rt, g.extra_e0[w], g.extra_deg[w], a.qpos, ms_corr_of(a));
}

/* build-time experiment hook: -DLDPC_LINK_WIDE_WAVES=n asks the compiler for n waves per SIMD */
#ifdef LDPC_LINK_WIDE_WAVES
#define LDPC_LINK_WIDE_ATTR __attribute__((amdgpu_waves_per_eu(LDPC_LINK_WIDE_WAVES, LDPC_LINK_WIDE_WAVES)))
#else
#define LDPC_LINK_WIDE_ATTR
#endif
template <int ALGO, int D, int V, typename T>
__global__ __launch_bounds__(kBlock) LDPC_LINK_WIDE_ATTR void check_link_kernel(const CheckArgs a, const LinkArgs g)
{
    constexpr size_t F = 64 * V;
    const int lane = threadIdx.x & 63;
    const GridPos gp = grid_pos(a.tiles_first);
    const int tile = tile_select<V>(a.tail, a.done, gp.row);
    if (tile < 0) return;
    if (gp.block >= g.link_blocks) { link_extra_rows<ALGO, V, T>(a, g, tile, gp.block); return; }
    const int wave = gp.block * kWavesPerBlock + wave_id_in_block();
    int r_begin, r_end;
    link_chunk_rows(wave, a.rows_per_wave, g.n_big, g.small_rows, a.n_rows, &r_begin, &r_end);
    const size_t lane_off = (size_t)lane * V;
    /* Q: wave-uniform row addresses plus a 32-bit lane offset (scalar base + vector offset addressing: the slots of a
     * row are unrelated, one 64-bit vector address each would cost 2 registers per message in flight) */
    const unsigned lane_q = (unsigned)lane * V;
    const T *Qt = static_cast<const T *>(a.Q) + (size_t)tile * (size_t)a.E * F;
    T *Qwt = static_cast<T *>(g.Qw) + (size_t)tile * (size_t)a.E * F;
    T *Rt = static_cast<T *>(a.R) + (size_t)tile * (size_t)a.E * F + lane_off;
    const T *chan_t = static_cast<const T *>(g.chan) + (size_t)tile * (size_t)g.N * F + lane_off;
    uint64_t *hard_t = g.hard + (size_t)tile * (size_t)g.N * V;
    uint64_t frozen[V];
#pragma unroll
    for (int v = 0; v < V; ++v) frozen[v] = a.done[(size_t)tile * V + v];

    int pend_col = -1, pend_edge = 0, pend_kb = 0;   /* column opened by the previous row */
    float pend_r[V];
#pragma unroll
    for (int v = 0; v < V; ++v) pend_r[v] = 0.0f;

    /* software pipeline: row r+1's messages are requested before row r is worked on */
    float x[D][V];
    int qc[D], qn[D];                /* Q slots (CheckArgs::qpos) of this row's and of the next row's messages */
#pragma unroll
    for (int k = 0; k < D; ++k) qc[k] = qn[k] = 0;
    if (r_begin < r_end) {
        row_slots<D>(a.qpos, a.cls_e0[r_begin], lane, qc);
#pragma unroll
        for (int k = 0; k < D; ++k) vload<V>(x[k], Qt + (size_t)qc[k] * F + lane_q);
    }
    for (int r = r_begin; r < r_end; ++r) {
        const int e0 = a.cls_e0[r];
        const int next_col = (r + 1 < r_end) ? g.link_col[r] : -1;
        const int pos = g.link_pos[r];
        const int ka = next_col >= 0 ? (pos & 255) : -1;      /* this row's edge into next_col */
        const int kb = pend_col >= 0 ? pend_kb : -1;          /* this row's edge into pend_col */
        /* the next row's slots: asked for here, ahead of the row's arithmetic */
        if (r + 1 < r_end) row_slots<D>(a.qpos, a.cls_e0[r + 1], lane, qn);
        /* everything the pending column needs besides this row's result: request it now */
        float ch[V];
        uint64_t old_w[V];
        if (pend_col >= 0) {
            vload<V>(ch, chan_t + (size_t)pend_col * F);
#pragma unroll
            for (int v = 0; v < V; ++v) old_w[v] = hard_t[(size_t)pend_col * V + v];
        }
        float out[D][V];
        check_node<ALGO, D, V, T>(x, out, ms_corr_of(a));
        if (r + 1 < r_end) {
#pragma unroll
            for (int k = 0; k < D; ++k) vload<V>(x[k], Qt + (size_t)qn[k] * F + lane_q);
        }
#pragma unroll
        for (int k = 0; k < D; ++k)
            if ((k != ka && k != kb) || g.store_all) vstore<V>(Rt + (size_t)(e0 + k) * F, out[k]);

        if (pend_col >= 0) {
            /* variable node of pend_col: edges (previous row, ka') then (this row, kb), ascending */
            float rr[2][V], q[2][V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                rr[0][v] = pend_r[v];
                float t = out[0][v];
#pragma unroll
                for (int k = 1; k < D; ++k) t = (k == kb) ? out[k][v] : t;
                rr[1][v] = t;
            }
            uint64_t new_w[V];
            if (ALGO == kAlgoSP) {
                float f0[V], f1[V];
                var_sp<2, V>(ch, rr, q, f0, f1);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const bool oldb = (old_w[v] >> lane) & 1ull;
                    const bool b = (f0[v] > f1[v]) ? false : ((f0[v] < f1[v]) ? true : oldb);
                    new_w[v] = __ballot(b);
                }
            } else {
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    float p = ch[v];
                    p += rr[0][v];
                    p += rr[1][v];
                    q[0][v] = p - rr[0][v];
                    q[1][v] = p - rr[1][v];
                    new_w[v] = __ballot(!(p > 0.0f));
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int v = 0; v < V; ++v)
                    hard_t[(size_t)pend_col * V + v] = (old_w[v] & frozen[v]) | (new_w[v] & ~frozen[v]);
            }
            if (g.write_q) {
                int qw1 = qc[0];                              /* slot of this row's edge kb */
#pragma unroll
                for (int k = 1; k < D; ++k) qw1 = (k == kb) ? qc[k] : qw1;
                vstore<V>(Qwt + (size_t)pend_edge * F + lane_q, q[0]);
                vstore<V>(Qwt + (size_t)qw1 * F + lane_q, q[1]);
            }
        }
        pend_col = next_col;
        if (next_col >= 0) {
            pend_edge = qc[0];                                /* SLOT of this row's edge ka: written by the next row */
#pragma unroll
            for (int k = 1; k < D; ++k) pend_edge = (k == ka) ? qc[k] : pend_edge;
            pend_kb = (pos >> 8) & 255;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float t = out[0][v];
#pragma unroll
                for (int k = 1; k < D; ++k) t = (k == ka) ? out[k][v] : t;
                pend_r[v] = t;
            }
        }
#pragma unroll
        for (int k = 0; k < D; ++k) qc[k] = qn[k];
    }
}

/* check_link_kernel in NARROW waves (1 value per lane, V sub-waves per row chunk): the register
 * footprint of the wide version (114 VGPRs, 4 waves/SIMD) made it the one kernel whose time
 * varied between boxes (1.31-1.55 ms); here 8 waves/SIMD hide the same latency.  Hard bits:
 * sub-wave j holds frames 64j..64j+63 of the tile, i.e. the 64/V-bit field [j*64/V, (j+1)*64/V)
 * of each of the V mask words (bit l of word v = frame V*l+v) -- written as that field alone
 * (16-bit stores at V = 4), no atomics: the fields of different sub-waves are disjoint. */
template <int ALGO, int D, int V, typename T, int W = 1>
__global__ __launch_bounds__(kBlock) void check_link_narrow_kernel(const CheckArgs a, const LinkArgs g)
{
    /* W values per lane: V / W sub-waves cover a row's 64*V-frame segment (W = 1: the narrow kernel;
     * W = 2 at V = 4: 8 bytes per lane, half the registers of the wide kernel at twice its occupancy). */
    constexpr size_t F = 64 * V;
    constexpr int SUBS = V / W;                      /* sub-waves per row chunk */
    constexpr int FB = 64 / SUBS;                    /* bits per field */
    const int lane = threadIdx.x & 63;
    const GridPos gp = grid_pos(a.tiles_first);
    const int tile = tile_select<V>(a.tail, a.done, gp.row);
    if (tile < 0) return;
    if (gp.block >= g.link_blocks) { link_extra_rows<ALGO, V, T>(a, g, tile, gp.block); return; }
    const int wave = gp.block * kWavesPerBlock + wave_id_in_block();
    const int sub = wave % SUBS;
    int r_begin, r_end;
    link_chunk_rows(wave / SUBS, a.rows_per_wave, g.n_big, g.small_rows, a.n_rows, &r_begin, &r_end);
    const size_t lane_off = (size_t)sub * 64 * W + (size_t)lane * W;
    const unsigned lane_q = (unsigned)lane_off;      /* Q: wave-uniform row addresses + 32-bit lane offset (check_link_kernel) */
    const T *Qt = static_cast<const T *>(a.Q) + (size_t)tile * (size_t)a.E * F;
    T *Qwt = static_cast<T *>(g.Qw) + (size_t)tile * (size_t)a.E * F;
    T *Rt = static_cast<T *>(a.R) + (size_t)tile * (size_t)a.E * F + lane_off;
    const T *chan_t = static_cast<const T *>(g.chan) + (size_t)tile * (size_t)g.N * F + lane_off;
    /* this lane's value w is frame 64*W*sub + W*lane + w of the tile = V*l' + v'
     *   ->  word v' = (W*lane + w) % V, bit sub*FB + (W*lane + w) / V */
    uint8_t *hard_b = reinterpret_cast<uint8_t *>(g.hard + (size_t)tile * (size_t)g.N * V) + (size_t)sub * (FB / 8);
    /* frozen frames of this sub-wave, per word (lanes 0..V-1 keep the field of word `lane`) */
    const uint64_t frozen_field = (a.done[(size_t)tile * V + (lane < V ? lane : 0)] >> (sub * FB)) &
                                  (FB == 64 ? ~0ull : ((1ull << (FB & 63)) - 1ull));

    auto load_field = [&](int col, int word) -> uint64_t {
        const uint8_t *p = hard_b + ((size_t)col * V + word) * 8;
        if (FB == 64) return *reinterpret_cast<const uint64_t *>(p);
        if (FB == 32) return *reinterpret_cast<const uint32_t *>(p);
        return *reinterpret_cast<const uint16_t *>(p);
    };

    int pend_col = -1, pend_edge = 0, pend_kb = 0;
    float pend_r[W];
#pragma unroll
    for (int w = 0; w < W; ++w) pend_r[w] = 0.0f;
    float x[D][W];
    int qc[D], qn[D];                /* Q slots of this row's and of the next row's messages */
#pragma unroll
    for (int k = 0; k < D; ++k) qc[k] = qn[k] = 0;
    if (r_begin < r_end) {
        row_slots<D>(a.qpos, a.cls_e0[r_begin], lane, qc);
#pragma unroll
        for (int k = 0; k < D; ++k) vload<W>(x[k], Qt + (size_t)qc[k] * F + lane_q);
    }
    for (int r = r_begin; r < r_end; ++r) {
        const int e0 = a.cls_e0[r];
        const int next_col = (r + 1 < r_end) ? g.link_col[r] : -1;
        const int pos = g.link_pos[r];
        const int ka = next_col >= 0 ? (pos & 255) : -1;
        const int kb = pend_col >= 0 ? pend_kb : -1;
        if (r + 1 < r_end) row_slots<D>(a.qpos, a.cls_e0[r + 1], lane, qn);
        float ch[W];
        uint64_t old_mine[W];
#pragma unroll
        for (int w = 0; w < W; ++w) { ch[w] = 0.0f; old_mine[w] = 0; }
        if (pend_col >= 0) {
            vload<W>(ch, chan_t + (size_t)pend_col * F);
#pragma unroll
            for (int w = 0; w < W; ++w) old_mine[w] = load_field(pend_col, (W * lane + w) % V);
        }
        float out[D][W];
        check_node<ALGO, D, W, T>(x, out, ms_corr_of(a));
        if (r + 1 < r_end) {
#pragma unroll
            for (int k = 0; k < D; ++k) vload<W>(x[k], Qt + (size_t)qn[k] * F + lane_q);
        }
#pragma unroll
        for (int k = 0; k < D; ++k)
            if ((k != ka && k != kb) || g.store_all) vstore<W>(Rt + (size_t)(e0 + k) * F, out[k]);

        if (pend_col >= 0) {
            float rr[2][W], q[2][W];
#pragma unroll
            for (int w = 0; w < W; ++w) {
                rr[0][w] = pend_r[w];
                float t = out[0][w];
#pragma unroll
                for (int k = 1; k < D; ++k) t = (k == kb) ? out[k][w] : t;
                rr[1][w] = t;
            }
            uint64_t ballot[W];
            if (ALGO == kAlgoSP) {
                float f0[W], f1[W];
                var_sp<2, W>(ch, rr, q, f0, f1);
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const bool oldb = (old_mine[w] >> ((W * lane + w) / V)) & 1ull;
                    const bool bit = (f0[w] > f1[w]) ? false : ((f0[w] < f1[w]) ? true : oldb);
                    ballot[w] = __ballot(bit);
                }
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    float p = ch[w];
                    p += rr[0][w];
                    p += rr[1][w];
                    q[0][w] = p - rr[0][w];
                    q[1][w] = p - rr[1][w];
                    ballot[w] = __ballot(!(p > 0.0f));
                }
            }
            if (lane < V) {
                /* field of word `lane` = W*j + w: value w of the lanes j, j + SUBS, j + 2*SUBS, ... */
                uint64_t bw = ballot[0];
#pragma unroll
                for (int w = 1; w < W; ++w) bw = (lane % W == w) ? ballot[w] : bw;
                const uint64_t nf = compress_stride<SUBS>(bw >> (lane / W));
                const uint64_t of = load_field(pend_col, lane);
                const uint64_t res = (of & frozen_field) | (nf & ~frozen_field);
                uint8_t *p = hard_b + ((size_t)pend_col * V + lane) * 8;
                if (FB == 64) *reinterpret_cast<uint64_t *>(p) = res;
                else if (FB == 32) *reinterpret_cast<uint32_t *>(p) = (uint32_t)res;
                else *reinterpret_cast<uint16_t *>(p) = (uint16_t)res;
            }
            if (g.write_q) {
                int qw1 = qc[0];
#pragma unroll
                for (int k = 1; k < D; ++k) qw1 = (k == kb) ? qc[k] : qw1;
                vstore<W>(Qwt + (size_t)pend_edge * F + lane_q, q[0]);
                vstore<W>(Qwt + (size_t)qw1 * F + lane_q, q[1]);
            }
        }
        pend_col = next_col;
        if (next_col >= 0) {
            pend_edge = qc[0];                                /* SLOT of this row's edge ka */
#pragma unroll
            for (int k = 1; k < D; ++k) pend_edge = (k == ka) ? qc[k] : pend_edge;
            pend_kb = (pos >> 8) & 255;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                float t = out[0][w];
#pragma unroll
                for (int k = 1; k < D; ++k) t = (k == ka) ? out[k][w] : t;
                pend_r[w] = t;
            }
        }
#pragma unroll
        for (int k = 0; k < D; ++k) qc[k] = qn[k];
    }
}

/* The same kernel with the row inputs requested TWO rows ahead (three buffers in rotation): a wave
 * of the kernel above has one row (7 x 256 B) in flight while it works -- 57 KB per CU at 32 waves --
 * and runs at 83-94 % of the box's copy rate depending on the box; this one keeps two. */
template <int ALGO, int D, int V, typename T>
__global__ __launch_bounds__(kBlock) void check_link_narrow2_kernel(const CheckArgs a, const LinkArgs g)
{
    constexpr size_t F = 64 * V;
    constexpr int FB = 64 / V;                       /* bits per field */
    const int lane = threadIdx.x & 63;
    const GridPos gp = grid_pos(a.tiles_first);
    const int tile = tile_select<V>(a.tail, a.done, gp.row);
    if (tile < 0) return;
    if (gp.block >= g.link_blocks) { link_extra_rows<ALGO, V, T>(a, g, tile, gp.block); return; }
    const int wave = gp.block * kWavesPerBlock + wave_id_in_block();
    const int sub = wave % V;
    int r_begin, r_end;
    link_chunk_rows(wave / V, a.rows_per_wave, g.n_big, g.small_rows, a.n_rows, &r_begin, &r_end);
    const size_t lane_off = (size_t)sub * 64 + lane;
    const T *Qt = static_cast<const T *>(a.Q) + (size_t)tile * (size_t)a.E * F + lane_off;
    T *Qwt = static_cast<T *>(g.Qw) + (size_t)tile * (size_t)a.E * F + lane_off;
    T *Rt = static_cast<T *>(a.R) + (size_t)tile * (size_t)a.E * F + lane_off;
    const T *chan_t = static_cast<const T *>(g.chan) + (size_t)tile * (size_t)g.N * F + lane_off;
    /* this lane's frame 64*sub + lane = V*l' + v'  ->  word v' = lane % V, bit sub*FB + lane / V */
    const int my_word = lane % V, my_bit = lane / V;
    uint8_t *hard_b = reinterpret_cast<uint8_t *>(g.hard + (size_t)tile * (size_t)g.N * V) + (size_t)sub * (FB / 8);
    /* frozen frames of this sub-wave, per word (lanes 0..V-1 keep the field of word `lane`) */
    const uint64_t frozen_field = (a.done[(size_t)tile * V + (lane < V ? lane : 0)] >> (sub * FB)) &
                                  (FB == 64 ? ~0ull : ((1ull << FB) - 1ull));

    auto load_field = [&](int col, int word) -> uint64_t {
        const uint8_t *p = hard_b + ((size_t)col * V + word) * 8;
        if (V == 1) return *reinterpret_cast<const uint64_t *>(p);
        if (V == 2) return *reinterpret_cast<const uint32_t *>(p);
        return *reinterpret_cast<const uint16_t *>(p);
    };

    int pend_col = -1, pend_edge = 0, pend_kb = 0;
    float pend_r = 0.0f;
    /* three row buffers in rotation: while row r is worked on, rows r+1 and r+2 are in flight */
    float b0[D], b1[D], b2[D];
    auto load_row = [&](float (&dst)[D], int r) {
        const int e = a.cls_e0[r];
#pragma unroll
        for (int k = 0; k < D; ++k) { float t[1]; vload<1>(t, Qt + (size_t)edge_slot(a.qpos, e + k) * F); dst[k] = t[0]; }
    };
    if (r_begin < r_end) load_row(b0, r_begin);
    if (r_begin + 1 < r_end) load_row(b1, r_begin + 1);
    auto step = [&](int r, float (&x)[D], float (&pre)[D]) {
        const int e0 = a.cls_e0[r];
        const int next_col = (r + 1 < r_end) ? g.link_col[r] : -1;
        const int pos = g.link_pos[r];
        const int ka = next_col >= 0 ? (pos & 255) : -1;
        const int kb = pend_col >= 0 ? pend_kb : -1;
        float ch[1] = {0.0f};
        uint64_t old_mine = 0;
        if (pend_col >= 0) {
            vload<1>(ch, chan_t + (size_t)pend_col * F);
            old_mine = load_field(pend_col, my_word);
        }
        if (r + 2 < r_end) load_row(pre, r + 2);
        float xx[D][1], out[D][1];
#pragma unroll
        for (int k = 0; k < D; ++k) xx[k][0] = x[k];
        check_node<ALGO, D, 1, T>(xx, out, ms_corr_of(a));
#pragma unroll
        for (int k = 0; k < D; ++k)
            if ((k != ka && k != kb) || g.store_all) vstore<1>(Rt + (size_t)(e0 + k) * F, out[k]);

        if (pend_col >= 0) {
            float rr[2][1], q[2][1];
            rr[0][0] = pend_r;
            float t = out[0][0];
#pragma unroll
            for (int k = 1; k < D; ++k) t = (k == kb) ? out[k][0] : t;
            rr[1][0] = t;
            bool bit;
            if (ALGO == kAlgoSP) {
                float f0[1], f1[1];
                var_sp<2, 1>(ch, rr, q, f0, f1);
                const bool oldb = (old_mine >> my_bit) & 1ull;
                bit = (f0[0] > f1[0]) ? false : ((f0[0] < f1[0]) ? true : oldb);
            } else {
                float p = ch[0];
                p += rr[0][0];
                p += rr[1][0];
                q[0][0] = p - rr[0][0];
                q[1][0] = p - rr[1][0];
                bit = !(p > 0.0f);
            }
            const uint64_t ballot = __ballot(bit);
            if (lane < V) {
                const uint64_t nf = compress_stride<V>(ballot >> lane);
                const uint64_t of = load_field(pend_col, lane);
                const uint64_t res = (of & frozen_field) | (nf & ~frozen_field);
                uint8_t *p = hard_b + ((size_t)pend_col * V + lane) * 8;
                if (V == 1) *reinterpret_cast<uint64_t *>(p) = res;
                else if (V == 2) *reinterpret_cast<uint32_t *>(p) = (uint32_t)res;
                else *reinterpret_cast<uint16_t *>(p) = (uint16_t)res;
            }
            if (g.write_q) {
                vstore<1>(Qwt + (size_t)edge_slot(a.qpos, pend_edge) * F, q[0]);
                vstore<1>(Qwt + (size_t)edge_slot(a.qpos, e0 + kb) * F, q[1]);
            }
        }
        pend_col = next_col;
        if (next_col >= 0) {
            pend_edge = e0 + ka;
            pend_kb = (pos >> 8) & 255;
            float t = out[0][0];
#pragma unroll
            for (int k = 1; k < D; ++k) t = (k == ka) ? out[k][0] : t;
            pend_r = t;
        }
    };
    for (int r = r_begin; r < r_end; r += 3) {
        step(r, b0, b2);
        if (r + 1 < r_end) step(r + 1, b1, b0);
        if (r + 2 < r_end) step(r + 2, b2, b1);
    }
}

}  // namespace ldpc
