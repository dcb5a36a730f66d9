/*
 * engine_flood.hip -- the streaming flooding engine: the per-degree work lists built from the edge list (build_classes),
 * the launch plan (plan_launches), the creation-time choice of the column-fused check kernel's form (calibrate_link) and
 * of the message arrays' placement (placement_search), and the rounds, driven the way the reference's host loops do
 * (decodeOnceSP MyLdpc.cpp:977-1059, decodeOnceMS :786-848) -- minus the per-kernel queue.finish() and the blocking
 * flags read-back every iteration (:1024-1034): frames freeze on the device (state_kernel) and the host only polls an
 * "anything still running" word every poll_interval rounds.
 *
 * Round i (1-based), for every tile of F = 64*V frames:
 *   check_i    : R_i = check(Q_{i-1})
 *   var_i      : bits_i = hard(R_i) (frozen frames keep theirs); Q_i = var(R_i)
 *   syndrome_i : fail_i = any parity check of bits_i odd          } early_term only
 *   crc_i      : (cfg.crc_kind) fail_i &= ~(CRC of bits_i passes)  } (crc_term_kernels.hpp)
 *   soft_i     : (soft calls) the frames that settle in round i leave y + sum R_i in the caller's buffer (soft_kernels.hpp)
 *   state_i    : frames with clean bits_i freeze, iters = i        } (and after the last round)
 *   tail_i     : (asynchronous callers) hand the last running frames over to the overflow tiles
 * then pack.
 *
 * The message kernels themselves are instantiated per arithmetic in flood_sp / flood_ms* / flood_msc*
 * (flood_tables.hpp); the bookkeeping kernels of a round (flood_round.hpp) and of the hand-over (flood_handover.hpp)
 * are instantiated here.  Declared in
 * engines.hpp like the other engines; unlike them it works on the handle (decoder.hpp), because it needs the stream,
 * the timing spans and the tail-compaction child.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <vector>

#include "flood_round.hpp"
#include "flood_handover.hpp"
#include "crc_term_kernels.hpp"
#include "soft_kernels.hpp"
#include "decoder.hpp"
#include "graph.hpp"

using ldpc::set_error;

namespace {

using ldpc::DevBuf;
using ldpc::RowClass;
using ldpc::ColClass;
using ldpc::ClassGroup;
using ldpc::kIdleFat;
using ldpc::dispatch_v;
using ldpc::span_begin;
using ldpc::span_end;
using ldpc::kVarBuckets;
using ldpc::kCheckBuckets;
using ldpc::kVarBucketLo;
using ldpc::kVarBucketHi;
using ldpc::kCheckBucketLo;
using ldpc::kCheckBucketHi;

/* summary[0] = max over frames of iters (the reference's `Time=`), summary[1] =
 * number of frames whose syndrome ended clean. */
template <int V>
__global__ void summary_kernel(const int32_t *iters, const uint64_t *done, const uint64_t *fail,
                               int64_t frames, int32_t freeze, int32_t *summary)
{
    constexpr int F = 64 * V;
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= frames) return;
    const int64_t tile = f / F;
    const int fi = (int)(f % F);
    const int l = fi / V, v = fi % V;
    atomicMax(&summary[0], iters[f]);
    const uint64_t ok = freeze ? done[tile * V + v] : ~fail[tile * V + v];
    if ((ok >> l) & 1ull) atomicAdd(&summary[1], 1);
}

/* grid of a flooding launch: (tiles, blocks) -- flood_common.hpp: grid_pos() -- when the blocks fit gridDim.y */
static inline dim3 flood_grid(const ldpc_decoder *d, unsigned blocks, unsigned tiles, int32_t *tiles_first, bool linked = false)
{
    /* tune_tiles_first: 0 automatic = the column-fused check launch only (-8 % there; the variable-node
     * launches gather anyway and lose 4 %, the plain check launches of the rate-9/10 code 1.7 %), 1 all,
     * 2 none */
    const bool want = d->tune.tiles_first == 1 || (d->tune.tiles_first == 0 && linked);
    *tiles_first = (blocks <= 65535u && want) ? 1 : 0;
    return *tiles_first ? dim3(tiles, blocks) : dim3(blocks, tiles);
}

/* The arguments every check launch of round `it` shares: the message arrays, the frozen frames, the min-sum
 * correction, the Q slots, the tail and -- where round 1 reads q = y (first_round_from_chan; never the column-fused
 * launch) -- the channel array by column.  e0 / n_rows / degree: the class of a launch of its own (a bucket launch
 * takes them from its table). */
static ldpc::CheckArgs check_args(const ldpc_decoder *d, const ldpc::TailRef &tr, int rows_per_wave, bool from_chan,
                                  const int32_t *e0 = nullptr, int n_rows = 0, int degree = 0)
{
    ldpc::CheckArgs a{d->flood.Q.p, d->flood.R.p, e0, d->done.p, d->E, n_rows, rows_per_wave, degree, d->ms_scale, tr};
    a.ms_offset = d->ms_offset;
    a.qpos = d->flood.qpos.p;
    /* both index tables in every launch, whichever one the round reads through: check_rows chooses by a per-lane
     * pointer, and where the compiler lowers that choice to exec masks without a skip branch -- the degree-1 body of the
     * corrected arithmetics, short enough -- the wave-uniform load of the side not taken is a scalar load, which no
     * exec mask holds back.  From a null edge_col it faulted in every round that read Q (CheckArgs::edge_col). */
    a.edge_col = d->edge_col.p;
    a.N = d->N;
    if (from_chan) a.first_chan = d->flood.chan.p;
    return a;
}

template <int V> int run_flooding(ldpc_decoder *d, const ldpc::LlrIn &llr, int64_t frames,
                                  uint8_t *out_dev, int64_t out_bytes, int32_t *iters_dev,
                                  hipStream_t s, int start_round = 1);

/* The check phase of round `it` (R_i = check(Q_{i-1})) over `tiles` tiles: the column-fused launch, the bucket
 * launches and the classes launched alone.  Also what the placement search times. */
template <int V> int enqueue_check_phase(ldpc_decoder *d, hipStream_t s, int tiles, int64_t frames, int it, int max_iter,
                                         bool fat, const ldpc::TailRef &tr)
{
    using namespace ldpc;
    const int64_t msz = d->flood.msg_size;
    const bool from_chan = it == 1 && d->flood.first_round_from_chan;      /* CheckArgs::first_chan */
    for (auto &rc : d->flood.row_classes) {
        if (!rc.linked) continue;
        /* algorithmic bytes: the fused columns' messages and channel values count as in the
         * two-kernel formulation (16 E + 4 N per frame-iteration in total).
         * moved: every Q of the class and the fused columns' channel values in; R of the unfused
         * edges and the fused columns' new Q out.  Rows riding along: Q in, R out. */
        LDPC_HIP_TRY(span_begin(d, s, 4, rc.degree,
                           (2 * msz * rc.degree * rc.count + msz * 5 * rc.linked + 2 * msz * d->flood.extra_edges) * frames,
                           msz * ((int64_t)rc.degree * rc.count + rc.linked +
                                  ((int64_t)rc.degree * rc.count - 2 * rc.linked) +
                                  (it < max_iter ? 2 * rc.linked : 0) + 2 * d->flood.extra_edges) * frames));
        CheckArgs a = check_args(d, tr, d->flood.link_rpw, false, rc.e0.p, rc.count, rc.degree);
        /* soft output reads the fused columns' R like a tap does: stored in every round a frame can settle in */
        const bool soft_reads = d->soft.dst && (d->cfg.early_term || it == max_iter);
        LinkArgs lk{rc.link_col.p, rc.link_pos.p, d->flood.chan.p, d->flood.Q.p, d->hard.p, d->N,
                    (it < max_iter) ? 1 : 0, (d->tm.tap_iter || soft_reads) ? 1 : 0, d->flood.extra_e0.p, d->flood.extra_deg.p, d->flood.n_extra, 0,
                    rc.n_big, rc.small_rows};
        const int variant = (d->flood.link_form == 2 && !d->flood.fns.link_half[rc.degree]) ? 1 : d->flood.link_form;
        const int waves = link_chunk_count(d->flood.link_rpw, rc.n_big, rc.small_rows, rc.count) * (variant == 1 ? V : variant == 2 ? V / 2 : 1);
        lk.link_blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
        /* tiles vary fastest: the short chunks of all tiles are the launch's last blocks */
        const dim3 grid = flood_grid(d, lk.link_blocks + (d->flood.n_extra + kWavesPerBlock - 1) / kWavesPerBlock, tiles, &a.tiles_first, true);
        (variant == 2 ? d->flood.fns.link_half : variant == 1 ? (d->flood.link_deep ? d->flood.fns.link_deep : d->flood.fns.link_narrow) : d->flood.fns.link)
            [rc.degree]<<<grid, kBlock, 0, s>>>(a, lk);
        LDPC_HIP_TRY(span_end(d, s));
    }
    for (auto &g : d->flood.check_groups) {
        int64_t edges = 0;
        for (int i : g.members) edges += (int64_t)d->flood.row_classes[i].degree * d->flood.row_classes[i].count;
        LDPC_HIP_TRY(span_begin(d, s, 5, g.hi, 2 * msz * edges * frames, -1, g.lo));
        CheckArgs a = check_args(d, tr, (d->tune.rows_per_wave ? d->tune.rows_per_wave : 2) * (fat ? kIdleFat : 1), from_chan);
        const dim3 grid = flood_grid(d, fat ? g.blocks_fat : g.blocks, tiles, &a.tiles_first);
        d->flood.fns.check_group[g.bucket]<<<grid, kBlock, 0, s>>>(a, fat ? g.table_fat.p : g.table.p, (int)g.members.size());
        LDPC_HIP_TRY(span_end(d, s));
    }
    for (int ci : d->flood.check_solo) {
        RowClass &rc = d->flood.row_classes[ci];
        LDPC_HIP_TRY(span_begin(d, s, 0, rc.degree, 2 * msz * rc.degree * rc.count * frames));
        const int slotk = rc.degree <= d->flood.fns.max_check_unrolled ? rc.degree : 0;
        const bool narrow = slotk && (!d->flood.check_wide || rc.degree > kMaxUnrolledDegree);
        const int rpw = (d->tune.rows_per_wave ? d->tune.rows_per_wave : (narrow ? 2 : 1)) * (fat ? kIdleFat : 1);
        CheckArgs a = check_args(d, tr, rpw, from_chan, rc.e0.p, rc.count, rc.degree);
        const int waves = ((rc.count + rpw - 1) / rpw) * (narrow ? V : 1);
        const dim3 grid = flood_grid(d, (waves + kWavesPerBlock - 1) / kWavesPerBlock, tiles, &a.tiles_first);
        (narrow ? d->flood.fns.check : d->flood.fns.check_wide)[slotk]<<<grid, kBlock, 0, s>>>(a);
        LDPC_HIP_TRY(span_end(d, s));
    }
    return LDPC_OK;
}

/* The variable-node phase of round `it`: bits_i = hard(R_i); Q_i = var(R_i) unless this is the last round. */
template <int V> int enqueue_var_phase(ldpc_decoder *d, hipStream_t s, int tiles, int64_t frames, int it, int max_iter,
                                       bool fat, const ldpc::TailRef &tr)
{
    using namespace ldpc;
    const int64_t msz = d->flood.msg_size;
    /* var_i: bits_i = hard(R_i); Q_i = var(R_i) unless this is the last round */
    const int wq = (it < max_iter) ? 1 : 0;
    for (auto &g : d->flood.var_groups) {
        int64_t units = 0;          /* messages read + written + channel values read, per frame */
        for (int i : g.members) units += (int64_t)((wq ? 2 : 1) * d->flood.col_classes[i].degree + 1) * d->flood.col_classes[i].count;
        LDPC_HIP_TRY(span_begin(d, s, 6, g.hi, msz * units * frames, -1, g.lo));
        VarArgs a{d->flood.R.p, d->flood.Q.p, d->flood.chan.p, d->hard.p, d->done.p, nullptr, nullptr,
                  d->E, d->N, 0, (d->tune.cols_per_wave ? d->tune.cols_per_wave : 1) * (fat ? kIdleFat : 1), wq, 0, tr};
        const dim3 grid = flood_grid(d, fat ? g.blocks_fat : g.blocks, tiles, &a.tiles_first);
        d->flood.fns.var_group[g.bucket]<<<grid, kBlock, 0, s>>>(a, fat ? g.table_fat.p : g.table.p, (int)g.members.size());
        LDPC_HIP_TRY(span_end(d, s));
    }
    for (int ci : d->flood.var_solo) {
        ColClass &cc = d->flood.col_classes[ci];
        LDPC_HIP_TRY(span_begin(d, s, 1, cc.degree, msz * ((wq ? 2 : 1) * cc.degree + 1) * cc.count * frames));
        VarArgs a{d->flood.R.p, d->flood.Q.p, d->flood.chan.p, d->hard.p, d->done.p, cc.col.p, cc.edge.p,
                  d->E, d->N, cc.count, 1, wq, cc.degree, tr};
        const int cpw = (d->tune.cols_per_wave ? d->tune.cols_per_wave : 1) * (fat ? kIdleFat : 1);
        a.cols_per_wave = cpw;
        a.q_base = cc.q_base;
        const int slotk = cc.degree <= kMaxUnrolledDegree ? cc.degree : 0;
        const int waves = (cc.count + cpw - 1) / cpw;
        const dim3 grid = flood_grid(d, (waves + kWavesPerBlock - 1) / kWavesPerBlock, tiles, &a.tiles_first);
        d->flood.fns.var[slotk]<<<grid, kBlock, 0, s>>>(a);
        LDPC_HIP_TRY(span_end(d, s));
    }
    return LDPC_OK;
}

/* soft_i of a soft call (soft_kernels.hpp), between the CRC test and state_i: the frames that settle in this round --
 * running and passed by `fail`, or every running frame where fail is nullptr (the last round launched) -- leave
 * y + sum R (or that minus y) in the caller's buffer.  Min-sum only: the entry point refuses sum-product. */
template <int V> int enqueue_soft(ldpc_decoder *d, hipStream_t s, int tiles, int64_t frames, const uint64_t *fail,
                                  const ldpc::TailRef &tr)
{
    using namespace ldpc;
    /* priced as if every frame settled here: channel value and column messages in, one float out */
    LDPC_HIP_TRY(span_begin(d, s, 7, 0, ((int64_t)d->flood.msg_size * (d->E + d->N) + 4 * (int64_t)d->N) * frames));
    SoftArgs a{d->flood.chan.p, d->flood.R.p, d->col_ptr.p, d->col_edge.p, d->done.p, fail, d->soft.dst, nullptr,
               d->soft.fmap, d->flood.tail_map.p, d->E, frames, d->N, d->soft.kind == LDPC_SOFT_EXTRINSIC ? 1 : 0, tr};
    const dim3 grid((unsigned)((d->N + kInitCols - 1) / kInitCols), (unsigned)tiles);
    dispatch_msg(d->flood.msg_kind, [&](auto t) { soft_settle_kernel<V, decltype(t)><<<grid, kBlock, 0, s>>>(a); });
    LDPC_HIP_TRY(span_end(d, s));
    return LDPC_OK;
}

/* Hand the `count` frames that are still running after round `it` over to the child decoder, let it
 * finish them (rounds it+1 ...), and bring their bits, iteration counts and converged flags back. */
template <int V> int compact_and_finish(ldpc_decoder *d, int64_t frames, int count, int it, hipStream_t s)
{
    using namespace ldpc;
    /* the smallest decoder of the chain (1024 frames in tiles of 256 -> 512 in tiles of 64 -> one tile of 64) that holds them:
     * a tile of 256 frames for a dozen stragglers would cost four times the traffic per round, eight tiles of 64 with one
     * straggler each eight times that of one tile */
    ldpc_decoder *c = d->flood.child.get();
    while (c->flood.child && count <= c->flood.child->cfg.max_batch) c = c->flood.child.get();
    const int cv = c->V, cf = 64 * cv;                      /* its frames per lane and per tile */
    const unsigned ct = (unsigned)((count + cf - 1) / cf);  /* child tiles in use */
    const unsigned cg = ct * (unsigned)cv;                  /* ... in groups of 64 slots */
    if (cg > (unsigned)kBackWords) return set_error(LDPC_ERR_STATE, "hand-over of %d frames: more than %d mask words per column", count, kBackWords);
    LDPC_HIP_TRY(hipMemsetAsync(d->active.p, 0, sizeof(int32_t), s));
    compact_list_kernel<V><<<(unsigned)((frames + kBlock - 1) / kBlock), kBlock, 0, s>>>(d->done.p, frames, d->flood.cmap.p,
                                                                                         d->active.p, d->flood.child_capacity);
    const dim3 ge((unsigned)((d->E + kWavesPerBlock - 1) / kWavesPerBlock), cg);
    const dim3 gn((unsigned)((d->N + kWavesPerBlock - 1) / kWavesPerBlock), cg);
    /* many frames: one coalesced pass over the parent's rows through LDS; few: one sector per value */
    const bool rowwise = count >= 128;
    const int ptiles = (int)((frames + 64 * V - 1) / (64 * V));
    dispatch_msg(d->flood.msg_kind, [&](auto t) {
        using T = decltype(t);
        const T *pq = (const T *)d->flood.Q.p, *pc = (const T *)d->flood.chan.p;
        T *cq = (T *)c->flood.Q.p, *cc = (T *)c->flood.chan.p;
        if (rowwise) {
            constexpr int rpb = gather_rows_per_block<T>();
            compact_gather_rows_kernel<V, T><<<(unsigned)((d->E + rpb - 1) / rpb), kBlock, 0, s>>>(pq, cq, d->flood.cmap.p, count, d->E, ptiles, cf, d->flood.qpos.p, c->flood.qpos.p);
            compact_gather_rows_kernel<V, T><<<(unsigned)((d->N + rpb - 1) / rpb), kBlock, 0, s>>>(pc, cc, d->flood.cmap.p, count, d->N, ptiles, cf);
        } else {
            compact_gather_kernel<V, T><<<ge, kBlock, 0, s>>>(pq, cq, d->flood.cmap.p, count, d->E, cf, d->flood.qpos.p, c->flood.qpos.p);
            compact_gather_kernel<V, T><<<gn, kBlock, 0, s>>>(pc, cc, d->flood.cmap.p, count, d->N, cf);
        }
    });
    /* the hard bits travel only where the next decision can depend on the previous one: the sum-product rule keeps the old
     * bit on a tie or a NaN (decodeCL.c:78-82); min-sum decides every bit anew in every round (bit = !(p > 0), :161-165) */
    LDPC_HIP_TRY(hipMemsetAsync(c->hard.p, 0, (size_t)ct * d->N * cv * sizeof(uint64_t), s));
    if (d->cfg.algo == LDPC_ALGO_SP) {
        if (ptiles * V <= kGatherParentWords && count <= 2 * kCompactCapacity)
            compact_hard_lds_kernel<V><<<(unsigned)((d->N + 63) / 64), kBlock, 0, s>>>(d->hard.p, c->hard.p, d->flood.cmap.p, count, d->N, cv, ptiles, (int)cg);
        else
            compact_hard_kernel<V><<<gn, kBlock, 0, s>>>(d->hard.p, c->hard.p, d->flood.cmap.p, count, d->N, cv);
    }
    compact_child_state_kernel<0><<<ct, 64, 0, s>>>(c->done.p, c->iters.p, count, d->cfg.max_iter, cv);
    LDPC_HIP_TRY(hipGetLastError());
    c->tm.timing = false;
    c->tm.tap_iter = 0;
    c->soft = SoftReq{};
    if (d->soft.dst) {
        /* the child runs soft_i in its own rounds and addresses the caller's frames: its slots through cmap, and through
         * this decoder's own map where it is a child itself */
        LDPC_HIP_TRY(c->flood.soft_map.ensure((size_t)c->cfg.max_batch));
        soft_map_kernel<0><<<(unsigned)((count + kBlock - 1) / kBlock), kBlock, 0, s>>>(c->flood.soft_map.p, d->flood.cmap.p, d->soft.fmap, count);
        c->soft = SoftReq{d->soft.dst, d->soft.kind, c->flood.soft_map.p};
    }
    const int rc = dispatch_v(cv, [&](auto v) { return run_flooding<decltype(v)::value>(c, ldpc::LlrIn{}, count, nullptr, 0, nullptr, s, it + 1); });
    c->soft = SoftReq{};
    if (rc) return rc;
    d->flood.handed_to = c;
    /* the bits back: every parent word collects its moved frames' bits (no atomics; the per-bit atomic scatter of
     * compact_hard_kernel took 53-80 us for a few dozen frames, this takes 10-30) */
    LDPC_HIP_TRY(hipMemsetAsync(d->flood.cmoved.p, 0, d->flood.cmoved.n * sizeof(unsigned long long), s));
    compact_inverse_kernel<V><<<(unsigned)((count + 255) / 256), 256, 0, s>>>(d->flood.cmap.p, count, d->flood.cinv.p, d->flood.cmoved.p, cv);
    compact_hard_back_kernel<V><<<dim3((unsigned)((d->N + kBlock - 1) / kBlock), (unsigned)ptiles), kBlock, 0, s>>>(
        d->hard.p, c->hard.p, d->flood.cinv.p, d->flood.cmoved.p, d->N, cv, (int)cg);
    compact_finish_kernel<V><<<(unsigned)((count + 63) / 64), 64, 0, s>>>(d->done.p, d->iters.p, c->done.p, c->iters.p, d->flood.cmap.p, count, cv);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

template <int V> int run_flooding(ldpc_decoder *d, const ldpc::LlrIn &llr, int64_t frames,
                                  uint8_t *out_dev, int64_t out_bytes, int32_t *iters_dev,
                                  hipStream_t s, int start_round)
{
    using namespace ldpc;
    const int F = 64 * V;
    const int tiles = (int)((frames + F - 1) / F);
    const int64_t msz = d->flood.msg_size;
    const int max_iter = d->cfg.max_iter;
    const int rounds = d->tm.tap_iter ? std::min(d->tm.tap_iter, max_iter) : max_iter;
    const bool freeze = d->cfg.early_term != 0;
    const size_t slot = (size_t)d->flood.TA * V;  /* words per fail slot */

    const bool resume = start_round > 1;    /* a child taking over running frames: their state is in place */
    LDPC_HIP_TRY(hipMemsetAsync(d->failw.p, 0, d->failw.n * sizeof(uint64_t), s));
    LDPC_HIP_TRY(hipMemsetAsync(d->summary.p, 0, 4 * sizeof(int32_t), s));
    d->flood.handed_to = nullptr;
    /* idle hint from the previous call (asynchronous early termination only) */
    if (!resume && d->flood.summary_pending) {
        if (hipEventQuery(d->flood.ev_summary.e) == hipSuccess) {
            d->flood.summary_pending = false;
            d->flood.idle_after = (d->flood.h_summary.p[0] > 0 && d->flood.h_summary.p[0] < max_iter) ? d->flood.h_summary.p[0] + 1 : 0;
        } else {
            (void)hipGetLastError();        /* "not ready" is not an error of this call */
        }
    }
    const int idle_after = (freeze && !resume && !d->tm.tap_iter && d->cfg.poll_interval == 0) ? d->flood.idle_after : 0;
    /* device-side tail: only when the call has clearly more tiles than the overflow area */
    const bool use_tail = d->flood.tail_enabled && freeze && !resume && !d->tm.tap_iter && tiles >= 4 * d->flood.TO;
    const TailRef tr{use_tail ? d->flood.tail_state.p : nullptr, d->T, d->flood.TO};
    TailArgs ta{};
    if (use_tail) {
        LDPC_HIP_TRY(hipMemsetAsync(d->flood.tail_state.p, 0, 4 * sizeof(int32_t), s));
        LDPC_HIP_TRY(hipMemsetAsync(d->flood.running.p, 0, d->flood.running.n * sizeof(int32_t), s));
        ta = TailArgs{d->flood.tail_state.p, d->flood.tail_map.p, d->flood.running.p, d->done.p, d->iters.p, d->flood.Q.p, d->flood.chan.p, d->hard.p,
                      d->E, frames, d->N, tiles, d->T, d->flood.TO * F, std::min(d->flood.compact_threshold, d->flood.TO * F), 0, max_iter};
    }

    /* min-sum / box-plus whose check phase is made of the unrolled bucket / single-class kernels only: round 1 reads q = y from the
     * channel array and the input transpose writes no Q (CheckArgs::first_chan); not with a debug tap */
    bool q_less = (d->cfg.algo == LDPC_ALGO_MS || d->cfg.algo == LDPC_ALGO_BP) && !resume && !d->tm.tap_iter && max_iter > 1 && d->flood.n_extra == 0;
    for (auto &rc : d->flood.row_classes) if (rc.linked) q_less = false;
    for (int ci : d->flood.check_solo) if (d->flood.row_classes[ci].degree > d->flood.fns.max_check_unrolled) q_less = false;
    d->flood.first_round_from_chan = q_less;
    if (!resume) {
        LDPC_HIP_TRY(span_begin(d, s, 3));
        InitArgs a{llr.p, d->flood.chan.p, q_less ? nullptr : d->flood.Q.p, d->hard.p, d->col_ptr.p, d->flood.col_qedge.p,
                   d->E, frames, d->N, d->cfg.llr_scale, llr.unit};
        dim3 grid((d->N + kInitCols - 1) / kInitCols, tiles);
        d->flood.fns.init_in[llr.type]<<<grid, kBlock, 0, s>>>(a);
        StateArgs st{d->done.p, nullptr, d->iters.p, nullptr, frames, 0, max_iter, freeze ? 1 : 0};
        /* overflow tiles (and unused tiles in between) are born finished: frames beyond `frames` */
        state_kernel<V><<<use_tail ? d->flood.TA : tiles, 64, 0, s>>>(st);
        LDPC_HIP_TRY(span_end(d, s));
    }

    int launched = start_round - 1;
    /* host polling: every poll_interval rounds -- and every round once a poll has seen a tenth of the frames
     * finished: from there on the running count falls fast (rate 9/10 at 4096 frames: 4096, 3501, 681, 41
     * frames take part in rounds 4..7), and the round after which a quarter is left is the one to hand over at */
    bool poll_dense = false;
    for (int it = start_round; it <= rounds; ++it) {
        const bool fat = idle_after > 0 && it > idle_after;      /* probably idle: fewer, fatter workgroups */
        /* check_i: R_i = check(Q_{i-1}) */
        {
            const int rcp = enqueue_check_phase<V>(d, s, tiles, frames, it, max_iter, fat, tr);
            if (rcp) return rcp;
        }
        {
            const int rcv = enqueue_var_phase<V>(d, s, tiles, frames, it, max_iter, fat, tr);
            if (rcv) return rcv;
        }
        launched = it;
        /* syndrome of bits_i, then freeze the frames that are clean (iters = i) */
        if (freeze || it == rounds) {
            LDPC_HIP_TRY(span_begin(d, s, 3));
            uint64_t *fw = d->failw.p + (size_t)it * slot;
            const int rbk = (d->M + kBlock - 1) / kBlock;
            SyndromeArgs sa{d->row_ptr.p, d->edge_col.p, d->hard.p, fw, d->done.p, d->M, d->N,
                            d->flood.syn_xcd ? tiles : 0, rbk, tr};
            dim3 sgrid = d->flood.syn_xcd ? dim3(8 * rbk * ((tiles + 7) / 8)) : dim3(rbk, tiles);
            syndrome_kernel<V><<<sgrid, kBlock, 0, s>>>(sa);
            if (d->cfg.crc_kind) {
                /* frames whose information bits pass the CRC count as clean from here on; those the syndrome had not
                 * passed go into summary[3] */
                CrcTermArgs ca{d->hard.p, fw, d->done.p, d->crc_w.p, d->summary.p + 3, d->N, d->cfg.crc_bits, tr};
                crc_term_kernel<V><<<dim3((unsigned)tiles, V), 64 * crc_term_waves(d->cfg.crc_bits), 0, s>>>(ca);
            }
            if (d->soft.dst) {
                /* soft_i: `done` still holds the frames frozen before this round and fw this round's verdict, so
                 * ~done & ~fw settle here; in the last round launched every running frame does.  Before state_i and
                 * tail_i: a hand-over marks every batch tile finished, which is not "settled". */
                LDPC_HIP_TRY(span_end(d, s));
                const int rcs = enqueue_soft<V>(d, s, tiles, frames, (freeze && it < rounds) ? fw : nullptr, tr);
                if (rcs) return rcs;
                LDPC_HIP_TRY(span_begin(d, s, 3));
            }
            StateArgs st{d->done.p, fw, d->iters.p, nullptr, frames, it, max_iter, 1, tr, use_tail ? d->flood.running.p : nullptr,
                         d->summary.p + 2};
            const bool poll = freeze && it < rounds && d->cfg.poll_interval > 0 && !d->host.suppress_poll &&
                              ((it % d->cfg.poll_interval) == 0 || poll_dense);
            if (poll) {
                LDPC_HIP_TRY(hipMemsetAsync(d->active.p, 0, sizeof(int32_t), s));
                st.active = d->active.p;
            }
            state_kernel<V><<<tiles, 64, 0, s>>>(st);
            if (use_tail && it < rounds) {
                /* hand the last running frames over to the overflow tiles if their number has fallen
                 * below the threshold after this round (decided by the kernel; usually it just returns) */
                ta.iter = it;
                const unsigned tg = (unsigned)std::min<int64_t>(1024, d->E + 2 * (int64_t)d->N);
                dispatch_msg(d->flood.msg_kind, [&](auto t) { tail_gather_kernel<V, decltype(t)><<<tg, kBlock, 0, s>>>(ta); });
            }
            LDPC_HIP_TRY(span_end(d, s));
            if (poll) {
                LDPC_HIP_TRY(hipMemcpyAsync(d->flood.h_active.p, d->active.p, sizeof(int32_t),
                                       hipMemcpyDeviceToHost, s));
                LDPC_HIP_TRY(hipStreamSynchronize(s));
                const int running = *d->flood.h_active.p;
                if (running == 0) break;        /* every frame frozen: MyLdpc.cpp:1035-1036 */
                /* ... where a round is long enough for a host round trip (about 25 us) not to matter: from 1.5 GB of
                 * message traffic per round (about 0.3 ms) */
                if ((int64_t)running * 10 <= frames * 9 && d->flood.child && tiles > 1 &&
                    (double)d->E * (double)frames * 4.0 * (double)msz > 1.5e9) poll_dense = true;
                if (d->flood.child && running <= d->flood.compact_threshold && (int64_t)running * 4 <= frames && tiles > 1 && !d->tm.tap_iter) {
                    const int rc = compact_and_finish<V>(d, frames, running, it, s);
                    if (rc) return rc;
                    launched = d->flood.handed_to->last_iterations;
                    break;
                }
            }
        }
    }
    d->last_iterations = launched;
    d->last_tiles = tiles;
    if (resume) return LDPC_OK;             /* the parent packs */

    LDPC_HIP_TRY(span_begin(d, s, 3));
    if (use_tail) tail_scatter_kernel<V><<<2048, kBlock, 0, s>>>(ta);
    {
        PackArgs pa{d->hard.p, out_dev, d->iters.p, iters_dev, frames, out_bytes, d->N, d->cfg.K,
                    d->cfg.pack_mode};
        /* the pack launch also carries the iteration counts out: it runs for either buffer (out_dev NULL: out_bytes is 0) */
        const bool pack = (out_dev || iters_dev) && frames;
        if (d->cfg.pack_mode == LDPC_PACK_BYTES) {
            if (pack) pack_kernel<V><<<pack_grid<V>(d->cfg.K, tiles), kBlock, 0, s>>>(pa);
        } else {
            const int64_t n = std::max<int64_t>(out_bytes, frames);
            dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
            if (pack) pack_kernel<V><<<grid, kBlock, 0, s>>>(pa);
        }
        /* after the final state_kernel `done` marks exactly the converged frames */
        summary_kernel<V><<<(unsigned)((frames + 255) / 256), 256, 0, s>>>(
            d->iters.p, d->done.p, d->failw.p, frames, 1, d->summary.p);
        if (!d->flood.is_child && d->cfg.poll_interval == 0 && freeze && !d->flood.summary_pending) {
            /* the next call's idle hint */
            LDPC_HIP_TRY(hipMemcpyAsync(d->flood.h_summary.p, d->summary.p, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            LDPC_HIP_TRY(hipEventRecord(d->flood.ev_summary.e, s));
            d->flood.summary_pending = true;
        }
    }
    LDPC_HIP_TRY(span_end(d, s));
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int build_classes(ldpc_decoder *d, const ldpc_graph *g)
{
    std::map<int, std::vector<int32_t>> rows_by_deg, cols_by_deg, rowids_by_deg;
    for (int32_t m = 0; m < g->M; ++m) {
        const int deg = g->row_ptr[m + 1] - g->row_ptr[m];
        if (deg > 0) { rows_by_deg[deg].push_back(g->row_ptr[m]); rowids_by_deg[deg].push_back(m); }
    }
    /* column-local fusion: degree-2 columns whose checks are consecutive list rows of one wave */
    std::vector<char> fused_col((size_t)g->N, 0);
    d->flood.row_classes.resize(rows_by_deg.size());
    size_t i = 0;
    for (auto &kv : rows_by_deg) {
        RowClass &rc = d->flood.row_classes[i++];
        rc.degree = kv.first;
        rc.count = (int)kv.second.size();
        rc.h_e0 = kv.second;
        LDPC_HIP_TRY(rc.e0.upload(kv.second));
        const std::vector<int32_t> &ids = rowids_by_deg[kv.first];
        const int rpw = d->flood.link_rpw;
        if (rpw >= 2 && rc.degree >= 2 && rc.degree <= ldpc::kMaxUnrolledDegree) {
            /* Guided chunks: what the chip holds at once (16 waves per CU) is the launch's last
             * generation of waves; that many chunks per tile, at the end of the row list, are cut to
             * a quarter of the rows (>= 2), so that the launch drains over a short chunk's time.  With
             * fewer than 4 tiles everything would be "last generation": equal chunks then. */
            rc.n_big = (rc.count + rpw - 1) / rpw;
            rc.small_rows = rpw;
            const int small = std::max(2, rpw / 4);
            const bool forced = ldpc::tune_forced_on(d->tune.link_guided);         /* tests: also on small launches */
            if ((d->T >= 4 || forced) && small < rpw && !ldpc::tune_forced_off(d->tune.link_guided)) {
                const int64_t last_generation = (int64_t)d->flood.cus * 16 / d->T;       /* chunks per tile */
                int64_t big = (int64_t)rc.n_big - last_generation;
                if (big <= 0 && forced) big = rc.n_big - std::max(1, rc.n_big / 3);
                if (big > 0) { rc.n_big = (int)big; rc.small_rows = small; }
            }
            std::vector<char> chunk_end((size_t)rc.count, 0);
            for (int c = 0, nc = ldpc::link_chunk_count(rpw, rc.n_big, rc.small_rows, rc.count); c < nc; ++c) {
                int rb, re;
                ldpc::link_chunk_rows(c, rpw, rc.n_big, rc.small_rows, rc.count, &rb, &re);
                if (re > rb) chunk_end[(size_t)re - 1] = 1;
            }
            std::vector<int32_t> lcol((size_t)rc.count, -1), lpos((size_t)rc.count, 0);
            for (int idx = 0; idx + 1 < rc.count; ++idx) {
                if (chunk_end[idx]) continue;                  /* next row belongs to another wave */
                const int32_t m = ids[idx], m2 = ids[idx + 1];
                for (int32_t p = g->row_ptr[m]; p < g->row_ptr[m + 1]; ++p) {
                    const int32_t c = g->cols[p];
                    if (g->col_ptr[c + 1] - g->col_ptr[c] != 2 || fused_col[c]) continue;
                    const int32_t ea = g->col_edge[g->col_ptr[c]], eb = g->col_edge[g->col_ptr[c] + 1];
                    if (ea != p || g->rows[eb] != m2) continue;   /* edges ascending: row m first */
                    lcol[idx] = c;
                    lpos[idx] = (p - g->row_ptr[m]) | ((eb - g->row_ptr[m2]) << 8);
                    fused_col[c] = 1;
                    ++rc.linked;
                    break;
                }
            }
            if (rc.linked * 4 >= rc.count) {                    /* worth a specialised kernel */
                LDPC_HIP_TRY(rc.link_col.upload(lcol));
                LDPC_HIP_TRY(rc.link_pos.upload(lpos));
            } else {
                for (int idx = 0; idx < rc.count; ++idx)
                    if (lcol[idx] >= 0) fused_col[lcol[idx]] = 0;
                rc.linked = 0;
            }
        }
    }
    for (int32_t n = 0; n < g->N; ++n) {
        const int deg = g->col_ptr[n + 1] - g->col_ptr[n];
        if (!fused_col[n]) cols_by_deg[deg].push_back(n);   /* degree 0: still needs its hard bit */
    }
    d->flood.col_classes.resize(cols_by_deg.size());
    i = 0;
    for (auto &kv : cols_by_deg) {
        ColClass &cc = d->flood.col_classes[i++];
        cc.degree = kv.first;
        cc.count = (int)kv.second.size();
        std::vector<int32_t> edges;
        edges.reserve((size_t)cc.count * std::max(cc.degree, 1));
        for (int32_t n : kv.second)
            for (int32_t p = g->col_ptr[n]; p < g->col_ptr[n + 1]; ++p) edges.push_back(g->col_edge[p]);
        if (edges.empty()) edges.push_back(0);
        LDPC_HIP_TRY(cc.col.upload(kv.second));
        LDPC_HIP_TRY(cc.edge.upload(edges));
    }
    {
        /* Q in the order its writers produce it (CheckArgs::qpos): the column classes one after the other, a class of degree D
         * as D streams of its columns' k-th messages -- the variable-node waves at work write D moving fronts --, then the
         * fused columns' edges, which the column-fused check kernel writes row by row, in row order */
        d->flood.h_qpos.assign((size_t)g->E, -1);
        int64_t slot = 0;
        if (d->tune.q_order >= 0)
            for (ColClass &cc : d->flood.col_classes) {
                cc.q_base = slot;
                const std::vector<int32_t> &members = cols_by_deg[cc.degree];
                for (size_t ci = 0; ci < members.size(); ++ci)
                    for (int k = 0; k < cc.degree; ++k)
                        d->flood.h_qpos[(size_t)g->col_edge[(size_t)g->col_ptr[members[ci]] + k]] = (int32_t)(slot + (int64_t)k * cc.count + (int64_t)ci);
                slot += (int64_t)cc.degree * cc.count;
            }
        /* (tune_q_order = -1: every edge in its own slot, as in R) */
        for (int64_t e = 0; e < g->E; ++e)
            if (d->flood.h_qpos[(size_t)e] < 0) d->flood.h_qpos[(size_t)e] = d->tune.q_order >= 0 ? (int32_t)slot++ : (int32_t)e;
        std::vector<int32_t> cq((size_t)g->E);
        for (int64_t p = 0; p < g->E; ++p) cq[(size_t)p] = d->flood.h_qpos[(size_t)g->col_edge[(size_t)p]];
        LDPC_HIP_TRY(d->flood.qpos.upload(d->flood.h_qpos));
        LDPC_HIP_TRY(d->flood.col_qedge.upload(cq));
    }
    return LDPC_OK;
}

/* Which classes share a launch (degree buckets), which go alone, and whether the few rows outside a
 * linked class ride along with its launch.  LDPC_TUNE_OFF(LDPC_TUNE_MERGE): one launch per class. */
int plan_launches(ldpc_decoder *d)
{
    using ldpc::GroupClass;
    const int V = d->V;
    const bool merge = ldpc::tune_pick(d->tune.merge, true) && !d->flood.check_wide;
    d->flood.check_groups.clear(); d->flood.var_groups.clear(); d->flood.check_solo.clear(); d->flood.var_solo.clear();
    d->flood.n_extra = 0; d->flood.extra_edges = 0;
    int linked_classes = 0;
    int64_t unlinked_rows = 0;
    for (auto &rc : d->flood.row_classes) { if (rc.linked) ++linked_classes; else unlinked_rows += rc.count; }
    const bool as_extra = merge && linked_classes == 1 && unlinked_rows > 0 && unlinked_rows <= 64;
    std::vector<int> cb[kCheckBuckets], vb[kVarBuckets];
    std::vector<int32_t> xe0, xdeg;
    for (int i = 0; i < (int)d->flood.row_classes.size(); ++i) {
        RowClass &rc = d->flood.row_classes[i];
        if (rc.linked) continue;
        if (as_extra) {
            for (int32_t e : rc.h_e0) { xe0.push_back(e); xdeg.push_back(rc.degree); d->flood.extra_edges += rc.degree; }
            continue;
        }
        int b = -1;
        for (int k = 0; k < kCheckBuckets; ++k)
            if (rc.degree >= kCheckBucketLo[k] && rc.degree <= kCheckBucketHi[k] && rc.degree <= d->flood.fns.max_check_unrolled &&
                d->flood.fns.check_group[k]) b = k;
        if (merge && b >= 0) cb[b].push_back(i); else d->flood.check_solo.push_back(i);
    }
    if (as_extra) {
        d->flood.n_extra = (int)xe0.size();
        LDPC_HIP_TRY(d->flood.extra_e0.upload(xe0));
        LDPC_HIP_TRY(d->flood.extra_deg.upload(xdeg));
    }
    for (int i = 0; i < (int)d->flood.col_classes.size(); ++i) {
        const ColClass &cc = d->flood.col_classes[i];
        int b = -1;
        for (int k = 0; k < kVarBuckets; ++k)
            if (cc.degree >= kVarBucketLo[k] && cc.degree <= kVarBucketHi[k] && d->flood.fns.var_group[k]) b = k;
        if (merge && b >= 0) vb[b].push_back(i); else d->flood.var_solo.push_back(i);
    }
    const int rpw = d->tune.rows_per_wave ? d->tune.rows_per_wave : 2, cpw = d->tune.cols_per_wave ? d->tune.cols_per_wave : 1;
    auto make = [&](std::vector<ClassGroup> &groups, std::vector<int> &solo, const std::vector<int> &members, int bucket,
                    int lo, int hi, bool rows) -> hipError_t {
        if (members.size() < 2) { for (int i : members) solo.push_back(i); return hipSuccess; }
        groups.emplace_back();
        ClassGroup &g = groups.back();
        g.bucket = bucket; g.lo = lo; g.hi = hi; g.members = members;
        std::vector<GroupClass> tab, tabf;
        constexpr int fatk = kIdleFat;
        for (int i : members) {
            GroupClass gc{};
            if (rows) {
                const RowClass &rc = d->flood.row_classes[i];
                gc.degree = rc.degree; gc.count = rc.count; gc.ids = rc.e0.p; gc.edges = nullptr; gc.q_base = -1;
            } else {
                const ColClass &cc = d->flood.col_classes[i];
                gc.degree = cc.degree; gc.count = cc.count; gc.ids = cc.col.p; gc.edges = cc.edge.p; gc.q_base = cc.q_base;
            }
            auto blocks_of = [&](int per_wave) {
                const int waves = ((gc.count + per_wave - 1) / per_wave) * (rows ? V / d->flood.fns.check_group_width : 1);
                return (waves + ldpc::kWavesPerBlock - 1) / ldpc::kWavesPerBlock;
            };
            gc.block_begin = g.blocks;
            tab.push_back(gc);
            g.blocks += blocks_of(rows ? rpw : cpw);
            gc.block_begin = g.blocks_fat;
            tabf.push_back(gc);
            g.blocks_fat += blocks_of((rows ? rpw : cpw) * fatk);
        }
        const hipError_t e = g.table.upload(tab);
        return e != hipSuccess ? e : g.table_fat.upload(tabf);
    };
    for (int k = 0; k < kCheckBuckets; ++k) LDPC_HIP_TRY(make(d->flood.check_groups, d->flood.check_solo, cb[k], k, kCheckBucketLo[k], kCheckBucketHi[k], true));
    for (int k = 0; k < kVarBuckets; ++k) LDPC_HIP_TRY(make(d->flood.var_groups, d->flood.var_solo, vb[k], k, kVarBucketLo[k], kVarBucketHi[k], false));
    return LDPC_OK;
}

/* HBM message arrays, per-degree work lists and kernel tables of a streaming flooding decoder. */
int setup_flooding(ldpc_decoder *d, const ldpc_graph *g, size_t TF)
{
    const ldpc_decoder_config *cfg = &d->cfg;
    const bool i8 = cfg->msg_dtype == LDPC_MSG_I8;
    d->flood.msg_kind = cfg->msg_dtype;
    d->flood.msg_bits = i8 ? (cfg->msg_bits ? cfg->msg_bits : 8) : 0;
    d->flood.msg_size = (i8 || cfg->msg_dtype == LDPC_MSG_F8) ? 1 : cfg->msg_dtype == LDPC_MSG_F16 ? 2 : 4;
    LDPC_HIP_TRY(d->flood.chan.alloc(TF * d->N * d->flood.msg_size));
    LDPC_HIP_TRY(d->flood.Q.alloc(TF * (size_t)d->E * d->flood.msg_size));
    LDPC_HIP_TRY(d->flood.R.alloc(TF * (size_t)d->E * d->flood.msg_size));
    int rc = build_classes(d, g);
    if (rc) return rc;
    /* the kernels live in flood_sp.hip / flood_ms*.hip / flood_msc*.hip / flood_bp*.hip (flood_tables.hpp) */
    ldpc::FloodFns *fns = &d->flood.fns;
    if (cfg->algo == LDPC_ALGO_SP) ldpc::fill_flood_sp(d->V, fns);
    else if (i8) {
        /* fixed point: the width is the kernels' compile-time L (ldpc_decoder_create has refused every other algorithm and width) */
        const int q = d->flood.msg_bits;
        if (d->ms_corr) (q == 4 ? ldpc::fill_flood_msci4 : q == 5 ? ldpc::fill_flood_msci5 : q == 6 ? ldpc::fill_flood_msci6 : ldpc::fill_flood_msci8)(d->V, fns);
        else (q == 4 ? ldpc::fill_flood_msi4 : q == 5 ? ldpc::fill_flood_msi5 : q == 6 ? ldpc::fill_flood_msi6 : ldpc::fill_flood_msi8)(d->V, fns);
    }
    else if (cfg->algo == LDPC_ALGO_BP && cfg->msg_dtype == LDPC_MSG_F16) ldpc::fill_flood_bp16(d->V, fns);
    else if (cfg->algo == LDPC_ALGO_BP) ldpc::fill_flood_bp(d->V, fns);
    else if (d->ms_corr && cfg->msg_dtype == LDPC_MSG_F8) ldpc::fill_flood_msc8(d->V, fns);
    else if (cfg->msg_dtype == LDPC_MSG_F8) ldpc::fill_flood_ms8(d->V, fns);
    else if (d->ms_corr && cfg->msg_dtype == LDPC_MSG_F16) ldpc::fill_flood_msc16(d->V, fns);
    else if (d->ms_corr) ldpc::fill_flood_msc(d->V, fns);
    else if (cfg->msg_dtype == LDPC_MSG_F16) ldpc::fill_flood_ms16(d->V, fns);
    else ldpc::fill_flood_ms(d->V, fns);
    return plan_launches(d);
}

/* The column-fused check kernel exists in wide waves (V values per lane, 128 VGPRs), in narrow waves (1 value per
 * lane, 46 VGPRs) and, for tiles of 256 frames, with 2 values per lane (68 VGPRs).  Which one is fastest was
 * different from box to box in rounds 1 and 2 (narrow ahead by 2 % on round 1's boxes, wide 6-17 % ahead on round
 * 2's: profiles/r02_ab_link_wide.txt) -- part of which was the placement effect the search below deals with: the
 * forms do not slow down by the same factor on a slow pair of allocations.  Unless the caller fixes the choice
 * (LDPC_TUNE_LINK_NARROW / LINK_HALF), a decoder with more than one frame per lane therefore times the forms on
 * its own arrays when it is created -- interleaved launches, a few milliseconds -- and keeps the fastest (wide
 * also wins at 256 ... 1024 frames: +4 ... +8 % on the whole decode).  The arrays hold zeros, which the first
 * decode overwrites; results do not depend on the choice (the tests run all forms). */
template <int V> int calibrate_link(ldpc_decoder *d)
{
    using namespace ldpc;
    RowClass *rcp = nullptr;
    for (auto &rc : d->flood.row_classes) if (rc.linked) rcp = &rc;
    if (!rcp || !d->flood.fns.link[rcp->degree] || !d->flood.fns.link_narrow[rcp->degree]) return LDPC_OK;
    RowClass &rc = *rcp;
    const int tiles = d->T;
    hipStream_t s = d->stream.s;
    LDPC_HIP_TRY(hipMemsetAsync(d->flood.Q.p, 0, d->flood.Q.n, s));
    LDPC_HIP_TRY(hipMemsetAsync(d->flood.chan.p, 0, d->flood.chan.n, s));
    LDPC_HIP_TRY(hipMemsetAsync(d->done.p, 0, d->done.n * sizeof(uint64_t), s));
    ldpc::Event ev[2];
    LDPC_HIP_TRY(ev[0].create());
    LDPC_HIP_TRY(ev[1].create());
    float best[3] = {1e30f, 1e30f, 1e30f};
    const int candidates = d->flood.fns.link_half[rc.degree] ? 3 : 2;
    /* fp8 messages: the narrow form moves one byte per lane (64 B per wave-instruction) and is no candidate; wide
     * and, at V = 4, half are */
    const bool skip_narrow = d->flood.msg_size == 1;
    hipError_t err = hipSuccess;
    for (int rep = 0; rep < 4 && err == hipSuccess; ++rep) {
        for (int nar = 0; nar < candidates && err == hipSuccess; ++nar) {
            if (nar == 1 && skip_narrow) continue;
            CheckArgs a = check_args(d, TailRef{nullptr, 0, 0}, d->flood.link_rpw, false, rc.e0.p, rc.count, rc.degree);
            LinkArgs lk{rc.link_col.p, rc.link_pos.p, d->flood.chan.p, d->flood.Q.p, d->hard.p, d->N, 1, 0, nullptr, nullptr, 0, 0,
                        rc.n_big, rc.small_rows};
            const int waves = link_chunk_count(d->flood.link_rpw, rc.n_big, rc.small_rows, rc.count) * (nar == 1 ? V : nar == 2 ? V / 2 : 1);
            lk.link_blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
            const dim3 grid = flood_grid(d, lk.link_blocks, tiles, &a.tiles_first, true);
            err = hipEventRecord(ev[0].e, s);
            (nar == 2 ? d->flood.fns.link_half : nar == 1 ? d->flood.fns.link_narrow : d->flood.fns.link)[rc.degree]<<<grid, kBlock, 0, s>>>(a, lk);
            if (err == hipSuccess) err = hipEventRecord(ev[1].e, s);
            if (err == hipSuccess) err = hipEventSynchronize(ev[1].e);
            float ms = 0;
            if (err == hipSuccess) err = hipEventElapsedTime(&ms, ev[0].e, ev[1].e);
            if (err == hipSuccess && rep > 0 && ms < best[nar]) best[nar] = ms;      /* rep 0 warms up */
        }
    }
    if (err != hipSuccess) return set_error(LDPC_ERR_HIP, "link calibration: %s", hipGetErrorString(err));
    LDPC_HIP_TRY(hipGetLastError());
    int pick = 0;
    for (int k = 0; k < candidates; ++k) { d->flood.link_cal_ms[k] = best[k]; if (best[k] < best[pick]) pick = k; }
    d->flood.link_form = pick;
    d->flood.link_calibrated = true;
    return LDPC_OK;
}

/* One message round (check phase + variable-node phase) over all tiles of the decoder on zeroed arrays, best of three
 * timed repetitions (ms). */
template <int V> int time_check_phase(ldpc_decoder *d, float *ms_out)
{
    hipStream_t s = d->stream.s;
    LDPC_HIP_TRY(hipMemsetAsync(d->flood.Q.p, 0, d->flood.Q.n, s));
    LDPC_HIP_TRY(hipMemsetAsync(d->flood.chan.p, 0, d->flood.chan.n, s));
    LDPC_HIP_TRY(hipMemsetAsync(d->done.p, 0, d->done.n * sizeof(uint64_t), s));
    ldpc::Event ev[2];
    LDPC_HIP_TRY(ev[0].create());
    LDPC_HIP_TRY(ev[1].create());
    float best = 1e30f;
    hipError_t err = hipSuccess;
    int rc = LDPC_OK;
    for (int rep = 0; rep < 4 && err == hipSuccess && rc == LDPC_OK; ++rep) {
        err = hipEventRecord(ev[0].e, s);
        rc = enqueue_check_phase<V>(d, s, d->T, (int64_t)d->T * d->F, 1, d->cfg.max_iter, false, ldpc::TailRef{nullptr, 0, 0});
        if (rc == LDPC_OK)
            rc = enqueue_var_phase<V>(d, s, d->T, (int64_t)d->T * d->F, 1, d->cfg.max_iter, false, ldpc::TailRef{nullptr, 0, 0});
        if (err == hipSuccess) err = hipEventRecord(ev[1].e, s);
        if (err == hipSuccess) err = hipEventSynchronize(ev[1].e);
        float ms = 0;
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, ev[0].e, ev[1].e);
        if (err == hipSuccess && rep > 0 && ms < best) best = ms;          /* rep 0 warms up */
    }
    if (rc) return rc;
    if (err != hipSuccess) return set_error(LDPC_ERR_HIP, "placement search: %s", hipGetErrorString(err));
    *ms_out = best;
    return LDPC_OK;
}

/* Where the message arrays lie in device memory decides how fast the streaming check kernels run: the same
 * kernel on the same data takes 1.27, 1.35 or 1.53 ms per launch depending on the allocations it works on, for
 * as long as they live (tools/gpu_placement_probe2.py: six decoders alive in one process, each with its own time,
 * round after round; virtual addresses, offsets inside an allocation, clocks, power and temperature do not predict
 * it -- rounds 2 and 3 looked; profiles/r03_placement_search.txt).  This was the "123 ms or 137 ms regime" of the
 * headline step.  It is a property of the PAIR of allocations behind Q and R: with Q fixed some fresh R allocations
 * are fast and some slow, with R fixed the same holds for Q, the channel array does not matter
 * (tools/gpu_array_trials.py), and consecutive allocations tend to share their luck.  So a decoder whose arrays are
 * large does not take its first allocations as they come: holding what it has, it tries up to `tune_place`
 * (default 6) fresh allocations for R, then for Q, times one message round (check + variable-node phase) with each,
 * keeps the fastest and
 * releases the rest at the end; after at least four measurements a stage stops as soon as it has seen the fast speed next to the slow one (a
 * candidate at least 9 % faster than another).  No guarantee: in some processes every pair is slow.  About 10 ms and 4 GB per candidate while the decoder is being created. */
template <int V> int placement_search(ldpc_decoder *d, size_t TF)
{
    const size_t bq = TF * (size_t)d->E * d->flood.msg_size, bc = TF * d->N * d->flood.msg_size;
    const int want = d->tune.place == 0 ? (2 * bq + bc >= ((size_t)256 << 20) ? 6 : 1) : d->tune.place;
    if (want <= 1) return LDPC_OK;
    float best_ms = 0.0f;
    int rc = time_check_phase<V>(d, &best_ms);
    if (rc) return rc;
    std::vector<DevBuf<uint8_t>> held;           /* the allocations that lost: kept alive until the search ends */
    d->flood.place_ms[0] = best_ms;
    d->flood.place_candidates = 1;
    d->flood.place_kept = 0;
    float lo = best_ms, hi = best_ms;
    for (int stage = 0; stage < 2; ++stage) {
        DevBuf<uint8_t> &arr = stage == 0 ? d->flood.R : d->flood.Q;
        for (int c = 1; c < want; ++c) {
            /* three speeds of the check phase occur (about 1 : 0.88 : 0.83, i.e. 1 : 0.93 : 0.895 for the whole round):
             * stop once the fastest of them has been seen next to the slowest -- but not before four measurements: the
             * speeds within the fast class still differ by 2-3 % (14 processes: a search that stopped after 2.63, 2.61,
             * 2.36 ms kept 2.36 where its neighbours found 2.28-2.31) */
            if (lo < 0.91f * hi && best_ms <= lo && d->flood.place_candidates >= 4) break;
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < 2 * bq + ((size_t)2 << 30)) break;
            /* Device memory comes in two classes that alternate every 16 GiB of (physical) address space, and a read
             * stream and a write stream in DIFFERENT classes do not get in each other's way (tools/offset_map.hip: a copy
             * inside one 40 GiB allocation runs at 6.2 TB/s to a destination less than 16 GiB away, 6.4 beyond, 6.8 at
             * the transition, and back to 6.2 from 32 GiB on; tools/pair_map.hip: separate 4 GiB allocations come in
             * alternating blocks of four).  Physical addresses are not visible, but allocations made one after the other
             * mostly are neighbours: a spacer that brings the distance to the array's partner to about 16 GiB, held while
             * the candidate is allocated, makes the other class likely.  The timing below decides. */
            DevBuf<uint8_t> cand, spacer;
            const size_t period = (size_t)16 << 30;
            if (c == 1 && arr.n < period && free_b > period + 2 * bq + ((size_t)2 << 30)) {
                if (spacer.alloc(period - arr.n) != hipSuccess) (void)hipGetLastError();
            }
            if (cand.alloc(arr.n) != hipSuccess) { (void)hipGetLastError(); break; }
            spacer.release();
            std::swap(arr, cand);                                        /* the candidate is the decoder's array now */
            float ms = 0.0f;
            rc = time_check_phase<V>(d, &ms);
            if (rc) return rc;
            if (d->flood.place_candidates < 16) d->flood.place_ms[d->flood.place_candidates] = ms;
            lo = std::min(lo, ms); hi = std::max(hi, ms);
            if (ms < best_ms) {
                best_ms = ms;
                d->flood.place_kept = d->flood.place_candidates;
            } else {
                std::swap(arr, cand);                                    /* back to the array it had */
            }
            ++d->flood.place_candidates;
            held.push_back(std::move(cand));
        }
    }
    return LDPC_OK;                                                      /* `held` releases the losers here */
}

}  // namespace

/* Message arrays, work lists, kernel tables and launch plan; a decoder that is no hand-over child (top_level) then
 * times the forms of the column-fused check kernel, unless the caller says which, and searches a fast placement. */
int ldpc::engine_flood_setup(ldpc_decoder *d, const ldpc_graph *g, size_t TF, bool top_level)
{
    int rc = setup_flooding(d, g, TF);
    if (rc || !top_level) return rc;
    const ldpc::Tune &tune = d->tune;
    if (tune.link_narrow == 0 && tune.link_half == 0 && !tune.link_deep && d->V >= 2) {
        rc = dispatch_v(d->V, [&](auto v) { return calibrate_link<decltype(v)::value>(d); });
        if (rc) return rc;
    }
    return dispatch_v(d->V, [&](auto v) { return placement_search<decltype(v)::value>(d, TF); });
}

int ldpc::engine_flood_run(ldpc_decoder *d, const LlrIn &llr, int64_t frames, uint8_t *out_dev, int64_t out_bytes,
                           int32_t *iters_dev, hipStream_t s)
{
    return dispatch_v(d->V, [&](auto v) { return run_flooding<decltype(v)::value>(d, llr, frames, out_dev, out_bytes, iters_dev, s); });
}
