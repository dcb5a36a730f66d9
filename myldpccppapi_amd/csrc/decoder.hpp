/*
 * decoder.hpp -- struct ldpc_decoder, the handle behind the C ABI (include/ldpc_hip.h), as the translation units that
 * work on it see it: ldpc_hip.hip (creation, destruction, ldpc_decode_device), engine_flood.hip (the streaming flooding
 * engine), host_path.hip (ldpc_decode) and introspect.hip (timing, statistics, debug taps).
 *
 * At top level: what every algorithm uses.  Then one member per concern: `flood` (only a streaming flooding decoder
 * fills it), `host` (only the host-buffer entry point), `tm` (timing spans and the record of the last call).  Every HIP
 * resource is held by an owner of hip_host.hpp, so the destructor only does what needs an order.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <type_traits>
#include <vector>

#include "../../include/ldpc_hip.h"
#include "flood_tables.hpp"
#include "layered_kernels.hpp"
#include "bitflip_kernels.hpp"
#include "fused_kernels.hpp"
#include "ldsp_kernels.hpp"
#include "engines.hpp"
#include "tune.hpp"
#include "decoder_config_host.hpp"
#include "host_stage.hpp"
#include "hip_host.hpp"

#ifndef LDPC_IDLE_FAT
#define LDPC_IDLE_FAT 8
#endif

namespace ldpc {

/* the run-time frames per lane (1, 2 or 4) as a template argument: fn(std::integral_constant<int, V>) */
template <typename Fn> inline int dispatch_v(int V, Fn &&fn)
{
    return V == 1 ? fn(std::integral_constant<int, 1>{})
                  : V == 2 ? fn(std::integral_constant<int, 2>{}) : fn(std::integral_constant<int, 4>{});
}

/* the run-time message kind (enum ldpc_msg_dtype: float, fp16, fp8 or fixed-point storage) as a type: fn(T{}).  fp8 and
 * fixed point are both one byte, so the size does not tell them apart.  For kernels that load, copy and zero-fill only:
 * every fixed-point width is q8any there (flood_common.hpp); the kernels that store come from the tables. */
template <typename Fn> inline void dispatch_msg(int msg_kind, Fn &&fn)
{
    if (msg_kind == LDPC_MSG_I8) fn(q8any{});
    else if (msg_kind == LDPC_MSG_F8) fn(f8{});
    else if (msg_kind == LDPC_MSG_F16) fn(_Float16{});
    else fn(float{});
}

struct RowClass {
    int degree = 0;
    int count = 0;
    DevBuf<int32_t> e0;
    std::vector<int32_t> h_e0;
    /* column-local fusion (check_link_kernel): per list row, the degree-2 column shared with
     * the next list row when both fall in one wave's chunk of link_rpw rows */
    DevBuf<int32_t> link_col, link_pos;
    int linked = 0;          /* number of fused columns */
    /* guided chunks (flood_link.hpp: LinkArgs): n_big chunks of link_rpw rows, then chunks of small_rows */
    int n_big = 0, small_rows = 1;
};
struct ColClass {
    int degree = 0;
    int count = 0;
    DevBuf<int32_t> col, edge;
    int64_t q_base = -1;     /* first Q slot of the class when Q is stored in writer order (VarArgs::q_base) */
};

/* the classes of one degree bucket that share a launch */
struct ClassGroup {
    int bucket = 0, lo = 0, hi = 0;
    int blocks = 0;                       /* gridDim.x */
    int blocks_fat = 0;                   /* ... with kIdleFat times the rows / columns per wave */
    std::vector<int> members;             /* indices into row_classes / col_classes */
    DevBuf<GroupClass> table, table_fat;
};

/* rounds that are probably idle (the idle hint of run_flooding) launch this many times the rows / columns per wave */
constexpr int kIdleFat = LDPC_IDLE_FAT;

/* The streaming flooding decoder (engine_flood.hip): message arrays, work lists, launch plan, kernel tables and what the
 * creation-time measurements chose.  A handle that runs a layered or a one-launch kernel leaves all of it empty. */
struct FloodPlan {
    DevBuf<uint8_t> chan, Q, R;         /* message arrays: msg_size bytes per element */
    int msg_size = 4;                   /* 4 = fp32, 2 = fp16 (LDPC_MSG_F16), 1 = fp8 E4M3 (LDPC_MSG_F8) or fixed point (LDPC_MSG_I8) */
    int msg_kind = LDPC_MSG_F32;        /* enum ldpc_msg_dtype: what dispatch_msg goes by */
    int msg_bits = 0;                   /* LDPC_MSG_I8: 4, 5, 6 or 8 (config value 0 resolved to 8); otherwise 0 */
    /* Q in writer order (CheckArgs::qpos): slot of every edge, and col_edge with slots in place of edge ids (init_kernel) */
    DevBuf<int32_t> qpos, col_qedge;
    std::vector<int32_t> h_qpos;
    std::vector<RowClass> row_classes;
    std::vector<ColClass> col_classes;
    /* launch plan of a round (plan_launches): classes that share a launch, classes launched alone,
     * and the left-over rows a linked check launch takes along */
    std::vector<ClassGroup> check_groups, var_groups;
    std::vector<int> check_solo, var_solo;
    DevBuf<int32_t> extra_e0, extra_deg;
    int n_extra = 0;
    int64_t extra_edges = 0;
    FloodFns fns;                       /* the kernels of this decoder's arithmetic (flood_tables.hpp) */

    /* tuning choices resolved at creation (the plain fields are read from ldpc_decoder::tune) */
    int link_form = 1;                  /* linked check kernel: 0 wide (V values per lane), 1 narrow (1), 2 half (2) */
    bool link_deep = false;             /* narrow form with inputs two rows ahead */
    bool syn_xcd = true;                /* false: plain 2-D syndrome grid */
    bool check_wide = false;            /* check kernels move V floats per lane */
    int link_rpw = 16;                  /* rows per wave of the fused check kernel; 0 = fusion off */
    int cus = 256;                      /* compute units of the device */
    bool link_calibrated = false;       /* link_form chosen by timing the candidates at creation */
    float link_cal_ms[3] = {0, 0, 0};   /* what the calibration measured per launch: [0] wide, [1] narrow, [2] half */
    /* placement search (cfg.tune_place): the column-fused check kernel's time on each candidate set of arrays */
    int place_candidates = 0, place_kept = 0;
    float place_ms[16] = {};            /* the original pair, then up to 7 fresh R and 7 fresh Q allocations */

    /* device-side tail (flood_common.hpp: TailRef, flood_handover.hpp: tail_gather_kernel): TO overflow tiles follow the T
     * tiles of max_batch in every array (TA = T + TO allocated) */
    bool tail_enabled = false;
    int TO = 0, TA = 0;
    DevBuf<int32_t> tail_state, tail_map, running;

    /* tail compaction (flood_handover.hpp): a V = 1, one-tile decoder that takes over the last running
     * frames of a polled, early-terminating decode */
    std::unique_ptr<ldpc_decoder> child;
    DevBuf<int32_t> cmap;               /* [child_capacity] frame indices handed to the child */
    DevBuf<int32_t> cinv;               /* [max_batch] where a handed-over frame's bit sits in the child (valid where cmoved says so) */
    DevBuf<unsigned long long> cmoved;  /* [T][V] bits of each mask word whose frames were handed over */
    int child_capacity = kCompactCapacity;      /* frames the child holds: 512, or 1024 for batches of >= 4096 frames */
    int compact_threshold = kCompactCapacity;   /* cfg.tune_compact: 0 = off, else hand over when <= this many frames run */
    bool is_child = false;
    ldpc_decoder *handed_to = nullptr;  /* the decoder (child, or the child's child) that finished the last call's stragglers */
    HostBuf<int32_t> h_active;          /* pinned: the polled "frames still running" word */
    DevBuf<int32_t> soft_map;           /* a child: [max_batch] its slots as frames of the soft call's batch; made by the first
                                           hand-over of a soft call (soft_kernels.hpp: soft_map_kernel) */

    /* Rounds beyond the previous call's iteration count are probably idle: they are launched with
     * kIdleFat times as many rows / columns per wave, i.e. that many times fewer workgroups (an idle
     * workgroup costs about a clock of dispatch chip-wide: 312 000 of them per round for the rate-9/10
     * code at 4096 frames).  The count arrives through a pinned word copied at the end of every call;
     * it is read only once that copy has completed.  (Block-strided loops inside the kernels were
     * tried instead and cost 17-27 % at full work: profiles/r02_ab_block_strided_negative.txt.) */
    HostBuf<int32_t> h_summary;         /* pinned [2] */
    Event ev_summary;
    bool summary_pending = false;
    int idle_after = 0;                 /* 0: no hint */

    bool first_round_from_chan = false; /* this call's round 1 reads q = y from the channel array (min-sum) */
};

/* The host-buffer entry point (host_path.hip).  Three staging slots, so the H2D copy of group k+1 (copy_stream)
 * overlaps the decode of group k (the handle's stream) and the copy-out of group k-1. */
struct HostSlot {
    DevBuf<float> llr;
    DevBuf<uint8_t> out;
    DevBuf<int32_t> iters;
    HostBuf<uint8_t> h_out;             /* pinned: D2H completes without blocking the host */
    HostBuf<int32_t> h_iters;
    DevBuf<float> soft;                 /* soft output, [max_batch][N]: both made by the handle's first ldpc_decode_soft */
    HostBuf<float> h_soft;
    HostBuf<uint8_t> h_head;           /* pinned, kStageBytes: a whole small group, or a large group's bytes before
                                           its first page boundary and (last group) after its last one */
    Event h2d_done, all_done;
    bool busy = false;
    int64_t off = 0, n = 0, dst = 0, copy_bytes = 0;
    /* the group's counts for the call's statistics: the decoder's summary words (and those of the decoders its
     * stragglers were handed to), copied out behind the group's decode, before the next group resets them */
    HostBuf<int32_t> h_sum;             /* pinned: [4][4] */
    int g_iterations = 0, g_tiles = 0, g_children = 0, g_child_f[3] = {0, 0, 0};
};
struct RingChunk { HostBuf<uint8_t> h; Event ev; bool used = false; };
/* counts of the last ldpc_decode() call over ALL its launch groups (ldpc_decoder_stats) */
struct CallCounts { bool valid = false; int32_t iterations = 0, batch_time = 0; int64_t frames = 0, converged = 0, frame_rounds = 0, crc_stops = 0; };

struct HostPath {
    Stream copy_stream;                 /* declared before the slots and the ring: their events and memory go first */
    HostSlot slot[3];
    CallCounts call;
    bool suppress_poll = false;
    /* LDPC_HOST_INPUT_STAGED: a ring of pinned chunks the caller's channel values pass through, filled by
     * the stager thread (and its copy helpers) while the calling thread enqueues -- or, with polling,
     * sits in -- the previous group's decode.  Threads and ring are made by the first large host-buffer
     * call and live until the handle is destroyed. */
    std::vector<RingChunk> ring;
    size_t ring_next = 0;
    std::unique_ptr<Worker> stager;
    std::vector<std::unique_ptr<Worker>> copy_helpers;
    std::vector<Job> copy_jobs;         /* one per helper, reused chunk after chunk */
    Job stage_job[3];                   /* one per slot */
    bool stage_pending[3] = {false, false, false};
    /* LDPC_HOST_INPUT_LOCK_PAGES: blocks of the caller's buffer this handle has page-locked (empty between
     * calls), and blocks it could not release (reported by the call and by ldpc_decoder_destroy) */
    std::vector<void *> locked_blocks, stuck_blocks;
};

struct TimedSpan {
    Event a, b;
    int kind = 0;       /* 0 check, 1 var, 2 layer, 3 other, 4 check with column-local fusion, 5 check group, 6 var group,
                           7 soft_settle_kernel (soft output), 8 llr_widen_kernel (typed input in front of a one-launch kernel) */
    int degree = 0;     /* groups: the bucket's highest degree */
    int64_t bytes = 0;  /* algorithmic bytes of the launch in the two-kernel formulation (16 E + 4 N in total) */
    int64_t moved = 0;  /* bytes this kernel's own loads and stores move (less when columns are fused in) */
    int lo = 0;         /* groups: the bucket's lowest degree */
};

/* timing spans (introspect.hip reads them) and the record of the last device call */
struct Timing {
    bool timing = false;                /* the call being enqueued is timed */
    int timing_every = 0;               /* 0 off, k: every k-th device call is timed */
    int64_t timing_calls = 0;
    std::vector<TimedSpan> spans;
    size_t spans_used = 0;
    Event ev_begin, ev_end;
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    int32_t tap_iter = 0;
};

/* Soft output of the call being enqueued (ldpc_decode_soft_device sets it around the plain entry point and clears it
 * again: nothing of it outlives the call).  dst == nullptr: a plain call. */
struct SoftReq {
    float *dst = nullptr;               /* [frames][N] the caller's device buffer */
    int32_t kind = 0;                   /* LDPC_SOFT_POSTERIOR / LDPC_SOFT_EXTRINSIC */
    const int32_t *fmap = nullptr;      /* a hand-over child: its slots as frames of the caller's batch (FloodPlan::soft_map) */
};

}  // namespace ldpc

struct ldpc_decoder {
    /* Destruction order relied on: the destructor's body stops the threads and drains the handle's streams; the members
     * then go in reverse order of declaration, so `stream` (first) outlives every array and event that was used on it,
     * as host.copy_stream does inside `host`. */
    ldpc::Stream stream;
    ldpc_decoder_config cfg{};
    int32_t M = 0, N = 0;
    int64_t E = 0;
    int V = 1, F = 64, T = 0; /* frames per lane, per tile, tiles at max_batch */
    std::vector<int32_t> h_cols;
    ldpc::Tune tune;                    /* cfg.tune_* unpacked (tune.hpp) */

    ldpc::DevBuf<int32_t> row_ptr, edge_col, col_ptr, col_edge;
    ldpc::DevBuf<uint64_t> hard, failw, done;
    ldpc::DevBuf<int32_t> iters, active;
    ldpc::DevBuf<int32_t> summary;      /* [4]: max iters, converged count, tile-rounds that did work (early termination),
                                           frames stopped by the CRC alone (cfg.crc_kind) */
    ldpc::DevBuf<uint32_t> crc_w;       /* cfg.crc_kind != 0: [crc_bits] column weights of crc_term_kernel (crc_term_host.hpp) */

    /* The engine this handle runs, chosen once at creation (decoder_config_host.hpp: engine_candidates); only that
     * engine's plan below is filled. */
    ldpc::Engine engine = ldpc::Engine::Flood;
    /* whole decode in one launch: frames leave inside it, the kernels read float channel values */
    bool one_launch() const { return engine == ldpc::Engine::Fused || engine == ldpc::Engine::Ldsp || engine == ldpc::Engine::LdspFx; }
    ldpc::LayeredPlan layered;          /* Engine::Layered: streaming, one launch per layer */
    ldpc::BitflipPlan bitflip;          /* Engine::Bitflip: received bits, syndrome words, votes (hard holds x at V = 1) */
    ldpc::FusedPlan fused;              /* Engine::Fused, short QC codes: whole decode in LDS */
    ldpc::LdspPlan ldsp;                /* Engine::Ldsp, mid-size QC codes: posterior in LDS, check records in cache;
                                           Engine::LdspFx (LDPC_ALGO_LAYERED_FX with LDPC_TUNE_FX_RECORD): the same in fixed point */
    /* normalized / offset min-sum (cfg.ms_scale / ms_offset): the streaming kernels of kAlgoMSC (flooding) or
     * layer_corr_kernel (layered) run with alpha = ms_scale (1 when 0) and beta = ms_offset */
    bool ms_corr = false;
    float ms_scale = 1.0f, ms_offset = 0.0f;

    int32_t last_iterations = 0;
    int64_t last_frames = 0;
    int32_t last_tiles = 0;

    ldpc::DevBuf<float> llr_wide;       /* one-launch and record kernels: [max_batch][N] floats a typed call (llr_type != F32)
                                           widens into (llr_input.hpp: llr_widen_kernel); made by the handle's first typed call */

    ldpc::FloodPlan flood;
    ldpc::HostPath host;
    ldpc::Timing tm;
    ldpc::SoftReq soft;

    /* a handle over several devices (ldpc_decoder_create_multi): one single-device decoder per entry
     * of the device list, and one persistent host thread per entry that runs its frame range; this
     * object then owns no device state of its own */
    std::vector<ldpc_decoder *> shards;
    std::vector<std::unique_ptr<ldpc::Worker>> shard_workers;

    /* Waits for the handle's OWN work: its two streams and, through the end-of-decode event, the
     * caller's stream of the last ldpc_decode_device call -- not for the device, which other handles
     * and the caller's other streams keep using. */
    void wait_for_own_work()
    {
        if (!stream.s) return;              /* a device-list handle, or a creation that failed before its first enqueue */
        if (flood.child) flood.child->wait_for_own_work();
        (void)hipSetDevice(cfg.device);
        if (tm.have_last && tm.ev_end.e) (void)hipEventSynchronize(tm.ev_end.e);
        (void)hipStreamSynchronize(stream.s);
        if (host.copy_stream.s) (void)hipStreamSynchronize(host.copy_stream.s);
    }

    ~ldpc_decoder()
    {
        /* threads first: nothing of this handle runs any more when its streams and buffers go */
        for (auto &w : shard_workers) w->stop();
        if (host.stager) host.stager->stop();
        for (auto &w : host.copy_helpers) w->stop();
        for (ldpc_decoder *sh : shards) (void)ldpc_decoder_destroy(sh);
        wait_for_own_work();                /* also on a creation that failed half way */
    }
};

namespace ldpc {

/* a typed call's (llr, llr_type, llr_unit): LDPC_OK or LDPC_ERR_ARG with the message set (ldpc_hip.hip) */
int llr_in_check(const void *p, int32_t type, float unit);

inline hipError_t span_begin(ldpc_decoder *d, hipStream_t s, int kind, int degree = 0, int64_t bytes = 0, int64_t moved = -1,
                             int lo = 0)
{
    Timing &t = d->tm;
    if (!t.timing) return hipSuccess;
    if (t.spans_used == t.spans.size()) {
        TimedSpan sp;
        hipError_t e = sp.a.create();
        if (e == hipSuccess) e = sp.b.create();
        if (e != hipSuccess) return e;
        t.spans.push_back(std::move(sp));
    }
    TimedSpan &sp = t.spans[t.spans_used];
    sp.kind = kind;
    sp.degree = degree;
    sp.bytes = bytes;
    sp.moved = moved < 0 ? bytes : moved;
    sp.lo = lo;
    return hipEventRecord(sp.a.e, s);
}

inline hipError_t span_end(ldpc_decoder *d, hipStream_t s)
{
    if (!d->tm.timing) return hipSuccess;
    return hipEventRecord(d->tm.spans[d->tm.spans_used++].b.e, s);
}

}  // namespace ldpc
