/*
 * host_path.hip -- the host-buffer entry point and its staging rule (decode_host), and how a handle over several devices
 * shares a call out (shard_unit, one host thread per device range).
 *
 * ldpc_decode: the reference's Coder::decode signature (MyLdpc.cpp:571-618; its copies are the blocking
 * enqueueWriteBuffer / enqueueReadBuffer of :796 and :988).  What moves the caller's channel values is
 * chosen per call (enum ldpc_host_input, include/ldpc_hip.h):
 *   direct -- the caller has page-locked the buffer itself: plain asynchronous copies;
 *   staged -- the default: worker threads of the handle copy each launch group through a ring of this
 *             library's own pinned chunks; the HIP runtime never sees the caller's pointer;
 *   lock   -- opt-in: whole pages strictly inside the call's byte range are page-locked for the call
 *             and read in place by the copy engine (host_stage.hpp: plan_group_blocks, PageLockRegistry).
 * Groups of up to kStageBytes are copied by the calling thread into the slot's pinned scratch in the
 * last two modes (one frame of the (648, 324) code is 2.6 KB: no thread hop on the latency path). */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "decoder.hpp"

using ldpc::set_error;

namespace {

constexpr size_t kStageBytes = (size_t)4 << 20;
constexpr size_t kRingChunk = (size_t)8 << 20;
constexpr int kRingChunks = 4;

enum InputMode { kInputDirect = 0, kInputStaged = 1, kInputLock = 2 };

InputMode resolve_input_mode(const ldpc_decoder_config &cfg, const void *p, size_t bytes)
{
    if (ldpc::PageLockRegistry::instance().caller_locked(p, (const uint8_t *)p + bytes - 1)) return kInputDirect;
    return cfg.host_input == LDPC_HOST_INPUT_LOCK_PAGES ? kInputLock : kInputStaged;
}

/* the pinned ring, the stager thread and its copy helpers: made once, by the first call that needs them */
int ensure_stager(ldpc_decoder *d)
{
    if (d->host.stager) return LDPC_OK;
    if (d->host.ring.empty()) d->host.ring.resize(kRingChunks);
    for (auto &c : d->host.ring) {
        LDPC_HIP_TRY(c.h.ensure(kRingChunk));
        LDPC_HIP_TRY(c.ev.ensure(false));
    }
    const int threads = d->cfg.host_copy_threads > 0 ? d->cfg.host_copy_threads : 4;
    while ((int)d->host.copy_helpers.size() < threads - 1) {
        std::unique_ptr<ldpc::Worker> w(new (std::nothrow) ldpc::Worker(ldpc::last_error_text));
        if (!w || !w->start()) return set_error(LDPC_ERR_NOMEM, "cannot start a copy thread");
        d->host.copy_helpers.push_back(std::move(w));
    }
    d->host.copy_jobs.resize(d->host.copy_helpers.size());
    std::unique_ptr<ldpc::Worker> st(new (std::nothrow) ldpc::Worker(ldpc::last_error_text));
    if (!st || !st->start()) return set_error(LDPC_ERR_NOMEM, "cannot start the staging thread");
    d->host.stager = std::move(st);
    return LDPC_OK;
}

/* n bytes into a pinned chunk, the helpers taking equal page-aligned parts */
void ring_fill(ldpc_decoder *d, uint8_t *dst, const uint8_t *src, size_t n)
{
    const size_t parts = d->host.copy_helpers.size() + 1;
    if (parts == 1 || n < ((size_t)1 << 20)) { memcpy(dst, src, n); return; }
    const size_t per = ((n + parts - 1) / parts + 4095) & ~(size_t)4095;
    size_t used = 0;
    for (size_t i = 0; i < d->host.copy_helpers.size(); ++i) {
        const size_t lo = (i + 1) * per;
        if (lo >= n) break;
        const size_t len = std::min(per, n - lo);
        d->host.copy_jobs[i].fn = [dst, src, lo, len]() -> int { memcpy(dst + lo, src + lo, len); return 0; };
        d->host.copy_helpers[i]->submit(&d->host.copy_jobs[i]);
        ++used;
    }
    memcpy(dst, src, std::min(per, n));
    for (size_t i = 0; i < used; ++i) (void)d->host.copy_helpers[i]->wait(&d->host.copy_jobs[i]);
}

/* `bytes` from pageable memory to the device through the ring, on the copy stream.  One thread at a
 * time per decoder (the stager thread; in lock mode the calling thread, for a block that could not be
 * locked).  A chunk is reused once the copy that read it has completed. */
hipError_t staged_copy(ldpc_decoder *d, uint8_t *dst, const uint8_t *src, size_t bytes)
{
    for (size_t o = 0; o < bytes; o += kRingChunk) {
        const size_t n = std::min(kRingChunk, bytes - o);
        auto &c = d->host.ring[d->host.ring_next++ % d->host.ring.size()];
        hipError_t e = c.used ? hipEventSynchronize(c.ev.e) : hipSuccess;
        if (e != hipSuccess) return e;
        ring_fill(d, c.h.p, src + o, n);
        e = hipMemcpyAsync(dst + o, c.h.p, n, hipMemcpyHostToDevice, d->host.copy_stream.s);
        if (e == hipSuccess) e = hipEventRecord(c.ev.e, d->host.copy_stream.s);
        if (e != hipSuccess) return e;
        c.used = true;
    }
    return hipSuccess;
}

/* ldpc_decode on ONE device; `mode` was decided once per ldpc_decode call, before any thread of a device
 * list has touched the buffer. */
int decode_host(ldpc_decoder *d, const ldpc::LlrIn &in, int64_t frames, uint8_t *out_host,
                int64_t out_bytes, int32_t *iters, InputMode mode, float *soft_host = nullptr, int32_t soft_kind = 0)
{
    /* launch groups, the pinned ring and the copies are sized in bytes of the element type; the device staging slots hold
     * the caller's elements as they are (a slot has room for max_batch * N floats) and the init kernels read them there */
    const size_t esz = ldpc::llr_elem_size(in.type);
    const uint8_t *llr_host = static_cast<const uint8_t *>(in.p);
    const int64_t total = ldpc_out_bytes(d->cfg.K, frames, d->cfg.pack_mode);
    LDPC_HIP_TRY(hipSetDevice(d->cfg.device));
    int64_t B = d->cfg.max_batch;
    /* A large call that is ONE launch group is cut into two: the second half's channel values travel while the first
     * half is decoded (one group exposes its whole copy: 21 ms of PCIe in front of a 94 ms decode for 4096 frames of the
     * headline code; half batches decode at 0.99 of the full batch's rate).  Only where the grouping cannot be seen in
     * the output: K a multiple of 8 (MyLdpc.cpp:577-616 starts every group at byte off*K/8).  The threshold is in bytes
     * of the caller's element type: a narrow call is cut later (4x the frames with int8 values), its copy being shorter. */
    if (frames <= B && frames >= 2048 && d->cfg.K % 8 == 0 &&
        (size_t)frames * d->N * esz >= ((size_t)256 << 20))
        B = ((frames + 1) / 2 + 255) / 256 * 256;
    if (d->cfg.pack_mode == LDPC_PACK_BITS && (d->cfg.K % 8) && frames > B)
        return set_error(LDPC_ERR_UNSUPPORTED, "bit-packed output with K %% 8 != 0 cannot be chunked: "
                    "raise max_batch to cover all %lld frames", (long long)frames);
    const int64_t Bmax = d->cfg.max_batch;      /* the slots hold a full group whatever this call's groups are */
    const int64_t stage_out = ldpc_out_bytes(d->cfg.K, Bmax, d->cfg.pack_mode) + 8;
    /* more than one group: three staging slots, so that group k+1's channel values are copied in while
     * group k is decoded (the host may block in group k's early-termination polls) and group k-1's
     * results are copied out */
    const int nslots = frames > B ? 3 : 1;
    const int64_t ngroups = (frames + B - 1) / B;
    LDPC_HIP_TRY(d->host.copy_stream.ensure());
    for (int i = 0; i < nslots; ++i) {
        auto &sl = d->host.slot[i];
        LDPC_HIP_TRY(sl.llr.ensure((size_t)Bmax * d->N));
        LDPC_HIP_TRY(sl.out.ensure((size_t)stage_out));
        LDPC_HIP_TRY(sl.iters.ensure((size_t)Bmax));
        LDPC_HIP_TRY(sl.h_out.ensure((size_t)stage_out));
        LDPC_HIP_TRY(sl.h_iters.ensure((size_t)Bmax));
        if (soft_host) {        /* soft output: made by the handle's first soft call */
            LDPC_HIP_TRY(sl.soft.ensure((size_t)Bmax * d->N));
            LDPC_HIP_TRY(sl.h_soft.ensure((size_t)Bmax * d->N));
        }
        LDPC_HIP_TRY(sl.h_head.ensure(kStageBytes));
        LDPC_HIP_TRY(sl.h_sum.ensure(16));
        LDPC_HIP_TRY(sl.h2d_done.ensure(false));
        LDPC_HIP_TRY(sl.all_done.ensure(false));
    }
    if (mode != kInputDirect && (size_t)std::min(B, frames) * d->N * esz > kStageBytes) {
        const int rs = ensure_stager(d);
        if (rs) return rs;
    }
    ldpc::PageLockRegistry &registry = ldpc::PageLockRegistry::instance();
    /* a finished group's bytes go from the pinned slot to the caller's buffers */
    ldpc::CallCounts counts;
    const bool flooding_counts = d->engine == ldpc::Engine::Flood;
    auto drain = [&](ldpc::HostSlot &sl) -> int {
        if (!sl.busy) return LDPC_OK;
        sl.busy = false;
        LDPC_HIP_TRY(hipEventSynchronize(sl.all_done.e));
        if (sl.copy_bytes > 0) memcpy(out_host + sl.dst, sl.h_out.p, (size_t)sl.copy_bytes);
        if (iters) memcpy(iters + sl.off, sl.h_iters.p, (size_t)sl.n * sizeof(int32_t));
        if (soft_host) memcpy(soft_host + (size_t)sl.off * d->N, sl.h_soft.p, (size_t)sl.n * d->N * sizeof(float));
        /* the call's counts: sums over its groups, maxima for the iteration numbers (as ldpc_decoder_stats forms them) */
        counts.frames += sl.n;
        counts.converged += sl.h_sum.p[1];
        counts.batch_time = std::max(counts.batch_time, sl.h_sum.p[0]);
        counts.iterations = std::max(counts.iterations, sl.g_iterations);
        if (flooding_counts) {
            counts.frame_rounds += d->cfg.early_term ? (int64_t)sl.h_sum.p[2] * d->F : (int64_t)sl.g_iterations * sl.g_tiles * d->F;
            for (int c = 0; c < sl.g_children; ++c) counts.frame_rounds += (int64_t)sl.h_sum.p[4 * (c + 1) + 2] * sl.g_child_f[c];
        }
        if (d->cfg.crc_kind) {       /* frames stopped by the CRC alone: this decoder's and those of the hand-over chain */
            counts.crc_stops += sl.h_sum.p[3];
            for (int c = 0; c < sl.g_children; ++c) counts.crc_stops += sl.h_sum.p[4 * (c + 1) + 3];
        }
        return LDPC_OK;
    };
    int rc = LDPC_OK;
#ifdef LDPC_TRACE_HOST
    const auto t_start = std::chrono::steady_clock::now();
#define LDPC_STAMP(what, kk)                                                                             \
    fprintf(stderr, "[ldpc_decode] %8.2f ms  group %lld  %s\n",                                          \
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(), \
            (long long)(kk), what)
#else
#define LDPC_STAMP(what, kk) ((void)0)
#endif
    /* Coder::decode, MyLdpc.cpp:577-616: groups of batchSize frames, last one short.
     * stage_in(k): group k's channel values -> slot k % nslots, on the copy stream (a copy from pageable
     * memory handed to the runtime as it is would wait for the device's other work -- measured: 151 ms
     * behind a 140 ms decode instead of 19 ms -- so the input never travels that way). */
    auto stage_in = [&](int64_t kk) -> int {
        const int si = (int)(kk % nslots);
        auto &sl = d->host.slot[si];
        const int r1 = drain(sl);                /* the slot's previous tenant (group kk - nslots) */
        if (r1) return r1;
        const int64_t off = kk * B, n = std::min(B, frames - off);
        const uint8_t *src = llr_host + (size_t)off * d->N * esz;
        const size_t bytes = (size_t)n * d->N * esz;
        uint8_t *dst = reinterpret_cast<uint8_t *>(sl.llr.p);
        hipError_t e = hipSuccess;
        if (mode == kInputDirect) {
            e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, d->host.copy_stream.s);
        } else if (bytes <= kStageBytes) {
            memcpy(sl.h_head.p, src, bytes);
            e = hipMemcpyAsync(dst, sl.h_head.p, bytes, hipMemcpyHostToDevice, d->host.copy_stream.s);
        } else if (mode == kInputStaged) {
            ldpc::Job &job = d->host.stage_job[si];
            hipEvent_t done = sl.h2d_done.e;
            job.fn = [d, dst, src, bytes, done]() -> int {
                hipError_t je = hipSetDevice(d->cfg.device);
                if (je == hipSuccess) je = staged_copy(d, dst, src, bytes);
                if (je == hipSuccess) je = hipEventRecord(done, d->host.copy_stream.s);
                return je == hipSuccess ? LDPC_OK
                                        : set_error(LDPC_ERR_HIP, "staging through the pinned ring: %s", hipGetErrorString(je));
            };
            d->host.stager->submit(&job);
            d->host.stage_pending[si] = true;
            LDPC_STAMP("staging submitted", kk);
            return LDPC_OK;                      /* the job records h2d_done */
        } else {
            /* float channel values only: decode_entry stages a typed call (the page arithmetic is float-sized) */
            const ldpc::GroupBlocks gb = ldpc::plan_group_blocks((uintptr_t)llr_host, frames, d->N, B, kk);
            bool locked = false;
            if (!gb.whole_by_cpu) {
                bool overlap = false;
                locked = registry.lock((void *)gb.b0, (size_t)(gb.b1 - gb.b0), &overlap) == hipSuccess;
                if (locked) d->host.locked_blocks.push_back((void *)gb.b0);
            }
            if (!locked) {
                e = staged_copy(d, dst, src, bytes);      /* somebody else holds these pages: stage */
            } else {
                const size_t head = (size_t)(gb.b0 - gb.s0), body = (size_t)(gb.body_end - gb.b0),
                             tail = (size_t)(gb.s1 - gb.body_end);
                if (head) {
                    memcpy(sl.h_head.p, src, head);
                    e = hipMemcpyAsync(dst, sl.h_head.p, head, hipMemcpyHostToDevice, d->host.copy_stream.s);
                }
                if (e == hipSuccess)
                    e = hipMemcpyAsync(dst + head, (const void *)gb.b0, body, hipMemcpyHostToDevice, d->host.copy_stream.s);
                if (e == hipSuccess && tail) {
                    memcpy(sl.h_head.p + ldpc::kPage, (const void *)gb.body_end, tail);
                    e = hipMemcpyAsync(dst + head + body, sl.h_head.p + ldpc::kPage, tail, hipMemcpyHostToDevice, d->host.copy_stream.s);
                }
            }
        }
        if (e == hipSuccess) e = hipEventRecord(sl.h2d_done.e, d->host.copy_stream.s);
        if (e != hipSuccess) return set_error(LDPC_ERR_HIP, "host-to-device staging: %s", hipGetErrorString(e));
        LDPC_STAMP("H2D enqueued", kk);
        return LDPC_OK;
    };
    /* the staging job of slot si has run: its copies and h2d_done are on the copy stream */
    auto staged_ready = [&](int si) -> int {
        if (!d->host.stage_pending[si]) return LDPC_OK;
        d->host.stage_pending[si] = false;
        const int r = d->host.stager->wait(&d->host.stage_job[si]);
        if (r) ldpc::restore_error(d->host.stage_job[si].err);
        return r;
    };
    rc = stage_in(0);
    for (int64_t k = 0; k < ngroups && rc == LDPC_OK; ++k) {
        const int si = (int)(k % nslots);
        auto &sl = d->host.slot[si];
        const int64_t off = k * B, n = std::min(B, frames - off);
        if (k + 1 < ngroups && (rc = stage_in(k + 1))) break;   /* runs beside this group's decode */
        if ((rc = staged_ready(si))) break;
        hipError_t e = hipStreamWaitEvent(d->stream.s, sl.h2d_done.e, 0);
        if (e != hipSuccess) { rc = set_error(LDPC_ERR_HIP, "host-to-device staging: %s", hipGetErrorString(e)); break; }
        const int64_t chunk_bytes = ldpc_out_bytes(d->cfg.K, n, d->cfg.pack_mode);
        /* LDPC_LLR_F32 with unit 1: these are ldpc_decode_soft_device and ldpc_decode_device */
        if (soft_host)
            rc = ldpc_decode_soft_typed_device(d, sl.llr.p, in.type, in.unit, n, sl.out.p, chunk_bytes, iters ? sl.iters.p : nullptr,
                                               sl.soft.p, n * (int64_t)d->N, soft_kind, d->stream.s);
        else
            rc = ldpc_decode_typed_device(d, sl.llr.p, in.type, in.unit, n, sl.out.p, chunk_bytes, iters ? sl.iters.p : nullptr,
                                          d->stream.s);
        if (rc) break;
        LDPC_STAMP("decode enqueued", k);
        /* byte offset of this group's first frame: (off*K)/8 in both packings */
        sl.off = off; sl.n = n;
        sl.dst = off * (int64_t)d->cfg.K / 8;
        sl.copy_bytes = std::max<int64_t>(0, std::min(std::min(out_bytes, total) - sl.dst, chunk_bytes));
        if (sl.copy_bytes > 0)
            e = hipMemcpyAsync(sl.h_out.p, sl.out.p, (size_t)sl.copy_bytes, hipMemcpyDeviceToHost, d->stream.s);
        if (e == hipSuccess && iters)
            e = hipMemcpyAsync(sl.h_iters.p, sl.iters.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, d->stream.s);
        if (e == hipSuccess && soft_host)
            e = hipMemcpyAsync(sl.h_soft.p, sl.soft.p, (size_t)n * d->N * sizeof(float), hipMemcpyDeviceToHost, d->stream.s);
        sl.g_iterations = d->last_iterations; sl.g_tiles = d->last_tiles; sl.g_children = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(sl.h_sum.p, d->summary.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, d->stream.s);
        for (const ldpc_decoder *p = d->flood.handed_to; p && sl.g_children < 3 && e == hipSuccess; p = p->flood.handed_to) {
            sl.g_child_f[sl.g_children] = p->F;
            e = hipMemcpyAsync(sl.h_sum.p + 4 * (sl.g_children + 1), p->summary.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, d->stream.s);
            ++sl.g_children;
        }
        if (e == hipSuccess) e = hipEventRecord(sl.all_done.e, d->stream.s);
        if (e != hipSuccess) { rc = set_error(LDPC_ERR_HIP, "device-to-host staging: %s", hipGetErrorString(e)); break; }
        sl.busy = true;
    }
#undef LDPC_STAMP
    std::string first_error = rc ? ldpc::last_error_text() : std::string();
    /* every exit path: no staging job still reads the caller's buffer, nothing of this call is in flight */
    for (int i = 0; i < nslots; ++i) {
        const int r2 = staged_ready(i);
        if (rc == LDPC_OK && r2) { rc = r2; first_error = ldpc::last_error_text(); }
    }
    for (int i = 0; i < nslots; ++i) {          /* oldest first: slot (ngroups % nslots) was filled earliest */
        const int r2 = drain(d->host.slot[(ngroups + i) % nslots]);
        if (rc == LDPC_OK && r2) { rc = r2; first_error = ldpc::last_error_text(); }
    }
    hipError_t es = hipStreamSynchronize(d->host.copy_stream.s);
    const hipError_t es2 = hipStreamSynchronize(d->stream.s);
    if (es == hipSuccess) es = es2;
    if (es != hipSuccess && rc == LDPC_OK) {
        rc = set_error(LDPC_ERR_HIP, "ldpc_decode: draining the streams: %s", hipGetErrorString(es));
        first_error = ldpc::last_error_text();
    }
    /* lock mode: the pages go back to the caller; a block that cannot be released stays on record */
    for (void *p : d->host.locked_blocks) {
        const hipError_t eu = registry.unlock(p);
        if (eu == hipSuccess) continue;
        d->host.stuck_blocks.push_back(p);
        if (rc == LDPC_OK) {
            rc = set_error(LDPC_ERR_HIP, "hipHostUnregister(%p) failed: %s -- the block stays page-locked and on this "
                      "library's record", p, hipGetErrorString(eu));
            first_error = ldpc::last_error_text();
        }
    }
    d->host.locked_blocks.clear();
    if (!first_error.empty()) ldpc::restore_error(first_error);
    counts.valid = rc == LDPC_OK && ngroups > 1;       /* one group: the decoder's own record is the call's */
    d->host.call = counts;
    return rc;
}

/* Shard boundaries that keep a multi-device result byte-identical to the single-device one: with
 * K % 8 != 0 a frame's first byte is (frame*K)/8 with the division applied per launch group
 * (MyLdpc.cpp:577-616 passes &srcCode[off*K/8]), so ranges must start where frame*K is a multiple
 * of 8 -- and on a group boundary once the stream is longer than one group. */
int32_t shard_unit(const ldpc_decoder_config &cfg, int64_t frames)
{
    if (cfg.K % 8 == 0) return 1;
    int64_t u = 8;
    while (u > 1 && ((u / 2) * (int64_t)cfg.K) % 8 == 0) u /= 2;
    if (frames > cfg.max_batch) {
        int64_t a = u, b = cfg.max_batch;
        while (b) { const int64_t t = a % b; a = b; b = t; }
        u = u / a * cfg.max_batch;               /* lcm(u, max_batch) */
    }
    return (int32_t)std::min<int64_t>(u, 0x7fffffff);
}

/* ldpc_decode (soft_host == nullptr) and ldpc_decode_soft: one device, or the frame ranges of a device list */
int decode_entry(ldpc_decoder *d, const ldpc::LlrIn &in, int64_t frames, uint8_t *out_host, int64_t out_bytes, int32_t *iters,
                 float *soft_host, int32_t soft_kind)
{
    if (!d) return set_error(LDPC_ERR_ARG, "decoder is NULL");
    if (int rc = ldpc::llr_in_check(in.p, in.type, in.unit)) return rc;
    const uint8_t *llr_host = static_cast<const uint8_t *>(in.p);
    const size_t esz = ldpc::llr_elem_size(in.type);
    if (frames < 0) return set_error(LDPC_ERR_ARG, "frames < 0");
    if (frames == 0) return LDPC_OK;
    if (!llr_host || !out_host) return set_error(LDPC_ERR_ARG, "llr/out is NULL");
    if (out_bytes < 0) return set_error(LDPC_ERR_ARG, "out_bytes < 0");
    /* asked once, before any thread touches the buffer */
    InputMode mode = resolve_input_mode(d->cfg, llr_host, (size_t)frames * d->N * esz);
    /* narrow channel values: staged, or direct from memory the caller page-locked; LOCK_PAGES is treated as staged */
    if (in.type != LDPC_LLR_F32 && mode == kInputLock) mode = kInputStaged;
    if (d->shards.empty()) return decode_host(d, in, frames, out_host, out_bytes, iters, mode, soft_host, soft_kind);

    /* several devices: each entry's own host thread decodes a contiguous frame range */
    const int n = (int)d->shards.size();
    const int32_t unit = shard_unit(d->cfg, frames);
    std::vector<int64_t> lo((size_t)n), hi((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int rc = ldpc_shard_range(frames, i, n, unit, &lo[i], &hi[i]);
        if (rc) return rc;
    }
    std::vector<ldpc::Job> jobs((size_t)n);
    for (int i = 0; i < n; ++i) {
        ldpc_decoder *sh = d->shards[i];
        sh->tm.have_last = false;
        if (hi[i] <= lo[i]) continue;
        const int64_t base = lo[i] * (int64_t)d->cfg.K / 8;      /* exact: lo is a multiple of the unit */
        const int64_t room = std::max<int64_t>(0, out_bytes - base);
        const int64_t lo_i = lo[i], cnt = hi[i] - lo[i];
        const int64_t obytes = std::min(room, ldpc_out_bytes(d->cfg.K, cnt, d->cfg.pack_mode));
        const int32_t N = d->N;
        const ldpc::LlrIn part{llr_host + (size_t)lo_i * N * esz, in.type, in.unit};
        jobs[i].fn = [sh, part, out_host, iters, lo_i, cnt, base, obytes, N, mode, soft_host, soft_kind]() -> int {
            return decode_host(sh, part, cnt, out_host + base, obytes,
                               iters ? iters + lo_i : nullptr, mode, soft_host ? soft_host + (size_t)lo_i * N : nullptr, soft_kind);
        };
        d->shard_workers[i]->submit(&jobs[i]);
    }
    int rc = LDPC_OK;
    for (int i = 0; i < n; ++i) {
        if (hi[i] <= lo[i]) continue;
        const int r = d->shard_workers[i]->wait(&jobs[i]);     /* all of them, also after a failure */
        if (r && rc == LDPC_OK) { rc = r; ldpc::restore_error(jobs[i].err); }
    }
    if (rc) return rc;
    d->tm.have_last = true;
    d->last_frames = frames;
    return LDPC_OK;
}

}  // namespace

extern "C" {

int ldpc_decode(ldpc_decoder *d, const float *llr_host, int64_t frames, uint8_t *out_host,
                int64_t out_bytes, int32_t *iters)
{
    return decode_entry(d, ldpc::llr_in_float(llr_host), frames, out_host, out_bytes, iters, nullptr, 0);
}

int ldpc_decode_typed(ldpc_decoder *d, const void *llr_host, int32_t llr_type, float llr_unit, int64_t frames,
                      uint8_t *out_host, int64_t out_bytes, int32_t *iters)
{
    return decode_entry(d, ldpc::LlrIn{llr_host, llr_type, llr_unit}, frames, out_host, out_bytes, iters, nullptr, 0);
}

/* ldpc_decode_soft and ldpc_decode_soft_typed */
static int decode_soft_in(ldpc_decoder *d, const ldpc::LlrIn &in, int64_t frames, uint8_t *out_host, int64_t out_bytes,
                          int32_t *iters, float *soft_host, int64_t soft_floats, int32_t soft_kind)
{
    if (!d) return set_error(LDPC_ERR_ARG, "decoder is NULL");
    /* what ldpc_decode_soft_device refuses, before any launch group is staged */
    if (soft_kind != LDPC_SOFT_POSTERIOR && soft_kind != LDPC_SOFT_EXTRINSIC)
        return set_error(LDPC_ERR_ARG, "unknown soft_kind %d", soft_kind);
    if (d->cfg.algo == LDPC_ALGO_SP)
        return set_error(LDPC_ERR_UNSUPPORTED, "soft output: LDPC_ALGO_SP has no usable soft value (include/ldpc_hip.h); "
                    "the min-sum algorithms, LDPC_ALGO_BP and LDPC_ALGO_LAYERED_BP carry it");
    if (d->cfg.algo == LDPC_ALGO_BITFLIP)
        return set_error(LDPC_ERR_UNSUPPORTED, "soft output: LDPC_ALGO_BITFLIP is a hard-decision decoder, its state is one bit per variable");
    if (d->tm.tap_iter) return set_error(LDPC_ERR_STATE, "soft output while a debug tap is set");
    if (frames > 0 && !soft_host) return set_error(LDPC_ERR_ARG, "soft is NULL");
    if (frames > 0 && soft_floats < frames * (int64_t)d->N)
        return set_error(LDPC_ERR_ARG, "soft_floats=%lld < %lld", (long long)soft_floats, (long long)(frames * (int64_t)d->N));
    return decode_entry(d, in, frames, out_host, out_bytes, iters, soft_host, soft_kind);
}

int ldpc_decode_soft(ldpc_decoder *d, const float *llr_host, int64_t frames, uint8_t *out_host, int64_t out_bytes,
                     int32_t *iters, float *soft_host, int64_t soft_floats, int32_t soft_kind)
{
    return decode_soft_in(d, ldpc::llr_in_float(llr_host), frames, out_host, out_bytes, iters, soft_host, soft_floats, soft_kind);
}

int ldpc_decode_soft_typed(ldpc_decoder *d, const void *llr_host, int32_t llr_type, float llr_unit, int64_t frames,
                           uint8_t *out_host, int64_t out_bytes, int32_t *iters, float *soft_host, int64_t soft_floats,
                           int32_t soft_kind)
{
    return decode_soft_in(d, ldpc::LlrIn{llr_host, llr_type, llr_unit}, frames, out_host, out_bytes, iters, soft_host, soft_floats,
                          soft_kind);
}

int ldpc_host_block_plan(uint64_t base, int64_t frames, int32_t N, int32_t max_batch, int64_t group, uint64_t out[6])
{
    if (!out) return set_error(LDPC_ERR_ARG, "out is NULL");
    if (frames <= 0 || N <= 0 || max_batch <= 0 || group < 0 || group * (int64_t)max_batch >= frames)
        return set_error(LDPC_ERR_ARG, "block_plan(frames=%lld, N=%d, max_batch=%d, group=%lld)", (long long)frames, N, max_batch,
                    (long long)group);
    const ldpc::GroupBlocks g = ldpc::plan_group_blocks((uintptr_t)base, frames, N, max_batch, group);
    out[0] = g.s0; out[1] = g.s1; out[2] = g.b0; out[3] = g.b1; out[4] = g.body_end; out[5] = g.whole_by_cpu ? 1 : 0;
    return LDPC_OK;
}

int ldpc_host_locked_ranges(int64_t *live, int64_t *stale)
{
    if (live) *live = (int64_t)ldpc::PageLockRegistry::instance().live_count();
    if (stale) *stale = (int64_t)ldpc::PageLockRegistry::instance().stale_count();
    return LDPC_OK;
}

}  /* extern "C" */
