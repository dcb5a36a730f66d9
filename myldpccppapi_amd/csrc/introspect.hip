/*
 * introspect.hip -- what the C ABI tells about a handle besides decoding with it: the timing spans (the engines record
 * them through span_begin / span_end of decoder.hpp), the statistics of the last call, what the creation-time
 * measurements chose (link form, placement), the array addresses, and the debug taps.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "decoder.hpp"

using ldpc::set_error;

extern "C" {

int ldpc_decoder_set_timing(ldpc_decoder *d, int enable)
{
    if (!d) return set_error(LDPC_ERR_ARG, "decoder is NULL");
    if (!d->shards.empty()) {
        for (ldpc_decoder *sh : d->shards) {
            const int rc = ldpc_decoder_set_timing(sh, enable);
            if (rc) return rc;
        }
        return LDPC_OK;
    }
    if (d->tm.have_last) {   /* events of earlier calls may still be pending */
        LDPC_HIP_TRY(hipSetDevice(d->cfg.device));
        LDPC_HIP_TRY(hipEventSynchronize(d->tm.ev_end.e));
    }
    d->tm.timing_every = enable > 0 ? enable : 0;
    d->tm.timing_calls = 0;
    d->tm.timing = false;
    d->tm.spans_used = 0;
    return LDPC_OK;
}

int ldpc_decoder_stats(ldpc_decoder *d, ldpc_decode_stats *st)
{
    if (!d || !st) return set_error(LDPC_ERR_ARG, "decoder/stats is NULL");
    memset(st, 0, sizeof *st);
    if (!d->tm.have_last) return set_error(LDPC_ERR_STATE, "no decode call to report on");
    if (!d->shards.empty()) {
        /* the devices ran side by side: counts add up, times and iteration numbers take the maximum.
         * Each device's counts cover all launch groups of its range, its times the last group. */
        for (ldpc_decoder *sh : d->shards) {
            if (!sh->tm.have_last) continue;
            ldpc_decode_stats one;
            const int rc = ldpc_decoder_stats(sh, &one);
            if (rc) return rc;
            st->iterations_launched = std::max(st->iterations_launched, one.iterations_launched);
            st->batch_time = std::max(st->batch_time, one.batch_time);
            st->frames += one.frames;
            st->frames_converged += one.frames_converged;
            st->ms_total = std::max(st->ms_total, one.ms_total);
            st->ms_check += one.ms_check; st->ms_var += one.ms_var; st->ms_other += one.ms_other;
            st->launches_check += one.launches_check; st->launches_var += one.launches_var;
            st->frame_rounds += one.frame_rounds;
        }
        return LDPC_OK;
    }
    LDPC_HIP_TRY(hipSetDevice(d->cfg.device));
    LDPC_HIP_TRY(hipEventSynchronize(d->tm.ev_end.e));
    st->iterations_launched = d->last_iterations;
    st->frames = d->last_frames;
    LDPC_HIP_TRY(hipEventElapsedTime(&st->ms_total, d->tm.ev_begin.e, d->tm.ev_end.e));
    int32_t summary[4] = {0, 0, 0, 0};
    LDPC_HIP_TRY(hipMemcpy(summary, d->summary.p, sizeof summary, hipMemcpyDeviceToHost));
    st->batch_time = summary[0];
    st->frames_converged = summary[1];
    /* frame-rounds the message kernels really worked on (tiles that were finished when a round began leave
     * at kernel entry): counted on the device with early termination, all launched rounds without; the
     * one-launch kernels (frames leave individually inside the launch) report 0 */
    st->frame_rounds = 0;
    if (d->engine == ldpc::Engine::Flood) {
        st->frame_rounds = d->cfg.early_term ? (int64_t)summary[2] * d->F
                                             : (int64_t)d->last_iterations * d->last_tiles * d->F;
        for (const ldpc_decoder *p = d->flood.handed_to; p; p = p->flood.handed_to) {      /* the child, and whom it handed over to */
            int32_t cs[4] = {0, 0, 0, 0};
            LDPC_HIP_TRY(hipMemcpy(cs, p->summary.p, sizeof cs, hipMemcpyDeviceToHost));
            st->frame_rounds += (int64_t)cs[2] * p->F;
        }
    }
    if (d->host.call.valid) {            /* a host-buffer call of several launch groups: its counts cover all of them */
        st->iterations_launched = d->host.call.iterations;
        st->batch_time = d->host.call.batch_time;
        st->frames = d->host.call.frames;
        st->frames_converged = d->host.call.converged;
        st->frame_rounds = d->host.call.frame_rounds;
    }
    for (size_t i = 0; i < d->tm.spans_used; ++i) {
        float ms = 0;
        LDPC_HIP_TRY(hipEventElapsedTime(&ms, d->tm.spans[i].a.e, d->tm.spans[i].b.e));
        const int kind = d->tm.spans[i].kind;
        if (kind == 0 || kind == 4 || kind == 5) { st->ms_check += ms; ++st->launches_check; }
        else if (kind == 1 || kind == 2 || kind == 6) { st->ms_var += ms; ++st->launches_var; }
        else st->ms_other += ms;
    }
    return LDPC_OK;
}

int ldpc_decoder_crc_stops(ldpc_decoder *d, int64_t *frames)
{
    if (!d || !frames) return set_error(LDPC_ERR_ARG, "decoder/frames is NULL");
    *frames = 0;
    if (!d->tm.have_last) return set_error(LDPC_ERR_STATE, "no decode call to report on");
    if (!d->shards.empty()) {
        for (ldpc_decoder *sh : d->shards) {
            if (!sh->tm.have_last) continue;
            int64_t one = 0;
            const int rc = ldpc_decoder_crc_stops(sh, &one);
            if (rc) return rc;
            *frames += one;
        }
        return LDPC_OK;
    }
    if (!d->cfg.crc_kind) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(d->cfg.device));
    LDPC_HIP_TRY(hipEventSynchronize(d->tm.ev_end.e));
    if (d->host.call.valid) {            /* a host-buffer call of several launch groups */
        *frames = d->host.call.crc_stops;
        return LDPC_OK;
    }
    /* summary[3] of this decoder and of those its stragglers were handed to, as frame_rounds sums summary[2] */
    for (const ldpc_decoder *p = d; p; p = p->flood.handed_to) {
        int32_t cs[4] = {0, 0, 0, 0};
        LDPC_HIP_TRY(hipMemcpy(cs, p->summary.p, sizeof cs, hipMemcpyDeviceToHost));
        *frames += cs[3];
    }
    return LDPC_OK;
}

int ldpc_decoder_kernel_times(ldpc_decoder *d, ldpc_kernel_time *out, int32_t capacity, int32_t *count)
{
    if (!d || !out || !count || capacity <= 0) return set_error(LDPC_ERR_ARG, "bad arguments");
    *count = 0;
    if (!d->shards.empty()) return ldpc_decoder_kernel_times(d->shards[0], out, capacity, count);
    if (!d->tm.have_last) return set_error(LDPC_ERR_STATE, "no decode call to report on");
    LDPC_HIP_TRY(hipSetDevice(d->cfg.device));
    LDPC_HIP_TRY(hipEventSynchronize(d->tm.ev_end.e));
    /* the half form exists for tiles of 256 frames only: below that the launch takes the narrow kernel (enqueue_check_phase) */
    const int link_form = (d->flood.link_form == 2 && d->V != 4) ? 1 : d->flood.link_form;
    const ldpc::AlgoInfo &a = *ldpc::algo_info(d->cfg.algo);
    const bool layered = a.family == ldpc::Family::Layered;
    /* the fixed-point layered algorithms launch one rule, corrected or not */
    const char *phase_name[] = {"check_kernel", "var_kernel", d->ms_corr && !a.fixed ? "layer_corr_kernel" : "layer_kernel", "other",
                                link_form == 2 ? "check_link_half_kernel"
                                : link_form ? "check_link_narrow_kernel" : "check_link_kernel"};
    /* the arithmetic a streaming kernel was instantiated for: the algorithm's short name, `c` for corrected flooding
     * min-sum (kAlgoMSC), then the message type: none fp32, 16 fp16, 8 fp8, i<q> fixed point of q bits */
    char algo_name[32], suffix[8] = "";
    if (d->flood.msg_kind == LDPC_MSG_I8) snprintf(suffix, sizeof suffix, "i%d", d->flood.msg_bits);
    else if (d->flood.msg_size != 4) snprintf(suffix, sizeof suffix, "%d", d->flood.msg_size == 1 ? 8 : 16);
    snprintf(algo_name, sizeof algo_name, "%s%s%s", a.short_name, d->ms_corr && a.family == ldpc::Family::Flood ? "c" : "", suffix);
    for (size_t i = 0; i < d->tm.spans_used; ++i) {
        const ldpc::TimedSpan &sp = d->tm.spans[i];
        float ms = 0;
        LDPC_HIP_TRY(hipEventElapsedTime(&ms, sp.a.e, sp.b.e));
        const int phase = (sp.kind == 4 || sp.kind == 5) ? 0 : (sp.kind == 6 ? 1 : ((sp.kind == 7 || sp.kind == 8) ? 3 : sp.kind));   /* check / variable node */
        char name[64];
        if (sp.kind == 3) snprintf(name, sizeof name, "other");
        else if (sp.kind == 7) snprintf(name, sizeof name, "soft_settle_kernel");     /* soft calls only */
        else if (sp.kind == 8) snprintf(name, sizeof name, "llr_widen_kernel");       /* typed calls on a one-launch kernel only */
        else if (d->engine == ldpc::Engine::LdspFx)
            snprintf(name, sizeof name, "layered_ldsp_fx_kernel[%dx%d,%d]", d->ldsp.grid, d->ldsp.block, d->ldsp.wg_frames);
        else if (d->engine == ldpc::Engine::Ldsp)   /* whole decode in one launch; [persistent grid x workgroup size, frames per workgroup] */
            snprintf(name, sizeof name, "%s_ldsp%s_kernel[%dx%d,%d]", layered ? "layered" : "flood", d->ms_corr ? "_corr" : "",
                     d->ldsp.grid, d->ldsp.block, d->ldsp.wg_frames);
        else if (d->engine == ldpc::Engine::Fused)      /* bytes = channel values in + packed bits out */
            snprintf(name, sizeof name, "%s", d->cfg.algo == LDPC_ALGO_SP ? "fused_sp_kernel"
                     : layered ? "fused_layered_kernel" : "fused_flood_kernel");
        else if (d->engine == ldpc::Engine::Bitflip)       /* check, and the two passes of the variable phase (degree 1, 2) */
            snprintf(name, sizeof name, "%s", sp.kind == 0 ? "bitflip_check_kernel" : sp.degree == 1 ? "bitflip_vote_kernel" : "bitflip_flip_kernel");
        else if (sp.kind == 5 || sp.kind == 6)
            snprintf(name, sizeof name, "%s<%s,%d-%d,%d>", sp.kind == 5 ? "check_group_kernel" : "var_group_kernel",
                     algo_name, sp.lo, sp.degree, d->V);
        else snprintf(name, sizeof name, "%s<%s,%d,%d>", phase_name[sp.kind], algo_name, sp.degree, d->V);
        int k = 0;
        for (; k < *count; ++k)
            if (!strcmp(out[k].name, name)) break;
        if (k == *count) {
            if (*count == capacity) continue;
            ++*count;
            memset(&out[k], 0, sizeof out[k]);
            out[k].phase = phase;
            out[k].degree = sp.degree;
            memcpy(out[k].name, name, sizeof name);
        }
        ++out[k].launches;
        out[k].ms_total += ms;
        out[k].bytes_total += sp.bytes;
        out[k].bytes_moved += sp.moved;
    }
    return LDPC_OK;
}

int ldpc_decoder_link_form(ldpc_decoder *d, int32_t *form, int32_t *calibrated, float ms[3])
{
    if (!d) return set_error(LDPC_ERR_ARG, "decoder is NULL");
    if (!d->shards.empty()) return ldpc_decoder_link_form(d->shards[0], form, calibrated, ms);
    bool linked = false;
    for (auto &rc : d->flood.row_classes) linked = linked || rc.linked;
    if (form) *form = linked ? d->flood.link_form : -1;
    if (calibrated) *calibrated = d->flood.link_calibrated ? 1 : 0;
    if (ms) for (int k = 0; k < 3; ++k) ms[k] = d->flood.link_calibrated && d->flood.link_cal_ms[k] < 1e29f ? d->flood.link_cal_ms[k] : 0.0f;
    return LDPC_OK;
}

int ldpc_decoder_placement(ldpc_decoder *d, int32_t *candidates, int32_t *kept, float ms[16])
{
    if (!d) return set_error(LDPC_ERR_ARG, "decoder is NULL");
    if (!d->shards.empty()) return ldpc_decoder_placement(d->shards[0], candidates, kept, ms);
    if (candidates) *candidates = d->flood.place_candidates;
    if (kept) *kept = d->flood.place_kept;
    if (ms) for (int k = 0; k < 16; ++k) ms[k] = k < d->flood.place_candidates ? d->flood.place_ms[k] : 0.0f;
    return LDPC_OK;
}

int ldpc_decoder_array_addresses(ldpc_decoder *d, uint64_t out[4])
{
    if (!d || !out) return set_error(LDPC_ERR_ARG, "decoder/out is NULL");
    if (!d->shards.empty()) return ldpc_decoder_array_addresses(d->shards[0], out);
    out[0] = (uint64_t)(uintptr_t)d->flood.Q.p; out[1] = (uint64_t)(uintptr_t)d->flood.R.p;
    out[2] = (uint64_t)(uintptr_t)d->flood.chan.p; out[3] = (uint64_t)(uintptr_t)d->hard.p;
    return LDPC_OK;
}

int ldpc_decoder_set_tap(ldpc_decoder *d, int32_t iter)
{
    if (!d) return set_error(LDPC_ERR_ARG, "decoder is NULL");
    if (iter < 0) return set_error(LDPC_ERR_ARG, "iter < 0");
    if (!d->shards.empty()) return set_error(LDPC_ERR_STATE, "debug taps need a single-device handle");
    d->tm.tap_iter = iter;
    return LDPC_OK;
}

/* an OCP E4M3 byte (1-4-3, bias 7, no infinities, S.1111.111 = NaN) as the float it stands for: exact */
static float e4m3_widen(uint8_t b)
{
    const uint32_t sign = (uint32_t)(b & 0x80) << 24, e = (b >> 3) & 15, m = b & 7;
    uint32_t bits;
    if (e == 15 && m == 7) bits = 0x7fc00000u;
    else if (e == 0) {
        const float sub = (float)m * 0.001953125f;              /* m * 2^-9 */
        memcpy(&bits, &sub, 4);
    } else bits = ((e + 120) << 23) | (m << 20);                /* exponent e - 7 + 127 */
    bits |= sign;
    float out;
    memcpy(&out, &bits, 4);
    return out;
}

int ldpc_decoder_dump(ldpc_decoder *d, int32_t which, float *host_out, int64_t count)
{
    if (!d || !host_out) return set_error(LDPC_ERR_ARG, "decoder/host_out is NULL");
    if (!d->shards.empty()) return set_error(LDPC_ERR_STATE, "debug taps need a single-device handle");
    if (!d->tm.have_last) return set_error(LDPC_ERR_STATE, "no decode call to dump");
    LDPC_HIP_TRY(hipSetDevice(d->cfg.device));
    d->wait_for_own_work();
    const int64_t frames = d->last_frames;
    const int V = d->V, F = d->F;
    const int tiles = (int)((frames + F - 1) / F);
    if (d->engine == ldpc::Engine::Fused && d->cfg.algo == LDPC_ALGO_SP) {
        if (!d->fused.dump_p.p) return set_error(LDPC_ERR_STATE, "fused dump needs set_tap() before the decode");
        const int64_t per = (which == 0 || which == 1) ? d->E : d->N;
        if (which < 0 || which > 3 || count != frames * per) return set_error(LDPC_ERR_ARG, "bad `which`/count");
        if (which == 3) {
            std::vector<uint8_t> b((size_t)count);
            LDPC_HIP_TRY(hipMemcpy(b.data(), d->fused.dump_b.p, (size_t)count, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < count; ++i) host_out[i] = (float)b[i];
            return LDPC_OK;
        }
        const float *src = which == 0 ? d->fused.dump_r.p : (which == 1 ? d->fused.dump_q.p : d->fused.dump_p.p);
        LDPC_HIP_TRY(hipMemcpy(host_out, src, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
        return LDPC_OK;
    }
    if (d->one_launch()) {
        const bool lds_resident = d->engine == ldpc::Engine::Fused;
        const float *dump_r = lds_resident ? d->fused.dump_r.p : d->ldsp.dump_r.p;
        const float *dump_p = lds_resident ? d->fused.dump_p.p : d->ldsp.dump_p.p;
        const float *src = which == 0 ? dump_r : (which == 2 ? dump_p : nullptr);
        const int64_t per = which == 0 ? d->E : d->N;
        if (which == 3) {           /* hard bits = P < 0 */
            if (!dump_p || count != frames * d->N) return set_error(LDPC_ERR_ARG, "fused dump needs set_tap() and count = frames*N");
            LDPC_HIP_TRY(hipMemcpy(host_out, dump_p, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
            const bool notpos = d->cfg.algo == LDPC_ALGO_MS;      /* MS chain: bit = !(p > 0) */
            for (int64_t i = 0; i < count; ++i)
                host_out[i] = (notpos ? !(host_out[i] > 0.0f) : (host_out[i] < 0.0f)) ? 1.0f : 0.0f;
            return LDPC_OK;
        }
        if (!src || count != frames * per) return set_error(LDPC_ERR_ARG, "fused dump: set_tap() first; which in {0,2,3}");
        LDPC_HIP_TRY(hipMemcpy(host_out, src, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
        return LDPC_OK;
    }
    if (d->engine == ldpc::Engine::Bitflip && which == 0) {       /* the syndrome words; which == 3 (bits) is read below */
        hipError_t e = ldpc::bitflip_dump_syndrome(&d->bitflip, host_out, count, frames);
        if (e == hipErrorInvalidValue) return set_error(LDPC_ERR_ARG, "count must be frames*M");
        if (e != hipSuccess) return set_error(LDPC_ERR_HIP, "bit-flipping dump: %s", hipGetErrorString(e));
        return LDPC_OK;
    }
    if (d->engine == ldpc::Engine::Bitflip && which != 3) return set_error(LDPC_ERR_ARG, "LDPC_ALGO_BITFLIP taps: 0 = syndrome words, 3 = bits");
    if (d->engine == ldpc::Engine::Layered) {
        hipError_t e = ldpc::layered_dump(&d->layered, which, host_out, count, frames, d->hard.p,
                                          d->h_cols.data());
        if (e == hipErrorInvalidValue) return set_error(LDPC_ERR_ARG, "bad `which`/count for layered dump");
        if (e != hipSuccess) return set_error(LDPC_ERR_HIP, "layered dump: %s", hipGetErrorString(e));
        return LDPC_OK;
    }
    if (which == 0 || which == 1 || which == 2) {
        const int64_t per = (which == 2) ? d->N : d->E;
        if (count != frames * per) return set_error(LDPC_ERR_ARG, "count must be frames*%lld", (long long)per);
        const uint8_t *src = which == 0 ? d->flood.R.p : (which == 1 ? d->flood.Q.p : d->flood.chan.p);
        const size_t esz = (size_t)d->flood.msg_size;
        std::vector<uint8_t> tile((size_t)per * F * esz);
        for (int t = 0; t < tiles; ++t) {
            LDPC_HIP_TRY(hipMemcpy(tile.data(), src + (size_t)t * per * F * esz, tile.size(), hipMemcpyDeviceToHost));
            for (int fi = 0; fi < F; ++fi) {
                const int64_t f = (int64_t)t * F + fi;
                if (f >= frames) break;
                for (int64_t i = 0; i < per; ++i) {
                    const size_t ir = (which == 1 && !d->flood.h_qpos.empty()) ? (size_t)d->flood.h_qpos[(size_t)i] : (size_t)i;   /* Q: slot of edge i */
                    if (esz == 4) {
                        memcpy(&host_out[f * per + i], &tile[(ir * F + fi) * 4], 4);
                    } else if (esz == 2) {
                        _Float16 h;
                        memcpy(&h, &tile[(ir * F + fi) * 2], 2);
                        host_out[f * per + i] = (float)h;
                    } else if (d->flood.msg_kind == LDPC_MSG_I8) {
                        host_out[f * per + i] = (float)(int8_t)tile[ir * F + fi];
                    } else {
                        host_out[f * per + i] = e4m3_widen(tile[ir * F + fi]);
                    }
                }
            }
        }
        return LDPC_OK;
    }
    if (which == 3) {
        if (count != frames * d->N) return set_error(LDPC_ERR_ARG, "count must be frames*N");
        std::vector<uint64_t> w((size_t)tiles * d->N * V);
        LDPC_HIP_TRY(hipMemcpy(w.data(), d->hard.p, w.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (int64_t f = 0; f < frames; ++f) {
            const int64_t t = f / F;
            const int fi = (int)(f % F);
            for (int32_t n = 0; n < d->N; ++n)
                host_out[f * d->N + n] =
                    (float)((w[((size_t)t * d->N + n) * V + fi % V] >> (fi / V)) & 1ull);
        }
        return LDPC_OK;
    }
    return set_error(LDPC_ERR_ARG, "unknown `which` %d", which);
}

}  /* extern "C" */
