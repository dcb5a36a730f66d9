/*
 * ldpc_hip.hip -- the handle's life behind the C ABI (include/ldpc_hip.h): the calling thread's error message, the
 * graph, ldpc_decoder_create, destruction, decoders over several devices (ldpc_decoder_create_multi: one host thread per
 * device range) and ldpc_decode_device, which hands the call to the engine chosen at creation.
 *
 * ldpc_decoder_create is a sequence: config_in, config_check, the device, the arrays every engine shares, then the walk
 * over engine_candidates with one plan per engine tried (make_plan) and, for the streaming flooding engine, the
 * hand-over child (create_handover_child).  What a configuration means -- accepted struct sizes, the table of
 * algorithms, every refusal in front of the device check, frames per lane, which engines may run it and in what order --
 * is decided in decoder_config_host.hpp, which needs no HIP; this file allocates what was decided there.
 *
 * Not here: the handle itself (decoder.hpp), the engines (engines.hpp: engine_flood / engine_ldsp / engine_fused /
 * engine_layered, each a translation unit that instantiates its kernels; this one launches none), the host-buffer path
 * (host_path.hip), timing, statistics and debug taps (introspect.hip), the entry points that need no decoder
 * (channel.hip: AWGN channel, error counter, HBM probes) and the encoder, rate-matching and modem sections (encoder.hip,
 * ratematch.hip, modem.hip).  What all of them share lives in hip_host.hpp: LDPC_HIP_TRY, the owners of device memory,
 * pinned memory, events and streams (every such resource of the handle and of the engine plans has one, so a handle
 * frees what it took on whichever path it goes) and the declaration of set_error, whose body and message are below.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "decoder.hpp"
#include "graph.hpp"
#include "decoder_config_host.hpp"

using ldpc::set_error;

namespace {

thread_local std::string g_err;

/* the limits config_check quotes are the kernels' own */
static_assert(ldpc::kCfgUnrolledDegree == ldpc::kMaxUnrolledDegree && ldpc::kCfgUnrolledLayerDegree == ldpc::kMaxUnrolledLayerDegree &&
              ldpc::kCfgBitflipDegree == ldpc::kBitflipMaxDegree && ldpc::kCfgBpFracBits == ldpc::kBpFxMaxFracBits,
              "decoder_config_host.hpp quotes a limit its kernel header has changed");
static_assert(sizeof(ldpc_decoder_config::bf_threshold) / sizeof(int32_t) == ldpc::kBitflipThresholds, "bf_threshold[] and kBitflipThresholds");

}  // namespace

/* struct ldpc_graph: graph.hpp (shared with encoder.hip and engine_flood.hip) */

int ldpc::set_error(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

std::string ldpc::last_error_text() { return g_err; }

/* the element type, unit and address of a typed call's channel buffer (include/ldpc_hip.h: enum ldpc_llr_type) */
int ldpc::llr_in_check(const void *p, int32_t type, float unit)
{
    if (type != LDPC_LLR_F32 && type != LDPC_LLR_F16 && type != LDPC_LLR_I8) return set_error(LDPC_ERR_ARG, "unknown llr_type %d", type);
    /* written so that NaN fails it */
    if (!(unit > 0.0f && unit <= 3.402823466e38f)) return set_error(LDPC_ERR_ARG, "llr_unit must be positive and finite");
    if (type == LDPC_LLR_F32 && unit != 1.0f)
        return set_error(LDPC_ERR_ARG, "LDPC_LLR_F32: llr_unit must be exactly 1 (float channel values are read as they are)");
    if (type == LDPC_LLR_F16 && (reinterpret_cast<uintptr_t>(p) & 1)) return set_error(LDPC_ERR_ARG, "llr: fp16 values need 2-byte alignment");
    return LDPC_OK;
}
void ldpc::restore_error(const std::string &text) { g_err = text; }

/* ================================================================== C ABI */

/* set while a decoder creates its tail-compaction child: the child must not create one of its own */
/* 0 while an ordinary decoder is created, 1 for its hand-over child, 2 for the child's own child */
static thread_local int t_child_depth = 0;

extern "C" {

int ldpc_abi_version(void) { return LDPC_HIP_ABI_VERSION; }

const char *ldpc_last_error(void) { return g_err.c_str(); }

int ldpc_device_count(int *count)
{
    if (!count) return set_error(LDPC_ERR_ARG, "count is NULL");
    *count = 0;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return set_error(LDPC_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    *count = n;
    return LDPC_OK;
}

int ldpc_bp_fx_table(int32_t f, int32_t *out, int32_t cap, int32_t *count)
{
    if (!count) return set_error(LDPC_ERR_ARG, "count is NULL");
    *count = 0;
    if (f < 0 || f > ldpc::kBpFxMaxFracBits) return set_error(LDPC_ERR_ARG, "bp_frac_bits=%d must be in [0, %d]", f, ldpc::kBpFxMaxFracBits);
    int32_t t[ldpc::kBpFxTable];
    const int n = ldpc::bp_fx_table_build(f, t, ldpc::kBpFxTable);
    *count = n;
    if (!out) return LDPC_OK;
    if (cap < n) return set_error(LDPC_ERR_ARG, "the table of bp_frac_bits=%d has %d entries, out holds %d", f, n, cap);
    std::copy(t, t + n, out);
    return LDPC_OK;
}

int64_t ldpc_out_bytes(int32_t K, int64_t frames, int32_t pack_mode)
{
    if (frames <= 0 || K <= 0) return 0;
    if (pack_mode == LDPC_PACK_BYTES) return (frames - 1) * (int64_t)K / 8 + K / 8;
    return (frames * (int64_t)K + 7) / 8;
}

int ldpc_graph_create(const int32_t *rows, const int32_t *cols, int64_t E, int32_t M, int32_t N,
                      ldpc_graph **out)
{
    if (!out) return set_error(LDPC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!rows || !cols) return set_error(LDPC_ERR_ARG, "rows/cols is NULL");
    if (M <= 0 || N <= 0 || E <= 0) return set_error(LDPC_ERR_ARG, "M, N, E must be positive");
    if (E > 0x7fffffffLL) return set_error(LDPC_ERR_ARG, "E does not fit int32 edge ids");
    for (int64_t e = 0; e < E; ++e) {
        if (rows[e] < 0 || rows[e] >= M || cols[e] < 0 || cols[e] >= N)
            return set_error(LDPC_ERR_ARG, "edge %lld = (%d, %d) outside %d x %d", (long long)e, rows[e],
                        cols[e], M, N);
        if (e && (rows[e] < rows[e - 1] || (rows[e] == rows[e - 1] && cols[e] <= cols[e - 1])))
            return set_error(LDPC_ERR_ARG, "edges must be in strictly ascending row-major order (edge %lld)",
                        (long long)e);
    }
    ldpc_graph *g = new (std::nothrow) ldpc_graph;
    if (!g) return set_error(LDPC_ERR_NOMEM, "out of memory");
    g->M = M; g->N = N; g->E = E;
    g->rows.assign(rows, rows + E);
    g->cols.assign(cols, cols + E);
    g->row_ptr.assign((size_t)M + 1, 0);
    g->col_ptr.assign((size_t)N + 1, 0);
    for (int64_t e = 0; e < E; ++e) { ++g->row_ptr[rows[e] + 1]; ++g->col_ptr[cols[e] + 1]; }
    for (int32_t m = 0; m < M; ++m) {
        g->max_row_deg = std::max(g->max_row_deg, g->row_ptr[m + 1]);
        g->row_ptr[m + 1] += g->row_ptr[m];
    }
    for (int32_t n = 0; n < N; ++n) {
        g->max_col_deg = std::max(g->max_col_deg, g->col_ptr[n + 1]);
        g->col_ptr[n + 1] += g->col_ptr[n];
    }
    /* column lists in ascending edge id, as the reference's linked lists are
     * appended in edge order (MyLdpc.cpp:209-218) */
    g->col_edge.assign((size_t)E, 0);
    std::vector<int32_t> fill(g->col_ptr.begin(), g->col_ptr.end() - 1);
    for (int64_t e = 0; e < E; ++e) g->col_edge[fill[cols[e]]++] = (int32_t)e;
    *out = g;
    return LDPC_OK;
}

int ldpc_graph_destroy(ldpc_graph *g)
{
    delete g;
    return LDPC_OK;
}

int ldpc_graph_info(const ldpc_graph *g, int32_t *M, int32_t *N, int64_t *E, int32_t *max_row_deg,
                    int32_t *max_col_deg)
{
    if (!g) return set_error(LDPC_ERR_ARG, "graph is NULL");
    if (M) *M = g->M;
    if (N) *N = g->N;
    if (E) *E = g->E;
    if (max_row_deg) *max_row_deg = g->max_row_deg;
    if (max_col_deg) *max_col_deg = g->max_col_deg;
    return LDPC_OK;
}

int ldpc_decoder_config_init_sized(ldpc_decoder_config *cfg, uint32_t struct_size)
{
    if (!cfg) return set_error(LDPC_ERR_ARG, "config is NULL");
    char msg[512];
    if (int rc = ldpc::config_size_check(struct_size, msg, sizeof msg)) return set_error(rc, "%s", msg);
    /* every field that has a non-zero default lies in front of ms_scale */
    memset(cfg, 0, struct_size);
    cfg->struct_size = struct_size;
    cfg->max_batch = 1;
    cfg->algo = LDPC_ALGO_SP;
    cfg->msg_dtype = LDPC_MSG_F32;
    cfg->max_iter = 40;       /* MyLdpc.cpp:24 */
    cfg->llr_scale = 8.0f;    /* decodeCL.c:9 */
    cfg->early_term = 1;
    cfg->pack_mode = LDPC_PACK_BYTES;
    return LDPC_OK;
}

/* the symbol callers built against the header before crc_kind / crc_bits call with their shorter struct (the header's
 * macro of the same name sends callers of this header to the function above with their own size) */
#undef ldpc_decoder_config_init
void ldpc_decoder_config_init(ldpc_decoder_config *cfg)
{
    (void)ldpc_decoder_config_init_sized(cfg, (uint32_t)offsetof(ldpc_decoder_config, crc_kind));
}

/* ---- ldpc_decoder_create: the pieces ---- */

using ldpc::Engine;
using ldpc::Family;

/* the caller's config as the current struct (decoder_config_host.hpp), the refusal as the thread's message */
static int config_in(const ldpc_decoder_config *cfg, ldpc_decoder_config *full)
{
    char msg[512];
    const int rc = ldpc::config_in(cfg, full, msg, sizeof msg);
    return rc ? set_error(rc, "%s", msg) : LDPC_OK;
}

static ldpc::GraphFacts graph_facts(const ldpc_graph *g)
{
    ldpc::GraphFacts f;
    f.M = g->M; f.N = g->N; f.E = g->E;
    f.max_row_deg = g->max_row_deg; f.max_col_deg = g->max_col_deg;
    f.rows_one_weight = true;
    for (int32_t m = 1; m < g->M; ++m)
        if (g->row_ptr[m + 1] - g->row_ptr[m] != g->row_ptr[1] - g->row_ptr[0]) f.rows_one_weight = false;
    return f;
}

/* Tail compaction: with host polling on, the last running frames of a batch of several tiles are finished by a small
 * child decoder (cfg.tune_compact = -1: off, n: threshold), itself made by ldpc_decoder_create one level down. */
static int create_handover_child(ldpc_decoder *d, const ldpc_graph *g)
{
    const ldpc_decoder_config *cfg = &d->cfg;
    /* the child takes over once at most a quarter of the batch still runs: 1024 frames for the 4096-frame
     * batches of the benchmark configurations (rate 9/10, fp16: 681 frames still run after round 5 of 8 and
     * sit in all 16 tiles; a 512-frame child had to wait for round 6), 512 otherwise */
    if (t_child_depth == 0) d->flood.child_capacity = cfg->max_batch >= 4096 ? 2 * ldpc::kCompactCapacity : ldpc::kCompactCapacity;
    else d->flood.child_capacity = cfg->max_batch > ldpc::kCompactCapacity ? ldpc::kCompactCapacity : ldpc::kLastCapacity;
    d->flood.compact_threshold = d->flood.child_capacity;
    if (d->tune.compact) d->flood.compact_threshold = d->tune.compact < 0 ? 0 : std::min(d->flood.child_capacity, d->tune.compact);
    /* the 1024-frame child has a 512-frame child of its own (rate 9/10: of the 681 frames handed over after round 5
     * only 41 still run after round 6, spread over the child's three tiles of 256), and that one a single tile of 64
     * frames (sum-product at 5 dB: a handful of frames in 4096 run all 50 rounds, one in each of its tiles) */
    const bool may_have_child = t_child_depth == 0 || cfg->max_batch > ldpc::kLastCapacity;
    if (!(cfg->early_term && cfg->poll_interval > 0 && d->T > 1 && d->flood.compact_threshold > 0 && may_have_child)) return LDPC_OK;
    ldpc_decoder_config cc = *cfg;
    cc.max_batch = d->flood.child_capacity;
    /* tiles of 64 frames for the 512-frame child (the last few stragglers of a batch); tiles of 256 for the
     * 1024-frame child, which takes over hundreds of frames: dense tiles, 8- / 16-byte accesses */
    cc.frames_per_lane = (d->flood.child_capacity > ldpc::kCompactCapacity && d->V == 4) ? 4 : 1;
    cc.layer_rows = 0;                 /* streaming kernels, same arithmetic */
    cc.tune_compact = d->flood.child_capacity > ldpc::kLastCapacity ? 0 : -1;     /* all but the last hand over once more */
    ++t_child_depth;
    ldpc_decoder *child = nullptr;
    const int rc = ldpc_decoder_create(g, &cc, &child);
    --t_child_depth;
    if (rc) return rc;
    d->flood.child.reset(child);
    d->flood.child->flood.is_child = true;
    LDPC_HIP_TRY(hipSetDevice(cfg->device));
    LDPC_HIP_TRY(d->flood.cmap.alloc((size_t)d->flood.child_capacity));
    LDPC_HIP_TRY(d->flood.cinv.alloc((size_t)d->T * d->F));
    LDPC_HIP_TRY(d->flood.cmoved.alloc((size_t)d->T * d->V));
    return LDPC_OK;
}

/* the saturation limits of the fixed-point layered algorithms: q-bit messages, post_bits-bit posteriors */
static float fx_msg_limit(const ldpc_decoder_config &c) { return (float)((1 << ((c.msg_bits ? c.msg_bits : 8) - 1)) - 1); }
static float fx_post_limit(const ldpc_decoder_config &c) { return (float)((1 << ((c.post_bits ? c.post_bits : 16) - 1)) - 1); }

/* The plan of one candidate engine (decoder_config_host.hpp: engine_candidates).  *taken: the candidate's guard holds and
 * the handle runs this engine; a plan that is not taken is dropped, the next candidate gets its turn. */
static int make_plan(ldpc_decoder *d, const ldpc_graph *g, const ldpc::Candidate &c, size_t TF, bool *taken)
{
    const ldpc_decoder_config *cfg = &d->cfg;
    const ldpc::AlgoInfo &a = *ldpc::algo_info(cfg->algo);
    *taken = true;
    switch (c.engine) {
    case Engine::Bitflip: {
        /* x lives in `hard`; received bits, syndrome words and votes in the plan.  No hand-over child and no
         * device-side tail: a round is too cheap to be worth moving frames for */
        const hipError_t e = ldpc::bitflip_plan_create(&d->bitflip, g->M, g->N, g->E, g->rows, g->col_edge, d->T, cfg->bf_threshold);
        if (e != hipSuccess) return set_error(LDPC_ERR_HIP, "bit-flipping plan allocation failed: %s", hipGetErrorString(e));
        return LDPC_OK;
    }
    case Engine::Ldsp: {
        /* flood_ldsp_kernel / layered_ldsp_kernel (posteriors in LDS, 16-byte check records in cache), the CORR forms with
         * ms_scale / ms_offset.  Layered: 1.2-2.9x the LDS-resident kernel on short codes (exact-width rows, bit-level sign
         * algebra: 800 against 280 G edge updates/s).  Flooding min-sum: 2-2.9x the LDS-resident and the streaming kernels
         * on the 802.16e codes at any batch size, 2.4 / 2.0 / 1.7 / 1.2x the streaming kernels on BG1-profile codes at
         * Z = 64 / 128 / 256 / 384. */
        d->ldsp.corr = d->ms_corr;
        d->ldsp.mc = ldpc::MsCorr{d->ms_scale, d->ms_offset};
        const int flood = a.family == Family::Reference ? 2 : a.family == Family::Flood ? 1 : 0;
        LDPC_HIP_TRY(ldpc::engine_ldsp_plan_create(&d->ldsp, g->M, g->N, g->E, g->row_ptr, g->cols, cfg->layer_rows, cfg->K,
                                                   cfg->max_batch, cfg->device, d->tune, flood));
        *taken = d->ldsp.eligible && (!c.lds_limit || d->ldsp.lds_bytes <= (size_t)ldpc::kCfgLdsLimit);
        if (!*taken) d->ldsp = ldpc::LdspPlan();
        return LDPC_OK;
    }
    case Engine::LdspFx:
        /* layered_ldsp_fx_kernel (int16 posteriors in LDS, 8-byte check records in cache) where the code fits it:
         * quasi-cyclic at layer_rows, rows of at most 24 entries, posteriors within the LDS limit */
        d->ldsp.mc = ldpc::MsCorr{d->ms_scale, d->ms_offset};
        d->ldsp.fx_L = (int32_t)fx_msg_limit(*cfg);
        d->ldsp.fx_LP = (int32_t)fx_post_limit(*cfg);
        LDPC_HIP_TRY(ldpc::engine_ldsp_fx_plan_create(&d->ldsp, g->M, g->N, g->E, g->row_ptr, g->cols, cfg->layer_rows, cfg->K,
                                                      cfg->max_batch, cfg->device, d->tune));
        *taken = d->ldsp.eligible;
        if (!*taken) d->ldsp = ldpc::LdspPlan();
        return LDPC_OK;
    case Engine::Fused:
        /* fused_flood_kernel / fused_sp_kernel / fused_layered_kernel: the same arithmetic in one LDS-resident launch */
        LDPC_HIP_TRY(ldpc::fused_plan_create(&d->fused, g->M, g->N, g->E, g->row_ptr, g->cols, cfg->layer_rows));
        *taken = d->fused.eligible && (!c.needs_sp || d->fused.eligible_sp);
        return LDPC_OK;
    case Engine::Layered: {
        /* the streaming plan and its P / R arrays in HBM: made only when no one-launch kernel was taken */
        ldpc::LayeredPlan &pl = d->layered;
        pl.rule = a.fixed ? (a.box_plus ? ldpc::kLayerBpFx : ldpc::kLayerFx)
                  : a.box_plus ? ldpc::kLayerBp
                  : cfg->algo == LDPC_ALGO_LAYERED_HOST ? ldpc::kLayerHost : d->ms_corr ? ldpc::kLayerCorr : ldpc::kLayerFused;
        if (cfg->algo != LDPC_ALGO_LAYERED) pl.llr_scale = cfg->llr_scale;      /* LDPC_ALGO_LAYERED reads y as it is */
        pl.ms_scale = d->ms_scale;      /* plain min-sum is the corrected row with scale 1, offset 0: the identity on [0, L] */
        pl.ms_offset = d->ms_offset;
        if (a.fixed) { pl.L = fx_msg_limit(*cfg); pl.LP = fx_post_limit(*cfg); }
        if (a.fixed && a.box_plus) {    /* the kernels index the table with |a| + |b| <= 254 and never clamp: zeros behind its last entry */
            int32_t t[ldpc::kBpFxTable];
            const int n = ldpc::bp_fx_table_build(cfg->bp_frac_bits, t, ldpc::kBpFxTable);
            std::vector<uint8_t> bytes((size_t)ldpc::kBpFxTable, 0);
            for (int i = 0; i < n; ++i) bytes[(size_t)i] = (uint8_t)t[i];
            LDPC_HIP_TRY(pl.bp_table.upload(bytes));
        }
        /* a detected QC structure already implies that rows of a layer share no column; here nothing was detected */
        const int rc = ldpc::layered_plan_create(&pl, g->M, g->N, g->E, g->row_ptr, g->cols, cfg->layer_rows, d->T, d->V);
        if (rc == -1) return set_error(LDPC_ERR_ARG, "layer_rows=%d must divide M=%d and rows of a layer "
                                  "must not share a column", cfg->layer_rows, g->M);
        if (rc) return set_error(LDPC_ERR_HIP, "layered plan allocation failed: %s", hipGetErrorString(hipGetLastError()));
        return LDPC_OK;
    }
    case Engine::Flood: {
        /* work lists, kernel tables, launch plan; the column-fused check kernel's form and the arrays' placement are
         * measured there unless the caller says which (engine_flood.hip) */
        if (int rc = ldpc::engine_flood_setup(d, g, TF, t_child_depth == 0)) return rc;
        if (d->flood.tail_enabled) {
            LDPC_HIP_TRY(d->flood.tail_state.alloc(4));
            LDPC_HIP_TRY(d->flood.tail_map.alloc((size_t)d->flood.TO * d->F));
            LDPC_HIP_TRY(d->flood.running.alloc((size_t)cfg->max_iter + 2));
        }
        return create_handover_child(d, g);
    }
    }
    return set_error(LDPC_ERR_STATE, "unknown engine");
}

int ldpc_decoder_create(const ldpc_graph *g, const ldpc_decoder_config *cfg_in, ldpc_decoder **out)
{
    if (!out) return set_error(LDPC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!g || !cfg_in) return set_error(LDPC_ERR_ARG, "graph/config is NULL");
    ldpc_decoder_config cfg_full;
    if (int rc = config_in(cfg_in, &cfg_full)) return rc;
    const ldpc_decoder_config *cfg = &cfg_full;
    const ldpc::GraphFacts facts = graph_facts(g);
    {
        char msg[512];
        if (int rc = ldpc::config_check(*cfg, facts, msg, sizeof msg)) return set_error(rc, "%s", msg);
    }
    const ldpc::AlgoInfo &a = *ldpc::algo_info(cfg->algo);

    int ndev = 0;
    LDPC_HIP_TRY(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev)
        return set_error(LDPC_ERR_HIP, "device %d not present (%d HIP devices)", cfg->device, ndev);
    LDPC_HIP_TRY(hipSetDevice(cfg->device));

    /* the arrays and choices every engine shares */
    ldpc_decoder *d = new (std::nothrow) ldpc_decoder;
    if (!d) return set_error(LDPC_ERR_NOMEM, "out of memory");
    std::unique_ptr<ldpc_decoder> guard(d);
    d->cfg = *cfg;
    d->ms_corr = ldpc::has_ms_corr(*cfg);
    d->ms_scale = cfg->ms_scale != 0.0f ? cfg->ms_scale : 1.0f;
    d->ms_offset = cfg->ms_offset;
    d->M = g->M; d->N = g->N; d->E = g->E;
    d->h_cols = g->cols;
    const ldpc::Tune tune = d->tune = ldpc::tune_from_config(*cfg);
    d->flood.syn_xcd = ldpc::tune_pick(tune.syn_xcd, true);
    /* one-byte messages (fp8 and fixed point alike): the forms that move a dword per lane at V = 4 are the automatic choice -- check kernels in wide waves
     * where every row has one (degree <= kMaxUnrolledDegree; above, the bucket launches, V values per lane), the
     * column-fused kernel wide unless the creation-time measurement prefers the half form.  The narrow forms move one
     * byte per lane; the tuning fields still select them, results never depend on the choice. */
    const bool f8 = ldpc::one_byte_messages(*cfg);
    d->flood.check_wide = ldpc::tune_pick(tune.check_wide, f8 && g->max_row_deg <= ldpc::kMaxUnrolledDegree);
    d->flood.link_form = ldpc::tune_pick(tune.link_half, false) ? 2 : (ldpc::tune_pick(tune.link_narrow, !f8 || ldpc::tune_forced_on(tune.link_deep)) ? 1 : 0);   /* deep is a narrow form */
    d->flood.link_deep = ldpc::tune_pick(tune.link_deep, false);
    if (tune.link_rows) d->flood.link_rpw = tune.link_rows < 0 ? 0 : tune.link_rows;
    LDPC_HIP_TRY(hipDeviceGetAttribute(&d->flood.cus, hipDeviceAttributeMultiprocessorCount, cfg->device));
    d->V = a.family == Family::Bitflip ? 1 : ldpc::pick_frames_per_lane(*cfg, g->max_row_deg, g->max_col_deg);       /* bit flipping: a word is 64 frames */
    d->F = 64 * d->V;
    d->T = (cfg->max_batch + d->F - 1) / d->F;
    /* a single tile is latency-bound (one wave walks its rows one after the other): shorter row
     * chunks per wave, 4.1 -> 3.4 ms for one 50-iteration decode of the (64800, 32400) code */
    if (d->T == 1 && !tune.link_rows) d->flood.link_rpw = 4;

    LDPC_HIP_TRY(d->stream.create());
    LDPC_HIP_TRY(d->tm.ev_begin.create());
    LDPC_HIP_TRY(d->tm.ev_end.create());
    LDPC_HIP_TRY(d->flood.h_active.alloc(1));
    LDPC_HIP_TRY(d->flood.h_summary.alloc(2));
    LDPC_HIP_TRY(d->flood.ev_summary.create(false));
    LDPC_HIP_TRY(d->row_ptr.upload(g->row_ptr));
    LDPC_HIP_TRY(d->edge_col.upload(g->cols));
    LDPC_HIP_TRY(d->col_ptr.upload(g->col_ptr));
    LDPC_HIP_TRY(d->col_edge.upload(g->col_edge));
    /* Device-side tail: for asynchronous callers (poll_interval == 0) of the streaming flooding kernels
     * with early termination, when the batch has clearly more tiles than the overflow area.
     * LDPC_TUNE_OFF(LDPC_TUNE_DEVICE_TAIL) switches it off. */
    d->flood.TO = (ldpc::kCompactCapacity + d->F - 1) / d->F;
    d->flood.tail_enabled = cfg->early_term && cfg->poll_interval == 0 && ldpc::tune_pick(tune.device_tail, true) &&
                      a.handover && d->T >= 4 * d->flood.TO && t_child_depth == 0;
    if (!d->flood.tail_enabled) d->flood.TO = 0;
    d->flood.TA = d->T + d->flood.TO;
    const size_t TF = (size_t)d->flood.TA * d->F;
    LDPC_HIP_TRY(d->hard.alloc((size_t)d->flood.TA * d->N * d->V));
    LDPC_HIP_TRY(d->failw.alloc((size_t)(cfg->max_iter + 2) * d->flood.TA * d->V));
    LDPC_HIP_TRY(d->done.alloc((size_t)d->flood.TA * d->V));
    LDPC_HIP_TRY(d->iters.alloc(TF));
    LDPC_HIP_TRY(d->active.alloc(1));
    LDPC_HIP_TRY(d->summary.alloc(4));
    if (cfg->crc_kind) {
        std::vector<uint32_t> w((size_t)cfg->crc_bits);
        ldpc::crc_term_weights(cfg->crc_kind, cfg->crc_bits, w.data());
        LDPC_HIP_TRY(d->crc_w.upload(w));
    }

    /* the first candidate engine whose plan takes the code runs it */
    const ldpc::Candidates cand = ldpc::engine_candidates(*cfg, facts, tune);
    if (cand.code) return set_error(cand.code, "%s", cand.refusal);
    bool taken = false;
    for (int k = 0; k < cand.n && !taken; ++k) {
        if (int rc = make_plan(d, g, cand.c[k], TF, &taken)) return rc;
        if (taken) d->engine = cand.c[k].engine;
    }
    if (!taken)         /* only LDPC_ALGO_MS_FUSED has no streaming engine behind its one-launch kernels */
        return set_error(LDPC_ERR_UNSUPPORTED, "MS_FUSED needs a quasi-cyclic H (circulant size = layer_rows) whose "
                    "posteriors fit in LDS");
    *out = guard.release();
    return LDPC_OK;
}

int ldpc_decoder_destroy(ldpc_decoder *d)
{
    if (!d) return LDPC_OK;
    /* blocks of caller memory an LDPC_HOST_INPUT_LOCK_PAGES call could not release: said loudly, here too */
    size_t stuck = d->host.stuck_blocks.size() + d->host.locked_blocks.size();
    for (ldpc_decoder *sh : d->shards) stuck += sh->host.stuck_blocks.size() + sh->host.locked_blocks.size();
    delete d;            /* joins the handle's threads, drains its streams; a multi-device handle destroys its per-device decoders */
    if (stuck) {
        fprintf(stderr, "ldpc_decoder_destroy: %zu page-locked block(s) of caller memory were never released\n", stuck);
        return set_error(LDPC_ERR_STATE, "%zu page-locked block(s) of caller memory could not be released "
                    "(hipHostUnregister failed in an earlier ldpc_decode)", stuck);
    }
    return LDPC_OK;
}

int ldpc_shard_range(int64_t frames, int32_t part, int32_t parts, int32_t unit, int64_t *lo, int64_t *hi)
{
    if (!lo || !hi) return set_error(LDPC_ERR_ARG, "lo/hi is NULL");
    if (frames < 0 || parts <= 0 || part < 0 || part >= parts || unit <= 0)
        return set_error(LDPC_ERR_ARG, "shard_range(frames=%lld, part=%d, parts=%d, unit=%d)", (long long)frames, part, parts, unit);
    const int64_t nu = (frames + unit - 1) / unit, base = nu / parts, rem = nu % parts;
    const int64_t lo_u = part * base + std::min<int64_t>(part, rem);
    const int64_t hi_u = lo_u + base + (part < rem ? 1 : 0);
    *lo = std::min(lo_u * unit, frames);
    *hi = std::min(hi_u * unit, frames);
    return LDPC_OK;
}

int ldpc_decoder_create_multi(const ldpc_graph *g, const ldpc_decoder_config *cfg, const int32_t *devices,
                              int32_t n_devices, ldpc_decoder **out)
{
    if (!out) return set_error(LDPC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!g || !cfg) return set_error(LDPC_ERR_ARG, "graph/config is NULL");
    if (!devices || n_devices <= 0 || n_devices > 64) return set_error(LDPC_ERR_ARG, "devices[] must hold 1..64 ordinals");
    ldpc_decoder_config cfg_full;
    if (int rc = config_in(cfg, &cfg_full)) return rc;
    cfg = &cfg_full;
    ldpc_decoder *grp = new (std::nothrow) ldpc_decoder;
    if (!grp) return set_error(LDPC_ERR_NOMEM, "out of memory");
    std::unique_ptr<ldpc_decoder> guard(grp);
    for (int32_t i = 0; i < n_devices; ++i) {
        ldpc_decoder_config c = *cfg;
        c.device = devices[i];
        ldpc_decoder *sh = nullptr;
        const int rc = ldpc_decoder_create(g, &c, &sh);
        if (rc) return rc;                       /* the guard destroys the shards made so far */
        grp->shards.push_back(sh);
        /* the host thread that runs this device's frame range in every ldpc_decode of the handle */
        grp->shard_workers.emplace_back(new (std::nothrow) ldpc::Worker(ldpc::last_error_text));
        if (!grp->shard_workers.back() || !grp->shard_workers.back()->start())
            return set_error(LDPC_ERR_NOMEM, "cannot start the host thread of device-list entry %d", i);
    }
    grp->cfg = *cfg;
    grp->cfg.device = devices[0];
    grp->M = g->M; grp->N = g->N; grp->E = g->E;
    *out = guard.release();
    return LDPC_OK;
}

/* ldpc_decode_device and ldpc_decode_typed_device: `in` has passed ldpc::llr_in_check */
static int decode_device_in(ldpc_decoder *d, const ldpc::LlrIn &in, int64_t frames, uint8_t *out_dev,
                            int64_t out_bytes, int32_t *iters_dev, void *stream)
{
    if (!d) return set_error(LDPC_ERR_ARG, "decoder is NULL");
    if (!d->shards.empty())
        return set_error(LDPC_ERR_STATE, "a multi-device handle decodes host buffers only (ldpc_decode): device "
                    "pointers belong to one device");
    if (frames < 0 || frames > d->cfg.max_batch)
        return set_error(LDPC_ERR_ARG, "frames=%lld outside [0, max_batch=%d]", (long long)frames,
                    d->cfg.max_batch);
    if (out_bytes < 0) return set_error(LDPC_ERR_ARG, "out_bytes < 0");
    if (frames == 0) { d->last_frames = 0; d->tm.have_last = false; return LDPC_OK; }
    if (!in.p) return set_error(LDPC_ERR_ARG, "llr is NULL");
    const int64_t need = ldpc_out_bytes(d->cfg.K, frames, d->cfg.pack_mode);
    /* bytes this call may store: none without out_dev (iteration counts and stats only) */
    const int64_t room = out_dev ? std::min(out_bytes, need) : 0;
    if (out_dev && out_bytes < need && d->cfg.pack_mode == LDPC_PACK_BITS)
        return set_error(LDPC_ERR_ARG, "out_bytes=%lld < %lld", (long long)out_bytes, (long long)need);
    LDPC_HIP_TRY(hipSetDevice(d->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    d->tm.timing = d->tm.timing_every > 0 && (d->tm.timing_calls++ % d->tm.timing_every) == 0;
    d->tm.last_stream = s;
    d->last_frames = frames;
    d->host.call.valid = false;          /* ldpc_decode() sets it again once all its groups are in */
    LDPC_HIP_TRY(hipEventRecord(d->tm.ev_begin.e, s));
    /* gaps between frames (K % 8 != 0, decodeCL.c:191-192 leaves them alone) read as 0 */
    if (out_dev) LDPC_HIP_TRY(hipMemsetAsync(out_dev, 0, (size_t)room, s));
    int rc = LDPC_OK;
    /* what the streaming engines that work on the handle's own arrays are handed (engines.hpp: StreamRun) */
    auto fill = [&](ldpc::StreamRun &run) {
        run.span_begin = [](void *c, hipStream_t st, int kind, int deg, int64_t bytes) {
            return ldpc::span_begin((ldpc_decoder *)c, st, kind, deg, bytes);
        };
        run.span_end = [](void *c, hipStream_t st) { return ldpc::span_end((ldpc_decoder *)c, st); };
        run.span_ctx = d;
        run.llr = in; run.frames = frames; run.out_dev = out_dev;
        run.out_bytes = room; run.iters_dev = iters_dev;
        run.K = d->cfg.K; run.max_iter = d->cfg.max_iter; run.tap_iter = d->tm.tap_iter;
        run.early_term = d->cfg.early_term; run.pack_mode = d->cfg.pack_mode;
        run.hard = d->hard.p; run.failw = d->failw.p; run.done = d->done.p; run.iters = d->iters.p;
        run.row_ptr = d->row_ptr.p; run.edge_col = d->edge_col.p; run.summary = d->summary.p;
        run.crc_w = d->crc_w.p; run.crc_bits = d->cfg.crc_kind ? d->cfg.crc_bits : 0;
    };
    switch (d->engine) {
    case Engine::Fused:
    case Engine::Ldsp:
    case Engine::LdspFx: {
        /* the one-launch and record kernels read floats: a typed call widens into the handle's own buffer first, made by
         * the handle's first typed call (a plain call launches and moves what it always did) */
        const float *llr_dev = static_cast<const float *>(in.p);
        if (in.type != LDPC_LLR_F32) {
            LDPC_HIP_TRY(d->llr_wide.ensure((size_t)d->cfg.max_batch * d->N));
            hipError_t e = ldpc::span_begin(d, s, 8, 0, frames * (int64_t)d->N * (int64_t)(4 + ldpc::llr_elem_size(in.type)));
            if (e == hipSuccess) e = ldpc::engine_llr_widen(in, d->llr_wide.p, frames * (int64_t)d->N, s);
            if (e == hipSuccess) e = ldpc::span_end(d, s);
            if (e != hipSuccess) return set_error(LDPC_ERR_HIP, "widening the channel values: %s", hipGetErrorString(e));
            llr_dev = d->llr_wide.p;
        }
        ldpc::FusedRun run{llr_dev, frames, out_dev, room, iters_dev, d->cfg.K,
                           d->cfg.max_iter, d->tm.tap_iter, d->cfg.early_term, d->summary.p,
                           d->cfg.algo == LDPC_ALGO_MS_FUSED ? 1 : (d->cfg.algo == LDPC_ALGO_MS ? 2 : (d->cfg.algo == LDPC_ALGO_SP ? 3 : 0)),
                           d->cfg.llr_scale, ldpc::tune_pick(d->tune.fused_loop, false) ? 1 : 0,
                           ldpc::tune_pick(d->tune.fused_pack, true) ? 0 : 1};
        run.soft = d->soft.dst;
        run.soft_extrinsic = d->soft.kind == LDPC_SOFT_EXTRINSIC ? 1 : 0;
        hipError_t e = ldpc::span_begin(d, s, 2, 0, (int64_t)frames * (4 * d->N + d->cfg.K / 8));
        if (e == hipSuccess)
            e = d->engine == Engine::Fused ? ldpc::engine_fused_run(&d->fused, run, s, &d->last_iterations)
                : d->engine == Engine::LdspFx ? ldpc::engine_ldsp_fx_run(&d->ldsp, run, s, &d->last_iterations)
                                              : ldpc::engine_ldsp_run(&d->ldsp, run, s, &d->last_iterations);
        if (e == hipSuccess) e = ldpc::span_end(d, s);
        if (e != hipSuccess) rc = set_error(LDPC_ERR_HIP, "fused decode: %s", hipGetErrorString(e));
        break;
    }
    case Engine::Layered: {
        ldpc::LayeredRun run;
        fill(run);
        run.soft = d->soft.dst; run.soft_extrinsic = d->soft.kind == LDPC_SOFT_EXTRINSIC ? 1 : 0;
        const hipError_t e = ldpc::engine_layered_run(&d->layered, run, s, &d->last_iterations);
        if (e != hipSuccess) rc = set_error(LDPC_ERR_HIP, "layered decode: %s", hipGetErrorString(e));
        break;
    }
    case Engine::Bitflip: {
        ldpc::BitflipRun run;
        fill(run);
        run.col_ptr = d->col_ptr.p;
        const hipError_t e = ldpc::engine_bitflip_run(&d->bitflip, run, s, &d->last_iterations);
        if (e != hipSuccess) rc = set_error(LDPC_ERR_HIP, "bit-flipping decode: %s", hipGetErrorString(e));
        break;
    }
    case Engine::Flood:
        rc = ldpc::engine_flood_run(d, in, frames, out_dev, room, iters_dev, s);
        break;
    }
    if (rc) return rc;
    LDPC_HIP_TRY(hipEventRecord(d->tm.ev_end.e, s));
    d->tm.have_last = true;
    return LDPC_OK;
}

int ldpc_decode_device(ldpc_decoder *d, const float *llr_dev, int64_t frames, uint8_t *out_dev,
                       int64_t out_bytes, int32_t *iters_dev, void *stream)
{
    return decode_device_in(d, ldpc::llr_in_float(llr_dev), frames, out_dev, out_bytes, iters_dev, stream);
}

int ldpc_decode_typed_device(ldpc_decoder *d, const void *llr_dev, int32_t llr_type, float llr_unit, int64_t frames,
                             uint8_t *out_dev, int64_t out_bytes, int32_t *iters_dev, void *stream)
{
    if (int rc = ldpc::llr_in_check(llr_dev, llr_type, llr_unit)) return rc;
    return decode_device_in(d, ldpc::LlrIn{llr_dev, llr_type, llr_unit}, frames, out_dev, out_bytes, iters_dev, stream);
}

/* ldpc_decode_soft_device and ldpc_decode_soft_typed_device */
static int decode_soft_device_in(ldpc_decoder *d, const ldpc::LlrIn &in, int64_t frames, uint8_t *out_dev, int64_t out_bytes,
                                 int32_t *iters_dev, float *soft_dev, int64_t soft_floats, int32_t soft_kind, void *stream)
{
    if (!d) return set_error(LDPC_ERR_ARG, "decoder is NULL");
    if (!d->shards.empty())
        return set_error(LDPC_ERR_STATE, "a multi-device handle decodes host buffers only (ldpc_decode_soft): device "
                    "pointers belong to one device");
    if (soft_kind != LDPC_SOFT_POSTERIOR && soft_kind != LDPC_SOFT_EXTRINSIC)
        return set_error(LDPC_ERR_ARG, "unknown soft_kind %d", soft_kind);
    if (d->cfg.algo == LDPC_ALGO_SP)
        return set_error(LDPC_ERR_UNSUPPORTED, "soft output: LDPC_ALGO_SP works in the probability domain in fp32, where the "
                    "posterior saturates to exactly +-1 on nearly every bit of a frame that converges and is 0/0 on frames "
                    "that do not; the min-sum algorithms (MS, MS_FUSED, LAYERED, LAYERED_HOST) and the log-domain LDPC_ALGO_BP / LDPC_ALGO_LAYERED_BP carry it");
    if (d->cfg.algo == LDPC_ALGO_BITFLIP)
        return set_error(LDPC_ERR_UNSUPPORTED, "soft output: LDPC_ALGO_BITFLIP is a hard-decision decoder, its state is one bit per variable");
    if (d->tm.tap_iter)
        return set_error(LDPC_ERR_STATE, "soft output while a debug tap is set (ldpc_decoder_set_tap(d, 0) clears it)");
    if (frames < 0 || frames > d->cfg.max_batch)
        return set_error(LDPC_ERR_ARG, "frames=%lld outside [0, max_batch=%d]", (long long)frames, d->cfg.max_batch);
    if (frames > 0) {
        if (!soft_dev) return set_error(LDPC_ERR_ARG, "soft is NULL");
        if (reinterpret_cast<uintptr_t>(soft_dev) & 3) return set_error(LDPC_ERR_ARG, "soft is not 4-byte aligned");
        const int64_t need = frames * (int64_t)d->N;
        if (soft_floats < need) return set_error(LDPC_ERR_ARG, "soft_floats=%lld < %lld", (long long)soft_floats, (long long)need);
        const uintptr_t l0 = reinterpret_cast<uintptr_t>(in.p), l1 = l0 + (uintptr_t)need * ldpc::llr_elem_size(in.type);
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(soft_dev), s1 = s0 + (uintptr_t)need * sizeof(float);
        if (in.p && s0 < l1 && l0 < s1)
            return set_error(LDPC_ERR_ARG, "soft overlaps llr: the channel values are read while soft values are written");
    }
    /* the plain entry point does the rest; the request lives on the handle for exactly this call */
    d->soft = ldpc::SoftReq{frames > 0 ? soft_dev : nullptr, soft_kind, nullptr};
    const int rc = decode_device_in(d, in, frames, out_dev, out_bytes, iters_dev, stream);
    d->soft = ldpc::SoftReq{};
    return rc;
}

int ldpc_decode_soft_device(ldpc_decoder *d, const float *llr_dev, int64_t frames, uint8_t *out_dev, int64_t out_bytes,
                            int32_t *iters_dev, float *soft_dev, int64_t soft_floats, int32_t soft_kind, void *stream)
{
    return decode_soft_device_in(d, ldpc::llr_in_float(llr_dev), frames, out_dev, out_bytes, iters_dev, soft_dev, soft_floats,
                                 soft_kind, stream);
}

int ldpc_decode_soft_typed_device(ldpc_decoder *d, const void *llr_dev, int32_t llr_type, float llr_unit, int64_t frames,
                                  uint8_t *out_dev, int64_t out_bytes, int32_t *iters_dev, float *soft_dev, int64_t soft_floats,
                                  int32_t soft_kind, void *stream)
{
    if (int rc = ldpc::llr_in_check(llr_dev, llr_type, llr_unit)) return rc;
    return decode_soft_device_in(d, ldpc::LlrIn{llr_dev, llr_type, llr_unit}, frames, out_dev, out_bytes, iters_dev, soft_dev,
                                 soft_floats, soft_kind, stream);
}

}  /* extern "C" */
