/*
 * ldpc_hip.hip -- the handle's life behind the C ABI (include/ldpc_hip.h): the calling thread's error message, the
 * graph, config validation, ldpc_decoder_create with its choice of engine and the tail-compaction child, destruction,
 * decoders over several devices (ldpc_decoder_create_multi: one host thread per device range) and ldpc_decode_device,
 * which hands the call to the engine chosen at creation.
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
#include "crc_term_host.hpp"

using ldpc::set_error;

namespace {

thread_local std::string g_err;

int pick_frames_per_lane(const ldpc_decoder_config &cfg, int32_t max_row_deg, int32_t max_col_deg)
{
    if (cfg.frames_per_lane) return cfg.frames_per_lane;
    /* Wide tiles (4 values = 16 B fp32 / 8 B fp16 per lane) once there are enough frames to
     * fill them and the register arrays of the unrolled kernels stay moderate.  Flooding check
     * kernels run in narrow waves, so only the column degree counts there; the layered kernel
     * holds a whole row (P and R) per lane. */
    int deg = (cfg.algo == LDPC_ALGO_LAYERED || cfg.algo == LDPC_ALGO_LAYERED_BP) ? max_row_deg : max_col_deg;
    /* fixed-point layered: a row's R is a dword and its P a dwordx2 per lane at 4 frames per lane, whatever the row degree
     * (the unrolled kernels hold the row in registers up to degree 24, the run-time kernel holds none of it) */
    if (cfg.algo == LDPC_ALGO_LAYERED_FX || cfg.algo == LDPC_ALGO_LAYERED_BP_FX) return cfg.max_batch >= 256 ? 4 : 1;
    if (cfg.algo == LDPC_ALGO_MS || cfg.algo == LDPC_ALGO_BP) deg = (deg + 1) / 2;   /* min-sum variable nodes (BP's too) need half the registers */
    /* one-byte messages (fp8, fixed point): 4 values are one dword per lane, the least a lane should move -- from one full tile on */
    if ((cfg.msg_dtype == LDPC_MSG_F8 || cfg.msg_dtype == LDPC_MSG_I8) && cfg.max_batch >= 256 && deg <= 8) return 4;
    if (cfg.max_batch >= 1024 && deg <= 8) return 4;
    if (cfg.max_batch >= 256 && deg <= ldpc::kMaxUnrolledDegree) return 2;
    return 1;
}

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
    if (struct_size != sizeof(ldpc_decoder_config) && struct_size != offsetof(ldpc_decoder_config, bf_threshold) &&
        struct_size != offsetof(ldpc_decoder_config, msg_bits) &&
        struct_size != offsetof(ldpc_decoder_config, crc_kind) && struct_size != offsetof(ldpc_decoder_config, ms_scale))
        return set_error(LDPC_ERR_ARG, "config struct_size %u is none of %zu, %zu, %zu, %zu, %zu (ABI mismatch)", struct_size,
                    sizeof(ldpc_decoder_config), offsetof(ldpc_decoder_config, bf_threshold), offsetof(ldpc_decoder_config, msg_bits),
                    offsetof(ldpc_decoder_config, crc_kind), offsetof(ldpc_decoder_config, ms_scale));
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

/* The caller's config as the current struct: callers built against the header before ms_scale / ms_offset, before
 * crc_kind / crc_bits, before msg_bits or before bf_threshold pass a shorter struct, of which only struct_size bytes are
 * read; the fields it lacks are 0 (off; msg_bits: 8; bf_threshold: the default schedule). */
static int config_in(const ldpc_decoder_config *cfg, ldpc_decoder_config *full)
{
    constexpr size_t kSizeBeforeMsCorr = offsetof(ldpc_decoder_config, ms_scale);
    constexpr size_t kSizeBeforeCrc = offsetof(ldpc_decoder_config, crc_kind);
    constexpr size_t kSizeBeforeMsgBits = offsetof(ldpc_decoder_config, msg_bits);
    constexpr size_t kSizeBeforeBitflip = offsetof(ldpc_decoder_config, bf_threshold);
    if (cfg->struct_size != sizeof(ldpc_decoder_config) && cfg->struct_size != kSizeBeforeBitflip && cfg->struct_size != kSizeBeforeMsgBits &&
        cfg->struct_size != kSizeBeforeCrc && cfg->struct_size != kSizeBeforeMsCorr)
        return set_error(LDPC_ERR_ARG, "config struct_size %u is none of %zu, %zu, %zu, %zu, %zu (ABI mismatch)", cfg->struct_size,
                    sizeof(ldpc_decoder_config), kSizeBeforeBitflip, kSizeBeforeMsgBits, kSizeBeforeCrc, kSizeBeforeMsCorr);
    memset(full, 0, sizeof *full);
    memcpy(full, cfg, cfg->struct_size);
    full->struct_size = sizeof *full;
    return LDPC_OK;
}

int ldpc_decoder_create(const ldpc_graph *g, const ldpc_decoder_config *cfg_in, ldpc_decoder **out)
{
    if (!out) return set_error(LDPC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!g || !cfg_in) return set_error(LDPC_ERR_ARG, "graph/config is NULL");
    ldpc_decoder_config cfg_full;
    if (int rc = config_in(cfg_in, &cfg_full)) return rc;
    const ldpc_decoder_config *cfg = &cfg_full;
    if (cfg->K <= 0 || cfg->K > g->N) return set_error(LDPC_ERR_ARG, "K=%d out of range", cfg->K);
    if (cfg->max_batch <= 0) return set_error(LDPC_ERR_ARG, "max_batch must be positive");
    if (cfg->max_iter <= 0 || cfg->max_iter > 100000) return set_error(LDPC_ERR_ARG, "max_iter out of range");
    if (cfg->algo != LDPC_ALGO_SP && cfg->algo != LDPC_ALGO_MS && cfg->algo != LDPC_ALGO_LAYERED &&
        cfg->algo != LDPC_ALGO_MS_FUSED && cfg->algo != LDPC_ALGO_LAYERED_HOST && cfg->algo != LDPC_ALGO_BP &&
        cfg->algo != LDPC_ALGO_LAYERED_BP && cfg->algo != LDPC_ALGO_LAYERED_FX && cfg->algo != LDPC_ALGO_LAYERED_BP_FX &&
        cfg->algo != LDPC_ALGO_BITFLIP)
        return set_error(LDPC_ERR_ARG, "unknown algo %d", cfg->algo);
    const bool bitflip = cfg->algo == LDPC_ALGO_BITFLIP;
    const bool bpfx = cfg->algo == LDPC_ALGO_LAYERED_BP_FX;     /* LAYERED_FX's configuration, storage and schedule, another row */
    const bool fx = cfg->algo == LDPC_ALGO_LAYERED_FX || bpfx;
    const char *const fx_name = bpfx ? "LDPC_ALGO_LAYERED_BP_FX" : "LDPC_ALGO_LAYERED_FX";
    /* comparisons written so that NaN fails them */
    if (!(cfg->ms_scale >= 0.0f && cfg->ms_scale <= 1.0f))
        return set_error(LDPC_ERR_ARG, "ms_scale must be 0 (off) or in (0, 1]");
    if (!(cfg->ms_offset >= 0.0f && cfg->ms_offset < 1000.0f))
        return set_error(LDPC_ERR_ARG, "ms_offset must be 0 (off) or in (0, 1000)");
    const bool ms_corr = cfg->ms_scale != 0.0f || cfg->ms_offset != 0.0f;
    if (ms_corr && cfg->algo != LDPC_ALGO_MS && cfg->algo != LDPC_ALGO_LAYERED && !(fx && !bpfx))
        return set_error(LDPC_ERR_UNSUPPORTED, "ms_scale / ms_offset apply to LDPC_ALGO_MS and LDPC_ALGO_LAYERED only "
                    "(SP, BP, LAYERED_BP, LAYERED_BP_FX and BITFLIP have no minimum to correct; MS_FUSED and LAYERED_HOST reproduce reference kernels)");
    const bool bp_row = cfg->algo == LDPC_ALGO_BP || cfg->algo == LDPC_ALGO_LAYERED_BP;      /* box-plus check node */
    if (bp_row && !(cfg->llr_scale > 0.0f && cfg->llr_scale <= 3.402823466e38f))
        return set_error(LDPC_ERR_ARG, "%s: llr_scale must be positive and finite (chan = llr_scale * y is the LLR)",
                    cfg->algo == LDPC_ALGO_BP ? "LDPC_ALGO_BP" : "LDPC_ALGO_LAYERED_BP");
    if (cfg->algo == LDPC_ALGO_LAYERED_BP && (cfg->layer_rows <= 0 || g->M % cfg->layer_rows))
        return set_error(LDPC_ERR_ARG, "LDPC_ALGO_LAYERED_BP: layer_rows=%d must be positive and divide M=%d", cfg->layer_rows, g->M);
    if (cfg->algo == LDPC_ALGO_LAYERED_HOST) {
        for (int32_t m = 1; m < g->M; ++m)
            if (g->row_ptr[m + 1] - g->row_ptr[m] != g->row_ptr[1] - g->row_ptr[0])
                return set_error(LDPC_ERR_UNSUPPORTED, "LAYERED_HOST follows the reference's host-layered path, which sizes its "
                            "layers correctly only when every row of H has the same weight (MyLdpc.cpp:907,958)");
        if (g->max_row_deg > ldpc::kMaxUnrolledLayerDegree)
            return set_error(LDPC_ERR_UNSUPPORTED, "LAYERED_HOST: row weight %d > %d", g->max_row_deg, ldpc::kMaxUnrolledLayerDegree);
    }
    if (cfg->pack_mode != LDPC_PACK_BYTES && cfg->pack_mode != LDPC_PACK_BITS)
        return set_error(LDPC_ERR_ARG, "unknown pack_mode %d", cfg->pack_mode);
    if (cfg->frames_per_lane != 0 && cfg->frames_per_lane != 1 && cfg->frames_per_lane != 2 &&
        cfg->frames_per_lane != 4)
        return set_error(LDPC_ERR_ARG, "frames_per_lane must be 0, 1, 2 or 4");
    if (cfg->msg_dtype != LDPC_MSG_F32 && cfg->msg_dtype != LDPC_MSG_F16 && cfg->msg_dtype != LDPC_MSG_F8 && cfg->msg_dtype != LDPC_MSG_I8)
        return set_error(LDPC_ERR_ARG, "unknown msg_dtype %d", cfg->msg_dtype);
    if (cfg->msg_reserved3)
        return set_error(LDPC_ERR_ARG, "msg_reserved must be 0");
    for (int j = 0; j < ldpc::kBitflipThresholds; ++j) {
        if (cfg->bf_threshold[j] != 0 && !bitflip)
            return set_error(LDPC_ERR_ARG, "bf_threshold[%d]=%d belongs to LDPC_ALGO_BITFLIP (algo is %d)", j, cfg->bf_threshold[j], cfg->algo);
        if (cfg->bf_threshold[j] < 0 || cfg->bf_threshold[j] > ldpc::kBitflipMaxDegree)
            return set_error(LDPC_ERR_ARG, "bf_threshold[%d]=%d must be in [0, %d]", j, cfg->bf_threshold[j], ldpc::kBitflipMaxDegree);
    }
    if (bitflip && cfg->msg_dtype != LDPC_MSG_F32)
        return set_error(LDPC_ERR_UNSUPPORTED, "LDPC_ALGO_BITFLIP has no messages: msg_dtype must be LDPC_MSG_F32, not %d", cfg->msg_dtype);
    if (bitflip && g->max_col_deg > ldpc::kBitflipMaxDegree)
        return set_error(LDPC_ERR_UNSUPPORTED, "LDPC_ALGO_BITFLIP counts a column's votes in six bits: column degree %d > %d", g->max_col_deg,
                    ldpc::kBitflipMaxDegree);
    if (cfg->bp_frac_bits != 0 && !bpfx)
        return set_error(LDPC_ERR_ARG, "bp_frac_bits=%d belongs to LDPC_ALGO_LAYERED_BP_FX (algo is %d)", cfg->bp_frac_bits, cfg->algo);
    if (bpfx && (cfg->bp_frac_bits < 0 || cfg->bp_frac_bits > ldpc::kBpFxMaxFracBits))
        return set_error(LDPC_ERR_ARG, "bp_frac_bits=%d must be in [0, %d]", cfg->bp_frac_bits, ldpc::kBpFxMaxFracBits);
    if (cfg->post_bits != 0 && !fx)
        return set_error(LDPC_ERR_ARG, "post_bits=%d belongs to LDPC_ALGO_LAYERED_FX and LDPC_ALGO_LAYERED_BP_FX (algo is %d)", cfg->post_bits, cfg->algo);
    if (fx && cfg->msg_dtype != LDPC_MSG_I8)
        return set_error(LDPC_ERR_ARG, "%s is defined on fixed-point messages: msg_dtype must be LDPC_MSG_I8, not %d", fx_name, cfg->msg_dtype);
    if (cfg->msg_bits != 0 && cfg->msg_dtype != LDPC_MSG_I8)
        return set_error(LDPC_ERR_ARG, "msg_bits=%d belongs to LDPC_MSG_I8 (msg_dtype is %d)", cfg->msg_bits, cfg->msg_dtype);
    if (cfg->msg_bits != 0 && cfg->msg_bits != 4 && cfg->msg_bits != 5 && cfg->msg_bits != 6 && cfg->msg_bits != 8)
        return set_error(LDPC_ERR_ARG, "msg_bits must be 0 (8), 4, 5, 6 or 8, not %d", cfg->msg_bits);
    if (cfg->msg_dtype == LDPC_MSG_I8 && cfg->algo != LDPC_ALGO_MS && !fx)
        return set_error(LDPC_ERR_UNSUPPORTED, "fixed-point messages (LDPC_MSG_I8) are built for flooding min-sum and, as an algorithm of "
                    "their own, LDPC_ALGO_LAYERED_FX and LDPC_ALGO_LAYERED_BP_FX (SP and BP have no integer datapath here; LDPC_ALGO_LAYERED, LAYERED_BP and the "
                    "reference-reproducing decoders are fp32)");
    if (fx) {
        const int q = cfg->msg_bits ? cfg->msg_bits : 8;
        if (cfg->post_bits != 0 && (cfg->post_bits < q || cfg->post_bits > 16))
            return set_error(LDPC_ERR_ARG, "post_bits=%d must be 0 (16) or in [msg_bits=%d, 16]", cfg->post_bits, q);
        if (cfg->layer_rows <= 0 || g->M % cfg->layer_rows)
            return set_error(LDPC_ERR_ARG, "%s: layer_rows=%d must be positive and divide M=%d", fx_name, cfg->layer_rows, g->M);
    }
    /* written so that NaN fails it */
    if (cfg->msg_dtype == LDPC_MSG_I8 && !(cfg->llr_scale > 0.0f && cfg->llr_scale <= 3.402823466e38f))
        return set_error(LDPC_ERR_ARG, "LDPC_MSG_I8: llr_scale must be positive and finite (the LSBs per unit of channel value)");
    if (cfg->msg_dtype == LDPC_MSG_F8 && cfg->algo != LDPC_ALGO_MS)
        return set_error(LDPC_ERR_UNSUPPORTED, "fp8 messages are built for flooding min-sum only "
                    "(the probability-domain SP needs fp32 range; BP is fp32 / fp16; the layered decoders, LAYERED_BP among them, and the "
                    "reference-reproducing ones are fp32)");
    if (cfg->msg_dtype == LDPC_MSG_F16 && cfg->algo != LDPC_ALGO_MS && cfg->algo != LDPC_ALGO_BP)
        return set_error(LDPC_ERR_UNSUPPORTED, "fp16 messages are built for flooding min-sum and BP only "
                    "(the probability-domain SP needs fp32 range; the layered engine, LAYERED and LAYERED_BP, is fp32)");
    if (!ldpc::tune_valid(*cfg)) return set_error(LDPC_ERR_ARG, "tuning / streams config fields out of range");
    if (bitflip) {
        const ldpc::Tune t = ldpc::tune_from_config(*cfg);
        if (ldpc::tune_forced_on(t.fused) || ldpc::tune_forced_on(t.ldsp))
            return set_error(LDPC_ERR_UNSUPPORTED, "LDPC_ALGO_BITFLIP runs the bit-flipping engine: the one-launch and the record kernels "
                        "(LDPC_TUNE_FUSED / LDPC_TUNE_LDSP forced on) are soft decoders");
    }
    if (bp_row) {
        const ldpc::Tune t = ldpc::tune_from_config(*cfg);
        if (ldpc::tune_forced_on(t.fused) || ldpc::tune_forced_on(t.ldsp))
            return set_error(LDPC_ERR_UNSUPPORTED, "LDPC_ALGO_BP / LDPC_ALGO_LAYERED_BP: the LDS-resident one-launch kernels and the record kernels (LDPC_TUNE_FUSED / "
                        "LDPC_TUNE_LDSP forced on) carry no box-plus check node; the streaming kernels do");
    }
    if (cfg->msg_dtype == LDPC_MSG_F8 || cfg->msg_dtype == LDPC_MSG_I8) {
        const ldpc::Tune t = ldpc::tune_from_config(*cfg);
        if (ldpc::tune_forced_on(t.fused) || ldpc::tune_forced_on(t.ldsp))
            return set_error(LDPC_ERR_UNSUPPORTED, "%s messages: the LDS-resident one-launch kernels and the record kernels (LDPC_TUNE_FUSED / "
                        "LDPC_TUNE_LDSP forced on) are fp32; the streaming kernels carry the %s rule",
                        cfg->msg_dtype == LDPC_MSG_F8 ? "fp8" : "fixed-point", cfg->msg_dtype == LDPC_MSG_F8 ? "fp8" : "fixed-point");
    }
    /* CRC-aided early termination: the streaming kernels carry the rule (crc_term_kernel), nothing else does */
    const bool crc_term = cfg->crc_kind != 0;
    {
        char msg[256];
        if (ldpc::crc_term_check(cfg->crc_kind, cfg->crc_bits, cfg->K, cfg->early_term, msg, sizeof msg)) return set_error(LDPC_ERR_ARG, "%s", msg);
        if (crc_term && (cfg->algo == LDPC_ALGO_MS_FUSED || cfg->algo == LDPC_ALGO_LAYERED_HOST))
            return set_error(LDPC_ERR_UNSUPPORTED, "crc_kind: LDPC_ALGO_MS_FUSED and LDPC_ALGO_LAYERED_HOST reproduce reference kernels, which "
                        "stop on the syndrome alone; LDPC_ALGO_SP, LDPC_ALGO_MS, LDPC_ALGO_BP, LDPC_ALGO_LAYERED and LDPC_ALGO_LAYERED_BP carry the CRC rule");
        const ldpc::Tune t = ldpc::tune_from_config(*cfg);
        if (crc_term && (ldpc::tune_forced_on(t.fused) || ldpc::tune_forced_on(t.ldsp)))
            return set_error(LDPC_ERR_UNSUPPORTED, "crc_kind: the LDS-resident one-launch kernels and the record kernels (LDPC_TUNE_FUSED / "
                        "LDPC_TUNE_LDSP forced on) do not carry the CRC rule; the streaming kernels do");
    }
    const bool fx_record = ldpc::tune_from_config(*cfg).fx_record != 0;      /* tune_valid: a fixed-point layered algorithm */
    if (fx_record && bpfx)
        return set_error(LDPC_ERR_UNSUPPORTED, "LDPC_TUNE_FX_RECORD: a box-plus row sends D independent messages and the record "
                    "kernel's two-minimum record cannot hold them; LDPC_ALGO_LAYERED_BP_FX runs the streaming layered engine");
    if (fx_record && crc_term)
        return set_error(LDPC_ERR_UNSUPPORTED, "crc_kind: the fixed-point record kernel (LDPC_TUNE_FX_RECORD) does not carry the CRC "
                    "rule; the streaming kernels do");

    int ndev = 0;
    LDPC_HIP_TRY(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev)
        return set_error(LDPC_ERR_HIP, "device %d not present (%d HIP devices)", cfg->device, ndev);
    LDPC_HIP_TRY(hipSetDevice(cfg->device));

    ldpc_decoder *d = new (std::nothrow) ldpc_decoder;
    if (!d) return set_error(LDPC_ERR_NOMEM, "out of memory");
    std::unique_ptr<ldpc_decoder> guard(d);
    d->cfg = *cfg;
    d->ms_corr = ms_corr;
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
    const bool f8 = cfg->msg_dtype == LDPC_MSG_F8 || cfg->msg_dtype == LDPC_MSG_I8;
    d->flood.check_wide = ldpc::tune_pick(tune.check_wide, f8 && g->max_row_deg <= ldpc::kMaxUnrolledDegree);
    d->flood.link_form = ldpc::tune_pick(tune.link_half, false) ? 2 : (ldpc::tune_pick(tune.link_narrow, !f8 || ldpc::tune_forced_on(tune.link_deep)) ? 1 : 0);   /* deep is a narrow form */
    d->flood.link_deep = ldpc::tune_pick(tune.link_deep, false);
    if (tune.link_rows) d->flood.link_rpw = tune.link_rows < 0 ? 0 : tune.link_rows;
    LDPC_HIP_TRY(hipDeviceGetAttribute(&d->flood.cus, hipDeviceAttributeMultiprocessorCount, cfg->device));
    d->V = bitflip ? 1 : pick_frames_per_lane(*cfg, g->max_row_deg, g->max_col_deg);       /* bit flipping: a word is 64 frames */
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
                      (cfg->algo == LDPC_ALGO_SP || cfg->algo == LDPC_ALGO_MS || cfg->algo == LDPC_ALGO_BP) && d->T >= 4 * d->flood.TO && t_child_depth == 0;
    if (!d->flood.tail_enabled) d->flood.TO = 0;
    d->flood.TA = d->T + d->flood.TO;
    const size_t TF = (size_t)d->flood.TA * d->F;
    LDPC_HIP_TRY(d->hard.alloc((size_t)d->flood.TA * d->N * d->V));
    LDPC_HIP_TRY(d->failw.alloc((size_t)(cfg->max_iter + 2) * d->flood.TA * d->V));
    LDPC_HIP_TRY(d->done.alloc((size_t)d->flood.TA * d->V));
    LDPC_HIP_TRY(d->iters.alloc(TF));
    LDPC_HIP_TRY(d->active.alloc(1));
    LDPC_HIP_TRY(d->summary.alloc(4));
    if (crc_term) {
        std::vector<uint32_t> w((size_t)cfg->crc_bits);
        ldpc::crc_term_weights(cfg->crc_kind, cfg->crc_bits, w.data());
        LDPC_HIP_TRY(d->crc_w.upload(w));
    }

    if (bitflip) {
        /* the bit-flipping engine: x lives in `hard`; received bits, syndrome words and votes in the plan.  No hand-over
         * child and no device-side tail: a round is too cheap to be worth moving frames for */
        const hipError_t e = ldpc::bitflip_plan_create(&d->bitflip, g->M, g->N, g->E, g->rows, g->col_edge, d->T, cfg->bf_threshold);
        if (e != hipSuccess) return set_error(LDPC_ERR_HIP, "bit-flipping plan allocation failed: %s", hipGetErrorString(e));
    } else if (cfg->algo == LDPC_ALGO_MS_FUSED) {
        if (cfg->pack_mode != LDPC_PACK_BYTES && cfg->K % 8)
            return set_error(LDPC_ERR_UNSUPPORTED, "MS_FUSED packs whole bytes per frame only");
        /* flood_ldsp_kernel<.., CHAIN = false> (posteriors in LDS, 16-byte check records) wherever it fits
         * with two workgroups per CU, else / with LDPC_TUNE_OFF(LDPC_TUNE_LDSP) the LDS-resident fused_flood_kernel */
        if (!ldpc::tune_forced_off(tune.ldsp)) {
            LDPC_HIP_TRY(ldpc::engine_ldsp_plan_create(&d->ldsp, g->M, g->N, g->E, g->row_ptr, g->cols, cfg->layer_rows, cfg->K,
                                           cfg->max_batch, cfg->device, tune, /*flood=*/2));
            if (d->ldsp.eligible && (ldpc::tune_forced_on(tune.ldsp) || d->ldsp.lds_bytes <= 80 * 1024)) d->use_ldsp = true;
            else d->ldsp = ldpc::LdspPlan();
        }
        if (!d->use_ldsp) {
            LDPC_HIP_TRY(ldpc::fused_plan_create(&d->fused, g->M, g->N, g->E, g->row_ptr, g->cols, cfg->layer_rows));
            if (!d->fused.eligible)
                return set_error(LDPC_ERR_UNSUPPORTED, "MS_FUSED needs a quasi-cyclic H (circulant size = layer_rows) whose "
                            "posteriors fit in LDS");
        }
        d->use_fused = true;
    } else if (cfg->algo == LDPC_ALGO_LAYERED_HOST || cfg->algo == LDPC_ALGO_LAYERED_BP || fx) {
        /* the streaming layered engine (LAYERED_FX: unless LDPC_TUNE_FX_RECORD, below).  LAYERED_BP: the record kernels' 16-byte check record holds two minima and
         * cannot hold a row's D independent messages, and the LDS-resident kernel carries no box-plus row */
        d->layered.rule = bpfx ? ldpc::kLayerBpFx : fx ? ldpc::kLayerFx : cfg->algo == LDPC_ALGO_LAYERED_BP ? ldpc::kLayerBp : ldpc::kLayerHost;
        d->layered.llr_scale = cfg->llr_scale;
        if (fx) {       /* plain min-sum is the corrected row with scale 1, offset 0: the identity on [0, L] */
            d->layered.L = (float)((1 << ((cfg->msg_bits ? cfg->msg_bits : 8) - 1)) - 1);
            d->layered.LP = (float)((1 << ((cfg->post_bits ? cfg->post_bits : 16) - 1)) - 1);
            d->layered.ms_scale = d->ms_scale;
            d->layered.ms_offset = d->ms_offset;
        }
        if (bpfx) {     /* the kernels index the table with |a| + |b| <= 254 and never clamp: zeros behind its last entry */
            int32_t t[ldpc::kBpFxTable];
            const int n = ldpc::bp_fx_table_build(cfg->bp_frac_bits, t, ldpc::kBpFxTable);
            std::vector<uint8_t> bytes((size_t)ldpc::kBpFxTable, 0);
            for (int i = 0; i < n; ++i) bytes[(size_t)i] = (uint8_t)t[i];
            LDPC_HIP_TRY(d->layered.bp_table.upload(bytes));
        }
        /* LDPC_TUNE_FX_RECORD: layered_ldsp_fx_kernel (int16 posteriors in LDS, 8-byte check records in cache) where the code
         * fits it -- quasi-cyclic at layer_rows, rows of at most 24 entries, posteriors within the LDS limit, whole bytes per
         * frame -- and the streaming engine, with the same result, where it does not */
        if (fx_record && (cfg->pack_mode == LDPC_PACK_BYTES || cfg->K % 8 == 0)) {
            d->ldsp.mc = ldpc::MsCorr{d->ms_scale, d->ms_offset};
            d->ldsp.fx_L = (int32_t)d->layered.L;
            d->ldsp.fx_LP = (int32_t)d->layered.LP;
            LDPC_HIP_TRY(ldpc::engine_ldsp_fx_plan_create(&d->ldsp, g->M, g->N, g->E, g->row_ptr, g->cols, cfg->layer_rows,
                                              cfg->K, cfg->max_batch, cfg->device, tune));
            if (d->ldsp.eligible) d->use_fused = d->use_ldsp = true;
            else d->ldsp = ldpc::LdspPlan();
        }
        /* the streaming plan (and its P / R arrays in HBM) only when the record kernel does not apply */
        int rc = d->use_fused ? 0 : ldpc::layered_plan_create(&d->layered, g->M, g->N, g->E, g->row_ptr, g->cols, cfg->layer_rows, d->T, d->V);
        if (rc == -1) return set_error(LDPC_ERR_ARG, "layer_rows=%d must divide M=%d and rows of a layer "
                                  "must not share a column", cfg->layer_rows, g->M);
        if (rc) return set_error(LDPC_ERR_HIP, "layered plan allocation failed: %s", hipGetErrorString(hipGetLastError()));
    } else if (cfg->algo == LDPC_ALGO_LAYERED) {
        /* short quasi-cyclic codes decode entirely in LDS, one launch (fused_kernels.hpp);
         * LDPC_TUNE_OFF(LDPC_TUNE_FUSED) keeps the streaming kernels (same results, bit for bit) */
        /* the correction (ms_scale / ms_offset) is carried by the record kernel (layered_ldsp_corr_kernel) and the
         * streaming one (layer_corr_kernel), not by the LDS-resident fused_layered_kernel */
        if (d->ms_corr && ldpc::tune_forced_on(tune.fused) && ldpc::tune_forced_off(tune.ldsp))
            return set_error(LDPC_ERR_UNSUPPORTED, "ms_scale / ms_offset: the LDS-resident layered kernel (LDPC_TUNE_FUSED on, "
                        "LDPC_TUNE_LDSP off) carries no correction; the record or the streaming kernels do");
        if (!crc_term && !ldpc::tune_forced_off(tune.fused) && (cfg->pack_mode == LDPC_PACK_BYTES || cfg->K % 8 == 0)) {
            if (!d->ms_corr) {
                LDPC_HIP_TRY(ldpc::fused_plan_create(&d->fused, g->M, g->N, g->E, g->row_ptr, g->cols, cfg->layer_rows));
                d->use_fused = d->fused.eligible;
            }
            /* layered_ldsp_kernel (posterior in LDS, 16-byte check records in cache) is the default for
             * every QC code it fits: larger codes cannot use the fully LDS-resident kernel at all, and on
             * short ones it is 1.2-2.9x faster (exact-width rows, bit-level sign algebra: 800 against 280 G
             * edge updates/s; circulants of <= 32 rows run several frames per wave in both).
             * LDPC_TUNE_OFF(LDPC_TUNE_LDSP) forbids it (the LDS-resident kernel is then used where it applies). */
            if (!ldpc::tune_forced_off(tune.ldsp)) {
                d->ldsp.corr = d->ms_corr;
                d->ldsp.mc = ldpc::MsCorr{d->ms_scale, d->ms_offset};
                LDPC_HIP_TRY(ldpc::engine_ldsp_plan_create(&d->ldsp, g->M, g->N, g->E, g->row_ptr, g->cols, cfg->layer_rows,
                                               cfg->K, cfg->max_batch, cfg->device, tune, /*flood=*/0));
                if (d->ldsp.eligible) d->use_fused = d->use_ldsp = true;
            }
        }
        /* the streaming plan (and its P / R arrays in HBM) only when no LDS-resident kernel applies;
         * a detected QC structure already implies that rows of a layer share no column */
        d->layered.rule = d->ms_corr ? ldpc::kLayerCorr : ldpc::kLayerFused;
        d->layered.ms_scale = d->ms_scale;
        d->layered.ms_offset = d->ms_offset;
        int rc = d->use_fused ? 0 : ldpc::layered_plan_create(&d->layered, g->M, g->N, g->E, g->row_ptr, g->cols,
                                                              cfg->layer_rows, d->T, d->V);
        if (rc == -1) return set_error(LDPC_ERR_ARG, "layer_rows=%d must divide M=%d and rows of a layer "
                                  "must not share a column", cfg->layer_rows, g->M);
        if (rc) return set_error(LDPC_ERR_HIP, "layered plan allocation failed: %s",
                            hipGetErrorString(hipGetLastError()));
    } else {
        /* flooding min-sum on a short quasi-cyclic code (layer_rows = circulant size given): the
         * same arithmetic in one LDS-resident launch (fused_flood_kernel<.., CHAIN>) */
        /* Measured (tools/gpu_short.py): for the flooding schedules the streaming kernels win at
         * full work once the batch is large (HBM-bound, 1.3-1.9x), the fused kernels win on latency
         * and for small batches; crossover near max_batch * E = 2^23 edge-frames.
         * LDPC_TUNE_ON(LDPC_TUNE_FUSED) forces the fused kernels, LDPC_TUNE_OFF the streaming ones. */
        /* the correction (ms_scale / ms_offset) is carried by the record kernel (flood_ldsp_corr_kernel) and the streaming
         * kernels (kAlgoMSC), not by the LDS-resident fused_flood_kernel */
        if (d->ms_corr && ldpc::tune_forced_on(tune.fused) && ldpc::tune_forced_off(tune.ldsp))
            return set_error(LDPC_ERR_UNSUPPORTED, "ms_scale / ms_offset: the LDS-resident flooding kernel (LDPC_TUNE_FUSED on, "
                        "LDPC_TUNE_LDSP off) carries no correction; the record or the streaming kernels do");
        /* LDPC_ALGO_BP: the streaming kernels always (layer_rows does not select an engine) */
        if (cfg->algo != LDPC_ALGO_BP && !crc_term && cfg->msg_dtype == LDPC_MSG_F32 && cfg->layer_rows > 0 && cfg->frames_per_lane == 0 &&
            (cfg->pack_mode == LDPC_PACK_BYTES || cfg->K % 8 == 0)) {
            const bool small = (int64_t)cfg->max_batch * g->E <= (int64_t)1 << 23;
            if (!d->ms_corr && ldpc::tune_pick(tune.fused, small)) {
                LDPC_HIP_TRY(ldpc::fused_plan_create(&d->fused, g->M, g->N, g->E, g->row_ptr, g->cols, cfg->layer_rows));
                d->use_fused = d->fused.eligible && (cfg->algo == LDPC_ALGO_MS || d->fused.eligible_sp);
            }
            /* min-sum: posteriors in LDS (two images), one 16-byte record per check row (flood_ldsp_kernel).
             * Default wherever it fits with >= 2 workgroups per CU: 2-2.9x the LDS-resident kernel and the
             * streaming kernels on the 802.16e codes at any batch size ((2304, 1152): 9.9 / 4.0 / 2.9 Gbit/s
             * at 16 384 frames, 2.6 / 0.9 / 1.3 at full work), 2.4 / 2.0 / 1.7 / 1.2x the streaming kernels on
             * BG1-profile codes at Z = 64 / 128 / 256 / 384.  LDPC_TUNE_ON / OFF(LDPC_TUNE_LDSP) forces / forbids it. */
            if (cfg->algo == LDPC_ALGO_MS && !ldpc::tune_forced_off(tune.fused) && !ldpc::tune_forced_off(tune.ldsp)) {
                d->ldsp.corr = d->ms_corr;
                d->ldsp.mc = ldpc::MsCorr{d->ms_scale, d->ms_offset};
                LDPC_HIP_TRY(ldpc::engine_ldsp_plan_create(&d->ldsp, g->M, g->N, g->E, g->row_ptr, g->cols, cfg->layer_rows,
                                               cfg->K, cfg->max_batch, cfg->device, tune, /*flood=*/1));
                if (d->ldsp.eligible && (ldpc::tune_forced_on(tune.ldsp) || d->ldsp.lds_bytes <= 80 * 1024))
                    d->use_fused = d->use_ldsp = true;
                else
                    d->ldsp = ldpc::LdspPlan();
            }
        }
        if (!d->use_fused) {
            /* work lists, kernel tables, launch plan; the column-fused check kernel's form and the arrays' placement are
             * measured there unless the caller says which (engine_flood.hip) */
            int rc = ldpc::engine_flood_setup(d, g, TF, t_child_depth == 0);
            if (rc) return rc;
            if (d->flood.tail_enabled) {
                LDPC_HIP_TRY(d->flood.tail_state.alloc(4));
                LDPC_HIP_TRY(d->flood.tail_map.alloc((size_t)d->flood.TO * d->F));
                LDPC_HIP_TRY(d->flood.running.alloc((size_t)cfg->max_iter + 2));
            }
            /* tail compaction: with host polling on, the last <= 512 running frames of a batch of several
             * tiles are finished by a small (8 x 64 frames) child decoder (cfg.tune_compact = -1: off, n: threshold) */
            /* the child takes over once at most a quarter of the batch still runs: 1024 frames for the 4096-frame
             * batches of the benchmark configurations (rate 9/10, fp16: 681 frames still run after round 5 of 8 and
             * sit in all 16 tiles; a 512-frame child had to wait for round 6), 512 otherwise */
            if (t_child_depth == 0) d->flood.child_capacity = cfg->max_batch >= 4096 ? 2 * ldpc::kCompactCapacity : ldpc::kCompactCapacity;
            else d->flood.child_capacity = cfg->max_batch > ldpc::kCompactCapacity ? ldpc::kCompactCapacity : ldpc::kLastCapacity;
            d->flood.compact_threshold = d->flood.child_capacity;
            if (tune.compact) d->flood.compact_threshold = tune.compact < 0 ? 0 : std::min(d->flood.child_capacity, tune.compact);
            /* the 1024-frame child has a 512-frame child of its own (rate 9/10: of the 681 frames handed over after round 5
             * only 41 still run after round 6, spread over the child's three tiles of 256), and that one a single tile of 64
             * frames (sum-product at 5 dB: a handful of frames in 4096 run all 50 rounds, one in each of its tiles) */
            const bool may_have_child = t_child_depth == 0 || cfg->max_batch > ldpc::kLastCapacity;
            if (cfg->early_term && cfg->poll_interval > 0 && d->T > 1 && d->flood.compact_threshold > 0 && may_have_child) {
                ldpc_decoder_config cc = *cfg;
                cc.max_batch = d->flood.child_capacity;
                /* tiles of 64 frames for the 512-frame child (the last few stragglers of a batch); tiles of 256 for the
                 * 1024-frame child, which takes over hundreds of frames: dense tiles, 8- / 16-byte accesses */
                cc.frames_per_lane = (d->flood.child_capacity > ldpc::kCompactCapacity && d->V == 4) ? 4 : 1;
                cc.layer_rows = 0;                 /* streaming kernels, same arithmetic */
                cc.tune_compact = d->flood.child_capacity > ldpc::kLastCapacity ? 0 : -1;     /* all but the last hand over once more */
                ++t_child_depth;
                ldpc_decoder *child = nullptr;
                rc = ldpc_decoder_create(g, &cc, &child);
                --t_child_depth;
                if (rc) return rc;
                d->flood.child.reset(child);
                d->flood.child->flood.is_child = true;
                LDPC_HIP_TRY(hipSetDevice(cfg->device));
                LDPC_HIP_TRY(d->flood.cmap.alloc((size_t)d->flood.child_capacity));
                LDPC_HIP_TRY(d->flood.cinv.alloc((size_t)d->T * d->F));
                LDPC_HIP_TRY(d->flood.cmoved.alloc((size_t)d->T * d->V));
            }
        }
    }
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
    int rc;
    if (d->use_fused) {
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
            e = !d->use_ldsp ? ldpc::engine_fused_run(&d->fused, run, s, &d->last_iterations)
                : d->ldsp.fx ? ldpc::engine_ldsp_fx_run(&d->ldsp, run, s, &d->last_iterations)
                             : ldpc::engine_ldsp_run(&d->ldsp, run, s, &d->last_iterations);
        if (e == hipSuccess) e = ldpc::span_end(d, s);
        rc = (e == hipSuccess) ? LDPC_OK : set_error(LDPC_ERR_HIP, "fused decode: %s", hipGetErrorString(e));
    } else if (d->cfg.algo == LDPC_ALGO_LAYERED || d->cfg.algo == LDPC_ALGO_LAYERED_HOST || d->cfg.algo == LDPC_ALGO_LAYERED_BP ||
               d->cfg.algo == LDPC_ALGO_LAYERED_FX || d->cfg.algo == LDPC_ALGO_LAYERED_BP_FX) {
        ldpc::LayeredRun run;
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
        run.soft = d->soft.dst; run.soft_extrinsic = d->soft.kind == LDPC_SOFT_EXTRINSIC ? 1 : 0;
        hipError_t e = ldpc::engine_layered_run(&d->layered, run, s, &d->last_iterations);
        rc = (e == hipSuccess) ? LDPC_OK
                               : set_error(LDPC_ERR_HIP, "layered decode: %s", hipGetErrorString(e));
    } else if (d->cfg.algo == LDPC_ALGO_BITFLIP) {
        ldpc::BitflipRun run;
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
        run.row_ptr = d->row_ptr.p; run.edge_col = d->edge_col.p; run.col_ptr = d->col_ptr.p; run.summary = d->summary.p;
        run.crc_w = d->crc_w.p; run.crc_bits = d->cfg.crc_kind ? d->cfg.crc_bits : 0;
        hipError_t e = ldpc::engine_bitflip_run(&d->bitflip, run, s, &d->last_iterations);
        rc = (e == hipSuccess) ? LDPC_OK : set_error(LDPC_ERR_HIP, "bit-flipping decode: %s", hipGetErrorString(e));
    } else {
        rc = ldpc::engine_flood_run(d, in, frames, out_dev, room, iters_dev, s);
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
