/*
 * decoder_config_host.hpp -- what a decoder configuration means, decided on the host before a device is touched: the
 * accepted sizes of ldpc_decoder_config (config_in), one table of facts per algorithm (algo_info), every refusal
 * ldpc_decoder_create makes in front of the device check (config_check), the frames per lane (pick_frames_per_lane) and
 * the ordered list of engines a configuration may run on (engine_candidates).  No HIP in here:
 * tests/cpp/decoder_config_host_test.cpp includes this file alone.
 *
 * A new algorithm gets a row of kAlgos; a new rule a line of config_check at the place its refusal has among the others
 * (the first failing check names the error, so the order is part of the ABI's behaviour).
 */
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/ldpc_hip.h"
#include "tune.hpp"
#include "crc_term_host.hpp"

namespace ldpc {

/* ---- struct sizes: the current one and what callers built against earlier headers pass, newest first ---- */
constexpr size_t kConfigSizes[] = {sizeof(ldpc_decoder_config), offsetof(ldpc_decoder_config, bf_threshold),
                                   offsetof(ldpc_decoder_config, msg_bits), offsetof(ldpc_decoder_config, crc_kind),
                                   offsetof(ldpc_decoder_config, ms_scale)};

/* LDPC_OK, or LDPC_ERR_ARG with the message that lists the sizes */
inline int config_size_check(uint32_t size, char *msg, size_t cap)
{
    for (size_t s : kConfigSizes)
        if (size == s) return LDPC_OK;
    int at = snprintf(msg, cap, "config struct_size %u is none of", size);
    for (size_t s : kConfigSizes)
        if (at >= 0 && (size_t)at < cap) at += snprintf(msg + at, cap - (size_t)at, "%s %zu", s == kConfigSizes[0] ? "" : ",", s);
    if (at >= 0 && (size_t)at < cap) snprintf(msg + at, cap - (size_t)at, " (ABI mismatch)");
    return LDPC_ERR_ARG;
}

/* The caller's config as the current struct: a caller built against an earlier header passes a shorter struct, of which
 * only struct_size bytes are read; the fields it lacks are 0 (off; msg_bits: 8; bf_threshold: the default schedule). */
inline int config_in(const ldpc_decoder_config *cfg, ldpc_decoder_config *full, char *msg, size_t cap)
{
    if (int rc = config_size_check(cfg->struct_size, msg, cap)) return rc;
    memset(full, 0, sizeof *full);
    memcpy(full, cfg, cfg->struct_size);
    full->struct_size = sizeof *full;
    return LDPC_OK;
}

/* ---- the algorithms ---- */
enum class Family {
    Flood,          /* check and variable phase per round, messages in HBM (engine_flood) */
    Layered,        /* one launch per layer, posteriors in HBM (engine_layered) */
    Reference,      /* LDPC_ALGO_MS_FUSED: a reference kernel's arithmetic, always one launch */
    Bitflip         /* bits only (engine_bitflip) */
};
/* the degree that decides how many frames a lane takes (pick_frames_per_lane) */
enum class LaneDegree { Col, HalfCol, Row, None };

constexpr uint32_t msg_bit(int dtype) { return 1u << dtype; }

struct AlgoInfo {
    int32_t algo;
    const char *c_name;         /* as include/ldpc_hip.h spells it */
    const char *short_name;     /* in the labels of ldpc_decoder_kernel_times */
    Family family;
    uint32_t msg_dtypes;        /* msg_bit(LDPC_MSG_*) of every message type it accepts */
    bool ms_corr;               /* takes ms_scale / ms_offset */
    bool box_plus;              /* its check node is a box-plus row */
    bool fixed;                 /* an algorithm defined on fixed-point messages: msg_bits / post_bits are its own */
    bool layer_rows_divide;     /* layer_rows must be positive and divide M in front of the device check */
    bool crc;                   /* carries the CRC stopping rule */
    bool soft;                  /* has soft output */
    bool handover;              /* may hand its stragglers to a child or run the device-side tail */
    LaneDegree lane_degree;
};

constexpr uint32_t kF32 = msg_bit(LDPC_MSG_F32), kF16 = msg_bit(LDPC_MSG_F16), kF8 = msg_bit(LDPC_MSG_F8), kI8 = msg_bit(LDPC_MSG_I8);
constexpr AlgoInfo kAlgos[] = {
    /*                                                                                       corr   box    fixed  rows   crc    soft   hand */
    {LDPC_ALGO_SP, "LDPC_ALGO_SP", "sp", Family::Flood, kF32,                                false, false, false, false, true,  false, true,  LaneDegree::Col},
    {LDPC_ALGO_MS, "LDPC_ALGO_MS", "ms", Family::Flood, kF32 | kF16 | kF8 | kI8,             true,  false, false, false, true,  true,  true,  LaneDegree::HalfCol},
    {LDPC_ALGO_LAYERED, "LDPC_ALGO_LAYERED", "layered", Family::Layered, kF32,               true,  false, false, false, true,  true,  false, LaneDegree::Row},
    {LDPC_ALGO_MS_FUSED, "LDPC_ALGO_MS_FUSED", "ms_fused", Family::Reference, kF32,          false, false, false, false, false, true,  false, LaneDegree::Col},
    {LDPC_ALGO_LAYERED_HOST, "LDPC_ALGO_LAYERED_HOST", "layered_host", Family::Layered, kF32, false, false, false, false, false, true,  false, LaneDegree::Col},
    {LDPC_ALGO_BP, "LDPC_ALGO_BP", "bp", Family::Flood, kF32 | kF16,                         false, true,  false, false, true,  true,  true,  LaneDegree::HalfCol},
    {LDPC_ALGO_LAYERED_BP, "LDPC_ALGO_LAYERED_BP", "layered_bp", Family::Layered, kF32,      false, true,  false, true,  true,  true,  false, LaneDegree::Row},
    {LDPC_ALGO_LAYERED_FX, "LDPC_ALGO_LAYERED_FX", "lfx", Family::Layered, kI8,              true,  false, true,  true,  true,  true,  false, LaneDegree::None},
    {LDPC_ALGO_LAYERED_BP_FX, "LDPC_ALGO_LAYERED_BP_FX", "lbfx", Family::Layered, kI8,       false, true,  true,  true,  true,  true,  false, LaneDegree::None},
    {LDPC_ALGO_BITFLIP, "LDPC_ALGO_BITFLIP", "bitflip", Family::Bitflip, kF32,               false, false, false, false, true,  false, false, LaneDegree::Col},
};

/* the row of an assigned enum ldpc_algo value; nullptr for 7 and for anything unknown */
inline const AlgoInfo *algo_info(int32_t algo)
{
    for (const AlgoInfo &a : kAlgos)
        if (a.algo == algo) return &a;
    return nullptr;
}

/* ---- limits of the kernels that the checks quote (ldpc_hip.hip asserts that each equals its owner's constant) ---- */
constexpr int kCfgUnrolledDegree = 16;          /* kMaxUnrolledDegree, flood_common.hpp */
constexpr int kCfgUnrolledLayerDegree = 24;     /* kMaxUnrolledLayerDegree, layered_kernels.hpp */
constexpr int kCfgBitflipDegree = 62;           /* kBitflipMaxDegree, bitflip_kernels.hpp */
constexpr int kCfgBpFracBits = 4;               /* kBpFxMaxFracBits, layered_kernels.hpp */
constexpr int kCfgLdsLimit = 80 * 1024;         /* a record kernel is the automatic choice while two workgroups fit a CU */

/* what the checks need to know of the graph */
struct GraphFacts {
    int32_t M = 0, N = 0;
    int64_t E = 0;
    int32_t max_row_deg = 0, max_col_deg = 0;
    bool rows_one_weight = false;   /* every row of H has the same weight */
};

/* ---- named predicates ---- */
/* written so that NaN fails it */
inline bool positive_finite(float x) { return x > 0.0f && x <= 3.402823466e38f; }
/* LDPC_TUNE_FUSED / LDPC_TUNE_LDSP forced on: the caller insists on an LDS-resident one-launch or a record kernel */
inline bool forces_lds_kernel(const Tune &t) { return tune_forced_on(t.fused) || tune_forced_on(t.ldsp); }
inline bool one_byte_messages(const ldpc_decoder_config &c) { return c.msg_dtype == LDPC_MSG_F8 || c.msg_dtype == LDPC_MSG_I8; }
inline bool has_ms_corr(const ldpc_decoder_config &c) { return c.ms_scale != 0.0f || c.ms_offset != 0.0f; }
/* the one-launch and record kernels pack whole bytes per frame */
inline bool packs_whole_bytes(const ldpc_decoder_config &c) { return c.pack_mode == LDPC_PACK_BYTES || c.K % 8 == 0; }

/* Every refusal in front of the device check, first failing check first: an LDPC_* code, the message in msg. */
inline int config_check(const ldpc_decoder_config &c, const GraphFacts &g, char *msg, size_t cap)
{
#define LDPC_REFUSE(code, ...) return (void)snprintf(msg, cap, __VA_ARGS__), (code)
    if (c.K <= 0 || c.K > g.N) LDPC_REFUSE(LDPC_ERR_ARG, "K=%d out of range", c.K);
    if (c.max_batch <= 0) LDPC_REFUSE(LDPC_ERR_ARG, "max_batch must be positive");
    if (c.max_iter <= 0 || c.max_iter > 100000) LDPC_REFUSE(LDPC_ERR_ARG, "max_iter out of range");
    const AlgoInfo *const a = algo_info(c.algo);
    if (!a) LDPC_REFUSE(LDPC_ERR_ARG, "unknown algo %d", c.algo);
    const bool bitflip = a->family == Family::Bitflip;
    const bool layer_rows_ok = c.layer_rows > 0 && g.M % c.layer_rows == 0;
    /* comparisons written so that NaN fails them */
    if (!(c.ms_scale >= 0.0f && c.ms_scale <= 1.0f)) LDPC_REFUSE(LDPC_ERR_ARG, "ms_scale must be 0 (off) or in (0, 1]");
    if (!(c.ms_offset >= 0.0f && c.ms_offset < 1000.0f)) LDPC_REFUSE(LDPC_ERR_ARG, "ms_offset must be 0 (off) or in (0, 1000)");
    if (has_ms_corr(c) && !a->ms_corr)
        LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "ms_scale / ms_offset apply to LDPC_ALGO_MS and LDPC_ALGO_LAYERED only "
                    "(SP, BP, LAYERED_BP, LAYERED_BP_FX and BITFLIP have no minimum to correct; MS_FUSED and LAYERED_HOST reproduce reference kernels)");
    /* the float box-plus rows; the fixed-point one is checked with the fixed-point algorithms below */
    if (a->box_plus && !a->fixed) {
        if (!positive_finite(c.llr_scale))
            LDPC_REFUSE(LDPC_ERR_ARG, "%s: llr_scale must be positive and finite (chan = llr_scale * y is the LLR)", a->c_name);
        if (a->layer_rows_divide && !layer_rows_ok)
            LDPC_REFUSE(LDPC_ERR_ARG, "%s: layer_rows=%d must be positive and divide M=%d", a->c_name, c.layer_rows, g.M);
    }
    if (c.algo == LDPC_ALGO_LAYERED_HOST) {
        if (!g.rows_one_weight)
            LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "LAYERED_HOST follows the reference's host-layered path, which sizes its "
                        "layers correctly only when every row of H has the same weight (MyLdpc.cpp:907,958)");
        if (g.max_row_deg > kCfgUnrolledLayerDegree)
            LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "LAYERED_HOST: row weight %d > %d", g.max_row_deg, kCfgUnrolledLayerDegree);
    }
    if (c.pack_mode != LDPC_PACK_BYTES && c.pack_mode != LDPC_PACK_BITS) LDPC_REFUSE(LDPC_ERR_ARG, "unknown pack_mode %d", c.pack_mode);
    if (c.frames_per_lane != 0 && c.frames_per_lane != 1 && c.frames_per_lane != 2 && c.frames_per_lane != 4)
        LDPC_REFUSE(LDPC_ERR_ARG, "frames_per_lane must be 0, 1, 2 or 4");
    if (c.msg_dtype != LDPC_MSG_F32 && c.msg_dtype != LDPC_MSG_F16 && c.msg_dtype != LDPC_MSG_F8 && c.msg_dtype != LDPC_MSG_I8)
        LDPC_REFUSE(LDPC_ERR_ARG, "unknown msg_dtype %d", c.msg_dtype);
    const bool accepted = (a->msg_dtypes & msg_bit(c.msg_dtype)) != 0;
    if (c.msg_reserved3) LDPC_REFUSE(LDPC_ERR_ARG, "msg_reserved must be 0");
    for (size_t j = 0; j < sizeof c.bf_threshold / sizeof c.bf_threshold[0]; ++j) {
        if (c.bf_threshold[j] != 0 && !bitflip)
            LDPC_REFUSE(LDPC_ERR_ARG, "bf_threshold[%d]=%d belongs to LDPC_ALGO_BITFLIP (algo is %d)", (int)j, c.bf_threshold[j], c.algo);
        if (c.bf_threshold[j] < 0 || c.bf_threshold[j] > kCfgBitflipDegree)
            LDPC_REFUSE(LDPC_ERR_ARG, "bf_threshold[%d]=%d must be in [0, %d]", (int)j, c.bf_threshold[j], kCfgBitflipDegree);
    }
    if (bitflip && !accepted)
        LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "LDPC_ALGO_BITFLIP has no messages: msg_dtype must be LDPC_MSG_F32, not %d", c.msg_dtype);
    if (bitflip && g.max_col_deg > kCfgBitflipDegree)
        LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "LDPC_ALGO_BITFLIP counts a column's votes in six bits: column degree %d > %d", g.max_col_deg,
                    kCfgBitflipDegree);
    const bool bpfx = a->box_plus && a->fixed;
    if (c.bp_frac_bits != 0 && !bpfx)
        LDPC_REFUSE(LDPC_ERR_ARG, "bp_frac_bits=%d belongs to LDPC_ALGO_LAYERED_BP_FX (algo is %d)", c.bp_frac_bits, c.algo);
    if (bpfx && (c.bp_frac_bits < 0 || c.bp_frac_bits > kCfgBpFracBits))
        LDPC_REFUSE(LDPC_ERR_ARG, "bp_frac_bits=%d must be in [0, %d]", c.bp_frac_bits, kCfgBpFracBits);
    if (c.post_bits != 0 && !a->fixed)
        LDPC_REFUSE(LDPC_ERR_ARG, "post_bits=%d belongs to LDPC_ALGO_LAYERED_FX and LDPC_ALGO_LAYERED_BP_FX (algo is %d)", c.post_bits, c.algo);
    if (a->fixed && !accepted)
        LDPC_REFUSE(LDPC_ERR_ARG, "%s is defined on fixed-point messages: msg_dtype must be LDPC_MSG_I8, not %d", a->c_name, c.msg_dtype);
    if (c.msg_bits != 0 && c.msg_dtype != LDPC_MSG_I8)
        LDPC_REFUSE(LDPC_ERR_ARG, "msg_bits=%d belongs to LDPC_MSG_I8 (msg_dtype is %d)", c.msg_bits, c.msg_dtype);
    if (c.msg_bits != 0 && c.msg_bits != 4 && c.msg_bits != 5 && c.msg_bits != 6 && c.msg_bits != 8)
        LDPC_REFUSE(LDPC_ERR_ARG, "msg_bits must be 0 (8), 4, 5, 6 or 8, not %d", c.msg_bits);
    if (c.msg_dtype == LDPC_MSG_I8 && !accepted)
        LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "fixed-point messages (LDPC_MSG_I8) are built for flooding min-sum and, as an algorithm of "
                    "their own, LDPC_ALGO_LAYERED_FX and LDPC_ALGO_LAYERED_BP_FX (SP and BP have no integer datapath here; LDPC_ALGO_LAYERED, LAYERED_BP and the "
                    "reference-reproducing decoders are fp32)");
    if (a->fixed) {
        const int q = c.msg_bits ? c.msg_bits : 8;
        if (c.post_bits != 0 && (c.post_bits < q || c.post_bits > 16))
            LDPC_REFUSE(LDPC_ERR_ARG, "post_bits=%d must be 0 (16) or in [msg_bits=%d, 16]", c.post_bits, q);
        if (!layer_rows_ok)
            LDPC_REFUSE(LDPC_ERR_ARG, "%s: layer_rows=%d must be positive and divide M=%d", a->c_name, c.layer_rows, g.M);
    }
    if (c.msg_dtype == LDPC_MSG_I8 && !positive_finite(c.llr_scale))
        LDPC_REFUSE(LDPC_ERR_ARG, "LDPC_MSG_I8: llr_scale must be positive and finite (the LSBs per unit of channel value)");
    if (c.msg_dtype == LDPC_MSG_F8 && !accepted)
        LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "fp8 messages are built for flooding min-sum only "
                    "(the probability-domain SP needs fp32 range; BP is fp32 / fp16; the layered decoders, LAYERED_BP among them, and the "
                    "reference-reproducing ones are fp32)");
    if (c.msg_dtype == LDPC_MSG_F16 && !accepted)
        LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "fp16 messages are built for flooding min-sum and BP only "
                    "(the probability-domain SP needs fp32 range; the layered engine, LAYERED and LAYERED_BP, is fp32)");
    if (!tune_valid(c)) LDPC_REFUSE(LDPC_ERR_ARG, "tuning / streams config fields out of range");
    const Tune t = tune_from_config(c);
    /* who cannot run on the LDS-resident one-launch and the record kernels refuses to have them forced */
    if (forces_lds_kernel(t)) {
        if (bitflip)
            LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "LDPC_ALGO_BITFLIP runs the bit-flipping engine: the one-launch and the record kernels "
                        "(LDPC_TUNE_FUSED / LDPC_TUNE_LDSP forced on) are soft decoders");
        if (a->box_plus && !a->fixed)
            LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "LDPC_ALGO_BP / LDPC_ALGO_LAYERED_BP: the LDS-resident one-launch kernels and the record kernels (LDPC_TUNE_FUSED / "
                        "LDPC_TUNE_LDSP forced on) carry no box-plus check node; the streaming kernels do");
        if (one_byte_messages(c)) {
            const char *const what = c.msg_dtype == LDPC_MSG_F8 ? "fp8" : "fixed-point";
            LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "%s messages: the LDS-resident one-launch kernels and the record kernels (LDPC_TUNE_FUSED / "
                        "LDPC_TUNE_LDSP forced on) are fp32; the streaming kernels carry the %s rule", what, what);
        }
    }
    /* CRC-aided early termination: the streaming kernels carry the rule (crc_term_kernel), nothing else does */
    const bool crc_term = c.crc_kind != 0;
    if (crc_term_check(c.crc_kind, c.crc_bits, c.K, c.early_term, msg, cap < 256 ? cap : 256)) return LDPC_ERR_ARG;
    if (crc_term && !a->crc)
        LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "crc_kind: LDPC_ALGO_MS_FUSED and LDPC_ALGO_LAYERED_HOST reproduce reference kernels, which "
                    "stop on the syndrome alone; LDPC_ALGO_SP, LDPC_ALGO_MS, LDPC_ALGO_BP, LDPC_ALGO_LAYERED and LDPC_ALGO_LAYERED_BP carry the CRC rule");
    if (crc_term && forces_lds_kernel(t))
        LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "crc_kind: the LDS-resident one-launch kernels and the record kernels (LDPC_TUNE_FUSED / "
                    "LDPC_TUNE_LDSP forced on) do not carry the CRC rule; the streaming kernels do");
    if (t.fx_record && bpfx)            /* tune_valid: a fixed-point layered algorithm */
        LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "LDPC_TUNE_FX_RECORD: a box-plus row sends D independent messages and the record "
                    "kernel's two-minimum record cannot hold them; LDPC_ALGO_LAYERED_BP_FX runs the streaming layered engine");
    if (t.fx_record && crc_term)
        LDPC_REFUSE(LDPC_ERR_UNSUPPORTED, "crc_kind: the fixed-point record kernel (LDPC_TUNE_FX_RECORD) does not carry the CRC "
                    "rule; the streaming kernels do");
    return LDPC_OK;
#undef LDPC_REFUSE
}

/* ---- frames per lane ---- */
inline int pick_frames_per_lane(const ldpc_decoder_config &cfg, int32_t max_row_deg, int32_t max_col_deg)
{
    if (cfg.frames_per_lane) return cfg.frames_per_lane;
    /* Wide tiles (4 values = 16 B fp32 / 8 B fp16 per lane) once there are enough frames to
     * fill them and the register arrays of the unrolled kernels stay moderate.  Flooding check
     * kernels run in narrow waves, so only the column degree counts there; the layered kernel
     * holds a whole row (P and R) per lane. */
    const AlgoInfo *const a = algo_info(cfg.algo);
    const LaneDegree by = a ? a->lane_degree : LaneDegree::Col;
    /* fixed-point layered: a row's R is a dword and its P a dwordx2 per lane at 4 frames per lane, whatever the row degree
     * (the unrolled kernels hold the row in registers up to degree 24, the run-time kernel holds none of it) */
    if (by == LaneDegree::None) return cfg.max_batch >= 256 ? 4 : 1;
    int deg = by == LaneDegree::Row ? max_row_deg : max_col_deg;
    if (by == LaneDegree::HalfCol) deg = (deg + 1) / 2;     /* min-sum variable nodes (BP's too) need half the registers */
    /* one-byte messages (fp8, fixed point): 4 values are one dword per lane, the least a lane should move -- from one full tile on */
    if (one_byte_messages(cfg) && cfg.max_batch >= 256 && deg <= 8) return 4;
    if (cfg.max_batch >= 1024 && deg <= 8) return 4;
    if (cfg.max_batch >= 256 && deg <= kCfgUnrolledDegree) return 2;
    return 1;
}

/* ---- engines ---- */
enum class Engine {
    Flood,          /* the streaming flooding kernels (engine_flood) */
    Layered,        /* the streaming layered kernels (engine_layered) */
    Fused,          /* the LDS-resident one-launch kernels (engine_fused) */
    Ldsp,           /* the record kernels: posteriors in LDS, check records in cache (engine_ldsp) */
    LdspFx,         /* ... in fixed point (engine_ldsp_fx) */
    Bitflip         /* engine_bitflip */
};

/* An engine a configuration may run on.  Fused, Ldsp and LdspFx are taken only if their plan finds the code's structure
 * (quasi-cyclic at layer_rows, posteriors that fit LDS: the plan's `eligible`), and then only under the guards below; the
 * streaming engines and bit flipping take every graph (Layered still refuses rows of a layer that share a column, at
 * plan creation). */
struct Candidate {
    Engine engine;
    bool lds_limit;         /* Ldsp: only if its plan's LDS bytes are at most kCfgLdsLimit */
    bool needs_sp;          /* Fused under LDPC_ALGO_SP: only if the plan is eligible_sp */
};

/* The engines of a validated configuration in the order they are tried; the first whose guard holds runs.  A
 * configuration whose list runs out has none (LDPC_ALGO_MS_FUSED on a code that is not quasi-cyclic).  code != LDPC_OK:
 * a refusal that needs no plan but is made behind the device check, as it always was. */
struct Candidates {
    int n = 0;
    Candidate c[3] = {};
    int code = LDPC_OK;
    const char *refusal = nullptr;
    void add(Engine e, bool lds_limit = false, bool needs_sp = false) { c[n++] = Candidate{e, lds_limit, needs_sp}; }
};

inline Candidates engine_candidates(const ldpc_decoder_config &c, const GraphFacts &g, const Tune &t)
{
    Candidates out;
    const AlgoInfo &a = *algo_info(c.algo);
    const bool ms_corr = has_ms_corr(c), crc_term = c.crc_kind != 0;
    /* the record kernels are limited to two workgroups' worth of LDS unless the caller forces them */
    const bool lds_limit = !tune_forced_on(t.ldsp);
    /* the correction is carried by the record and the streaming kernels, not by the LDS-resident ones */
    const bool corr_on_lds_resident = ms_corr && tune_forced_on(t.fused) && tune_forced_off(t.ldsp);
    switch (a.family) {
    case Family::Bitflip:
        out.add(Engine::Bitflip);
        break;
    case Family::Reference:
        if (!packs_whole_bytes(c)) {
            out.code = LDPC_ERR_UNSUPPORTED;
            out.refusal = "MS_FUSED packs whole bytes per frame only";
            break;
        }
        /* the record kernel wherever it fits with two workgroups per CU, else the LDS-resident kernel; nothing streams */
        if (!tune_forced_off(t.ldsp)) out.add(Engine::Ldsp, lds_limit);
        out.add(Engine::Fused);
        break;
    case Family::Layered:
        if (a.fixed) {
            /* LDPC_TUNE_FX_RECORD: the fixed-point record kernel where the code fits it, the streaming engine, with the
             * same result, where it does not */
            if (t.fx_record && packs_whole_bytes(c)) out.add(Engine::LdspFx);
        } else if (c.algo == LDPC_ALGO_LAYERED) {
            if (corr_on_lds_resident) {
                out.code = LDPC_ERR_UNSUPPORTED;
                out.refusal = "ms_scale / ms_offset: the LDS-resident layered kernel (LDPC_TUNE_FUSED on, "
                              "LDPC_TUNE_LDSP off) carries no correction; the record or the streaming kernels do";
                break;
            }
            /* short quasi-cyclic codes decode in one launch: the record kernel is the default for every code it fits, the
             * LDS-resident kernel where LDPC_TUNE_LDSP is off; LDPC_TUNE_OFF(LDPC_TUNE_FUSED) keeps the streaming kernels */
            if (!crc_term && !tune_forced_off(t.fused) && packs_whole_bytes(c)) {
                if (!tune_forced_off(t.ldsp)) out.add(Engine::Ldsp);
                if (!ms_corr) out.add(Engine::Fused);
            }
        }
        /* LAYERED_HOST reproduces a reference path, and no one-launch kernel carries a float box-plus row */
        out.add(Engine::Layered);
        break;
    case Family::Flood:
        if (corr_on_lds_resident) {
            out.code = LDPC_ERR_UNSUPPORTED;
            out.refusal = "ms_scale / ms_offset: the LDS-resident flooding kernel (LDPC_TUNE_FUSED on, "
                          "LDPC_TUNE_LDSP off) carries no correction; the record or the streaming kernels do";
            break;
        }
        /* a short quasi-cyclic code (layer_rows = circulant size given) in fp32 at automatic frames per lane.  Min-sum: the
         * record kernel wherever it fits with two workgroups per CU.  The LDS-resident kernels win on latency and for
         * small batches, the streaming kernels once the batch is large: crossover near max_batch * E = 2^23 edge-frames
         * (LDPC_TUNE_FUSED forces either).  LDPC_ALGO_BP: the streaming kernels always. */
        if (!a.box_plus && !crc_term && c.msg_dtype == LDPC_MSG_F32 && c.layer_rows > 0 && c.frames_per_lane == 0 && packs_whole_bytes(c)) {
            const bool small = (int64_t)c.max_batch * g.E <= (int64_t)1 << 23;
            if (c.algo == LDPC_ALGO_MS && !tune_forced_off(t.fused) && !tune_forced_off(t.ldsp)) out.add(Engine::Ldsp, lds_limit);
            if (!ms_corr && tune_pick(t.fused, small)) out.add(Engine::Fused, false, c.algo == LDPC_ALGO_SP);
        }
        out.add(Engine::Flood);
        break;
    }
    return out;
}

}  // namespace ldpc
