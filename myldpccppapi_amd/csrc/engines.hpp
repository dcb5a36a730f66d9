/*
 * engines.hpp -- the entry points of the engines that instantiate kernels, compiled in translation units of
 * their own (engine_ldsp.hip, engine_ldsp_fx.hip, engine_fused.hip, engine_layered.hip, engine_layered_fx.hip, engine_layered_bpfx.hip, engine_bitflip.hip, engine_flood.hip) so that the library
 * builds in parallel.  The host driver calls these instead of the inline functions of the kernel headers;
 * plan structs and everything without kernels stay in the headers.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "tune.hpp"
#include "llr_input.hpp"

struct ldpc_decoder;
struct ldpc_graph;

namespace ldpc {

struct LdspPlan;
struct FusedPlan;
struct FusedRun;
struct LayeredPlan;
struct LayeredRun;
struct BitflipPlan;
struct BitflipRun;

/* What one call hands a streaming engine that keeps its state in the handle's own arrays (layered, bit flipping): the
 * host driver fills it in one place; LayeredRun and BitflipRun add what is their own. */
struct StreamRun {
    /* optional per-launch timing hooks (HIP events on the decode stream) */
    hipError_t (*span_begin)(void *ctx, hipStream_t s, int kind, int degree, int64_t bytes) = nullptr;
    hipError_t (*span_end)(void *ctx, hipStream_t s) = nullptr;
    void *span_ctx = nullptr;
    LlrIn llr;                      /* the caller's channel values: pointer, element type, unit (llr_input.hpp) */
    int64_t frames;
    uint8_t *out_dev;
    int64_t out_bytes;
    int32_t *iters_dev;
    int32_t K, max_iter, tap_iter, early_term, pack_mode;
    uint64_t *hard, *failw, *done;  /* [T][N][V], [max_iter + 2][T][V], [T][V] */
    int32_t *iters;
    const int32_t *row_ptr, *edge_col;
    int32_t *summary;
    /* CRC-aided early termination (ldpc_decoder_config::crc_kind): column weights and covered bits, 0 = off */
    const uint32_t *crc_w = nullptr;
    int32_t crc_bits = 0;
};

hipError_t engine_ldsp_plan_create(LdspPlan *pl, int32_t M, int32_t N, int64_t E, const std::vector<int32_t> &row_ptr,
                                   const std::vector<int32_t> &cols, int32_t z, int32_t K, int64_t max_batch, int device,
                                   const Tune &tune, int flood);
hipError_t engine_ldsp_run(LdspPlan *pl, const FusedRun &r, hipStream_t s, int32_t *launched);
/* engine_ldsp_fx.hip: layered_ldsp_fx_kernel (ldsp_fx_kernels.hpp), LDPC_ALGO_LAYERED_FX on the record organisation */
hipError_t engine_ldsp_fx_plan_create(LdspPlan *pl, int32_t M, int32_t N, int64_t E, const std::vector<int32_t> &row_ptr,
                                      const std::vector<int32_t> &cols, int32_t z, int32_t K, int64_t max_batch, int device,
                                      const Tune &tune);
hipError_t engine_ldsp_fx_run(LdspPlan *pl, const FusedRun &r, hipStream_t s, int32_t *launched);
hipError_t engine_fused_run(FusedPlan *pl, const FusedRun &r, hipStream_t s, int32_t *launched);
/* every rule of the streaming layered engine (LayeredPlan::rule); engine_layered_fx.hip holds the fixed-point storage's half,
 * engine_layered_bpfx.hip the kernels of the fixed-point box-plus rule */
hipError_t engine_layered_run(LayeredPlan *pl, const LayeredRun &r, hipStream_t s, int32_t *launched);
/* engine_bitflip.hip: LDPC_ALGO_BITFLIP, bits only (bitflip_kernels.hpp) */
hipError_t engine_bitflip_run(BitflipPlan *pl, const BitflipRun &r, hipStream_t s, int32_t *launched);
/* llr_input.hip: y[i] = x[i] * unit for count elements of a narrow type (LlrIn::type != kLlrF32), enqueued on s */
hipError_t engine_llr_widen(const LlrIn &in, float *y_dev, int64_t count, hipStream_t s);

/* The streaming flooding engine works on the handle (decoder.hpp: ldpc_decoder::flood) and returns LDPC_* codes with
 * the message set.  setup: message arrays of TF frames, work lists, kernel tables, launch plan and, for a decoder that
 * is no hand-over child (top_level), link calibration and placement search. */
int engine_flood_setup(ldpc_decoder *d, const ldpc_graph *g, size_t TF, bool top_level);
int engine_flood_run(ldpc_decoder *d, const LlrIn &llr, int64_t frames, uint8_t *out_dev, int64_t out_bytes,
                     int32_t *iters_dev, hipStream_t s);

}  // namespace ldpc
