/*
 * llr_input.hip -- the launches of llr_input.hpp that belong to no engine: the widen pass in front of the one-launch and
 * record kernels (engine_llr_widen, called by the driver for a typed call on such a handle) and the quantiser of the C ABI
 * (ldpc_llr_quantize_device).  The streaming engines read narrow channel values themselves (flood_round.hpp: init_kernel,
 * layered_kernels.hpp: layered_init_kernel).
 */
#include <hip/hip_runtime.h>

#include "../../include/ldpc_hip.h"
#include "engines.hpp"
#include "hip_host.hpp"
#include "llr_input.hpp"

using ldpc::set_error;

static_assert(ldpc::kLlrF32 == LDPC_LLR_F32 && ldpc::kLlrF16 == LDPC_LLR_F16 && ldpc::kLlrI8 == LDPC_LLR_I8,
              "llr_input.hpp restates enum ldpc_llr_type");

hipError_t ldpc::engine_llr_widen(const LlrIn &in, float *y_dev, int64_t count, hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    const int64_t blocks = (count + 255) / 256;
    if (blocks > 0x7fffffffLL || in.type == kLlrF32) return hipErrorInvalidValue;
    if (in.type == kLlrI8)
        llr_widen_kernel<int8_t><<<(unsigned)blocks, 256, 0, s>>>(static_cast<const int8_t *>(in.p), in.unit, y_dev, count);
    else
        llr_widen_kernel<_Float16><<<(unsigned)blocks, 256, 0, s>>>(static_cast<const _Float16 *>(in.p), in.unit, y_dev, count);
    return hipGetLastError();
}

extern "C" {

int ldpc_llr_quantize_device(const float *y_dev, int64_t count, int32_t llr_type, float llr_unit, void *out_dev,
                             int32_t device, void *stream)
{
    if (llr_type != LDPC_LLR_I8 && llr_type != LDPC_LLR_F16)
        return set_error(LDPC_ERR_ARG, "llr_type %d: the quantiser produces LDPC_LLR_I8 or LDPC_LLR_F16", llr_type);
    if (!(llr_unit > 0.0f && llr_unit <= 3.402823466e38f)) return set_error(LDPC_ERR_ARG, "llr_unit must be positive and finite");
    if (count < 0) return set_error(LDPC_ERR_ARG, "count < 0");
    if (count == 0) return LDPC_OK;
    if (!y_dev || !out_dev) return set_error(LDPC_ERR_ARG, "y_dev/out_dev is NULL");
    if (reinterpret_cast<uintptr_t>(y_dev) & 3) return set_error(LDPC_ERR_ARG, "y_dev is not 4-byte aligned");
    if (llr_type == LDPC_LLR_F16 && (reinterpret_cast<uintptr_t>(out_dev) & 1))
        return set_error(LDPC_ERR_ARG, "out_dev: fp16 values need 2-byte alignment");
    const uintptr_t y0 = reinterpret_cast<uintptr_t>(y_dev), y1 = y0 + (uintptr_t)count * 4;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(out_dev), o1 = o0 + (uintptr_t)count * ldpc::llr_elem_size(llr_type);
    if (y0 < o1 && o0 < y1) return set_error(LDPC_ERR_ARG, "y_dev and out_dev overlap");
    const int64_t blocks = (count + 255) / 256;
    if (blocks > 0x7fffffffLL) return set_error(LDPC_ERR_ARG, "too many values for one call");
    LDPC_HIP_TRY(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    if (llr_type == LDPC_LLR_I8)
        ldpc::llr_quantize_kernel<int8_t><<<(unsigned)blocks, 256, 0, s>>>(y_dev, llr_unit, static_cast<int8_t *>(out_dev), count);
    else
        ldpc::llr_quantize_kernel<_Float16><<<(unsigned)blocks, 256, 0, s>>>(y_dev, llr_unit, static_cast<_Float16 *>(out_dev), count);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

}  /* extern "C" */
