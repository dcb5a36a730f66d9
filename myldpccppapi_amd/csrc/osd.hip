/*
 * osd.hip -- the "ordered-statistics post-processing" section of the C ABI (include/ldpc_hip.h): the handle (dense bit
 * image of H, the graph's rows for the syndrome, one dirty flag per frame), the argument checks and the two launches of
 * osd_kernels.hpp.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "../../include/ldpc_hip.h"
#include "graph.hpp"
#include "hip_host.hpp"
#include "osd_host.hpp"
#include "osd_kernels.hpp"

using ldpc::set_error;
using ldpc::ranges_overlap;
using ldpc::DevBuf;

struct ldpc_osd {
    int32_t device = -1;       /* -1: created on a machine without a device; the compute calls answer LDPC_ERR_HIP */
    int32_t M = 0, N = 0, K = 0, max_frames = 0;
    ldpc::OsdLayout lay;
    DevBuf<uint32_t> image;
    DevBuf<int32_t> row_ptr, cols;
    DevBuf<uint8_t> flag;
    /* ldpc_osd_run(): made on its first call */
    DevBuf<float> soft_stage;
    DevBuf<uint8_t> out_stage, code_stage;
    DevBuf<int32_t> status_stage, metric_stage;
};

namespace {

int check_call(const ldpc_osd *o, const void *soft, int64_t frames, int32_t order, float weight_scale, const void *out, int64_t out_bytes,
               const void *code, const void *status, const void *metric, bool chunked, const char *suffix)
{
    if (!o) return set_error(LDPC_ERR_ARG, "osd handle is NULL");
    if (order != 0 && order != 1) return set_error(LDPC_ERR_ARG, "order = %d: orders 0 and 1 are built", order);
    if (!std::isfinite(weight_scale) || !(weight_scale > 0.0f))
        return set_error(LDPC_ERR_ARG, "weight_scale = %g must be finite and positive", (double)weight_scale);
    if (frames < 0) return set_error(LDPC_ERR_ARG, "frames = %lld is negative", (long long)frames);
    if (!chunked && frames > o->max_frames)
        return set_error(LDPC_ERR_ARG, "frames = %lld exceeds max_frames = %d", (long long)frames, o->max_frames);
    if (frames > ((int64_t)1 << 40) / o->N) return set_error(LDPC_ERR_ARG, "frames = %lld is too many", (long long)frames);
    if (!out && !code && !status && !metric)
        return set_error(LDPC_ERR_ARG, "out_%s, code_%s, status_%s and metric_%s are all NULL", suffix, suffix, suffix, suffix);
    const int64_t out_need = frames * (int64_t)(o->K / 8);
    if (out) {
        if (o->K % 8) return set_error(LDPC_ERR_ARG, "out_%s needs K %% 8 == 0 (K = %d)", suffix, o->K);
        if (out_bytes < out_need)
            return set_error(LDPC_ERR_ARG, "out_bytes = %lld, %lld frames of K = %d need %lld", (long long)out_bytes, (long long)frames, o->K,
                             (long long)out_need);
    }
    if (frames == 0) return LDPC_OK;
    if (!soft) return set_error(LDPC_ERR_ARG, "soft_%s is NULL", suffix);
    if ((uintptr_t)soft & 3u) return set_error(LDPC_ERR_ARG, "soft_%s is not aligned to 4 bytes", suffix);
    if (status && ((uintptr_t)status & 3u)) return set_error(LDPC_ERR_ARG, "status_%s is not aligned to 4 bytes", suffix);
    if (metric && ((uintptr_t)metric & 3u)) return set_error(LDPC_ERR_ARG, "metric_%s is not aligned to 4 bytes", suffix);
    const int64_t soft_bytes = frames * (int64_t)o->N * 4;
    const struct { const void *p; int64_t bytes; const char *name; } outs[4] = {
        {out, out_need, "out"}, {code, frames * (int64_t)o->N, "code"}, {status, frames * 4, "status"}, {metric, frames * 4, "metric"}};
    for (int i = 0; i < 4; ++i) {
        if (!outs[i].p) continue;
        if (ranges_overlap(soft, soft_bytes, outs[i].p, outs[i].bytes))
            return set_error(LDPC_ERR_ARG, "%s_%s overlaps soft_%s", outs[i].name, suffix, suffix);
        for (int j = i + 1; j < 4; ++j)
            if (outs[j].p && ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
                return set_error(LDPC_ERR_ARG, "%s_%s overlaps %s_%s", outs[i].name, suffix, outs[j].name, suffix);
    }
    return LDPC_OK;
}

int need_device(const ldpc_osd *o)
{
    if (o->device < 0) return set_error(LDPC_ERR_HIP, "no usable HIP device (ordered-statistics decoding has no CPU fallback)");
    LDPC_HIP_TRY(hipSetDevice(o->device));
    return LDPC_OK;
}

int enqueue(ldpc_osd *o, const float *soft, int64_t frames, int32_t order, float scale, uint8_t *out, uint8_t *code, int32_t *status,
            int32_t *metric, hipStream_t s)
{
    const ldpc::OsdOut oo{out, code, status, metric, o->N, o->K};
    const ldpc::OsdFlagArgs fa{soft, frames, o->row_ptr.p, o->cols.p, o->M, o->flag.p, oo};
    ldpc::osd_flag_kernel<<<(unsigned)std::min<int64_t>(frames, 4096), ldpc::kOsdFlagBlock, 0, s>>>(fa);
    const ldpc::OsdArgs ka{soft, o->image.p, o->flag.p, o->lay, order, scale, oo};
    ldpc::osd_kernel<<<(unsigned)frames, (unsigned)ldpc::osd_block(o->lay.W), o->lay.bytes(), s>>>(ka);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

}  // namespace

extern "C" {

int ldpc_osd_create(const ldpc_graph *g, int32_t K, int32_t max_frames, int32_t device, ldpc_osd **out)
{
    if (!out) return set_error(LDPC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!g) return set_error(LDPC_ERR_ARG, "graph is NULL");
    if (K <= 0 || K > g->N) return set_error(LDPC_ERR_ARG, "K = %d outside (0, N = %d]", K, g->N);
    if (max_frames <= 0) return set_error(LDPC_ERR_ARG, "max_frames = %d must be positive", max_frames);
    if (device < 0) return set_error(LDPC_ERR_ARG, "device = %d is negative", device);
    char msg[320];
    if (ldpc::osd_eligible(g->M, g->N, msg, sizeof msg)) return set_error(LDPC_ERR_UNSUPPORTED, "%s", msg);
    ldpc::OsdImage im;
    ldpc::osd_dense_image(g->M, g->N, g->row_ptr.data(), g->cols.data(), &im);
    ldpc_osd *o = new (std::nothrow) ldpc_osd;
    if (!o) return set_error(LDPC_ERR_NOMEM, "out of memory");
    o->M = g->M; o->N = g->N; o->K = K; o->max_frames = max_frames;
    o->lay = ldpc::osd_layout(im.R, g->N);
    /* no second eligibility rule: with R <= N rows in the image the layout of an eligible code always fits
     * (tests/cpp/osd_host_test.cpp walks the corners); a layout that does not is a defect of this library */
    if (o->lay.bytes() > ldpc::kOsdMaxLds) {
        const size_t bytes = o->lay.bytes();
        delete o;
        return set_error(LDPC_ERR_STATE, "internal: the LDS layout of an eligible code needs %zu bytes, more than %zu", bytes, ldpc::kOsdMaxLds);
    }
    /* a machine without a device still gets its handle: the argument checks of the compute calls answer there */
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        *out = o;
        return LDPC_OK;
    }
    if (device >= count) {
        delete o;
        return set_error(LDPC_ERR_ARG, "device %d of %d", device, count);
    }
    hipError_t err = hipSetDevice(device);
    if (err == hipSuccess) err = o->image.upload(im.bits);
    if (err == hipSuccess) err = o->row_ptr.upload(g->row_ptr);
    if (err == hipSuccess) err = o->cols.upload(g->cols);
    if (err == hipSuccess) err = o->flag.alloc((size_t)max_frames);
    if (err == hipSuccess)
        err = hipFuncSetAttribute((const void *)ldpc::osd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldpc::kOsdMaxLds);
    if (err != hipSuccess) {
        delete o;
        return set_error(err == hipErrorOutOfMemory ? LDPC_ERR_NOMEM : LDPC_ERR_HIP, "osd buffers: %s", hipGetErrorString(err));
    }
    o->device = device;
    *out = o;
    return LDPC_OK;
}

int ldpc_osd_destroy(ldpc_osd *o)
{
    if (!o) return LDPC_OK;
    if (o->device >= 0) {
        (void)hipSetDevice(o->device);
        (void)hipDeviceSynchronize();
    }
    delete o;
    return LDPC_OK;
}

int ldpc_osd_info(const ldpc_osd *o, int32_t out[4])
{
    if (!o) return set_error(LDPC_ERR_ARG, "osd handle is NULL");
    if (!out) return set_error(LDPC_ERR_ARG, "out is NULL");
    out[0] = o->M; out[1] = o->N; out[2] = o->lay.W; out[3] = (int32_t)o->lay.bytes();
    return LDPC_OK;
}

int ldpc_osd_device(ldpc_osd *o, const float *soft_dev, int64_t frames, int32_t order, float weight_scale, uint8_t *out_dev,
                    int64_t out_bytes, uint8_t *code_dev, int32_t *status_dev, int32_t *metric_dev, void *stream)
{
    if (int rc = check_call(o, soft_dev, frames, order, weight_scale, out_dev, out_bytes, code_dev, status_dev, metric_dev, false, "dev"))
        return rc;
    if (frames == 0) return LDPC_OK;
    if (int rc = need_device(o)) return rc;
    return enqueue(o, soft_dev, frames, order, weight_scale, out_dev, code_dev, status_dev, metric_dev, (hipStream_t)stream);
}

int ldpc_osd_run(ldpc_osd *o, const float *soft_host, int64_t frames, int32_t order, float weight_scale, uint8_t *out_host,
                 int64_t out_bytes, uint8_t *code_host, int32_t *status_host, int32_t *metric_host)
{
    if (int rc = check_call(o, soft_host, frames, order, weight_scale, out_host, out_bytes, code_host, status_host, metric_host, true, "host"))
        return rc;
    if (frames == 0) return LDPC_OK;
    if (int rc = need_device(o)) return rc;
    const int64_t B = o->max_frames, N = o->N, nb = o->K / 8;
    LDPC_HIP_TRY(o->soft_stage.ensure((size_t)(B * N)));
    if (out_host) LDPC_HIP_TRY(o->out_stage.ensure((size_t)std::max<int64_t>(B * nb, 1)));
    if (code_host) LDPC_HIP_TRY(o->code_stage.ensure((size_t)(B * N)));
    if (status_host) LDPC_HIP_TRY(o->status_stage.ensure((size_t)B));
    if (metric_host) LDPC_HIP_TRY(o->metric_stage.ensure((size_t)B));
    for (int64_t f0 = 0; f0 < frames; f0 += B) {
        const int64_t n = std::min(B, frames - f0);
        LDPC_HIP_TRY(hipMemcpy(o->soft_stage.p, soft_host + f0 * N, (size_t)(n * N) * sizeof(float), hipMemcpyHostToDevice));
        if (int rc = enqueue(o, o->soft_stage.p, n, order, weight_scale, out_host ? o->out_stage.p : nullptr,
                             code_host ? o->code_stage.p : nullptr, status_host ? o->status_stage.p : nullptr,
                             metric_host ? o->metric_stage.p : nullptr, nullptr))
            return rc;
        if (out_host) LDPC_HIP_TRY(hipMemcpy(out_host + f0 * nb, o->out_stage.p, (size_t)(n * nb), hipMemcpyDeviceToHost));
        if (code_host) LDPC_HIP_TRY(hipMemcpy(code_host + f0 * N, o->code_stage.p, (size_t)(n * N), hipMemcpyDeviceToHost));
        if (status_host) LDPC_HIP_TRY(hipMemcpy(status_host + f0, o->status_stage.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (metric_host) LDPC_HIP_TRY(hipMemcpy(metric_host + f0, o->metric_stage.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    return LDPC_OK;
}

}  // extern "C"
