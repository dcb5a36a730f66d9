/*
 * channel.hip -- the entry points of the C ABI (include/ldpc_hip.h) that need no decoder: the AWGN channel and the
 * error counter of channel_kernels.hpp, and the two measurement aids that report what the device's HBM sustains.
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/ldpc_hip.h"
#include "channel_kernels.hpp"
#include "flood_common.hpp"    /* ldpc::vf4 */
#include "hip_host.hpp"

using ldpc::set_error;

namespace {

/* a plain float4 copy (the measurement aid ldpc_hbm_probe_device) */
template <bool NT>
__global__ __launch_bounds__(256) void hbm_probe_copy_kernel(const ldpc::vf4 *__restrict__ src, ldpc::vf4 *__restrict__ dst, size_t n4)
{
    const size_t stride = (size_t)gridDim.x * 256 * 4;
    for (size_t i = (size_t)blockIdx.x * 256 * 4 + threadIdx.x; i < n4; i += stride) {
        ldpc::vf4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + (size_t)k * 256 < n4) v[k] = NT ? __builtin_nontemporal_load(&src[i + (size_t)k * 256]) : src[i + (size_t)k * 256];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + (size_t)k * 256 < n4) {
                if (NT) __builtin_nontemporal_store(v[k], &dst[i + (size_t)k * 256]);
                else dst[i + (size_t)k * 256] = v[k];
            }
    }
}

/* what the two probes share: the two arrays (the source filled), a stream and two events */
struct ProbeRig {
    ldpc::Stream stream;                /* before the arrays and events: they go first */
    ldpc::DevBuf<ldpc::vf4> src, dst;
    size_t n4 = 0;
    ldpc::Event a, b;
    hipError_t open(int64_t bytes)
    {
        n4 = (size_t)bytes / sizeof(ldpc::vf4);
        hipError_t e = src.alloc(n4);
        if (e == hipSuccess) e = dst.alloc(n4);
        if (e == hipSuccess) e = stream.create();
        if (e == hipSuccess) e = a.create();
        if (e == hipSuccess) e = b.create();
        if (e == hipSuccess) e = hipMemsetAsync(src.p, 0x3c, n4 * sizeof(ldpc::vf4), stream.s);
        return e;
    }
};

}  // namespace

extern "C" {

int ldpc_awgn_device(float *llr_dev, int64_t frames, int32_t N, const uint8_t *bits_dev, float sd,
                     uint64_t seed, int64_t first_frame, int32_t device, void *stream)
{
    if (!llr_dev) return set_error(LDPC_ERR_ARG, "llr_dev is NULL");
    if (frames < 0 || N <= 0 || first_frame < 0) return set_error(LDPC_ERR_ARG, "frames=%lld, N=%d, first_frame=%lld",
                                                             (long long)frames, N, (long long)first_frame);
    if (!(sd >= 0.0f)) return set_error(LDPC_ERR_ARG, "sd must be >= 0");
    if (frames == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(device));
    const int32_t groups = (N + 3) / 4;
    const int64_t threads = frames * groups;
    const int64_t blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffLL) return set_error(LDPC_ERR_ARG, "too many samples for one call");
    ldpc::awgn_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(llr_dev, bits_dev, frames, N, groups, sd,
                                                                         seed, first_frame);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int ldpc_count_errors_device(const uint8_t *out_dev, const uint8_t *ref_dev, int64_t frames,
                             int64_t bytes_per_frame, int64_t errors[3], int32_t device, void *stream)
{
    if (!out_dev || !errors) return set_error(LDPC_ERR_ARG, "out_dev/errors is NULL");
    if (frames < 0 || bytes_per_frame <= 0 || frames > 0x7fffffffLL) return set_error(LDPC_ERR_ARG, "bad frames/bytes_per_frame");
    errors[0] = errors[1] = errors[2] = 0;
    if (frames == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    ldpc::DevBuf<unsigned long long> totals;
    LDPC_HIP_TRY(totals.alloc(3));
    hipError_t e = hipMemsetAsync(totals.p, 0, 3 * sizeof(unsigned long long), s);
    if (e == hipSuccess) {
        ldpc::count_errors_kernel<<<(unsigned)frames, 256, 0, s>>>(out_dev, ref_dev, frames, bytes_per_frame, totals.p);
        e = hipGetLastError();
    }
    unsigned long long h[3] = {0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(h, totals.p, sizeof h, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return set_error(LDPC_ERR_HIP, "count_errors: %s", hipGetErrorString(e));
    for (int i = 0; i < 3; ++i) errors[i] = (int64_t)h[i];
    return LDPC_OK;
}

/* ---- measurement aid: what this box's HBM sustains right now (a float4 copy: the figure the
 *      microarchitecture guide quotes as achievable, 6.3 of 8.0 TB/s), with the default cache policy
 *      and with the non-temporal one the streaming kernels use; the better of the two ------------ */

int ldpc_hbm_probe_device(int32_t device, int64_t bytes, int32_t reps, double *copy_gbs, double *by_policy)
{
    if (!copy_gbs) return set_error(LDPC_ERR_ARG, "copy_gbs is NULL");
    *copy_gbs = 0.0;
    if (by_policy) by_policy[0] = by_policy[1] = 0.0;
    if (bytes < (1 << 20) || bytes > ((int64_t)16 << 30) || reps <= 0 || reps > 1000)
        return set_error(LDPC_ERR_ARG, "probe: bytes in [1 MiB, 16 GiB], reps in [1, 1000]");
    LDPC_HIP_TRY(hipSetDevice(device));
    ProbeRig rig;
    hipError_t e = rig.open(bytes);
    const size_t n4 = rig.n4;
    ldpc::vf4 *const src = rig.src.p, *const dst = rig.dst.p;
    const hipStream_t s = rig.stream.s;
    const hipEvent_t a = rig.a.e, b = rig.b.e;
    float best_ms[2] = {0.0f, 0.0f};                             /* default policy, non-temporal */
    if (e == hipSuccess) {
        const unsigned grid = (unsigned)std::min<size_t>((n4 + 1023) / 1024, 256 * 64);
        hbm_probe_copy_kernel<false><<<grid, 256, 0, s>>>(src, dst, n4);        /* warm-up */
        for (int r = 0; r < 2 * reps && e == hipSuccess; ++r) {
            e = hipEventRecord(a, s);
            if (r & 1) hbm_probe_copy_kernel<true><<<grid, 256, 0, s>>>(src, dst, n4);
            else hbm_probe_copy_kernel<false><<<grid, 256, 0, s>>>(src, dst, n4);
            if (e == hipSuccess) e = hipEventRecord(b, s);
            if (e == hipSuccess) e = hipEventSynchronize(b);
            float ms = 0.0f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
            if (e == hipSuccess && (best_ms[r & 1] == 0.0f || ms < best_ms[r & 1])) best_ms[r & 1] = ms;
        }
    }
    if (e != hipSuccess) return set_error(LDPC_ERR_HIP, "hbm probe: %s", hipGetErrorString(e));
    for (int k = 0; k < 2; ++k) {
        const double gbs = best_ms[k] > 0.0f ? 2.0 * (double)(n4 * sizeof(ldpc::vf4)) / (best_ms[k] * 1e-3) / 1e9 : 0.0;
        if (by_policy) by_policy[k] = gbs;
        if (gbs > *copy_gbs) *copy_gbs = gbs;
    }
    return LDPC_OK;
}

/* The same non-temporal copy, back to back for `milliseconds`: what the box sustains (its memory throttles
 * under load at times: a burst of a few launches does not see that). */
int ldpc_hbm_sustained_device(int32_t device, int64_t bytes, int32_t milliseconds, double *copy_gbs)
{
    if (!copy_gbs) return set_error(LDPC_ERR_ARG, "copy_gbs is NULL");
    *copy_gbs = 0.0;
    if (bytes < (1 << 20) || bytes > ((int64_t)16 << 30) || milliseconds < 1 || milliseconds > 10000)
        return set_error(LDPC_ERR_ARG, "sustained probe: bytes in [1 MiB, 16 GiB], milliseconds in [1, 10000]");
    LDPC_HIP_TRY(hipSetDevice(device));
    ProbeRig rig;
    hipError_t e = rig.open(bytes);
    const size_t n4 = rig.n4;
    ldpc::vf4 *const src = rig.src.p, *const dst = rig.dst.p;
    const hipStream_t s = rig.stream.s;
    const hipEvent_t a = rig.a.e, b = rig.b.e;
    const unsigned grid = (unsigned)std::min<size_t>((n4 + 1023) / 1024, 256 * 64);
    /* one launch's time from a short burst, then a third of the time untimed and two thirds timed */
    float one_ms = 0.0f;
    if (e == hipSuccess) {
        hbm_probe_copy_kernel<true><<<grid, 256, 0, s>>>(src, dst, n4);
        e = hipEventRecord(a, s);
        for (int r = 0; r < 4; ++r) hbm_probe_copy_kernel<true><<<grid, 256, 0, s>>>(src, dst, n4);
        if (e == hipSuccess) e = hipEventRecord(b, s);
        if (e == hipSuccess) e = hipEventSynchronize(b);
        if (e == hipSuccess) e = hipEventElapsedTime(&one_ms, a, b);
        one_ms /= 4.0f;
    }
    int timed = 0;
    float ms = 0.0f;
    if (e == hipSuccess && one_ms > 0.0f) {
        const int total = std::max(6, std::min(200000, (int)((float)milliseconds / one_ms)));
        const int lead = total / 3;
        timed = total - lead;
        for (int r = 0; r < lead; ++r) hbm_probe_copy_kernel<true><<<grid, 256, 0, s>>>(src, dst, n4);
        e = hipEventRecord(a, s);
        for (int r = 0; r < timed; ++r) hbm_probe_copy_kernel<true><<<grid, 256, 0, s>>>(src, dst, n4);
        if (e == hipSuccess) e = hipEventRecord(b, s);
        if (e == hipSuccess) e = hipEventSynchronize(b);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
    }
    if (e != hipSuccess) return set_error(LDPC_ERR_HIP, "hbm sustained probe: %s", hipGetErrorString(e));
    if (ms > 0.0f) *copy_gbs = 2.0 * (double)(n4 * sizeof(ldpc::vf4)) * timed / (ms * 1e-3) / 1e9;
    return LDPC_OK;
}

}  /* extern "C" */
