/*
 * bch.hip -- the "outer code" section of the C ABI (include/ldpc_hip.h): argument checks, the plan of bch_host.hpp (kept
 * in a small cache, since its lane weights cost a few hundred modular powers) and the launches of bch_kernels.hpp.  No
 * handle and no device state: the plan travels to the kernels by value.
 */
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/ldpc_hip.h"
#include "hip_host.hpp"
#include "bch_host.hpp"
#include "bch_kernels.hpp"

using ldpc::set_error;
using ldpc::ranges_overlap;

namespace {

/* the plans of the last few (spec, direction) pairs; a plan is a pure function of its key */
struct CachedPlan {
    ldpc_bch_spec spec;
    bool decode;
    ldpc::BchPlan plan;
};
constexpr int kPlanSlots = 16;
std::mutex g_plan_mutex;
std::vector<CachedPlan> g_plans;
size_t g_plan_next = 0;

bool same_spec(const ldpc_bch_spec &a, const ldpc_bch_spec &b)
{
    return a.m == b.m && a.prim == b.prim && a.t == b.t && a.n == b.n && a.row_bytes == b.row_bytes;
}

int get_plan(const ldpc_bch_spec *s, bool decode, ldpc::BchPlan *out)
{
    if (s && s->struct_size == sizeof(ldpc_bch_spec)) {
        std::lock_guard<std::mutex> lock(g_plan_mutex);
        for (const CachedPlan &c : g_plans)
            if (c.decode == decode && same_spec(c.spec, *s)) {
                *out = c.plan;
                return LDPC_OK;
            }
    }
    char msg[240];
    ldpc::BchGen G;
    if (ldpc::bch_check_spec(s, &G, nullptr, msg, sizeof msg)) return set_error(LDPC_ERR_ARG, "%s", msg);
    ldpc::bch_make_plan(s, G, decode, out);
    std::lock_guard<std::mutex> lock(g_plan_mutex);
    if (g_plans.size() < (size_t)kPlanSlots) g_plans.push_back(CachedPlan{*s, decode, *out});
    else g_plans[g_plan_next++ % kPlanSlots] = CachedPlan{*s, decode, *out};
    return LDPC_OK;
}

int check_frames(const ldpc::BchPlan &p, int64_t frames)
{
    if (frames < 0) return set_error(LDPC_ERR_ARG, "frames = %lld is negative", (long long)frames);
    if (frames > ((int64_t)1 << 40) / p.row_bytes) return set_error(LDPC_ERR_ARG, "frames = %lld is too many", (long long)frames);
    return LDPC_OK;
}

int check_encode(const ldpc_bch_spec *s, const void *payload, int64_t frames, const void *src, int64_t src_bytes, const char *suffix,
                 ldpc::BchPlan *p)
{
    if (int rc = get_plan(s, false, p)) return rc;
    if (int rc = check_frames(*p, frames)) return rc;
    if (src_bytes < frames * p->row_bytes)
        return set_error(LDPC_ERR_ARG, "src_bytes = %lld, %lld frames of row_bytes = %d need %lld", (long long)src_bytes, (long long)frames,
                         p->row_bytes, (long long)(frames * p->row_bytes));
    if (!payload || !src) return set_error(LDPC_ERR_ARG, "payload_%s/src_%s is NULL", suffix, suffix);
    if (ranges_overlap(payload, frames * (p->k / 8), src, frames * p->row_bytes))
        return set_error(LDPC_ERR_ARG, "payload_%s and src_%s overlap", suffix, suffix);
    return LDPC_OK;
}

int check_decode(const ldpc_bch_spec *s, const void *dec, int64_t frames, const void *payload, const void *status, const char *suffix,
                 ldpc::BchPlan *p)
{
    if (int rc = get_plan(s, true, p)) return rc;
    if (int rc = check_frames(*p, frames)) return rc;
    if (!dec) return set_error(LDPC_ERR_ARG, "dec_%s is NULL", suffix);
    if (!payload && !status) return set_error(LDPC_ERR_ARG, "payload_%s and status_%s are both NULL", suffix, suffix);
    if (status && ((uintptr_t)status & 3u)) return set_error(LDPC_ERR_ARG, "status_%s is not aligned to 4 bytes", suffix);
    const int64_t in_bytes = frames * p->row_bytes, pay_bytes = frames * (p->k / 8), st_bytes = frames * 4;
    if (payload && ranges_overlap(dec, in_bytes, payload, pay_bytes)) return set_error(LDPC_ERR_ARG, "dec_%s and payload_%s overlap", suffix, suffix);
    if (status && ranges_overlap(dec, in_bytes, status, st_bytes)) return set_error(LDPC_ERR_ARG, "dec_%s and status_%s overlap", suffix, suffix);
    if (payload && status && ranges_overlap(payload, pay_bytes, status, st_bytes))
        return set_error(LDPC_ERR_ARG, "payload_%s and status_%s overlap", suffix, suffix);
    return LDPC_OK;
}

/* four frames per workgroup; at most four resident rounds of 256 CUs x 2 workgroups, the rest by striding, so that the
 * tables a workgroup builds at entry serve several frames of a large batch */
unsigned bch_grid(int64_t frames)
{
    return (unsigned)std::min<int64_t>((frames + ldpc::kBchWaves - 1) / ldpc::kBchWaves, 2048);
}

int launch_encode(const ldpc::BchPlan &p, const uint8_t *payload, int64_t frames, uint8_t *src, hipStream_t s)
{
    const unsigned grid = bch_grid(frames), block = 64 * ldpc::kBchWaves;
    if (p.t <= 4) ldpc::bch_encode_kernel<4><<<grid, block, 0, s>>>(p, payload, frames, src);
    else if (p.t <= 8) ldpc::bch_encode_kernel<8><<<grid, block, 0, s>>>(p, payload, frames, src);
    else ldpc::bch_encode_kernel<12><<<grid, block, 0, s>>>(p, payload, frames, src);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int launch_decode(const ldpc::BchPlan &p, const uint8_t *dec, int64_t frames, uint8_t *payload, int32_t *status, hipStream_t s)
{
    const unsigned grid = bch_grid(frames), block = 64 * ldpc::kBchWaves;
    if (p.t <= 4) ldpc::bch_decode_kernel<4><<<grid, block, 0, s>>>(p, dec, frames, payload, status);
    else if (p.t <= 8) ldpc::bch_decode_kernel<8><<<grid, block, 0, s>>>(p, dec, frames, payload, status);
    else ldpc::bch_decode_kernel<12><<<grid, block, 0, s>>>(p, dec, frames, payload, status);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

}  // namespace

extern "C" {

void ldpc_bch_spec_init(ldpc_bch_spec *spec, int32_t n, int32_t t, int32_t row_bytes)
{
    if (spec) ldpc::bch_spec_init(spec, n, t, row_bytes);
}

int ldpc_bch_layout(const ldpc_bch_spec *spec, int32_t out[4])
{
    char msg[240];
    ldpc::BchGen G;
    ldpc::BchLayout lay;
    if (ldpc::bch_check_spec(spec, &G, &lay, msg, sizeof msg)) return set_error(LDPC_ERR_ARG, "%s", msg);
    if (!out) return set_error(LDPC_ERR_ARG, "out is NULL");
    out[0] = lay.k; out[1] = lay.r; out[2] = lay.nmin; out[3] = lay.m;
    return LDPC_OK;
}

int ldpc_bch_generator(int32_t m, uint32_t prim, int32_t t, uint8_t *g, int32_t cap, int32_t *r)
{
    char msg[240];
    ldpc::BchGen G;
    if (ldpc::bch_make_gen(m, prim, t, &G, msg, sizeof msg)) return set_error(LDPC_ERR_ARG, "%s", msg);
    if (!g && !r) return set_error(LDPC_ERR_ARG, "g and r are both NULL");
    if (r) *r = G.r;
    if (g) {
        if (cap < G.r + 1) return set_error(LDPC_ERR_ARG, "cap = %d, the generator has r + 1 = %d coefficients", cap, G.r + 1);
        for (int i = 0; i <= G.r; ++i) g[i] = (uint8_t)ldpc::bch_poly_bit(G.g, i);
    }
    return LDPC_OK;
}

int ldpc_bch_encode_device(const ldpc_bch_spec *spec, const uint8_t *payload_dev, int64_t frames, uint8_t *src_dev, int64_t src_bytes,
                           int32_t device, void *stream)
{
    ldpc::BchPlan p;
    if (int rc = check_encode(spec, payload_dev, frames, src_dev, src_bytes, "dev", &p)) return rc;
    if (frames == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(device));
    return launch_encode(p, payload_dev, frames, src_dev, (hipStream_t)stream);
}

int ldpc_bch_decode_device(const ldpc_bch_spec *spec, const uint8_t *dec_dev, int64_t frames, uint8_t *payload_dev, int32_t *status_dev,
                           int32_t device, void *stream)
{
    ldpc::BchPlan p;
    if (int rc = check_decode(spec, dec_dev, frames, payload_dev, status_dev, "dev", &p)) return rc;
    if (frames == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(device));
    return launch_decode(p, dec_dev, frames, payload_dev, status_dev, (hipStream_t)stream);
}

int ldpc_bch_tally_device(const int32_t *status_dev, const uint8_t *payload_dev, const uint8_t *ref_dev, int64_t frames,
                          int64_t bytes_per_frame, int64_t counts[6], int32_t device, void *stream)
{
    if (!status_dev || !payload_dev || !counts) return set_error(LDPC_ERR_ARG, "status_dev/payload_dev/counts is NULL");
    if ((uintptr_t)status_dev & 3u) return set_error(LDPC_ERR_ARG, "status_dev is not aligned to 4 bytes");
    if (frames < 0) return set_error(LDPC_ERR_ARG, "frames = %lld is negative", (long long)frames);
    if (bytes_per_frame <= 0) return set_error(LDPC_ERR_ARG, "bytes_per_frame = %lld must be positive", (long long)bytes_per_frame);
    for (int i = 0; i < 6; ++i) counts[i] = 0;
    if (frames == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    ldpc::DevBuf<unsigned long long> totals;
    LDPC_HIP_TRY(totals.alloc(6));
    hipError_t e = hipMemsetAsync(totals.p, 0, 6 * sizeof(unsigned long long), s);
    if (e == hipSuccess) {
        ldpc::bch_tally_kernel<<<(unsigned)std::min<int64_t>(frames, ldpc::kFrameTargetBlocks), 256, 0, s>>>(status_dev, payload_dev, ref_dev,
                                                                                                         frames, bytes_per_frame, totals.p);
        e = hipGetLastError();
    }
    unsigned long long h[6] = {0, 0, 0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(h, totals.p, sizeof h, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return set_error(LDPC_ERR_HIP, "bch_tally: %s", hipGetErrorString(e));
    for (int i = 0; i < 6; ++i) counts[i] = (int64_t)h[i];
    return LDPC_OK;
}

int ldpc_bch_encode(const ldpc_bch_spec *spec, const uint8_t *payload_host, int64_t frames, uint8_t *src_host, int64_t src_bytes,
                    int32_t device)
{
    ldpc::BchPlan p;
    if (int rc = check_encode(spec, payload_host, frames, src_host, src_bytes, "host", &p)) return rc;
    if (frames == 0) return LDPC_OK;
    if (int rc = ldpc::use_device(device, "the outer-code stage")) return rc;
    return ldpc::host_chunks(frames, {{(void *)payload_host, (int64_t)p.k / 8, true, false}, {src_host, (int64_t)p.row_bytes, false, true}},
                             [&](int64_t n, int64_t, void *const *dev) {
                                 return launch_encode(p, (const uint8_t *)dev[0], n, (uint8_t *)dev[1], nullptr);
                             });
}

int ldpc_bch_decode(const ldpc_bch_spec *spec, const uint8_t *dec_host, int64_t frames, uint8_t *payload_host, int32_t *status_host,
                    int32_t device)
{
    ldpc::BchPlan p;
    if (int rc = check_decode(spec, dec_host, frames, payload_host, status_host, "host", &p)) return rc;
    if (frames == 0) return LDPC_OK;
    if (int rc = ldpc::use_device(device, "the outer-code stage")) return rc;
    return ldpc::host_chunks(frames,
                             {{(void *)dec_host, (int64_t)p.row_bytes, true, false}, {payload_host, (int64_t)p.k / 8, false, true},
                              {status_host, 4, false, true}},
                             [&](int64_t n, int64_t, void *const *dev) {
                                 return launch_decode(p, (const uint8_t *)dev[0], n, (uint8_t *)dev[1], (int32_t *)dev[2], nullptr);
                             });
}

}  // extern "C"
