/*
 * tb.hip -- the "transport block" section of the C ABI (include/ldpc_hip.h): argument checks, the plan of tb_host.hpp and
 * the launches of tb_kernels.hpp.  No handle and no device state: the plan travels to the kernels by value.
 */
#include <hip/hip_runtime.h>

#include "../../include/ldpc_hip.h"
#include "hip_host.hpp"
#include "tb_host.hpp"
#include "crc_term_host.hpp"
#include "tb_kernels.hpp"

using ldpc::set_error;
using ldpc::frame_grid;
using ldpc::ranges_overlap;

namespace {

int check_spec(const ldpc_tb_spec *s, ldpc::TbLayout *lay)
{
    char msg[200];
    if (ldpc::tb_check_spec(s, lay, msg, sizeof msg)) return set_error(LDPC_ERR_ARG, "%s", msg);
    return LDPC_OK;
}

struct Sizes {
    int64_t prow, frow, frames;
};

int check_tbs(const ldpc_tb_spec *s, int64_t tbs, Sizes *z)
{
    if (tbs < 0) return set_error(LDPC_ERR_ARG, "tbs = %lld is negative", (long long)tbs);
    if (tbs > ((int64_t)1 << 40) / s->C) return set_error(LDPC_ERR_ARG, "tbs = %lld times C = %d is too many frames", (long long)tbs, s->C);
    z->prow = s->A / 8;
    z->frow = s->K / 8;
    z->frames = tbs * s->C;
    return LDPC_OK;
}

int check_attach(const ldpc_tb_spec *s, const void *payload, int64_t tbs, const void *src, int64_t src_bytes, const char *in,
                 const char *out, ldpc::TbLayout *lay, Sizes *z)
{
    if (int rc = check_spec(s, lay)) return rc;
    if (int rc = check_tbs(s, tbs, z)) return rc;
    if (src_bytes < z->frames * z->frow)
        return set_error(LDPC_ERR_ARG, "src_bytes = %lld, %lld transport blocks of C = %d frames of K = %d bits need %lld",
                         (long long)src_bytes, (long long)tbs, s->C, s->K, (long long)(z->frames * z->frow));
    if (!payload || !src) return set_error(LDPC_ERR_ARG, "%s/%s is NULL", in, out);
    if (ranges_overlap(payload, tbs * z->prow, src, z->frames * z->frow)) return set_error(LDPC_ERR_ARG, "%s and %s overlap", in, out);
    return LDPC_OK;
}

int check_check(const ldpc_tb_spec *s, const void *dec, int64_t tbs, const void *payload, const void *cb_ok, const void *tb_ok,
                const char *suffix, ldpc::TbLayout *lay, Sizes *z)
{
    if (int rc = check_spec(s, lay)) return rc;
    if (int rc = check_tbs(s, tbs, z)) return rc;
    if (!dec) return set_error(LDPC_ERR_ARG, "dec_%s is NULL", suffix);
    if (!payload && !cb_ok && !tb_ok) return set_error(LDPC_ERR_ARG, "payload_%s, cb_ok_%s and tb_ok_%s are all NULL", suffix, suffix, suffix);
    const void *outs[3] = {payload, cb_ok, tb_ok};
    const int64_t bytes[3] = {tbs * z->prow, z->frames, tbs};
    const char *names[3] = {"payload", "cb_ok", "tb_ok"};
    for (int i = 0; i < 3; ++i) {
        if (!outs[i]) continue;
        if (ranges_overlap(dec, z->frames * z->frow, outs[i], bytes[i]))
            return set_error(LDPC_ERR_ARG, "dec_%s and %s_%s overlap", suffix, names[i], suffix);
        for (int k = i + 1; k < 3; ++k)
            if (outs[k] && ranges_overlap(outs[i], bytes[i], outs[k], bytes[k]))
                return set_error(LDPC_ERR_ARG, "%s_%s and %s_%s overlap", names[i], suffix, names[k], suffix);
    }
    return LDPC_OK;
}

int launch_attach(const ldpc::TbPlan &p, const uint8_t *payload, int64_t tbs, uint8_t *src, hipStream_t s)
{
    const dim3 grid(1, frame_grid(tbs, 1));
    ldpc::tb_attach_kernel<<<grid, 64 * p.W, 0, s>>>(p, payload, tbs, src);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int launch_check(const ldpc::TbPlan &p, const uint8_t *dec, int64_t tbs, uint8_t *payload, uint8_t *cb_ok, uint8_t *tb_ok, hipStream_t s)
{
    const dim3 grid(1, frame_grid(tbs, 1));
    ldpc::tb_check_kernel<<<grid, 64 * p.W, 0, s>>>(p, dec, tbs, payload, cb_ok, tb_ok);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

}  // namespace

extern "C" {

void ldpc_tb_spec_init(ldpc_tb_spec *spec, int32_t A, int32_t K)
{
    if (spec) ldpc::tb_spec_init(spec, A, K);
}

int ldpc_tb_layout(const ldpc_tb_spec *spec, int32_t out[6])
{
    ldpc::TbLayout lay;
    if (int rc = check_spec(spec, &lay)) return rc;
    if (!out) return set_error(LDPC_ERR_ARG, "out is NULL");
    out[0] = lay.B; out[1] = lay.S; out[2] = lay.Kp; out[3] = lay.Kp; out[4] = spec->K; out[5] = spec->C;
    return LDPC_OK;
}

int ldpc_crc_bits(int32_t kind, const uint8_t *bytes, int64_t nbits, uint32_t *crc)
{
    uint32_t g;
    int L;
    if (!ldpc::tb_crc_poly(kind, &g, &L)) return set_error(LDPC_ERR_ARG, "kind = %d is none of 16, 24 (CRC24A), 25 (CRC24B)", kind);
    if (nbits < 0) return set_error(LDPC_ERR_ARG, "nbits = %lld is negative", (long long)nbits);
    if (!crc || (!bytes && nbits > 0)) return set_error(LDPC_ERR_ARG, "bytes/crc is NULL");
    *crc = ldpc::tb_crc_bits(g, L, bytes, nbits);
    return LDPC_OK;
}

int ldpc_crc_weights(int32_t kind, int32_t nbits, uint32_t *w)
{
    uint32_t g;
    int L;
    if (!ldpc::tb_crc_poly(kind, &g, &L)) return set_error(LDPC_ERR_ARG, "kind = %d is none of 16, 24 (CRC24A), 25 (CRC24B)", kind);
    if (nbits < 0) return set_error(LDPC_ERR_ARG, "nbits = %d is negative", nbits);
    if (!w && nbits > 0) return set_error(LDPC_ERR_ARG, "w is NULL");
    ldpc::crc_term_weights(kind, nbits, w);
    return LDPC_OK;
}

int ldpc_tb_frame_crc(const ldpc_tb_spec *spec, int32_t *kind, int32_t *bits)
{
    char msg[200];
    if (ldpc::tb_frame_crc(spec, kind, bits, msg, sizeof msg)) return set_error(LDPC_ERR_ARG, "%s", msg);
    return LDPC_OK;
}

int ldpc_tb_attach_device(const ldpc_tb_spec *spec, const uint8_t *payload_dev, int64_t tbs, uint8_t *src_dev, int64_t src_bytes,
                          int32_t device, void *stream)
{
    ldpc::TbLayout lay;
    Sizes z;
    if (int rc = check_attach(spec, payload_dev, tbs, src_dev, src_bytes, "payload_dev", "src_dev", &lay, &z)) return rc;
    if (tbs == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(device));
    ldpc::TbPlan p;
    ldpc::tb_make_plan(spec, lay, false, &p);
    return launch_attach(p, payload_dev, tbs, src_dev, (hipStream_t)stream);
}

int ldpc_tb_check_device(const ldpc_tb_spec *spec, const uint8_t *dec_dev, int64_t tbs, uint8_t *payload_dev, uint8_t *cb_ok_dev,
                         uint8_t *tb_ok_dev, int32_t device, void *stream)
{
    ldpc::TbLayout lay;
    Sizes z;
    if (int rc = check_check(spec, dec_dev, tbs, payload_dev, cb_ok_dev, tb_ok_dev, "dev", &lay, &z)) return rc;
    if (tbs == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(device));
    ldpc::TbPlan p;
    ldpc::tb_make_plan(spec, lay, true, &p);
    return launch_check(p, dec_dev, tbs, payload_dev, cb_ok_dev, tb_ok_dev, (hipStream_t)stream);
}

int ldpc_tb_tally_device(const uint8_t *tb_ok_dev, const uint8_t *payload_dev, const uint8_t *ref_dev, int64_t tbs,
                         int64_t bytes_per_tb, int64_t counts[4], int32_t device, void *stream)
{
    if (!tb_ok_dev || !payload_dev || !counts) return set_error(LDPC_ERR_ARG, "tb_ok_dev/payload_dev/counts is NULL");
    if (tbs < 0) return set_error(LDPC_ERR_ARG, "tbs = %lld is negative", (long long)tbs);
    if (bytes_per_tb <= 0) return set_error(LDPC_ERR_ARG, "bytes_per_tb = %lld must be positive", (long long)bytes_per_tb);
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (tbs == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    ldpc::DevBuf<unsigned long long> totals;
    LDPC_HIP_TRY(totals.alloc(4));
    hipError_t e = hipMemsetAsync(totals.p, 0, 4 * sizeof(unsigned long long), s);
    if (e == hipSuccess) {
        ldpc::tb_tally_kernel<<<(unsigned)std::min<int64_t>(tbs, ldpc::kFrameTargetBlocks), 256, 0, s>>>(tb_ok_dev, payload_dev, ref_dev, tbs,
                                                                                                     bytes_per_tb, totals.p);
        e = hipGetLastError();
    }
    unsigned long long h[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(h, totals.p, sizeof h, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return set_error(LDPC_ERR_HIP, "tb_tally: %s", hipGetErrorString(e));
    for (int i = 0; i < 4; ++i) counts[i] = (int64_t)h[i];
    return LDPC_OK;
}

int ldpc_tb_attach(const ldpc_tb_spec *spec, const uint8_t *payload_host, int64_t tbs, uint8_t *src_host, int64_t src_bytes,
                   int32_t device)
{
    ldpc::TbLayout lay;
    Sizes z;
    if (int rc = check_attach(spec, payload_host, tbs, src_host, src_bytes, "payload_host", "src_host", &lay, &z)) return rc;
    if (tbs == 0) return LDPC_OK;
    if (int rc = ldpc::use_device(device, "the transport-block stage")) return rc;
    ldpc::TbPlan p;
    ldpc::tb_make_plan(spec, lay, false, &p);
    return ldpc::host_chunks(tbs, {{(void *)payload_host, z.prow, true, false}, {src_host, z.frow * spec->C, false, true}},
                             [&](int64_t n, int64_t, void *const *dev) {
                                 return launch_attach(p, (const uint8_t *)dev[0], n, (uint8_t *)dev[1], nullptr);
                             });
}

int ldpc_tb_check(const ldpc_tb_spec *spec, const uint8_t *dec_host, int64_t tbs, uint8_t *payload_host, uint8_t *cb_ok_host,
                  uint8_t *tb_ok_host, int32_t device)
{
    ldpc::TbLayout lay;
    Sizes z;
    if (int rc = check_check(spec, dec_host, tbs, payload_host, cb_ok_host, tb_ok_host, "host", &lay, &z)) return rc;
    if (tbs == 0) return LDPC_OK;
    if (int rc = ldpc::use_device(device, "the transport-block stage")) return rc;
    ldpc::TbPlan p;
    ldpc::tb_make_plan(spec, lay, true, &p);
    return ldpc::host_chunks(tbs,
                             {{(void *)dec_host, z.frow * spec->C, true, false}, {payload_host, z.prow, false, true},
                              {cb_ok_host, (int64_t)spec->C, false, true}, {tb_ok_host, 1, false, true}},
                             [&](int64_t n, int64_t, void *const *dev) {
                                 return launch_check(p, (const uint8_t *)dev[0], n, (uint8_t *)dev[1], (uint8_t *)dev[2], (uint8_t *)dev[3],
                                                     nullptr);
                             });
}

}  // extern "C"
