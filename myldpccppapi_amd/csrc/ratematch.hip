/*
 * ratematch.hip -- the "rate matching" section of the C ABI (include/ldpc_hip.h): the circular-buffer index
 * arithmetic on the host, argument checks, and the launches of ratematch_kernels.hpp.  No handle and no device
 * state: the map is closed-form and travels to the kernels by value.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/ldpc_hip.h"
#include "hip_host.hpp"
#include "ratematch_kernels.hpp"

using ldpc::set_error;
using ldpc::frame_grid;

namespace {

/* the spec alone: fills the fields of the map that do not depend on the transmission */
int check_spec(const ldpc_rate_spec *s, ldpc::RateMap *m)
{
    if (!s) return set_error(LDPC_ERR_ARG, "spec is NULL");
    if (s->struct_size != sizeof(ldpc_rate_spec))
        return set_error(LDPC_ERR_ARG, "spec.struct_size = %u, this library's ldpc_rate_spec has %u bytes", s->struct_size,
                         (unsigned)sizeof(ldpc_rate_spec));
    if (s->N < 1) return set_error(LDPC_ERR_ARG, "spec.N = %d must be positive", s->N);
    if (s->punctured < 0 || s->punctured > s->N) return set_error(LDPC_ERR_ARG, "spec.punctured = %d outside [0, N = %d]", s->punctured, s->N);
    int32_t lo = s->filler_lo, hi = s->filler_hi;
    if (lo == hi) lo = hi = s->punctured;       /* no fillers: where the empty range lies does not matter */
    if (lo < s->punctured) return set_error(LDPC_ERR_ARG, "spec.filler_lo = %d lies in the punctured prefix [0, %d)", lo, s->punctured);
    if (hi < lo) return set_error(LDPC_ERR_ARG, "spec.filler_hi = %d is below filler_lo = %d", hi, lo);
    if (hi > s->N) return set_error(LDPC_ERR_ARG, "spec.filler_hi = %d exceeds N = %d", hi, s->N);
    const int32_t L = s->N - s->punctured - (hi - lo);
    if (L < 1) return set_error(LDPC_ERR_ARG, "spec: punctured = %d and fillers [%d, %d) leave L = %d transmittable bits of N = %d", s->punctured, lo, hi, L, s->N);
    if (!std::isfinite(s->fill_llr)) return set_error(LDPC_ERR_ARG, "spec.fill_llr must be finite");
    if (!(s->erasure_llr >= 0.0f) || !std::isfinite(s->erasure_llr))
        return set_error(LDPC_ERR_ARG, "spec.erasure_llr must be 0 or a positive finite value");
    if (s->erasure_llr > 0.0f && s->N > (1 << 22))
        return set_error(LDPC_ERR_ARG, "spec.erasure_llr > 0 needs N <= 2^22 (N = %d): the erasure values would not be pairwise distinct", s->N);
    m->N = s->N; m->P = s->punctured; m->lo = lo; m->hi = hi; m->L = L; m->E = 0; m->r0 = 0;
    m->fill_llr = s->fill_llr; m->erasure_llr = s->erasure_llr;
    return LDPC_OK;
}

/* spec + one transmission (k0, E) */
int make_map(const ldpc_rate_spec *s, int32_t k0, int32_t E, ldpc::RateMap *m)
{
    if (int rc = check_spec(s, m)) return rc;
    const int32_t Ncb = m->N - m->P;
    if (k0 < 0 || k0 >= Ncb) return set_error(LDPC_ERR_ARG, "k0 = %d outside the circular buffer [0, Ncb = %d)", k0, Ncb);
    if (E < 1) return set_error(LDPC_ERR_ARG, "E = %d must be at least 1", E);
    const int32_t before = std::min(std::max(k0 - (m->lo - m->P), 0), m->hi - m->lo);   /* fillers in front of k0 */
    m->r0 = (uint32_t)((k0 - before) % m->L);
    m->E = E;
    return LDPC_OK;
}

inline int32_t host_index(const ldpc::RateMap &m, int64_t e)
{
    const int64_t rank = ((int64_t)m.r0 + e) % m.L;
    return (int32_t)(m.P + rank + (rank >= m.lo - m.P ? m.hi - m.lo : 0));
}

int check_match(const ldpc::RateMap &m, int32_t code_format, int32_t tx_format)
{
    if (int rc = ldpc::known_code_format(code_format, "code_format")) return rc;
    if (int rc = ldpc::known_code_format(tx_format, "tx_format")) return rc;
    if (code_format == LDPC_CODE_PACKED && m.N % 8) return set_error(LDPC_ERR_ARG, "code_format LDPC_CODE_PACKED needs N %% 8 == 0 (N = %d)", m.N);
    if (tx_format == LDPC_CODE_PACKED && m.E % 8) return set_error(LDPC_ERR_ARG, "tx_format LDPC_CODE_PACKED needs E %% 8 == 0 (E = %d)", m.E);
    return LDPC_OK;
}

int launch_match(const ldpc::RateMap &m, const uint8_t *code, int32_t code_format, int64_t frames, uint8_t *tx, int32_t tx_format,
                 hipStream_t s)
{
    using namespace ldpc;
    const int64_t out_row = tx_format == LDPC_CODE_PACKED ? m.E / 8 : m.E;
    const int64_t code_bytes = frames * (int64_t)(code_format == LDPC_CODE_PACKED ? m.N / 8 : m.N);
    const unsigned gx = (unsigned)(((out_row + 6) / 4 + kRateBlock - 1) / kRateBlock);
    const dim3 grid(gx, frame_grid(frames, gx));
    if (code_format == LDPC_CODE_PACKED) {
        if (tx_format == LDPC_CODE_PACKED) rate_match_kernel<1, 1><<<grid, kRateBlock, 0, s>>>(m, code, code_bytes, frames, tx);
        else rate_match_kernel<1, 0><<<grid, kRateBlock, 0, s>>>(m, code, code_bytes, frames, tx);
    } else {
        if (tx_format == LDPC_CODE_PACKED) rate_match_kernel<0, 1><<<grid, kRateBlock, 0, s>>>(m, code, code_bytes, frames, tx);
        else rate_match_kernel<0, 0><<<grid, kRateBlock, 0, s>>>(m, code, code_bytes, frames, tx);
    }
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int launch_recover(const ldpc::RateMap &m, const float *rx, int64_t frames, float *soft, int32_t accumulate, float *y, hipStream_t s)
{
    using namespace ldpc;
    const int per = kRateBlock * kRateUnroll;
    const unsigned gx = (unsigned)((m.N + per - 1) / per);
    const dim3 grid(gx, frame_grid(frames, gx));
    rate_recover_kernel<<<grid, kRateBlock, 0, s>>>(m, rx, frames, soft, accumulate, y);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int check_recover_flags(bool have_soft, bool have_y, int32_t accumulate)
{
    if (!have_soft && !have_y) return set_error(LDPC_ERR_ARG, "soft and y are both NULL: nothing to write");
    if (accumulate && !have_soft) return set_error(LDPC_ERR_ARG, "accumulate needs a soft buffer");
    return LDPC_OK;
}

/* soft and y of a recover call must not alias (the same address counts even when no frame is written) */
bool soft_y_alias(const ldpc::RateMap &m, int64_t frames, const float *soft, const float *y)
{
    const int64_t span = frames * (int64_t)m.N * (int64_t)sizeof(float);
    return soft && y && (soft == y || ldpc::ranges_overlap(soft, span, y, span));
}

}  // namespace

extern "C" {

void ldpc_rate_spec_init(ldpc_rate_spec *spec, int32_t N)
{
    if (!spec) return;
    spec->struct_size = (uint32_t)sizeof(ldpc_rate_spec);
    spec->N = N;
    spec->punctured = 0;
    spec->filler_lo = spec->filler_hi = 0;
    spec->fill_llr = 10.0f;
    spec->erasure_llr = 0.0f;
}

int ldpc_rate_lengths(const ldpc_rate_spec *spec, int32_t *Ncb, int32_t *L)
{
    ldpc::RateMap m;
    if (int rc = check_spec(spec, &m)) return rc;
    if (Ncb) *Ncb = m.N - m.P;
    if (L) *L = m.L;
    return LDPC_OK;
}

int ldpc_rate_index(const ldpc_rate_spec *spec, int32_t k0, int32_t E, int32_t *index_out)
{
    ldpc::RateMap m;
    if (int rc = make_map(spec, k0, E, &m)) return rc;
    if (!index_out) return set_error(LDPC_ERR_ARG, "index_out is NULL");
    for (int64_t e = 0; e < E; ++e) index_out[e] = host_index(m, e);
    return LDPC_OK;
}

int ldpc_rate_match_device(const ldpc_rate_spec *spec, const uint8_t *code_dev, int32_t code_format, int64_t frames, int32_t k0,
                           int32_t E, uint8_t *tx_dev, int64_t tx_bytes, int32_t tx_format, int32_t device, void *stream)
{
    ldpc::RateMap m;
    if (int rc = make_map(spec, k0, E, &m)) return rc;
    if (int rc = check_match(m, code_format, tx_format)) return rc;
    if (!code_dev || !tx_dev) return set_error(LDPC_ERR_ARG, "code_dev/tx_dev is NULL");
    if (frames < 0) return set_error(LDPC_ERR_ARG, "frames = %lld is negative", (long long)frames);
    if (tx_bytes < ldpc_code_bytes(E, frames, tx_format))
        return set_error(LDPC_ERR_ARG, "tx_bytes = %lld, %lld frames of E = %d need %lld", (long long)tx_bytes, (long long)frames, E,
                         (long long)ldpc_code_bytes(E, frames, tx_format));
    if (frames == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(device));
    return launch_match(m, code_dev, code_format, frames, tx_dev, tx_format, (hipStream_t)stream);
}

int ldpc_rate_recover_device(const ldpc_rate_spec *spec, const float *rx_dev, int64_t frames, int32_t k0, int32_t E, float *soft_dev,
                             int32_t accumulate, float *y_dev, int32_t device, void *stream)
{
    ldpc::RateMap m;
    if (int rc = make_map(spec, k0, E, &m)) return rc;
    if (int rc = check_recover_flags(soft_dev != nullptr, y_dev != nullptr, accumulate)) return rc;
    if (!rx_dev) return set_error(LDPC_ERR_ARG, "rx_dev is NULL");
    if (frames < 0) return set_error(LDPC_ERR_ARG, "frames = %lld is negative", (long long)frames);
    if (soft_y_alias(m, frames, soft_dev, y_dev)) return set_error(LDPC_ERR_ARG, "soft_dev and y_dev overlap: they must not alias");
    if (frames == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(device));
    return launch_recover(m, rx_dev, frames, soft_dev, accumulate, y_dev, (hipStream_t)stream);
}

int ldpc_rate_match(const ldpc_rate_spec *spec, const uint8_t *code_host, int32_t code_format, int64_t frames, int32_t k0, int32_t E,
                    uint8_t *tx_host, int64_t tx_bytes, int32_t tx_format, int32_t device)
{
    ldpc::RateMap m;
    if (int rc = make_map(spec, k0, E, &m)) return rc;
    if (int rc = check_match(m, code_format, tx_format)) return rc;
    if (!code_host || !tx_host) return set_error(LDPC_ERR_ARG, "code_host/tx_host is NULL");
    if (frames < 0) return set_error(LDPC_ERR_ARG, "frames = %lld is negative", (long long)frames);
    if (tx_bytes < ldpc_code_bytes(E, frames, tx_format))
        return set_error(LDPC_ERR_ARG, "tx_bytes = %lld, %lld frames of E = %d need %lld", (long long)tx_bytes, (long long)frames, E,
                         (long long)ldpc_code_bytes(E, frames, tx_format));
    if (frames == 0) return LDPC_OK;
    if (int rc = ldpc::use_device(device, "rate matching")) return rc;
    const int64_t in_row = code_format == LDPC_CODE_PACKED ? m.N / 8 : m.N;
    const int64_t out_row = tx_format == LDPC_CODE_PACKED ? E / 8 : E;
    return ldpc::host_chunks(frames, {{(void *)code_host, in_row, true, false}, {tx_host, out_row, false, true}},
                             [&](int64_t n, int64_t, void *const *dev) {
                                 return launch_match(m, (const uint8_t *)dev[0], code_format, n, (uint8_t *)dev[1], tx_format, nullptr);
                             });
}

int ldpc_rate_recover(const ldpc_rate_spec *spec, const float *rx_host, int64_t frames, int32_t k0, int32_t E, float *soft_host,
                      int32_t accumulate, float *y_host, int32_t device)
{
    ldpc::RateMap m;
    if (int rc = make_map(spec, k0, E, &m)) return rc;
    if (int rc = check_recover_flags(soft_host != nullptr, y_host != nullptr, accumulate)) return rc;
    if (!rx_host) return set_error(LDPC_ERR_ARG, "rx_host is NULL");
    if (frames < 0) return set_error(LDPC_ERR_ARG, "frames = %lld is negative", (long long)frames);
    if (soft_y_alias(m, frames, soft_host, y_host)) return set_error(LDPC_ERR_ARG, "soft_host and y_host overlap: they must not alias");
    if (frames == 0) return LDPC_OK;
    if (int rc = ldpc::use_device(device, "rate matching")) return rc;
    const int64_t rx_row = (int64_t)E * sizeof(float), n_row = (int64_t)m.N * sizeof(float);
    return ldpc::host_chunks(frames, {{(void *)rx_host, rx_row, true, false}, {soft_host, n_row, accumulate != 0, true}, {y_host, n_row, false, true}},
                             [&](int64_t n, int64_t, void *const *dev) {
                                 return launch_recover(m, (const float *)dev[0], n, (float *)dev[1], accumulate, (float *)dev[2], nullptr);
                             });
}

}  // extern "C"
