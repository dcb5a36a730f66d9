/*
 * modem.hip -- the "modem" section of the C ABI (include/ldpc_hip.h): bit interleaver, Gray mapper and constellation
 * points on the host, argument checks, and the launches of modem_kernels.hpp.  No handle and no device state: the map is
 * closed-form and travels to the kernels by value.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/ldpc_hip.h"
#include "hip_host.hpp"
#include "modem_kernels.hpp"

using ldpc::set_error;
using ldpc::frame_grid;
using ldpc::ranges_overlap;

namespace {

int norm_of(int32_t Qm) { return Qm == 2 ? 2 : Qm == 4 ? 10 : Qm == 6 ? 42 : Qm == 8 ? 170 : 1; }

float scale_of(int32_t Qm) { return Qm == 1 ? 1.0f : (float)(1.0 / std::sqrt((double)norm_of(Qm))); }

int check_qm(int32_t Qm)
{
    if (Qm != 1 && Qm != 2 && Qm != 4 && Qm != 6 && Qm != 8)
        return set_error(LDPC_ERR_ARG, "Qm = %d is none of 1, 2, 4, 6, 8", Qm);
    return LDPC_OK;
}

int check_spec(const ldpc_modem_spec *s)
{
    if (!s) return set_error(LDPC_ERR_ARG, "spec is NULL");
    if (s->struct_size != sizeof(ldpc_modem_spec))
        return set_error(LDPC_ERR_ARG, "spec.struct_size = %u, this library's ldpc_modem_spec has %u bytes", s->struct_size,
                         (unsigned)sizeof(ldpc_modem_spec));
    if (int rc = check_qm(s->Qm)) return rc;
    if (s->interleave != 0 && s->interleave != 1) return set_error(LDPC_ERR_ARG, "spec.interleave = %d must be 0 or 1", s->interleave);
    return LDPC_OK;
}

/* spec + the bits of one frame */
int make_map(const ldpc_modem_spec *s, int32_t E, ldpc::ModemMap *m)
{
    if (int rc = check_spec(s)) return rc;
    if (E < 1) return set_error(LDPC_ERR_ARG, "E = %d must be at least 1", E);
    if (E % s->Qm) return set_error(LDPC_ERR_ARG, "E %% Qm != 0: E = %d bits do not fill symbols of Qm = %d", E, s->Qm);
    m->Qm = s->Qm; m->E = E; m->S = E / s->Qm;
    m->interleave = s->interleave && s->Qm > 1;
    m->row = s->Qm == 1 ? E : 2 * m->S;
    m->A = scale_of(s->Qm);
    return LDPC_OK;
}

inline int32_t host_position(const ldpc::ModemMap &m, int32_t i, int32_t j) { return m.interleave ? i * m.S + j : j * m.Qm + i; }

int check_transmit(const ldpc::ModemMap &m, int32_t tx_format, int64_t frames, float sd, int64_t first_frame, int64_t sym_floats)
{
    if (int rc = ldpc::known_code_format(tx_format, "tx_format")) return rc;
    if (tx_format == LDPC_CODE_PACKED && m.E % 8) return set_error(LDPC_ERR_ARG, "tx_format LDPC_CODE_PACKED needs E %% 8 == 0 (E = %d)", m.E);
    if (frames < 0) return set_error(LDPC_ERR_ARG, "frames = %lld is negative", (long long)frames);
    if (first_frame < 0) return set_error(LDPC_ERR_ARG, "first_frame = %lld is negative", (long long)first_frame);
    if (!(sd >= 0.0f) || !std::isfinite(sd)) return set_error(LDPC_ERR_ARG, "sd must be 0 or a positive finite value");
    if (sym_floats < frames * (int64_t)m.row)
        return set_error(LDPC_ERR_ARG, "sym_floats = %lld, %lld frames of E = %d at Qm = %d need %lld", (long long)sym_floats,
                         (long long)frames, m.E, m.Qm, (long long)(frames * (int64_t)m.row));
    return LDPC_OK;
}

int launch_transmit(const ldpc::ModemMap &m, const uint8_t *tx, int32_t tx_format, int64_t frames, float sd, uint64_t seed,
                    int64_t first_frame, float *sym, hipStream_t s)
{
    using namespace ldpc;
    const int64_t groups = ((int64_t)m.row + 3) / 4;
    const unsigned gx = (unsigned)((groups + kModemBlock - 1) / kModemBlock);
    const dim3 grid(gx, frame_grid(frames, gx));
    if (tx_format == LDPC_CODE_PACKED) modem_tx_kernel<1><<<grid, kModemBlock, 0, s>>>(m, tx, frames, sd, seed, first_frame, sym);
    else modem_tx_kernel<0><<<grid, kModemBlock, 0, s>>>(m, tx, frames, sd, seed, first_frame, sym);
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int launch_demap(const ldpc::ModemMap &m, const float *sym, int64_t frames, float *rx, hipStream_t s)
{
    using namespace ldpc;
    const unsigned gx = (unsigned)(((int64_t)m.S + kModemBlock - 1) / kModemBlock);
    const dim3 grid(gx, frame_grid(frames, gx));
    switch (m.Qm) {
    case 1: modem_demap_kernel<1><<<grid, kModemBlock, 0, s>>>(m, sym, frames, rx); break;
    case 2: modem_demap_kernel<2><<<grid, kModemBlock, 0, s>>>(m, sym, frames, rx); break;
    case 4: modem_demap_kernel<4><<<grid, kModemBlock, 0, s>>>(m, sym, frames, rx); break;
    case 6: modem_demap_kernel<6><<<grid, kModemBlock, 0, s>>>(m, sym, frames, rx); break;
    default: modem_demap_kernel<8><<<grid, kModemBlock, 0, s>>>(m, sym, frames, rx); break;
    }
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

}  // namespace

extern "C" {

void ldpc_modem_spec_init(ldpc_modem_spec *spec, int32_t Qm)
{
    if (!spec) return;
    spec->struct_size = (uint32_t)sizeof(ldpc_modem_spec);
    spec->Qm = Qm;
    spec->interleave = Qm >= 2;
}

int64_t ldpc_modem_symbol_floats(const ldpc_modem_spec *spec, int32_t E)
{
    ldpc::ModemMap m;
    if (make_map(spec, E, &m)) return 0;
    return m.row;
}

int ldpc_modem_index(const ldpc_modem_spec *spec, int32_t E, int32_t *index_out)
{
    ldpc::ModemMap m;
    if (int rc = make_map(spec, E, &m)) return rc;
    if (!index_out) return set_error(LDPC_ERR_ARG, "index_out is NULL");
    for (int32_t j = 0; j < m.S; ++j)
        for (int32_t i = 0; i < m.Qm; ++i) index_out[(int64_t)j * m.Qm + i] = host_position(m, i, j);
    return LDPC_OK;
}

int ldpc_modem_points(int32_t Qm, float *iq)
{
    if (int rc = check_qm(Qm)) return rc;
    if (!iq) return set_error(LDPC_ERR_ARG, "iq is NULL");
    if (Qm == 1) {
        iq[0] = 1.0f; iq[1] = 0.0f; iq[2] = -1.0f; iq[3] = 0.0f;
        return LDPC_OK;
    }
    const int half = Qm / 2;
    const float A = scale_of(Qm);
    for (uint32_t v = 0; v < (1u << Qm); ++v) {
        uint32_t axis[2] = {0, 0};                       /* axis labels, c0 as the top bit */
        for (int i = 0; i < Qm; ++i) axis[i & 1] = (axis[i & 1] << 1) | ((v >> (Qm - 1 - i)) & 1u);
        iq[2 * v] = (float)ldpc::modem_amp(half, axis[0]) * A;
        iq[2 * v + 1] = (float)ldpc::modem_amp(half, axis[1]) * A;
    }
    return LDPC_OK;
}

int ldpc_modem_transmit_device(const ldpc_modem_spec *spec, const uint8_t *tx_dev, int32_t tx_format, int64_t frames, int32_t E,
                               float sd, uint64_t seed, int64_t first_frame, float *sym_dev, int64_t sym_floats, int32_t device,
                               void *stream)
{
    ldpc::ModemMap m;
    if (int rc = make_map(spec, E, &m)) return rc;
    if (int rc = check_transmit(m, tx_format, frames, sd, first_frame, sym_floats)) return rc;
    if (!tx_dev || !sym_dev) return set_error(LDPC_ERR_ARG, "tx_dev/sym_dev is NULL");
    if (ranges_overlap(tx_dev, ldpc_code_bytes(E, frames, tx_format), sym_dev, frames * (int64_t)m.row * 4))
        return set_error(LDPC_ERR_ARG, "tx_dev and sym_dev overlap");
    if (frames == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(device));
    return launch_transmit(m, tx_dev, tx_format, frames, sd, seed, first_frame, sym_dev, (hipStream_t)stream);
}

int ldpc_modem_demap_device(const ldpc_modem_spec *spec, const float *sym_dev, int64_t frames, int32_t E, float *rx_dev,
                            int32_t device, void *stream)
{
    ldpc::ModemMap m;
    if (int rc = make_map(spec, E, &m)) return rc;
    if (frames < 0) return set_error(LDPC_ERR_ARG, "frames = %lld is negative", (long long)frames);
    if (!sym_dev || !rx_dev) return set_error(LDPC_ERR_ARG, "sym_dev/rx_dev is NULL");
    if (ranges_overlap(sym_dev, frames * (int64_t)m.row * 4, rx_dev, frames * (int64_t)E * 4))
        return set_error(LDPC_ERR_ARG, "sym_dev and rx_dev overlap");
    if (frames == 0) return LDPC_OK;
    LDPC_HIP_TRY(hipSetDevice(device));
    return launch_demap(m, sym_dev, frames, rx_dev, (hipStream_t)stream);
}

int ldpc_modem_transmit(const ldpc_modem_spec *spec, const uint8_t *tx_host, int32_t tx_format, int64_t frames, int32_t E, float sd,
                        uint64_t seed, int64_t first_frame, float *sym_host, int64_t sym_floats, int32_t device)
{
    ldpc::ModemMap m;
    if (int rc = make_map(spec, E, &m)) return rc;
    if (int rc = check_transmit(m, tx_format, frames, sd, first_frame, sym_floats)) return rc;
    if (!tx_host || !sym_host) return set_error(LDPC_ERR_ARG, "tx_host/sym_host is NULL");
    if (ranges_overlap(tx_host, ldpc_code_bytes(E, frames, tx_format), sym_host, frames * (int64_t)m.row * 4))
        return set_error(LDPC_ERR_ARG, "tx_host and sym_host overlap");
    if (frames == 0) return LDPC_OK;
    if (int rc = ldpc::use_device(device, "the modem stage")) return rc;
    const int64_t in_row = tx_format == LDPC_CODE_PACKED ? E / 8 : E, out_row = (int64_t)m.row * 4;
    return ldpc::host_chunks(frames, {{(void *)tx_host, in_row, true, false}, {sym_host, out_row, false, true}},
                             [&](int64_t n, int64_t f0, void *const *dev) {
                                 return launch_transmit(m, (const uint8_t *)dev[0], tx_format, n, sd, seed, first_frame + f0, (float *)dev[1], nullptr);
                             });
}

int ldpc_modem_demap(const ldpc_modem_spec *spec, const float *sym_host, int64_t frames, int32_t E, float *rx_host, int32_t device)
{
    ldpc::ModemMap m;
    if (int rc = make_map(spec, E, &m)) return rc;
    if (frames < 0) return set_error(LDPC_ERR_ARG, "frames = %lld is negative", (long long)frames);
    if (!sym_host || !rx_host) return set_error(LDPC_ERR_ARG, "sym_host/rx_host is NULL");
    if (ranges_overlap(sym_host, frames * (int64_t)m.row * 4, rx_host, frames * (int64_t)E * 4))
        return set_error(LDPC_ERR_ARG, "sym_host and rx_host overlap");
    if (frames == 0) return LDPC_OK;
    if (int rc = ldpc::use_device(device, "the modem stage")) return rc;
    const int64_t in_row = (int64_t)m.row * 4, out_row = (int64_t)E * 4;
    return ldpc::host_chunks(frames, {{(void *)sym_host, in_row, true, false}, {rx_host, out_row, false, true}},
                             [&](int64_t n, int64_t, void *const *dev) {
                                 return launch_demap(m, (const float *)dev[0], n, (float *)dev[1], nullptr);
                             });
}

}  // extern "C"
