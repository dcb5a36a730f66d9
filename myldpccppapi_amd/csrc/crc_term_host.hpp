/*
 * crc_term_host.hpp -- the host arithmetic of CRC-aided early termination (ldpc_decoder_config::crc_kind / crc_bits,
 * include/ldpc_hip.h): the checks of the two fields, the per-column weights crc_term_kernel (crc_term_kernels.hpp)
 * XORs together, and the CRC every frame of a transport-block spec carries.  No HIP in here:
 * tests/cpp/crc_term_host_test.cpp includes this file alone.  Polynomials and conventions: tb_host.hpp.
 *
 * The CRC is linear over GF(2): the remainder of bits b_0 .. b_(n-1) (ldpc_crc_bits: b(x) x^L mod g, register zero, no
 * reflection, bit 0 first) is the XOR over the set bits k of
 *     w_k = crc(e_k) = x^(n - 1 - k) x^L  mod g,
 * the remainder of the unit vector e_k.  x is invertible modulo g, so the remainder with the factor x^L is zero exactly
 * when the one without it is.  A table of n words turns the test into n independent select-and-XOR steps per frame:
 * no shift register, no order.
 */
#pragma once

#include <stdint.h>
#include <stdio.h>

#include "tb_host.hpp"

namespace ldpc {

/* w[k] = crc(e_k) for k < nbits, e_k of length nbits; false for an unknown kind or nbits < 0 */
inline bool crc_term_weights(int kind, int64_t nbits, uint32_t *w)
{
    uint32_t g;
    int L;
    if (!tb_crc_poly(kind, &g, &L) || nbits < 0 || (nbits > 0 && !w)) return false;
    uint32_t r = g ^ (1u << L);                    /* x^L mod g: the last bit's weight */
    for (int64_t k = nbits - 1; k >= 0; --k) {
        w[k] = r;
        r <<= 1;
        if ((r >> L) & 1u) r ^= g;                 /* times x */
    }
    return true;
}

/* the two config fields against the code's K and early_term: 0, or 1 with a message that names the field */
inline int crc_term_check(int32_t kind, int32_t bits, int32_t K, int32_t early_term, char *msg, size_t cap)
{
    if (kind == 0) return 0;                       /* off: crc_bits is not read */
    uint32_t g;
    int L;
    if (!tb_crc_poly(kind, &g, &L))
        return snprintf(msg, cap, "crc_kind = %d is none of 0 (off), LDPC_CRC16, LDPC_CRC24A, LDPC_CRC24B", kind), 1;
    if (bits <= L || bits > K)
        return snprintf(msg, cap, "crc_bits = %d must lie in (%d, K = %d]: the CRC's %d parity bits behind at least one data bit, "
                        "inside the information bits", bits, L, K, L), 1;
    if (!early_term) return snprintf(msg, cap, "crc_kind = %d needs early_term = 1: the CRC is a stopping rule", kind), 1;
    return 0;
}

/* The CRC every frame of a transport-block spec carries over its first Kp bits: CRC24B with a code-block CRC, the
 * transport block's own CRC when the block is one frame; 0, or 1 with a message (the frames have no CRC of their own). */
inline int tb_frame_crc(const ldpc_tb_spec *s, int32_t *kind, int32_t *bits, char *msg, size_t cap)
{
    TbLayout lay;
    if (tb_check_spec(s, &lay, msg, cap)) return 1;
    int32_t k = 0;
    if (s->cb_crc == 24) k = LDPC_CRC24B;
    else if (s->C == 1 && s->tb_crc == 16) k = LDPC_CRC16;
    else if (s->C == 1 && s->tb_crc == 24) k = LDPC_CRC24A;
    if (!k)
        return snprintf(msg, cap, "spec.cb_crc = 0 with spec.C = %d, spec.tb_crc = %d: the frames carry no CRC of their own", s->C,
                        s->tb_crc), 1;
    if (kind) *kind = k;
    if (bits) *bits = lay.Kp;
    return 0;
}

}  // namespace ldpc
