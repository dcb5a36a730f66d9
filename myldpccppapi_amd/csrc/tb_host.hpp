/*
 * tb_host.hpp -- the arithmetic of the "transport block" section of the C ABI (include/ldpc_hip.h) that needs no
 * device: the checks and derived quantities of an ldpc_tb_spec, the bitwise reference CRC, GF(2) polynomial arithmetic
 * modulo a CRC generator, and the plan (lane weights and segment weights) the kernels of tb_kernels.hpp run from.
 * No HIP in here: tests/cpp/tb_host_test.cpp includes this file alone.  The functions marked TB_HD are also compiled
 * for the device when a .hip unit includes the file.
 *
 * Polynomials over GF(2) are integers, bit k = coefficient of x^k ("normal form").  A generator g has degree L and is
 * given with its top bit (g24A = 0x1864CFB); remainders are below 2^L.  CRC of bits a_0 .. a_(n-1) (TS 38.212 section
 * 5.1, register zero, no reflection, no final XOR):
 *     crc(a) = (a_0 x^(n-1) + ... + a_(n-1)) x^L  mod g,       parity bit p_0 = its top bit.
 * Cut the bits into chunks c_0 .. c_(m-1), chunk i followed by b_i bits.  By linearity
 *     crc(a) = sum_i crc(c_i) * x^(b_i)  mod g                                        (the combine identity)
 * which is what lets a wave walk 64 runs of a block at once: lane partial times x^(bits behind the run), XOR-reduced.
 * x is invertible modulo g (g has constant term 1: x * (g >> 1) = g + 1), so zero padding behind the data is undone by
 * multiplying with a power of x^-1 = g >> 1.
 */
#pragma once

#include <stdint.h>
#include <stdio.h>

#include "../../include/ldpc_hip.h"

#if defined(__HIPCC__)
#define TB_HD __host__ __device__
#else
#define TB_HD
#endif

namespace ldpc {

constexpr uint32_t kG24A = 0x1864CFBu, kG24B = 0x1800063u, kG16 = 0x11021u;

/* generator and degree of a CRC kind (16, 24 = 24A, 25 = 24B); false for anything else */
inline bool tb_crc_poly(int kind, uint32_t *g, int *L)
{
    switch (kind) {
    case LDPC_CRC16: *g = kG16; *L = 16; return true;
    case LDPC_CRC24A: *g = kG24A; *L = 24; return true;
    case LDPC_CRC24B: *g = kG24B; *L = 24; return true;
    default: return false;
    }
}

/* a * b mod g; a, b < 2^L */
TB_HD inline uint32_t gf2_mulmod(uint32_t a, uint32_t b, uint32_t g, int L)
{
    const uint32_t top = 1u << (L - 1), low = g ^ (1u << L);
    uint32_t r = 0;
    for (int i = L - 1; i >= 0; --i) {
        r = (r & top) ? ((r ^ top) << 1) ^ low : r << 1;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

/* base^n mod g by square-and-multiply */
inline uint32_t gf2_powmod(uint32_t base, uint64_t n, uint32_t g, int L)
{
    uint32_t r = 1, s = base;
    for (; n; n >>= 1) {
        if (n & 1) r = gf2_mulmod(r, s, g, L);
        s = gf2_mulmod(s, s, g, L);
    }
    return r;
}

/* x^n mod g for any integer n: negative exponents are powers of x^-1 = g >> 1 */
inline uint32_t gf2_xpow(int64_t n, uint32_t g, int L)
{
    return n >= 0 ? gf2_powmod(2u, (uint64_t)n, g, L) : gf2_powmod(g >> 1, (uint64_t)(-n), g, L);
}

/* the L low bits of v in reverse order: normal form <-> the register whose bit 0 is p_0 (the project's bit order) */
TB_HD inline uint32_t tb_reflect(uint32_t v, int L)
{
    uint32_t r = 0;
    for (int i = 0; i < L; ++i) r |= ((v >> i) & 1u) << (L - 1 - i);
    return r;
}

/* one data bit into a normal-form register */
TB_HD inline uint32_t tb_crc_step(uint32_t r, uint32_t bit, uint32_t g, int L)
{
    const uint32_t top = (r >> (L - 1)) & 1u;
    r = (r << 1) & ((1u << L) - 1u);
    return (top ^ (bit & 1u)) ? r ^ (g ^ (1u << L)) : r;
}

/* entry b of the byte table of the reflected register: the eight steps of a byte whose bit 0 comes first */
TB_HD inline uint32_t tb_table_entry(uint32_t b, uint32_t g, int L)
{
    const uint32_t poly = tb_reflect(g ^ (1u << L), L);
    uint32_t r = b;
    for (int i = 0; i < 8; ++i) r = (r & 1u) ? (r >> 1) ^ poly : r >> 1;
    return r;
}

/* the reference: long division, one bit at a time, bit i = bit i % 8 of byte i / 8 */
inline uint32_t tb_crc_bits(uint32_t g, int L, const uint8_t *bytes, int64_t nbits)
{
    uint32_t r = 0;
    for (int64_t i = 0; i < nbits; ++i) r = tb_crc_step(r, (uint32_t)(bytes[i >> 3] >> (i & 7)), g, L);
    return r;
}

/* B, S, Kp of a spec that tb_check_spec accepted */
struct TbLayout {
    int32_t B, S, Kp;
};

/* 0, or 1 with a message that names the field */
inline int tb_check_spec(const ldpc_tb_spec *s, TbLayout *lay, char *msg, size_t cap)
{
    if (!s) return snprintf(msg, cap, "spec is NULL"), 1;
    if (s->struct_size != sizeof(ldpc_tb_spec))
        return snprintf(msg, cap, "spec.struct_size = %u, this library's ldpc_tb_spec has %u bytes", s->struct_size,
                        (unsigned)sizeof(ldpc_tb_spec)), 1;
    if (s->A < 8 || s->A % 8) return snprintf(msg, cap, "spec.A = %d must be a positive multiple of 8", s->A), 1;
    if (s->tb_crc != 0 && s->tb_crc != 16 && s->tb_crc != 24)
        return snprintf(msg, cap, "spec.tb_crc = %d is none of 0, 16, 24", s->tb_crc), 1;
    if (s->C < 1) return snprintf(msg, cap, "spec.C = %d must be at least 1", s->C), 1;
    if (s->cb_crc != 0 && s->cb_crc != 24) return snprintf(msg, cap, "spec.cb_crc = %d must be 0 or 24", s->cb_crc), 1;
    if (s->K < 8 || s->K % 8) return snprintf(msg, cap, "spec.K = %d must be a positive multiple of 8", s->K), 1;
    if (s->A > 0x7fffffff - 24) return snprintf(msg, cap, "spec.A = %d is too large", s->A), 1;
    const int32_t B = s->A + s->tb_crc;
    if (B % s->C) return snprintf(msg, cap, "B %% C != 0: B = A + tb_crc = %d bits do not cut into C = %d code blocks", B, s->C), 1;
    const int32_t S = B / s->C, Kp = S + s->cb_crc;
    if (Kp > s->K) return snprintf(msg, cap, "Kp = B / C + cb_crc = %d exceeds spec.K = %d", Kp, s->K), 1;
    if (lay) { lay->B = B; lay->S = S; lay->Kp = Kp; }
    return 0;
}

/* the rule of TS 38.212 section 5.2.2 with the code's K in place of Kcb */
inline void tb_spec_init(ldpc_tb_spec *s, int32_t A, int32_t K)
{
    s->struct_size = (uint32_t)sizeof(ldpc_tb_spec);
    s->A = A;
    s->K = K;
    s->tb_crc = A > 3824 ? 24 : 16;
    const int64_t B = (int64_t)A + s->tb_crc;
    if (B <= K) {
        s->C = 1;
        s->cb_crc = 0;
    } else {
        s->cb_crc = 24;
        s->C = K > 24 ? (int32_t)((B + (K - 24) - 1) / (K - 24)) : 0;
    }
}

/* What a kernel launch runs from, by value.  A wave walks `nb` bytes of a code block, lane l the run
 * [l R, (l + 1) R) of them; the lane's partial remainder is multiplied by w[l].
 *   attach: nb = ceil(S / 8); the last byte is padded with 8 nb - S zero bits, which the weights undo:
 *           wB[l] = x^(behind(l) - pad),  wA[l] = x^(behind(l) - pad - LA): the reduced values are the code block's
 *           CRC24B of its S bits and seg(x) mod gA, the segment itself without the factor x^LA.
 *   check:  nb = ceil(Kp / 8); both remainders are only tested for zero, so w[l] = x^behind(l) for both.
 * behind(l) = 8 max(0, nb - (l + 1) R) bits.  The transport block's remainder is sum_c segA_c x^((C - 1 - c) S): wave w
 * of W folds its code blocks c = w, w + W, ... with acc = acc * stepA + segA_c, stepA = x^(W S), and the W sums meet
 * as sum_w acc_w * finA[C - 1 - last_c(w)], finA[j] = x^(j S). */
constexpr int kTbMaxWaves = 4;
struct TbPlan {
    int32_t A, tb_crc, C, cb_crc, K;
    int32_t B, S, Kp;
    int32_t nb, R, W;
    int32_t cA;               /* first code block that holds transport-block parity bits (C: none) */
    uint32_t gA;              /* generator of the transport block's CRC (0: none) */
    int32_t LA;
    uint32_t stepA, finA[kTbMaxWaves];
    uint32_t wA[64], wB[64];
};

inline void tb_make_plan(const ldpc_tb_spec *s, const TbLayout &lay, bool check, TbPlan *p)
{
    p->A = s->A; p->tb_crc = s->tb_crc; p->C = s->C; p->cb_crc = s->cb_crc; p->K = s->K;
    p->B = lay.B; p->S = lay.S; p->Kp = lay.Kp;
    p->nb = ((check ? lay.Kp : lay.S) + 7) / 8;
    p->R = (p->nb + 63) / 64;
    p->W = s->C < kTbMaxWaves ? s->C : kTbMaxWaves;
    p->cA = s->tb_crc ? s->A / lay.S : s->C;
    p->gA = s->tb_crc == 24 ? kG24A : s->tb_crc == 16 ? kG16 : 0;
    p->LA = s->tb_crc;
    const int64_t pad = check ? 0 : 8 * (int64_t)p->nb - lay.S;
    for (int l = 0; l < 64; ++l) {
        const int64_t end = ((int64_t)l + 1) * p->R;
        const int64_t behind = end < p->nb ? 8 * (p->nb - end) : 0;
        p->wB[l] = gf2_xpow(behind - pad, kG24B, 24);
        p->wA[l] = p->gA ? gf2_xpow(behind - pad - (check ? 0 : p->LA), p->gA, p->LA) : 0;
    }
    p->stepA = p->gA ? gf2_xpow((int64_t)p->W * lay.S, p->gA, p->LA) : 0;
    for (int j = 0; j < kTbMaxWaves; ++j) p->finA[j] = p->gA ? gf2_xpow((int64_t)j * lay.S, p->gA, p->LA) : 0;
}

}  // namespace ldpc
