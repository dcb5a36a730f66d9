/*
 * bch_host.hpp -- the arithmetic of the "outer code" section of the C ABI (include/ldpc_hip.h) that needs no device: the
 * field GF(2^m), the check that its polynomial is primitive, cyclotomic cosets, minimal polynomials, the generator, the
 * checks and derived quantities of an ldpc_bch_spec, a bitwise reference (long division, direct syndromes) and the plan the
 * kernels of bch_kernels.hpp run from.  No HIP in here: tests/cpp/bch_host_test.cpp includes this file alone.  The
 * functions marked BCH_HD are also compiled for the device when a .hip unit includes the file.
 *
 * Polynomials over GF(2) are integers, bit k = coefficient of x^k; field elements are polynomials in alpha = x below
 * degree m.  Bit i of the n code bits is the coefficient of x^(n-1-i); a byte of a row, bit 0 first, is therefore the
 * polynomial whose bits are the byte's bits in reverse order.
 *
 * The walk.  g is the product of nmin <= t distinct minimal polynomials m_i of degree d_i <= 16.  Instead of one
 * 192-bit register modulo g a lane keeps one 16-bit register per m_i, all of them modulo M_i = m_i x^(16 - d_i), which
 * has degree exactly 16: a byte B then advances every register the same way,
 *     r' = (r_lo << 8) ^ T_i[r_hi] ^ B,      T_i[h] = h(x) x^16 mod M_i,
 * and v mod M_i is as good as v mod m_i wherever it is only evaluated at a root of m_i (the syndromes) and is reduced
 * once per frame where the remainder itself is wanted (the encoder).  A wave walks a row in 64 runs; the partial
 * remainders combine as sum_l (v_l mod M_i) (x^(bits behind run l) mod M_i) mod M_i, by linearity.
 *   decode: S_j = v(alpha^j) = u_c(alpha^j) = sum_b u_c[b] alpha^(j b), c the class of j, u_c = v mod M_c.
 *   encode: u_i = x^r a(x) mod m_i for every i determines p = x^r a(x) mod g (Chinese remainder theorem):
 *           p = sum_i ((u_i c_i) mod m_i) G_i,   G_i = g / m_i,   c_i = G_i^-1 mod m_i.
 */
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/ldpc_hip.h"

#if defined(__HIPCC__)
#define BCH_HD __host__ __device__
#else
#define BCH_HD
#endif

namespace ldpc {

constexpr int kBchMaxT = 12;
constexpr int kBchWords = 4;          /* 64-bit words of a polynomial modulo g: deg g <= 192 */

/* a * b mod `mod`, a polynomial of degree `deg` given with its top bit; a < 2^deg.  With mod = prim and deg = m this is
 * the product in GF(2^m), shift and add */
BCH_HD inline uint32_t bch_mulmod(uint32_t a, uint32_t b, uint32_t mod, int deg)
{
    uint32_t r = 0;
    for (int i = deg - 1; i >= 0; --i) {
        r <<= 1;
        if ((r >> deg) & 1u) r ^= mod;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

BCH_HD inline uint32_t bch_powmod(uint32_t base, uint64_t e, uint32_t mod, int deg)
{
    uint32_t r = 1, s = base;
    for (; e; e >>= 1) {
        if (e & 1) r = bch_mulmod(r, s, mod, deg);
        s = bch_mulmod(s, s, mod, deg);
    }
    return r;
}

/* entry h of the byte table of a 16-bit register modulo M (degree 16, top bit included): h(x) x^16 mod M */
BCH_HD inline uint32_t bch_table_entry(uint32_t h, uint32_t M)
{
    uint32_t v = h;
    for (int i = 0; i < 16; ++i) {
        v <<= 1;
        if (v >> 16) v ^= M;
    }
    return v;
}

/* the eight bits of a byte in reverse order: a row's byte as a polynomial */
BCH_HD inline uint32_t bch_rev8(uint32_t b)
{
    b = ((b & 0xf0u) >> 4) | ((b & 0x0fu) << 4);
    b = ((b & 0xccu) >> 2) | ((b & 0x33u) << 2);
    return ((b & 0xaau) >> 1) | ((b & 0x55u) << 1);
}

inline int bch_degree(uint32_t p)
{
    int d = -1;
    for (; p; p >>= 1) ++d;
    return d;
}

/* prim has degree m and x has the full order 2^m - 1 modulo it (then the residues are a field and prim is irreducible) */
inline bool bch_is_primitive(int m, uint32_t prim)
{
    if (m < 2 || m > 16 || (prim >> m) != 1u) return false;
    const uint32_t N = (1u << m) - 1u;
    if (bch_powmod(2u, N, prim, m) != 1u) return false;
    uint32_t rest = N;
    for (uint32_t q = 2; q * q <= rest; ++q) {
        if (rest % q) continue;
        if (bch_powmod(2u, N / q, prim, m) == 1u) return false;
        while (rest % q == 0) rest /= q;
    }
    if (rest > 1 && rest < N && bch_powmod(2u, N / rest, prim, m) == 1u) return false;
    return true;
}

/* the generator of the code (m, prim, t) and what it is made of */
struct BchGen {
    int32_t m, t, nmin, r;
    uint32_t prim;
    uint32_t mp[kBchMaxT];          /* the distinct minimal polynomials, in the order their first root alpha^j appears */
    int32_t deg[kBchMaxT], leader[kBchMaxT];
    int32_t cls[2 * kBchMaxT];      /* alpha^j, j = 1 .. 2t, is a root of mp[cls[j - 1]] */
    uint64_t g[kBchWords];
};

inline void bch_poly_mul(uint64_t *dst, const uint64_t *a, uint32_t b)
{
    uint64_t out[kBchWords] = {0, 0, 0, 0};
    for (int s = 0; s <= 16; ++s) {
        if (!((b >> s) & 1u)) continue;
        for (int w = 0; w < kBchWords; ++w) {
            out[w] ^= a[w] << s;
            if (s && w) out[w] ^= a[w - 1] >> (64 - s);
        }
    }
    memcpy(dst, out, sizeof out);
}

inline int bch_poly_bit(const uint64_t *a, int i)
{
    return (int)((a[i >> 6] >> (i & 63)) & 1u);
}

/* a mod q for a polynomial a of up to 256 bits and q of degree d <= 16 */
inline uint32_t bch_poly_mod(const uint64_t *a, uint32_t q, int d)
{
    uint32_t rem = 0;
    for (int i = 64 * kBchWords - 1; i >= 0; --i) {
        rem = (rem << 1) | (uint32_t)bch_poly_bit(a, i);
        if ((rem >> d) & 1u) rem ^= q;
    }
    return rem;
}

/* 0, or 1 with a message that names the field: m, prim, t alone */
inline int bch_make_gen(int32_t m, uint32_t prim, int32_t t, BchGen *G, char *msg, size_t cap)
{
    if (m < 4 || m > 16) return snprintf(msg, cap, "spec.m = %d is outside 4 .. 16", m), 1;
    if (!bch_is_primitive(m, prim)) return snprintf(msg, cap, "spec.prim = 0x%X is not a primitive polynomial of degree m = %d", prim, m), 1;
    const int32_t N = (1 << m) - 1;
    if (t < 1 || t > kBchMaxT || 2 * t >= N)
        return snprintf(msg, cap, "spec.t = %d is outside 1 .. %d with 2 t < 2^m - 1 = %d", t, kBchMaxT, N), 1;
    memset(G, 0, sizeof *G);
    G->m = m; G->t = t; G->prim = prim;
    G->g[0] = 1;
    for (int32_t j = 1; j <= 2 * t; ++j) {
        int32_t lead = j, e = j;
        do { if (e < lead) lead = e; e = (2 * e) % N; } while (e != j);
        int c = -1;
        for (int i = 0; i < G->nmin; ++i) if (G->leader[i] == lead) c = i;
        if (c < 0) {
            /* prod over the coset of (x + alpha^e), coefficients in GF(2^m); they end in GF(2) */
            uint32_t co[18] = {1};
            int d = 0;
            e = j;
            do {
                const uint32_t beta = bch_powmod(2u, (uint64_t)e, prim, m);
                for (int k = ++d; k >= 0; --k) co[k] = (k ? co[k - 1] : 0u) ^ (k < d ? bch_mulmod(co[k], beta, prim, m) : 0u);
                e = (2 * e) % N;
            } while (e != j);
            uint32_t p = 0;
            for (int k = 0; k <= d; ++k) p |= (co[k] & 1u) << k;
            c = G->nmin++;
            G->mp[c] = p; G->deg[c] = d; G->leader[c] = lead;
            bch_poly_mul(G->g, G->g, p);
            G->r += d;
        }
        G->cls[j - 1] = c;
    }
    return 0;
}

struct BchLayout {
    int32_t k, r, nmin, m;
};

/* 0, or 1 with a message that names the field */
inline int bch_check_spec(const ldpc_bch_spec *s, BchGen *G, BchLayout *lay, char *msg, size_t cap)
{
    if (!s) return snprintf(msg, cap, "spec is NULL"), 1;
    if (s->struct_size != sizeof(ldpc_bch_spec))
        return snprintf(msg, cap, "spec.struct_size = %u, this library's ldpc_bch_spec has %u bytes", s->struct_size,
                        (unsigned)sizeof(ldpc_bch_spec)), 1;
    if (bch_make_gen(s->m, s->prim, s->t, G, msg, cap)) return 1;
    if (s->n < 8 || s->n % 8 || s->n > (1 << s->m) - 1)
        return snprintf(msg, cap, "spec.n = %d must be a positive multiple of 8, at most 2^m - 1 = %d", s->n, (1 << s->m) - 1), 1;
    const int32_t k = s->n - G->r;
    if (k < 8 || k % 8)
        return snprintf(msg, cap, "k = spec.n - r = %d - %d = %d must be a positive multiple of 8", s->n, G->r, k), 1;
    if (s->row_bytes < s->n / 8)
        return snprintf(msg, cap, "spec.row_bytes = %d is less than n / 8 = %d", s->row_bytes, s->n / 8), 1;
    if (lay) { lay->k = k; lay->r = G->r; lay->nmin = G->nmin; lay->m = s->m; }
    return 0;
}

inline void bch_spec_init(ldpc_bch_spec *s, int32_t n, int32_t t, int32_t row_bytes)
{
    s->struct_size = (uint32_t)sizeof(ldpc_bch_spec);
    s->n = n; s->t = t; s->row_bytes = row_bytes;
    if (n <= 16383) { s->m = 14; s->prim = 0x402Bu; }
    else { s->m = 16; s->prim = 0x1002Du; }
}

/* ---- the bitwise reference ------------------------------------------------------------------------------------- */

inline int bch_row_bit(const uint8_t *row, int64_t i)
{
    return (row[i >> 3] >> (i & 7)) & 1;
}

/* x^r a(x) mod g by long division, one bit at a time; p[w] bit b = coefficient of x^(64 w + b) */
inline void bch_ref_parity(const BchGen &G, const uint8_t *row, int32_t k, uint64_t *p)
{
    uint64_t reg[kBchWords] = {0, 0, 0, 0};
    for (int32_t i = 0; i < k; ++i) {
        const int fb = bch_poly_bit(reg, G.r - 1) ^ bch_row_bit(row, i);
        for (int w = kBchWords - 1; w >= 0; --w) reg[w] = (reg[w] << 1) | (w ? reg[w - 1] >> 63 : 0);
        if (fb) for (int w = 0; w < kBchWords; ++w) reg[w] ^= G.g[w];
        reg[G.r >> 6] &= ~((uint64_t)1 << (G.r & 63));
    }
    memcpy(p, reg, sizeof reg);
}

/* S_j = v(alpha^j), Horner over the n bits */
inline uint32_t bch_ref_syndrome(const BchGen &G, const uint8_t *row, int32_t n, int32_t j)
{
    const uint32_t aj = bch_powmod(2u, (uint64_t)j, G.prim, G.m);
    uint32_t s = 0;
    for (int32_t i = 0; i < n; ++i) s = bch_mulmod(s, aj, G.prim, G.m) ^ (uint32_t)bch_row_bit(row, i);
    return s;
}

/* ---- the plan ---------------------------------------------------------------------------------------------------- */

/* What a kernel launch runs from, by value.  A wave walks `nb` bytes of a row (encode: the k / 8 payload bytes, decode:
 * the n / 8 code bytes), lane l the run [l R, (l + 1) R); w[i][l] = x^(bits behind the run, plus r for the encoder)
 * mod M_i.  Decode: E[j - 1][b] = alpha^(j b); the Chien search gives lane l the positions [l P, (l + 1) P) and starts it
 * at chien[l] = alpha^-(n - 1 - l P), the inverse locator of its first position; aj[j - 1] = alpha^j is the step of term
 * j.  Encode: c[i] and G[i] of the Chinese remainder theorem. */
struct BchPlan {
    int32_t m, t, n, k, r, row_bytes, nmin;
    int32_t nb, R, P;
    uint32_t prim;
    uint32_t M[kBchMaxT], mp[kBchMaxT];
    int32_t deg[kBchMaxT];
    uint16_t c[kBchMaxT], aj[kBchMaxT];
    uint8_t cls[2 * kBchMaxT];
    uint16_t w[kBchMaxT][64];
    uint16_t chien[64];
    uint16_t E[2 * kBchMaxT][16];
    uint64_t G[kBchMaxT][kBchWords];
};

/* x^e mod M for a modulus of degree 16 that need not be irreducible */
inline uint32_t bch_xpow16(uint64_t e, uint32_t M)
{
    return bch_powmod(2u, e, M, 16);
}

inline void bch_make_plan(const ldpc_bch_spec *s, const BchGen &G, bool decode, BchPlan *p)
{
    memset(p, 0, sizeof *p);
    p->m = s->m; p->t = s->t; p->n = s->n; p->r = G.r; p->k = s->n - G.r; p->row_bytes = s->row_bytes; p->nmin = G.nmin;
    p->prim = s->prim;
    p->nb = (decode ? p->n : p->k) / 8;
    p->R = (p->nb + 63) / 64;
    p->P = (p->n + 63) / 64;
    const int64_t N = ((int64_t)1 << s->m) - 1;
    for (int i = 0; i < G.nmin; ++i) {
        p->mp[i] = G.mp[i]; p->deg[i] = G.deg[i];
        p->M[i] = G.mp[i] << (16 - G.deg[i]);
        for (int l = 0; l < 64; ++l) {
            const int64_t end = ((int64_t)l + 1) * p->R;
            const int64_t behind = end < p->nb ? 8 * (p->nb - end) : 0;
            p->w[i][l] = (uint16_t)bch_xpow16((uint64_t)(behind + (decode ? 0 : G.r)), p->M[i]);
        }
    }
    if (decode) {
        for (int j = 1; j <= 2 * s->t; ++j) {
            p->cls[j - 1] = (uint8_t)G.cls[j - 1];
            for (int b = 0; b < 16; ++b) p->E[j - 1][b] = (uint16_t)bch_powmod(2u, (uint64_t)(((int64_t)j * b) % N), s->prim, s->m);
        }
        for (int j = 1; j <= s->t; ++j) p->aj[j - 1] = (uint16_t)bch_powmod(2u, (uint64_t)j, s->prim, s->m);
        for (int l = 0; l < 64; ++l) {
            int64_t e = -((int64_t)p->n - 1 - (int64_t)l * p->P) % N;
            if (e < 0) e += N;
            p->chien[l] = (uint16_t)bch_powmod(2u, (uint64_t)e, s->prim, s->m);
        }
    } else {
        for (int i = 0; i < G.nmin; ++i) {
            uint64_t Gi[kBchWords] = {1, 0, 0, 0};
            for (int q = 0; q < G.nmin; ++q) if (q != i) bch_poly_mul(Gi, Gi, G.mp[q]);
            memcpy(p->G[i], Gi, sizeof Gi);
            /* the inverse in the field GF(2)[x] / m_i of 2^d elements */
            const uint32_t rem = bch_poly_mod(Gi, G.mp[i], G.deg[i]);
            p->c[i] = (uint16_t)bch_powmod(rem, ((uint64_t)1 << G.deg[i]) - 2, G.mp[i], G.deg[i]);
        }
    }
}

/* a value below 2^16 modulo m_i (degree d) */
BCH_HD inline uint32_t bch_reduce16(uint32_t v, uint32_t mp, int d)
{
    for (int i = 15; i >= d; --i)
        if ((v >> i) & 1u) v ^= mp << (i - d);
    return v;
}

}  // namespace ldpc
