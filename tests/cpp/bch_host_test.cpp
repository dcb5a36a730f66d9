// csrc/bch_host.hpp on its own (no HIP, no library): the field product against repeated shifting, primitivity of the two
// default polynomials and of none of a few reducible or non-primitive ones, the table of generator degrees, g | x^(2^m-1)+1,
// the byte table against eight single steps, and the plan: a row is walked the way a wave walks it (64 runs, byte tables,
// lane weights) and the combined remainders must give the syndromes of the direct evaluation (decode plan) and, through
// the Chinese remainder theorem, the parity of the long division (encode plan).  Built with the address and
// undefined-behaviour sanitizers by tests/test_bch_cpu.py and run directly.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../myldpccppapi_amd/csrc/bch_host.hpp"

using namespace ldpc;

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) { ++fails; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static uint32_t mul_by_shifting(uint32_t a, uint32_t b, uint32_t mod, int deg)
{
    uint32_t r = 0, t = a;
    for (int i = 0; i < deg; ++i) {
        if ((b >> i) & 1u) r ^= t;
        t <<= 1;
        if ((t >> deg) & 1u) t ^= mod;
    }
    return r;
}

// the wave's walk of bch_kernels.hpp on the host: u[i] = (row's first nb bytes as a polynomial, times the plan's factor) mod M_i
static void walk(const BchPlan &p, const uint8_t *row, uint32_t *u)
{
    std::vector<std::vector<uint16_t>> T(p.nmin, std::vector<uint16_t>(256));
    for (int i = 0; i < p.nmin; ++i)
        for (uint32_t h = 0; h < 256; ++h) T[i][h] = (uint16_t)bch_table_entry(h, p.M[i]);
    for (int i = 0; i < p.nmin; ++i) u[i] = 0;
    for (int lane = 0; lane < 64; ++lane) {
        const int32_t j0 = std::min(lane * p.R, p.nb), j1 = std::min(j0 + p.R, p.nb);
        for (int i = 0; i < p.nmin; ++i) {
            uint32_t reg = 0;
            for (int32_t j = j0; j < j1; ++j) reg = ((reg & 0xffu) << 8) ^ T[i][reg >> 8] ^ bch_rev8(row[j]);
            u[i] ^= bch_mulmod(reg, p.w[i][lane], p.M[i], 16);
        }
    }
}

static void check_code(int m, uint32_t prim, int t, int n, int row_bytes, std::mt19937_64 &rng)
{
    ldpc_bch_spec s;
    bch_spec_init(&s, n, t, row_bytes);
    s.m = m;
    s.prim = prim;
    char msg[240];
    BchGen G;
    BchLayout lay;
    if (bch_check_spec(&s, &G, &lay, msg, sizeof msg)) {
        ++fails;
        printf("FAILED spec (%d, %d, %d): %s\n", m, t, n, msg);
        return;
    }
    // g divides x^(2^m - 1) + 1: g(x) | x^N + 1 iff x^N = 1 modulo every minimal polynomial
    for (int i = 0; i < G.nmin; ++i) EXPECT(bch_powmod(2u, ((uint64_t)1 << m) - 1, G.mp[i], G.deg[i]) == 1u);
    std::vector<uint8_t> row((size_t)row_bytes);
    for (int rep = 0; rep < 3; ++rep) {
        for (auto &b : row) b = (uint8_t)rng();
        // decode plan: the syndromes from the walk equal Horner over the bits
        auto dp = std::make_unique<BchPlan>();
        bch_make_plan(&s, G, true, dp.get());
        uint32_t u[kBchMaxT];
        walk(*dp, row.data(), u);
        for (int j = 1; j <= 2 * t; ++j) {
            uint32_t S = 0;
            for (int b = 0; b < 16; ++b)
                if ((u[dp->cls[j - 1]] >> b) & 1u) S ^= dp->E[j - 1][b];
            EXPECT(S == bch_ref_syndrome(G, row.data(), n, j));
        }
        // encode plan: the Chinese remainder theorem gives the parity of the long division
        auto ep = std::make_unique<BchPlan>();
        bch_make_plan(&s, G, false, ep.get());
        walk(*ep, row.data(), u);
        uint64_t acc[kBchWords] = {0, 0, 0, 0}, want[kBchWords];
        for (int i = 0; i < G.nmin; ++i) {
            const uint32_t z = bch_mulmod(bch_reduce16(u[i], G.mp[i], G.deg[i]), ep->c[i], G.mp[i], G.deg[i]);
            uint64_t prod[kBchWords];
            bch_poly_mul(prod, ep->G[i], z);
            for (int w = 0; w < kBchWords; ++w) acc[w] ^= prod[w];
        }
        bch_ref_parity(G, row.data(), lay.k, want);
        EXPECT(memcmp(acc, want, sizeof acc) == 0);
    }
    // the inverse locator of a lane's first position
    auto dp = std::make_unique<BchPlan>();
    bch_make_plan(&s, G, true, dp.get());
    for (int l = 0; l < 64; ++l) {
        const int64_t pos = (int64_t)l * dp->P;
        if (pos >= n) continue;
        const uint32_t X = bch_powmod(2u, (uint64_t)(n - 1 - pos), prim, m);
        EXPECT(bch_mulmod(X, dp->chien[l], prim, m) == 1u);
    }
}

int main()
{
    std::mt19937_64 rng(4711);
    for (int rep = 0; rep < 2000; ++rep) {
        const uint32_t a = (uint32_t)rng() & 0xffffu, b = (uint32_t)rng() & 0xffffu;
        EXPECT(bch_mulmod(a, b, 0x1002Du, 16) == mul_by_shifting(a, b, 0x1002Du, 16));
        EXPECT(bch_mulmod(a & 0x3fffu, b & 0x3fffu, 0x402Bu, 14) == mul_by_shifting(a & 0x3fffu, b & 0x3fffu, 0x402Bu, 14));
    }
    EXPECT(bch_is_primitive(16, 0x1002Du) && bch_is_primitive(14, 0x402Bu) && bch_is_primitive(8, 0x11Du) && bch_is_primitive(4, 0x13u));
    EXPECT(!bch_is_primitive(4, 0x1Fu));        // x^4+x^3+x^2+x+1: irreducible, x has order 5
    EXPECT(!bch_is_primitive(4, 0x15u));        // (x^2+x+1)^2
    EXPECT(!bch_is_primitive(8, 0x11Bu));       // the AES polynomial: irreducible, x has order 51
    EXPECT(!bch_is_primitive(16, 0x1002Cu) && !bch_is_primitive(16, 0x2Du) && !bch_is_primitive(16, 0x3002Du));
    // byte table = sixteen single steps of h(x) x^16
    for (uint32_t h = 0; h < 256; ++h) EXPECT(bch_table_entry(h, 0x1002Du) == bch_mulmod(h, bch_powmod(2u, 16, 0x1002Du, 16), 0x1002Du, 16));
    for (uint32_t b = 0; b < 256; ++b) {
        uint32_t r = 0;
        for (int i = 0; i < 8; ++i) r |= ((b >> i) & 1u) << (7 - i);
        EXPECT(bch_rev8(b) == r);
    }
    // the table of degrees
    const int ts[3] = {12, 10, 8}, r16[3] = {192, 160, 128}, r14[3] = {168, 140, 112};
    char msg[240];
    for (int i = 0; i < 3; ++i) {
        BchGen G;
        EXPECT(bch_make_gen(16, 0x1002Du, ts[i], &G, msg, sizeof msg) == 0 && G.r == r16[i] && G.nmin == ts[i]);
        EXPECT(bch_make_gen(14, 0x402Bu, ts[i], &G, msg, sizeof msg) == 0 && G.r == r14[i] && G.nmin == ts[i]);
    }
    {   // m = 6: alpha^9 has a minimal polynomial of degree 3, alpha^21 one of degree 2
        BchGen G;
        EXPECT(bch_make_gen(6, 0x43u, 11, &G, msg, sizeof msg) == 0);
        EXPECT(G.deg[G.cls[8]] == 3 && G.deg[G.cls[20]] == 2 && G.mp[G.cls[20]] == 0x7u);
    }
    check_code(8, 0x11Du, 2, 40, 5, rng);
    check_code(8, 0x11Du, 3, 248, 33, rng);
    check_code(10, 0x409u, 4, 1000, 125, rng);
    check_code(6, 0x43u, 4, 56, 7, rng);        // minimal polynomials of degree 6: moduli shifted by ten places
    check_code(7, 0x89u, 8, 120, 16, rng);
    check_code(14, 0x402Bu, 12, 7200, 900, rng);
    check_code(16, 0x1002Du, 12, 32400, 4050, rng);
    check_code(16, 0x1002Du, 8, 58320, 7290, rng);
    printf(fails ? "%d failures\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
