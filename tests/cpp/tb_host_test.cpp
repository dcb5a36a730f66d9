// csrc/tb_host.hpp on its own (no HIP, no library): GF(2) arithmetic modulo the three generators against repeated
// shifting, the byte table against eight single steps, the combine identity against the bitwise CRC on random rows cut
// at random points, and the plan's lane weights by walking a block the way a wave does.  Built with the address and
// undefined-behaviour sanitizers by tests/test_tb_cpu.py and run directly.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../myldpccppapi_amd/csrc/tb_host.hpp"

using namespace ldpc;

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) { ++fails; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// r * x mod g
static uint32_t shift1(uint32_t r, uint32_t g, int L)
{
    r <<= 1;
    return (r >> L) & 1u ? r ^ g : r;
}

static uint32_t mul_by_shifting(uint32_t a, uint32_t b, uint32_t g, int L)
{
    uint32_t r = 0, t = a;                      // t = a x^i
    for (int i = 0; i < L; ++i) {
        if ((b >> i) & 1u) r ^= t;
        t = shift1(t, g, L);
    }
    return r;
}

static uint32_t crc_of_bits(const std::vector<uint8_t> &bits, size_t lo, size_t hi, uint32_t g, int L)
{
    uint32_t r = 0;
    for (size_t i = lo; i < hi; ++i) r = tb_crc_step(r, bits[i], g, L);
    return r;
}

int main()
{
    std::mt19937_64 rng(12345);
    const int kinds[3] = {LDPC_CRC16, LDPC_CRC24A, LDPC_CRC24B};
    for (int kind : kinds) {
        uint32_t g;
        int L;
        EXPECT(tb_crc_poly(kind, &g, &L));
        const uint32_t mask = (1u << L) - 1u;
        // mulmod against shifting; x^n against n shifts; x^-n undoes x^n
        for (int rep = 0; rep < 2000; ++rep) {
            const uint32_t a = (uint32_t)rng() & mask, b = (uint32_t)rng() & mask;
            EXPECT(gf2_mulmod(a, b, g, L) == mul_by_shifting(a, b, g, L));
            EXPECT(gf2_mulmod(a, b, g, L) == gf2_mulmod(b, a, g, L));
        }
        uint32_t xn = 1;
        for (int n = 0; n < 3000; ++n) {
            EXPECT(gf2_xpow(n, g, L) == xn);
            EXPECT(gf2_mulmod(gf2_xpow(-n, g, L), xn, g, L) == 1u);
            xn = shift1(xn, g, L);
        }
        const int64_t big = 259199;              // the bits behind lane 0 of a 32400-byte block
        EXPECT(gf2_xpow(big, g, L) == gf2_mulmod(gf2_xpow(big - 2999, g, L), gf2_xpow(2999, g, L), g, L));
        EXPECT(gf2_xpow(8 - big, g, L) == gf2_mulmod(gf2_xpow(-big, g, L), gf2_xpow(8, g, L), g, L));
        // reflect is an involution; the byte table equals eight single steps
        for (uint32_t b = 0; b < 256; ++b) {
            uint32_t r = 0;
            for (int q = 0; q < 8; ++q) r = tb_crc_step(r, b >> q, g, L);
            EXPECT(tb_reflect(tb_table_entry(b, g, L), L) == r);
            EXPECT(tb_reflect(tb_reflect(b * 257u & mask, L), L) == (b * 257u & mask));
        }
        // a reflected register walking bytes through the table equals the bitwise CRC
        for (int rep = 0; rep < 50; ++rep) {
            const size_t nbytes = 1 + rng() % 300;
            std::vector<uint8_t> row(nbytes);
            for (auto &v : row) v = (uint8_t)rng();
            uint32_t rr = 0;
            for (uint8_t v : row) rr = (rr >> 8) ^ tb_table_entry((rr ^ v) & 0xffu, g, L);
            EXPECT(tb_reflect(rr, L) == tb_crc_bits(g, L, row.data(), (int64_t)nbytes * 8));
        }
        // the combine identity: random rows cut at random points, lengths that are no multiples of 8
        for (int rep = 0; rep < 300; ++rep) {
            const size_t n = 1 + rng() % 2500;
            std::vector<uint8_t> bits(n), packed((n + 7) / 8, 0);
            for (size_t i = 0; i < n; ++i) {
                bits[i] = (uint8_t)(rng() & 1);
                packed[i >> 3] |= (uint8_t)(bits[i] << (i & 7));
            }
            const uint32_t whole = tb_crc_bits(g, L, packed.data(), (int64_t)n);
            EXPECT(whole == crc_of_bits(bits, 0, n, g, L));
            const int cuts = 1 + (int)(rng() % 8);
            std::vector<size_t> at = {0, n};
            for (int c = 0; c < cuts; ++c) at.push_back(rng() % (n + 1));
            std::sort(at.begin(), at.end());
            uint32_t sum = 0;
            for (size_t k = 0; k + 1 < at.size(); ++k)
                sum ^= gf2_mulmod(crc_of_bits(bits, at[k], at[k + 1], g, L), gf2_xpow((int64_t)(n - at[k + 1]), g, L), g, L);
            EXPECT(sum == whole);
            // zero padding behind the data is undone by a negative power of x
            const int pad = (int)(rng() % 8);
            uint32_t padded = whole;
            for (int q = 0; q < pad; ++q) padded = tb_crc_step(padded, 0, g, L);
            EXPECT(gf2_mulmod(padded, gf2_xpow(-pad, g, L), g, L) == whole);
        }
    }

    // the plan: walk code blocks the way the attach kernel does (64 runs of R bytes, partials times the lane weights) and
    // meet the segment remainders the way its waves do
    struct Shape { int A, tb, C, cb, K; };
    const Shape shapes[] = {{8, 16, 1, 0, 24}, {312, 16, 1, 0, 352}, {4056, 24, 1, 0, 4080}, {1008, 24, 2, 24, 544}, {1008, 24, 8, 24, 160},
                            {1024, 16, 16, 24, 96}, {5176, 24, 65, 24, 104}, {32376, 24, 1, 0, 32400}, {1024, 0, 2, 24, 536}};
    for (const Shape &sh : shapes) {
        ldpc_tb_spec spec;
        tb_spec_init(&spec, sh.A, sh.K);
        spec.tb_crc = sh.tb; spec.C = sh.C; spec.cb_crc = sh.cb;
        TbLayout lay;
        char msg[200];
        EXPECT(tb_check_spec(&spec, &lay, msg, sizeof msg) == 0);
        TbPlan p;
        tb_make_plan(&spec, lay, false, &p);
        EXPECT(p.nb == (lay.S + 7) / 8 && p.R == (p.nb + 63) / 64 && p.W == (sh.C < 4 ? sh.C : 4));
        std::vector<uint8_t> stream((size_t)lay.B, 0);          // payload bits, zeros where the parity will stand
        for (int i = 0; i < sh.A; ++i) stream[(size_t)i] = (uint8_t)(rng() & 1);
        std::vector<uint32_t> acc((size_t)p.W, 0);
        for (int c = 0; c < sh.C; ++c) {
            uint32_t rB = 0, rA = 0;
            for (int l = 0; l < 64; ++l) {
                uint32_t pB = 0, pA = 0;
                for (int j = l * p.R; j < (l + 1) * p.R && j < p.nb; ++j)
                    for (int q = 0; q < 8; ++q) {
                        const int i = 8 * j + q;
                        const uint32_t bit = i < lay.S ? stream[(size_t)c * lay.S + i] : 0;
                        pB = tb_crc_step(pB, bit, kG24B, 24);
                        if (p.gA) pA = tb_crc_step(pA, bit, p.gA, p.LA);
                    }
                rB ^= gf2_mulmod(pB, p.wB[l], kG24B, 24);
                if (p.gA) rA ^= gf2_mulmod(pA, p.wA[l], p.gA, p.LA);
            }
            EXPECT(rB == crc_of_bits(stream, (size_t)c * lay.S, (size_t)(c + 1) * lay.S, kG24B, 24));
            if (p.gA) acc[(size_t)(c % p.W)] = gf2_mulmod(acc[(size_t)(c % p.W)], p.stepA, p.gA, p.LA) ^ rA;
        }
        if (p.gA) {
            uint32_t tot = 0;
            for (int w = 0; w < p.W; ++w) {
                const int last = w + ((sh.C - 1 - w) / p.W) * p.W;
                tot ^= gf2_mulmod(acc[(size_t)w], p.finA[sh.C - 1 - last], p.gA, p.LA);
            }
            EXPECT(tot == crc_of_bits(stream, 0, (size_t)sh.A, p.gA, p.LA));
        }
    }

    // the known answers: "123456789", each byte MSB first
    {
        const char *text = "123456789";
        uint8_t row[9];
        for (int i = 0; i < 9; ++i) {
            uint8_t v = 0;
            for (int q = 0; q < 8; ++q) v |= (uint8_t)((((uint8_t)text[i] >> (7 - q)) & 1) << q);
            row[i] = v;
        }
        EXPECT(tb_crc_bits(kG24A, 24, row, 72) == 0xCDE703u);
        EXPECT(tb_crc_bits(kG24B, 24, row, 72) == 0x23EF52u);
        EXPECT(tb_crc_bits(kG16, 16, row, 72) == 0x31C3u);
    }

    // spec: the rule and the refusals
    {
        ldpc_tb_spec s;
        char msg[200];
        tb_spec_init(&s, 3824, 8448);
        EXPECT(s.tb_crc == 16 && s.C == 1 && s.cb_crc == 0);
        tb_spec_init(&s, 3832, 8448);
        EXPECT(s.tb_crc == 24 && s.C == 1 && s.cb_crc == 0);
        tb_spec_init(&s, 8448 - 24 + 8, 8448);
        EXPECT(s.tb_crc == 24 && s.C == 2 && s.cb_crc == 24);
        tb_spec_init(&s, 312, 352);
        s.C = 3;
        EXPECT(tb_check_spec(&s, nullptr, msg, sizeof msg) == 1);
        s.C = 1; s.K = 320;
        EXPECT(tb_check_spec(&s, nullptr, msg, sizeof msg) == 1);
    }
    printf("%s\n", fails ? "failed" : "ok");
    return fails ? 1 : 0;
}
