// csrc/crc_term_host.hpp on its own (no HIP, no library): the column weights against the bitwise CRC of unit vectors and
// of random rows, at the lengths where an index could slip (one bit more than the parity, 64 +- 1, the largest block), the
// checks of the two config fields, and the CRC a transport-block spec's frames carry.  Built with the address and
// undefined-behaviour sanitizers by tests/test_crc_term_cpu.py and run directly.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../myldpccppapi_amd/csrc/crc_term_host.hpp"

using namespace ldpc;

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) { ++fails; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

int main()
{
    std::mt19937_64 rng(4711);
    const int kinds[3] = {LDPC_CRC16, LDPC_CRC24A, LDPC_CRC24B};
    const int lengths[] = {1, 17, 18, 25, 26, 63, 64, 65, 327, 328, 329, 352, 8447, 8448, 8449, 32400};
    for (int kind : kinds) {
        uint32_t g;
        int L;
        EXPECT(tb_crc_poly(kind, &g, &L));
        for (int n : lengths) {
            std::vector<uint32_t> w((size_t)n);               // exactly n entries: a write behind them is caught
            EXPECT(crc_term_weights(kind, n, w.data()));
            std::vector<uint8_t> row((size_t)(n + 7) / 8);
            // unit vectors: all of a short row, the ends and a sample of a long one
            for (int rep = 0; rep < (n <= 400 ? n : 200); ++rep) {
                const int k = n <= 400 ? rep : (rep == 0 ? 0 : rep == 1 ? n - 1 : (int)(rng() % (uint64_t)n));
                std::fill(row.begin(), row.end(), 0);
                row[(size_t)k >> 3] = (uint8_t)(1u << (k & 7));
                EXPECT(w[(size_t)k] == tb_crc_bits(g, L, row.data(), n));
                EXPECT(w[(size_t)k] < (1u << L) && w[(size_t)k] != 0);
            }
            // random rows: the XOR of the weights of the set bits is the row's CRC
            for (int rep = 0; rep < 20; ++rep) {
                for (auto &v : row) v = (uint8_t)rng();
                uint32_t x = 0;
                for (int k = 0; k < n; ++k)
                    if ((row[(size_t)k >> 3] >> (k & 7)) & 1) x ^= w[(size_t)k];
                EXPECT(x == tb_crc_bits(g, L, row.data(), n));
            }
        }
        EXPECT(crc_term_weights(kind, 0, nullptr));
        EXPECT(!crc_term_weights(kind, -1, nullptr));
        EXPECT(!crc_term_weights(kind, 8, nullptr));
    }
    EXPECT(!crc_term_weights(0, 8, nullptr) && !crc_term_weights(17, 8, nullptr));

    // the two config fields
    {
        char msg[256];
        EXPECT(crc_term_check(0, -5, 352, 0, msg, sizeof msg) == 0);                 // off: nothing else is read
        EXPECT(crc_term_check(LDPC_CRC16, 328, 352, 1, msg, sizeof msg) == 0);
        EXPECT(crc_term_check(LDPC_CRC16, 17, 352, 1, msg, sizeof msg) == 0);
        EXPECT(crc_term_check(LDPC_CRC24A, 25, 352, 1, msg, sizeof msg) == 0);
        EXPECT(crc_term_check(LDPC_CRC24B, 352, 352, 1, msg, sizeof msg) == 0);
        EXPECT(crc_term_check(LDPC_CRC16, 16, 352, 1, msg, sizeof msg) == 1 && strstr(msg, "crc_bits"));
        EXPECT(crc_term_check(LDPC_CRC24A, 24, 352, 1, msg, sizeof msg) == 1 && strstr(msg, "crc_bits"));
        EXPECT(crc_term_check(LDPC_CRC24B, 353, 352, 1, msg, sizeof msg) == 1 && strstr(msg, "crc_bits"));
        EXPECT(crc_term_check(LDPC_CRC24B, -1, 352, 1, msg, sizeof msg) == 1 && strstr(msg, "crc_bits"));
        EXPECT(crc_term_check(17, 328, 352, 1, msg, sizeof msg) == 1 && strstr(msg, "crc_kind"));
        EXPECT(crc_term_check(-16, 328, 352, 1, msg, sizeof msg) == 1 && strstr(msg, "crc_kind"));
        EXPECT(crc_term_check(LDPC_CRC16, 328, 352, 0, msg, sizeof msg) == 1 && strstr(msg, "early_term"));
    }

    // the CRC of a spec's frames
    {
        struct Shape { int A, tb, C, cb, K, kind, bits; };
        const Shape shapes[] = {{312, 16, 1, 0, 352, LDPC_CRC16, 328},    {4056, 24, 1, 0, 4080, LDPC_CRC24A, 4080},
                                {632, 24, 2, 24, 352, LDPC_CRC24B, 352},  {1024, 0, 2, 24, 536, LDPC_CRC24B, 536},
                                {1000, 24, 2, 0, 512, 0, 0},              {1000, 0, 1, 0, 1024, 0, 0}};
        for (const Shape &sh : shapes) {
            ldpc_tb_spec spec;
            tb_spec_init(&spec, sh.A, sh.K);
            spec.tb_crc = sh.tb; spec.C = sh.C; spec.cb_crc = sh.cb;
            int32_t kind = -1, bits = -1;
            char msg[256];
            const int rc = tb_frame_crc(&spec, &kind, &bits, msg, sizeof msg);
            if (sh.kind) EXPECT(rc == 0 && kind == sh.kind && bits == sh.bits);
            else EXPECT(rc == 1 && kind == -1 && bits == -1 && strstr(msg, "no CRC"));
        }
        ldpc_tb_spec bad;
        tb_spec_init(&bad, 312, 352);
        bad.C = 3;
        char msg[256];
        EXPECT(tb_frame_crc(&bad, nullptr, nullptr, msg, sizeof msg) == 1);
        EXPECT(tb_frame_crc(nullptr, nullptr, nullptr, msg, sizeof msg) == 1);
    }
    printf("%s\n", fails ? "failed" : "ok");
    return fails ? 1 : 0;
}
