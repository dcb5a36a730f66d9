// csrc/osd_host.hpp on its own (no HIP, no library): the eligibility arithmetic on the codes the header names, the dense
// image against the edge list bit by bit (N a multiple of 32 and not), the independent row subset of a graph with more rows
// than columns (rank and row space against a separate elimination), and the LDS layout: regions in order, disjoint, inside
// the workgroup's limit for every shape the rule admits.  Built with the address and undefined-behaviour sanitizers by
// tests/test_osd_cpu.py and run directly.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../myldpccppapi_amd/csrc/osd_host.hpp"

using namespace ldpc;

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) { ++fails; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

struct Csr {
    int32_t M, N;
    std::vector<int32_t> row_ptr, cols;
};

static Csr random_graph(int32_t M, int32_t N, int deg, uint32_t seed)
{
    std::mt19937 rng(seed);
    Csr g{M, N, {0}, {}};
    for (int32_t m = 0; m < M; ++m) {
        std::vector<int32_t> c;
        const int d = (m % 7 == 3) ? 0 : deg;                       // some rows without an edge
        while ((int)c.size() < std::min(d, N)) {
            const int32_t n = (int32_t)(rng() % (uint32_t)N);
            if (std::find(c.begin(), c.end(), n) == c.end()) c.push_back(n);
        }
        std::sort(c.begin(), c.end());
        g.cols.insert(g.cols.end(), c.begin(), c.end());
        g.row_ptr.push_back((int32_t)g.cols.size());
    }
    return g;
}

// rank over GF(2) of rows given as bit vectors of W words
static int rank_of(std::vector<std::vector<uint32_t>> rows, int W)
{
    int rank = 0;
    for (int c = 0; c < 32 * W && rank < (int)rows.size(); ++c) {
        int p = -1;
        for (int r = rank; r < (int)rows.size(); ++r)
            if ((rows[r][c >> 5] >> (c & 31)) & 1u) { p = r; break; }
        if (p < 0) continue;
        std::swap(rows[rank], rows[p]);
        for (int r = 0; r < (int)rows.size(); ++r)
            if (r != rank && ((rows[r][c >> 5] >> (c & 31)) & 1u))
                for (int w = 0; w < W; ++w) rows[r][w] ^= rows[rank][w];
        ++rank;
    }
    return rank;
}

static std::vector<std::vector<uint32_t>> rows_of(const Csr &g)
{
    const int W = osd_words(g.N);
    std::vector<std::vector<uint32_t>> rows(g.M, std::vector<uint32_t>(W, 0u));
    for (int32_t m = 0; m < g.M; ++m)
        for (int32_t k = g.row_ptr[m]; k < g.row_ptr[m + 1]; ++k) rows[m][g.cols[k] >> 5] |= 1u << (g.cols[k] & 31);
    return rows;
}

static void check_layout(int32_t R, int32_t N)
{
    const OsdLayout l = osd_layout(R, N);
    EXPECT(l.W == (N + 31) / 32 && l.P >= N && (l.P & (l.P - 1)) == 0 && (l.P == 2 || l.P / 2 < N));
    EXPECT(l.G >= l.W && (l.G & (l.G - 1)) == 0 && (1 << l.logG) == l.G && l.G <= kOsdMaxBlock);
    const uint32_t at[] = {l.A, l.keys, l.wt, l.hb, l.pm, l.cw, l.rowcol, l.s, l.list, l.ctl, l.total_words};
    const uint32_t need[] = {(uint32_t)R * l.W, (uint32_t)l.P, ((uint32_t)N + 1) / 2, (uint32_t)l.W, (uint32_t)l.W, (uint32_t)l.W,
                             ((uint32_t)R + 1) / 2, (uint32_t)R, ((uint32_t)R + 1) / 2, kOsdCtlWords};
    for (int i = 0; i < 10; ++i) EXPECT(at[i] + need[i] <= at[i + 1]);
    EXPECT(l.A == 0 && l.ctl % 2 == 0);
    const int32_t T = osd_block(l.W);                                   // whole waves, whole row groups
    EXPECT(T >= 256 && T <= kOsdMaxBlock && T % 64 == 0 && T % l.G == 0 && T / l.G >= 2);
    EXPECT(l.bytes() <= kOsdMaxLds);
}

int main()
{
    char msg[320];
    // the codes the header names
    EXPECT(osd_eligible(288, 576, msg, sizeof msg) == 0);
    EXPECT(osd_eligible(576, 1152, msg, sizeof msg) == 0);
    EXPECT(osd_eligible(192, 1152, msg, sizeof msg) == 0);
    EXPECT(osd_eligible(736, 1088, msg, sizeof msg) == 0);
    EXPECT(osd_eligible(1152, 2304, msg, sizeof msg) == 1 && strstr(msg, "N = 2304") && strstr(msg, "82944"));
    EXPECT(osd_eligible(4, 4097, msg, sizeof msg) == 1 && strstr(msg, "N = 4097") && strstr(msg, "516"));
    EXPECT(osd_eligible(224, 4096, msg, sizeof msg) == 0 && osd_eligible(225, 4096, msg, sizeof msg) == 1);
    EXPECT(osd_eligible(28672, 32, msg, sizeof msg) == 0 && osd_eligible(28673, 32, msg, sizeof msg) == 1);
    EXPECT(osd_eligible(0x7fffffff, 4096, msg, sizeof msg) == 1);              // no overflow in the product

    // the dense image, bit by bit
    for (int32_t N : {7, 32, 100, 576, 1088}) {
        const Csr g = random_graph(std::max(3, N / 2), N, 5, 1000u + (uint32_t)N);
        OsdImage im;
        osd_dense_image(g.M, g.N, g.row_ptr.data(), g.cols.data(), &im);
        EXPECT(im.R == g.M && im.W == osd_words(N) && im.bits.size() == (size_t)im.R * im.W);
        const auto rows = rows_of(g);
        for (int32_t m = 0; m < g.M; ++m)
            for (int w = 0; w < im.W; ++w) EXPECT(im.bits[(size_t)m * im.W + w] == rows[m][w]);
    }

    // more rows than columns: an independent subset of the same rank that spans the same space
    for (int32_t N : {5, 31, 33, 64}) {
        const Csr g = random_graph(3 * N + 1, N, 3, 2000u + (uint32_t)N);
        OsdImage im;
        osd_dense_image(g.M, g.N, g.row_ptr.data(), g.cols.data(), &im);
        auto all = rows_of(g);
        const int rank = rank_of(all, im.W);
        EXPECT(im.R == rank && im.R <= N && im.bits.size() == (size_t)im.R * im.W);
        std::vector<std::vector<uint32_t>> kept;
        for (int r = 0; r < im.R; ++r) kept.emplace_back(im.bits.begin() + (size_t)r * im.W, im.bits.begin() + (size_t)(r + 1) * im.W);
        EXPECT(rank_of(kept, im.W) == rank);
        for (const auto &k : kept) EXPECT(std::find(all.begin(), all.end(), k) != all.end());     // rows of H as they are
        auto both = all;
        both.insert(both.end(), kept.begin(), kept.end());
        EXPECT(rank_of(both, im.W) == rank);
        check_layout(im.R, N);
    }

    // the layout on the shapes of the tests and at the rule's corners
    EXPECT(osd_block(18) == 512 && osd_block(36) == 1024 && osd_block(1) == 256 && osd_block(128) == 1024);
    check_layout(288, 576);
    check_layout(576, 1152);
    check_layout(736, 1088);
    check_layout(192, 1152);
    check_layout(3, 7);
    check_layout(44, 100);
    check_layout(224, 4096);
    check_layout(1, 4096);
    check_layout(32, 32);
    for (int32_t N = 1; N <= 4096; N += 13) {          // the most rows the rule admits with M <= N
        const int32_t R = (int32_t)std::min<int64_t>(N, kOsdMaxWords / osd_words(N));
        check_layout(R, N);
    }

    printf(fails ? "%d failures\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
