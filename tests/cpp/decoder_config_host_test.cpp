// csrc/decoder_config_host.hpp on its own (no HIP, no library): the algorithm table, the accepted struct sizes and their
// zero extension, frames per lane at its thresholds, and the engine candidates of the four creation branches under every
// setting of LDPC_TUNE_FUSED / LDPC_TUNE_LDSP.  Built with the address and undefined-behaviour sanitizers by
// tests/test_decoder_config_cpu.py and run directly.  (Every refusal text of config_check is compared with recorded
// answers through the library: tests/decoder_config_cases.py.)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../myldpccppapi_amd/csrc/decoder_config_host.hpp"

using namespace ldpc;

static int fails = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) { ++fails; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// the (648, 324) code of the refusal sweep: K % 8 = 4, so LDPC_PACK_BITS does not pack whole bytes per frame
static ldpc_decoder_config base(int algo, int dtype = LDPC_MSG_F32)
{
    ldpc_decoder_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.K = 324; c.max_batch = 64; c.algo = algo; c.msg_dtype = dtype; c.max_iter = 40; c.llr_scale = 8.0f; c.early_term = 1;
    c.layer_rows = 27; c.pack_mode = LDPC_PACK_BYTES;
    return c;
}
static GraphFacts facts()
{
    GraphFacts g;
    g.M = 324; g.N = 648; g.E = 2048; g.max_row_deg = 7; g.max_col_deg = 6; g.rows_one_weight = false;
    return g;
}

static void test_table()
{
    const int assigned[] = {0, 1, 2, 3, 4, 5, 6, 8, 9, 10};
    EXPECT(sizeof kAlgos / sizeof kAlgos[0] == 10);
    for (int algo = -2; algo <= 13; ++algo) {
        bool want = false;
        for (int v : assigned) want = want || v == algo;
        const AlgoInfo *a = algo_info(algo);
        EXPECT((a != nullptr) == want);
        if (a) EXPECT(a->algo == algo && !strncmp(a->c_name, "LDPC_ALGO_", 10) && a->short_name[0] && a->msg_dtypes);
    }
    EXPECT(!algo_info(7) && !algo_info(11) && !algo_info(1 << 30));
    EXPECT(!strcmp(algo_info(LDPC_ALGO_LAYERED_BP_FX)->c_name, "LDPC_ALGO_LAYERED_BP_FX"));
    EXPECT(algo_info(LDPC_ALGO_MS)->msg_dtypes == (kF32 | kF16 | kF8 | kI8) && algo_info(LDPC_ALGO_BP)->msg_dtypes == (kF32 | kF16));
    EXPECT(algo_info(LDPC_ALGO_LAYERED_FX)->msg_dtypes == kI8 && algo_info(LDPC_ALGO_BITFLIP)->family == Family::Bitflip);
    EXPECT(algo_info(LDPC_ALGO_MS_FUSED)->family == Family::Reference && algo_info(LDPC_ALGO_LAYERED_HOST)->family == Family::Layered);
    for (const AlgoInfo &a : kAlgos) {
        EXPECT(a.handover == (a.family == Family::Flood));
        EXPECT(a.crc == (a.algo != LDPC_ALGO_MS_FUSED && a.algo != LDPC_ALGO_LAYERED_HOST));
        EXPECT(a.soft == (a.algo != LDPC_ALGO_SP && a.algo != LDPC_ALGO_BITFLIP));
        EXPECT(a.ms_corr == (a.algo == LDPC_ALGO_MS || a.algo == LDPC_ALGO_LAYERED || a.algo == LDPC_ALGO_LAYERED_FX));
        EXPECT(a.box_plus == (a.algo == LDPC_ALGO_BP || a.algo == LDPC_ALGO_LAYERED_BP || a.algo == LDPC_ALGO_LAYERED_BP_FX));
        EXPECT(a.layer_rows_divide == (a.algo == LDPC_ALGO_LAYERED_BP || a.fixed));
    }
}

static void test_config_in()
{
    const size_t full_size = sizeof(ldpc_decoder_config);
    const size_t sizes[] = {96, 104, 112, 128, 192};       // before ms_scale, crc_kind, msg_bits, bf_threshold; today's
    EXPECT(full_size == 192 && sizeof kConfigSizes / sizeof kConfigSizes[0] == 5);
    for (size_t k = 0; k < 5; ++k) EXPECT(kConfigSizes[k] == sizes[4 - k]);     // newest first
    for (size_t size = 0; size <= full_size + 8; ++size) {
        bool want = false;
        for (size_t s : sizes) want = want || s == size;
        // the caller's struct as exactly `size` bytes on the heap: a read behind them is caught
        const size_t have = size < 4 ? 4 : size;
        unsigned char *src = (unsigned char *)malloc(have);
        for (size_t i = 0; i < have; ++i) src[i] = (unsigned char)(0x11 + i % 200);
        const uint32_t sz = (uint32_t)size;
        memcpy(src, &sz, 4);
        ldpc_decoder_config full;
        memset(&full, 0xEE, sizeof full);
        char msg[512] = "";
        const int rc = config_in((const ldpc_decoder_config *)src, &full, msg, sizeof msg);
        EXPECT(rc == (want ? LDPC_OK : LDPC_ERR_ARG));
        if (want) {
            const unsigned char *got = (const unsigned char *)&full;
            EXPECT(full.struct_size == full_size && !msg[0]);
            EXPECT(!memcmp(got + 4, src + 4, size - 4));
            for (size_t i = size; i < full_size; ++i) EXPECT(got[i] == 0);
        } else {
            char text[128];
            snprintf(text, sizeof text, "config struct_size %u is none of 192, 128, 112, 104, 96 (ABI mismatch)", sz);
            EXPECT(!strcmp(msg, text));
            EXPECT(full.struct_size == 0xEEEEEEEEu);         // untouched
        }
        free(src);
    }
    char tiny[8];       // a short message buffer is cut, not overrun
    EXPECT(config_size_check(100, tiny, sizeof tiny) == LDPC_ERR_ARG && strlen(tiny) == 7);
}

static void test_frames_per_lane()
{
    EXPECT(kCfgUnrolledDegree == 16);
    const int U = kCfgUnrolledDegree;
    struct { int algo, dtype, batch, row_deg, col_deg, want; } t[] = {
        // flooding sum-product: the column degree as it is
        {LDPC_ALGO_SP, LDPC_MSG_F32, 255, 7, 3, 1}, {LDPC_ALGO_SP, LDPC_MSG_F32, 256, 7, 3, 2},
        {LDPC_ALGO_SP, LDPC_MSG_F32, 1023, 7, 3, 2}, {LDPC_ALGO_SP, LDPC_MSG_F32, 1024, 7, 3, 4},
        {LDPC_ALGO_SP, LDPC_MSG_F32, 1024, 99, 8, 4}, {LDPC_ALGO_SP, LDPC_MSG_F32, 1024, 1, 9, 2},
        {LDPC_ALGO_SP, LDPC_MSG_F32, 1024, 1, U, 2}, {LDPC_ALGO_SP, LDPC_MSG_F32, 1024, 1, U + 1, 1},
        {LDPC_ALGO_SP, LDPC_MSG_F32, 256, 1, U, 2}, {LDPC_ALGO_SP, LDPC_MSG_F32, 256, 1, U + 1, 1},
        // min-sum and BP: half the column degree, rounded up
        {LDPC_ALGO_MS, LDPC_MSG_F32, 1024, 1, 16, 4}, {LDPC_ALGO_MS, LDPC_MSG_F32, 1024, 1, 17, 2},
        {LDPC_ALGO_MS, LDPC_MSG_F32, 1024, 1, 2 * U, 2}, {LDPC_ALGO_MS, LDPC_MSG_F32, 1024, 1, 2 * U + 1, 1},
        {LDPC_ALGO_MS, LDPC_MSG_F16, 256, 1, 3, 2}, {LDPC_ALGO_MS, LDPC_MSG_F16, 1024, 1, 3, 4},
        {LDPC_ALGO_BP, LDPC_MSG_F32, 1024, 1, 15, 4}, {LDPC_ALGO_BP, LDPC_MSG_F32, 1024, 1, 17, 2}, {LDPC_ALGO_BP, LDPC_MSG_F16, 1023, 1, 3, 2},
        // one-byte messages: 4 from one full tile of 256 on
        {LDPC_ALGO_MS, LDPC_MSG_F8, 255, 1, 3, 1}, {LDPC_ALGO_MS, LDPC_MSG_F8, 256, 1, 16, 4}, {LDPC_ALGO_MS, LDPC_MSG_F8, 256, 1, 17, 2},
        {LDPC_ALGO_MS, LDPC_MSG_I8, 256, 1, 3, 4}, {LDPC_ALGO_MS, LDPC_MSG_I8, 256, 1, 17, 2}, {LDPC_ALGO_MS, LDPC_MSG_I8, 256, 1, 2 * U + 1, 1},
        // layered and layered BP: the row degree
        {LDPC_ALGO_LAYERED, LDPC_MSG_F32, 1024, 8, 99, 4}, {LDPC_ALGO_LAYERED, LDPC_MSG_F32, 1024, 9, 1, 2},
        {LDPC_ALGO_LAYERED, LDPC_MSG_F32, 1024, U, 1, 2}, {LDPC_ALGO_LAYERED, LDPC_MSG_F32, 1024, U + 1, 1, 1},
        {LDPC_ALGO_LAYERED, LDPC_MSG_F32, 255, 3, 1, 1}, {LDPC_ALGO_LAYERED, LDPC_MSG_F32, 256, 3, 1, 2},
        {LDPC_ALGO_LAYERED_BP, LDPC_MSG_F32, 1024, 8, 99, 4}, {LDPC_ALGO_LAYERED_BP, LDPC_MSG_F32, 256, U + 1, 1, 1},
        // the reference-reproducing ones and bit flipping (whose handle then takes 1): the column degree
        {LDPC_ALGO_LAYERED_HOST, LDPC_MSG_F32, 1024, 20, 6, 4}, {LDPC_ALGO_LAYERED_HOST, LDPC_MSG_F32, 1024, 6, 9, 2},
        {LDPC_ALGO_MS_FUSED, LDPC_MSG_F32, 1024, 1, 8, 4}, {LDPC_ALGO_MS_FUSED, LDPC_MSG_F32, 1024, 1, 9, 2},
        {LDPC_ALGO_BITFLIP, LDPC_MSG_F32, 1024, 1, 8, 4}, {LDPC_ALGO_BITFLIP, LDPC_MSG_F32, 1023, 1, 8, 2},
        // fixed-point layered: no degree counts
        {LDPC_ALGO_LAYERED_FX, LDPC_MSG_I8, 255, 99, 99, 1}, {LDPC_ALGO_LAYERED_FX, LDPC_MSG_I8, 256, 99, 99, 4},
        {LDPC_ALGO_LAYERED_BP_FX, LDPC_MSG_I8, 64, 3, 3, 1}, {LDPC_ALGO_LAYERED_BP_FX, LDPC_MSG_I8, 1023, 30, 30, 4},
    };
    for (const auto &e : t) {
        ldpc_decoder_config c = base(e.algo, e.dtype);
        c.max_batch = e.batch;
        const int got = pick_frames_per_lane(c, e.row_deg, e.col_deg);
        if (got != e.want) printf("algo %d dtype %d batch %d degrees %d/%d: %d, expected %d\n", e.algo, e.dtype, e.batch, e.row_deg, e.col_deg, got, e.want);
        EXPECT(got == e.want);
        for (int fpl : {1, 2, 4}) {             // the caller's own value wins
            c.frames_per_lane = fpl;
            EXPECT(pick_frames_per_lane(c, e.row_deg, e.col_deg) == fpl);
        }
    }
}

// R / r: record kernel with / without the LDS limit, X: fixed-point record kernel, U / u: LDS-resident kernel (u: needs
// eligible_sp), L: streaming layered, F: streaming flooding, B: bit flipping; "!" a refusal behind the device check
static std::string show(const Candidates &c)
{
    if (c.code) return c.code == LDPC_ERR_UNSUPPORTED && c.refusal && c.refusal[0] ? "!" : "?";
    std::string s;
    for (int k = 0; k < c.n; ++k) {
        const Candidate &x = c.c[k];
        if ((x.lds_limit && x.engine != Engine::Ldsp) || (x.needs_sp && x.engine != Engine::Fused)) return "?";
        s += x.engine == Engine::Ldsp ? (x.lds_limit ? 'R' : 'r') : x.engine == Engine::LdspFx ? 'X'
             : x.engine == Engine::Fused ? (x.needs_sp ? 'u' : 'U') : x.engine == Engine::Layered ? 'L'
             : x.engine == Engine::Flood ? 'F' : 'B';
    }
    return s;
}

// want[3 * fused + ldsp], each of automatic (0), forced on (1), forced off (2)
static void expect_candidates(const char *what, ldpc_decoder_config c, const char *const want[9])
{
    for (int fused = 0; fused < 3; ++fused)
        for (int ldsp = 0; ldsp < 3; ++ldsp) {
            c.tune_flags = (c.tune_flags & ~15) | (fused << LDPC_TUNE_FUSED) | (ldsp << LDPC_TUNE_LDSP);
            const std::string got = show(engine_candidates(c, facts(), tune_from_config(c)));
            if (got != want[3 * fused + ldsp]) printf("%s, fused %d ldsp %d: %s, expected %s\n", what, fused, ldsp, got.c_str(), want[3 * fused + ldsp]);
            EXPECT(got == want[3 * fused + ldsp]);
        }
}

static void test_engine_candidates()
{
    const auto with = [](ldpc_decoder_config c, const char *change) {
        if (!strcmp(change, "corr")) c.ms_scale = 0.75f;
        else if (!strcmp(change, "offset")) c.ms_offset = 0.25f;
        else if (!strcmp(change, "crc")) { c.crc_kind = LDPC_CRC16; c.crc_bits = 200; }
        else if (!strcmp(change, "bits")) c.pack_mode = LDPC_PACK_BITS;
        else if (!strcmp(change, "fx_record")) c.tune_flags |= 1 << LDPC_TUNE_FX_RECORD;
        else if (!strcmp(change, "large")) c.max_batch = 4097;          // 4097 * 2048 edges > 2^23 edge-frames
        else if (!strcmp(change, "edge")) c.max_batch = 4096;           // = 2^23: still small
        else abort();
        return c;
    };
    const char *const all_L[9] = {"L", "L", "L", "L", "L", "L", "L", "L", "L"};
    const char *const all_F[9] = {"F", "F", "F", "F", "F", "F", "F", "F", "F"};
    const char *const all_B[9] = {"B", "B", "B", "B", "B", "B", "B", "B", "B"};
    const char *const all_no[9] = {"!", "!", "!", "!", "!", "!", "!", "!", "!"};

    // LDPC_ALGO_MS_FUSED: the record kernel unless LDSP is off, then the LDS-resident one; FUSED does not matter
    const char *const msf[9] = {"RU", "rU", "U", "RU", "rU", "U", "RU", "rU", "U"};
    expect_candidates("ms_fused", base(LDPC_ALGO_MS_FUSED), msf);
    expect_candidates("ms_fused bits", with(base(LDPC_ALGO_MS_FUSED), "bits"), all_no);

    // LAYERED_HOST, LAYERED_BP and the fixed-point layered algorithms: the streaming layered engine, LAYERED_FX behind
    // the fixed-point record kernel with LDPC_TUNE_FX_RECORD
    const char *const all_XL[9] = {"XL", "XL", "XL", "XL", "XL", "XL", "XL", "XL", "XL"};
    expect_candidates("layered_host", base(LDPC_ALGO_LAYERED_HOST), all_L);
    expect_candidates("layered_host bits", with(base(LDPC_ALGO_LAYERED_HOST), "bits"), all_L);
    expect_candidates("layered_bp", base(LDPC_ALGO_LAYERED_BP), all_L);
    expect_candidates("layered_bp crc", with(base(LDPC_ALGO_LAYERED_BP), "crc"), all_L);
    expect_candidates("layered_fx", base(LDPC_ALGO_LAYERED_FX, LDPC_MSG_I8), all_L);
    expect_candidates("layered_fx corr", with(base(LDPC_ALGO_LAYERED_FX, LDPC_MSG_I8), "corr"), all_L);
    expect_candidates("layered_fx crc", with(base(LDPC_ALGO_LAYERED_FX, LDPC_MSG_I8), "crc"), all_L);
    expect_candidates("layered_fx fx_record", with(base(LDPC_ALGO_LAYERED_FX, LDPC_MSG_I8), "fx_record"), all_XL);
    expect_candidates("layered_fx fx_record corr", with(with(base(LDPC_ALGO_LAYERED_FX, LDPC_MSG_I8), "fx_record"), "corr"), all_XL);
    expect_candidates("layered_fx fx_record bits", with(with(base(LDPC_ALGO_LAYERED_FX, LDPC_MSG_I8), "fx_record"), "bits"), all_L);
    expect_candidates("layered_bp_fx", base(LDPC_ALGO_LAYERED_BP_FX, LDPC_MSG_I8), all_L);
    expect_candidates("layered_bp_fx bits", with(base(LDPC_ALGO_LAYERED_BP_FX, LDPC_MSG_I8), "bits"), all_L);

    // LDPC_ALGO_LAYERED: record kernel (no LDS limit), LDS-resident kernel, streaming; FUSED off keeps the streaming kernels
    const char *const lay[9] = {"rUL", "rUL", "UL", "rUL", "rUL", "UL", "L", "L", "L"};
    const char *const lay_corr[9] = {"rL", "rL", "L", "rL", "rL", "!", "L", "L", "L"};
    expect_candidates("layered", base(LDPC_ALGO_LAYERED), lay);
    expect_candidates("layered large", with(base(LDPC_ALGO_LAYERED), "large"), lay);
    expect_candidates("layered corr", with(base(LDPC_ALGO_LAYERED), "corr"), lay_corr);
    expect_candidates("layered offset", with(base(LDPC_ALGO_LAYERED), "offset"), lay_corr);
    expect_candidates("layered crc", with(base(LDPC_ALGO_LAYERED), "crc"), all_L);
    expect_candidates("layered bits", with(base(LDPC_ALGO_LAYERED), "bits"), all_L);
    const char *const lay_corr_off[9] = {"L", "L", "L", "L", "L", "!", "L", "L", "L"};      // the refusal comes first
    expect_candidates("layered corr bits", with(with(base(LDPC_ALGO_LAYERED), "corr"), "bits"), lay_corr_off);
    expect_candidates("layered corr crc", with(with(base(LDPC_ALGO_LAYERED), "corr"), "crc"), lay_corr_off);

    // flooding: min-sum has the record kernel (with the LDS limit unless forced); the LDS-resident kernel is the automatic
    // choice for small batches only
    const char *const ms[9] = {"RUF", "rUF", "UF", "RUF", "rUF", "UF", "F", "F", "F"};
    const char *const ms_large[9] = {"RF", "rF", "F", "RUF", "rUF", "UF", "F", "F", "F"};
    const char *const ms_corr[9] = {"RF", "rF", "F", "RF", "rF", "!", "F", "F", "F"};
    const char *const sp[9] = {"uF", "uF", "uF", "uF", "uF", "uF", "F", "F", "F"};
    const char *const sp_large[9] = {"F", "F", "F", "uF", "uF", "uF", "F", "F", "F"};
    const char *const ms_corr_off[9] = {"F", "F", "F", "F", "F", "!", "F", "F", "F"};
    expect_candidates("ms", base(LDPC_ALGO_MS), ms);
    expect_candidates("ms edge", with(base(LDPC_ALGO_MS), "edge"), ms);
    expect_candidates("ms large", with(base(LDPC_ALGO_MS), "large"), ms_large);
    expect_candidates("ms corr", with(base(LDPC_ALGO_MS), "corr"), ms_corr);
    expect_candidates("ms corr large", with(with(base(LDPC_ALGO_MS), "corr"), "large"), ms_corr);
    expect_candidates("ms crc", with(base(LDPC_ALGO_MS), "crc"), all_F);
    expect_candidates("ms bits", with(base(LDPC_ALGO_MS), "bits"), all_F);
    expect_candidates("ms corr crc", with(with(base(LDPC_ALGO_MS), "corr"), "crc"), ms_corr_off);
    expect_candidates("ms fp16", base(LDPC_ALGO_MS, LDPC_MSG_F16), all_F);
    expect_candidates("ms fp8", base(LDPC_ALGO_MS, LDPC_MSG_F8), all_F);
    expect_candidates("ms fixed point", base(LDPC_ALGO_MS, LDPC_MSG_I8), all_F);
    ldpc_decoder_config c = base(LDPC_ALGO_MS);
    c.layer_rows = 0;
    expect_candidates("ms without layer_rows", c, all_F);
    c = base(LDPC_ALGO_MS);
    c.frames_per_lane = 2;
    expect_candidates("ms at 2 frames per lane", c, all_F);
    expect_candidates("sp", base(LDPC_ALGO_SP), sp);
    expect_candidates("sp large", with(base(LDPC_ALGO_SP), "large"), sp_large);
    expect_candidates("sp crc", with(base(LDPC_ALGO_SP), "crc"), all_F);
    expect_candidates("sp bits", with(base(LDPC_ALGO_SP), "bits"), all_F);
    expect_candidates("bp", base(LDPC_ALGO_BP), all_F);
    expect_candidates("bp fp16", base(LDPC_ALGO_BP, LDPC_MSG_F16), all_F);
    expect_candidates("bp crc", with(base(LDPC_ALGO_BP), "crc"), all_F);

    expect_candidates("bitflip", base(LDPC_ALGO_BITFLIP), all_B);
    expect_candidates("bitflip crc bits", with(with(base(LDPC_ALGO_BITFLIP), "crc"), "bits"), all_B);
}

static void test_config_check()
{
    char msg[512];
    for (const AlgoInfo &a : kAlgos) {
        if (a.algo == LDPC_ALGO_LAYERED_HOST) continue;        // rows of several weights
        ldpc_decoder_config c = base(a.algo, a.fixed ? LDPC_MSG_I8 : LDPC_MSG_F32);
        EXPECT(config_check(c, facts(), msg, sizeof msg) == LDPC_OK);
    }
    ldpc_decoder_config c = base(LDPC_ALGO_LAYERED_HOST);
    GraphFacts g = facts();
    EXPECT(config_check(c, g, msg, sizeof msg) == LDPC_ERR_UNSUPPORTED && strstr(msg, "same weight"));
    g.rows_one_weight = true;
    EXPECT(config_check(c, g, msg, sizeof msg) == LDPC_OK);
    g.max_row_deg = kCfgUnrolledLayerDegree + 1;
    EXPECT(config_check(c, g, msg, sizeof msg) == LDPC_ERR_UNSUPPORTED && !strcmp(msg, "LAYERED_HOST: row weight 25 > 24"));
    c = base(LDPC_ALGO_MS);
    c.ms_offset = NAN;
    EXPECT(config_check(c, facts(), msg, sizeof msg) == LDPC_ERR_ARG && !strcmp(msg, "ms_offset must be 0 (off) or in (0, 1000)"));
    c = base(LDPC_ALGO_BP);
    c.llr_scale = INFINITY;
    EXPECT(config_check(c, facts(), msg, sizeof msg) == LDPC_ERR_ARG && !strncmp(msg, "LDPC_ALGO_BP: llr_scale", 23));
    c = base(LDPC_ALGO_MS, LDPC_MSG_I8);            // the longest text into a buffer that cannot hold it
    c.algo = LDPC_ALGO_SP;
    char small[16];
    EXPECT(config_check(c, facts(), small, sizeof small) == LDPC_ERR_UNSUPPORTED && strlen(small) == 15);
    EXPECT(positive_finite(1e-30f) && !positive_finite(0.0f) && !positive_finite(-1.0f) && !positive_finite(INFINITY) && !positive_finite(NAN));
}

int main()
{
    test_table();
    test_config_in();
    test_frames_per_lane();
    test_engine_candidates();
    test_config_check();
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("ok\n");
    return 0;
}
