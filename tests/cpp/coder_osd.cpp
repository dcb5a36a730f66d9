// Coder::setOsd end to end: Coder(288, 576, rate_1_2), 96 frames of random bytes, srand(1), encode -> test(0.78) -> five
// rounds of DecodeMS, once plain and once with setOsd(1), and the same chain through the C ABI (ldpc_decode_soft, then
// ldpc_osd_run) on the graph of hRows() / hCols().  The bytes of decode() with setOsd(1) must equal the chain's; the
// posterior and both byte streams are written to the directory argv[1] names, where tests/coder_osd_harness.py holds them
// against osd_ref.
// Prints "refused=<ok|bad> same=<ok|bad> counts=<ok|bad> before=<wrong frames> after=<wrong frames> processed=<n> flipped=<n>"; exit 0 when the
// chain ran.  With "host" as argv[1] it stops after the parts that need no device and prints "refused=<ok|bad>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "MyLdpc.h"
#include "ldpc_hip.h"

static bool dump(const std::string &path, const void *p, size_t bytes)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, bytes, f) == bytes;
    return fclose(f) == 0 && ok;
}

int main(int argc, char **argv)
{
    const int K = 288, N = 576, frames = 96, rounds = 5;
    const int srcLength = frames * (K / 8);

    // ---- refusals: orders that are not built, the rate matcher, decode types without soft output, a code too large
    bool refused = true;
    {
        Coder c(K, N, rate_1_2);
        refused = refused && c.setOsd(2) == LDPC_ERR_ARG && c.setOsd(-2) == LDPC_ERR_ARG && c.setOsd(-1) == 0;
        refused = refused && c.osdCounts().processed == 0 && c.osdCounts().flipped == 0;
        refused = refused && c.setOsd(1) == 0 && c.setRateMatch(512, 0) == LDPC_ERR_STATE && c.setOsd(-1) == 0 && c.setRateMatch(512, 0) == 0 &&
                  c.setOsd(0) == LDPC_ERR_STATE && c.setOsd(-1) == 0;
        Coder sp(K, N, rate_1_2);
        refused = refused && sp.setOsd(1) == 0 && sp.forDecoder(frames) == 0 && sp.addDecodeType(DecodeSP) == LDPC_ERR_UNSUPPORTED &&
                  strstr(sp.lastError(), "soft output") && sp.addDecodeType(DecodeCPU) == LDPC_ERR_UNSUPPORTED;
        Coder big(1152, 2304, rate_1_2);
        refused = refused && big.setOsd(1) == 0 && big.forDecoder(8) == 0 && big.addDecodeType(DecodeMS) == LDPC_ERR_UNSUPPORTED &&
                  strstr(big.lastError(), "N = 2304") && strstr(big.lastError(), "82944");
    }
    if (argc < 2 || !strcmp(argv[1], "host")) {
        printf("refused=%s\n", refused ? "ok" : "bad");
        return 0;
    }
    const std::string dir = argv[1];

    std::vector<char> src((size_t)srcLength), plainOut((size_t)srcLength), osdOut((size_t)srcLength + 1, 0);
    unsigned s = 13579u;
    for (auto &c : src) { s = s * 1664525u + 1013904223u; c = (char)(s >> 24); }
    Coder plain(K, N, rate_1_2), c(K, N, rate_1_2);
    plain.setMaxIterations(rounds);
    c.setMaxIterations(rounds);
    const int priorLength = c.getPriorCodeLength(srcLength);
    std::vector<char> prior((size_t)priorLength);
    std::vector<float> rx((size_t)c.getPostCodeLength(srcLength));
    srand(1);
    if (c.forEncoder() || c.encode(src.data(), prior.data(), srcLength) || c.test(prior.data(), rx.data(), priorLength, 0.78f)) {
        printf("encode: %s\n", c.lastError());
        return 1;
    }
    if (plain.forDecoder(frames) || plain.addDecodeType(DecodeMS) || plain.decode(rx.data(), plainOut.data(), srcLength, DecodeMS)) {
        printf("plain: %s\n", plain.lastError());
        return 1;
    }
    if (c.setOsd(1) || c.forDecoder(frames) || c.addDecodeType(DecodeMS) || c.decode(rx.data(), osdOut.data(), srcLength, DecodeMS)) {
        printf("osd: %s\n", c.lastError());
        return 1;
    }
    if (osdOut[(size_t)srcLength] != 0) { printf("decode wrote behind srcCode\n"); return 1; }
    refused = refused && c.setOsd(0) == LDPC_ERR_STATE;                     // a decoder exists

    // ---- the same chain through the C ABI
    const std::vector<int> &hr = c.hRows(), &hc = c.hCols();
    std::vector<int32_t> rows(hr.begin(), hr.end()), cols(hc.begin(), hc.end());
    ldpc_graph *g = nullptr;
    ldpc_decoder *d = nullptr;
    ldpc_osd *o = nullptr;
    ldpc_decoder_config cfg;
    ldpc_decoder_config_init(&cfg);
    cfg.K = K; cfg.max_batch = frames; cfg.max_iter = rounds; cfg.early_term = 1; cfg.poll_interval = 4; cfg.pack_mode = LDPC_PACK_BYTES;
    cfg.layer_rows = c.getZ(); cfg.algo = LDPC_ALGO_MS;
    std::vector<uint8_t> decOut((size_t)srcLength), chainOut((size_t)srcLength);
    std::vector<float> post((size_t)frames * N);
    std::vector<int32_t> status((size_t)frames);
    if (ldpc_graph_create(rows.data(), cols.data(), (int64_t)rows.size(), N - K, N, &g) || ldpc_decoder_create(g, &cfg, &d) ||
        ldpc_osd_create(g, K, 32, 0, &o) ||                                 // chunks of 32 frames
        ldpc_decode_soft(d, rx.data(), frames, decOut.data(), srcLength, nullptr, post.data(), (int64_t)post.size(), LDPC_SOFT_POSTERIOR) ||
        ldpc_osd_run(o, post.data(), frames, 1, 256.0f, chainOut.data(), srcLength, nullptr, status.data(), nullptr)) {
        printf("chain: %s\n", ldpc_last_error());
        return 1;
    }
    ldpc_osd_destroy(o);
    ldpc_decoder_destroy(d);
    ldpc_graph_destroy(g);

    const bool same = !memcmp(chainOut.data(), osdOut.data(), (size_t)srcLength) && !memcmp(decOut.data(), plainOut.data(), (size_t)srcLength);
    int before = 0, after = 0, processed = 0, flipped = 0;
    for (int f = 0; f < frames; ++f) {
        before += memcmp(&plainOut[(size_t)f * (K / 8)], &src[(size_t)f * (K / 8)], K / 8) != 0;
        after += memcmp(&osdOut[(size_t)f * (K / 8)], &src[(size_t)f * (K / 8)], K / 8) != 0;
        processed += status[(size_t)f] > 0;
        flipped += status[(size_t)f] == 2;
    }
    const bool counts = c.osdCounts().processed == processed && c.osdCounts().flipped == flipped && plain.osdCounts().processed == 0;
    if (!dump(dir + "/post.f32", post.data(), post.size() * 4) || !dump(dir + "/coder.u8", osdOut.data(), (size_t)srcLength) ||
        !dump(dir + "/chain.u8", chainOut.data(), (size_t)srcLength) || !dump(dir + "/status.i32", status.data(), status.size() * 4)) {
        printf("cannot write to %s\n", dir.c_str());
        return 1;
    }
    printf("refused=%s same=%s counts=%s before=%d after=%d processed=%d flipped=%d\n", refused ? "ok" : "bad", same ? "ok" : "bad",
           counts ? "ok" : "bad", before, after, processed, flipped);
    return 0;
}
