// Coder::setModulation end to end: Coder(1152, 2304, rate_1_2) whose test() sends 16-QAM symbols (Qm = 4, interleaved,
// sd = 0.3 per real dimension), encode -> test -> decode(DecodeTDMPCL); a second Coder without the setter, whose test() must
// write exactly the reference's BPSK + gaussian() samples; refusals of setModulation.
// Prints "refused=<ok|bad> plain=<ok|bad> ErrNum=<differing source bytes>"; exit 0 when the chain ran.  With an argument
// it stops after the parts that need no device and prints "refused=<ok|bad> plain=<ok|bad>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "MyLdpc.h"

int main(int argc, char **)
{
    const int K = 1152, N = 2304, frames = 24;
    const int srcLength = frames * (K / 8) - 5;             // a short last frame
    std::vector<char> src((size_t)srcLength), out((size_t)srcLength + 1, 0);
    unsigned s = 12345u;
    for (auto &c : src) { s = s * 1664525u + 1013904223u; c = (char)(s >> 24); }

    // ---- without setModulation: test() is the reference's loop, sample for sample
    Coder plain(K, N, rate_1_2);
    if (plain.forEncoder()) { printf("forEncoder: %s\n", plain.lastError()); return 1; }
    const int priorLength = plain.getPriorCodeLength(srcLength);
    std::vector<char> prior((size_t)priorLength);
    if (plain.encode(src.data(), prior.data(), srcLength)) { printf("encode: %s\n", plain.lastError()); return 1; }
    std::vector<float> post((size_t)plain.getPostCodeLength(srcLength)), want(post.size());
    srand(1);
    if (plain.test(prior.data(), post.data(), priorLength, 0.3f)) { printf("test: %s\n", plain.lastError()); return 1; }
    srand(1);
    for (int c = 0; c < priorLength; ++c)
        for (int b = 0; b < 8; ++b) want[(size_t)c * 8 + b] = (prior[c] & (1 << b)) ? -1.0f : 1.0f;
    for (size_t i = 0; i < want.size(); ++i) want[i] += gaussian(0, 0.3f);
    const bool plainOk = memcmp(post.data(), want.data(), post.size() * sizeof(float)) == 0;

    // ---- refusals: a Qm that does not exist; bits per frame that do not fill whole symbols
    Coder c(K, N, rate_1_2);
    bool refused = c.setModulation(3) != 0 && c.setModulation(0) != 0 && c.setModulation(16) != 0;
    {
        Coder r(K, N, rate_1_2);
        refused = refused && r.setRateMatch(1928, 0) == 0 && r.setModulation(6) != 0 && r.setModulation(8) == 0;   // 1928 = 8 * 241
    }

    if (argc > 1) {
        printf("refused=%s plain=%s\n", refused ? "ok" : "bad", plainOk ? "ok" : "bad");
        return 0;
    }

    // ---- 16-QAM
    if (c.setModulation(4)) { printf("setModulation: %s\n", c.lastError()); return 1; }
    if (c.getPostCodeLength(srcLength) != frames * N || c.getPriorCodeLength(srcLength) != priorLength) {
        printf("setModulation changed a length\n");
        return 1;
    }
    std::vector<float> rx(post.size() + 16, 1234.5f);
    srand(1);
    if (c.forEncoder() || c.encode(src.data(), prior.data(), srcLength) || c.forDecoder(frames) ||
        c.test(prior.data(), rx.data(), priorLength, 0.3f) || c.addDecodeType(DecodeTDMPCL) ||
        c.decode(rx.data(), out.data(), srcLength, DecodeTDMPCL)) { printf("chain: %s\n", c.lastError()); return 1; }
    for (size_t i = post.size(); i < rx.size(); ++i)
        if (rx[i] != 1234.5f) { printf("test wrote behind postCode\n"); return 1; }
    long err = 0, same = 0;
    for (int i = 0; i < srcLength; ++i) err += src[i] != out[i];
    for (size_t i = 0; i < post.size(); ++i) same += rx[i] == post[i];
    if (same > 8) { printf("the 16-QAM samples equal the BPSK ones\n"); return 1; }
    printf("refused=%s plain=%s ErrNum=%ld\n", refused ? "ok" : "bad", plainOk ? "ok" : "bad", err);
    return 0;
}
