// Coder::setRateMatch end to end: Coder(1152, 2304, rate_1_2) sending E = 1920 of its 2304 code bits per frame from
// buffer position 0 (the last 384 parity bits are not sent), encode -> test(sd = 0.3) -> decode(DecodeMS); a second Coder
// without the setter reports the lengths of the mother code.
// Prints "lengths=<ok|bad> plain=<ok|bad> ErrNum=<differing source bytes>"; exit 0 when the chain ran.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "MyLdpc.h"

int main()
{
    const int K = 1152, N = 2304, E = 1920, frames = 24;
    const int srcLength = frames * (K / 8) - 5;             // a short last frame
    std::vector<char> src((size_t)srcLength), out((size_t)srcLength + 1, 0);
    unsigned s = 12345u;
    for (auto &c : src) { s = s * 1664525u + 1013904223u; c = (char)(s >> 24); }

    Coder plain(K, N, rate_1_2);
    const bool plainOk = plain.getCodeSize(srcLength) == frames && plain.getPriorCodeLength(srcLength) == frames * (N / 8) &&
                         plain.getPostCodeLength(srcLength) == frames * N;

    Coder c(K, N, rate_1_2);
    if (c.setRateMatch(E + 4, 0) == 0 || c.setRateMatch(E, N) == 0 || c.setRateMatch(E, 0, 8, 4, 16) == 0) {
        printf("setRateMatch accepted a bad argument\n");
        return 1;
    }
    const bool untouched = c.getPriorCodeLength(srcLength) == frames * (N / 8);      // refused calls change nothing
    if (c.setRateMatch(E, 0)) { printf("setRateMatch: %s\n", c.lastError()); return 1; }
    const bool lengthsOk = untouched && c.getCodeSize(srcLength) == frames && c.getPriorCodeLength(srcLength) == frames * (E / 8) &&
                           c.getPostCodeLength(srcLength) == frames * E;
    if (c.forEncoder()) { printf("forEncoder: %s\n", c.lastError()); return 1; }
    std::vector<char> prior((size_t)c.getPriorCodeLength(srcLength) + 16, (char)0x5a);
    if (c.encode(src.data(), prior.data(), srcLength)) { printf("encode: %s\n", c.lastError()); return 1; }
    for (size_t i = prior.size() - 16; i < prior.size(); ++i)
        if (prior[i] != (char)0x5a) { printf("encode wrote behind priorCode\n"); return 1; }
    // k0 = 0, nothing punctured: the transmission is the first E bits of every codeword, systematic part first
    long sysDiffer = 0;
    for (int f = 0; f < frames; ++f)
        for (int i = 0; i < K / 8 && f * (K / 8) + i < srcLength; ++i)
            sysDiffer += prior[(size_t)f * (E / 8) + i] != src[(size_t)f * (K / 8) + i];
    if (sysDiffer) { printf("transmitted systematic bytes differ from the source: %ld\n", sysDiffer); return 1; }
    std::vector<float> post((size_t)c.getPostCodeLength(srcLength));
    srand(1);
    if (c.forDecoder(frames) || c.test(prior.data(), post.data(), c.getPriorCodeLength(srcLength), 0.3f) || c.addDecodeType(DecodeMS) ||
        c.decode(post.data(), out.data(), srcLength, DecodeMS)) { printf("decode chain: %s\n", c.lastError()); return 1; }
    long err = 0;
    for (int i = 0; i < srcLength; ++i) err += src[i] != out[i];
    printf("lengths=%s plain=%s ErrNum=%ld\n", lengthsOk ? "ok" : "bad", plainOk ? "ok" : "bad", err);
    return 0;
}
