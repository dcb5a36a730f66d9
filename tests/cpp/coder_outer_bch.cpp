// Coder::setOuterBch end to end: Coder(1152, 2304, rate_1_2) whose frames carry 1040 payload bits and the 112 parity bits
// of the BCH code with t = 8 over GF(2^14).  srand(1), encode -> test(0.4) -> decode(DecodeTDMPCL) returns the payload bytes
// with every frame clean.  Then the source rows of the code words (the code is systematic) get wrong bits -- three in
// frame 5, eight in frame 9, nine in frame 11 -- and are encoded again by a plain Coder, so that the inner decoder
// delivers exactly those rows: the outer code repairs frames 5 and 9 and reports frame 11 as not decodable.  Refusals of
// the setter, and that it and setTransportBlock exclude one another.
// Prints "refused=<ok|bad> lengths=<ok|bad> ErrNum=<differing payload bytes> clean=<ok|bad> repaired=<ok|bad>"; exit 0 when
// the chain ran.  With an argument it stops after the parts that need no device and prints "refused=<ok|bad> lengths=<ok|bad>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "MyLdpc.h"

int main(int argc, char **)
{
    const int K = 1152, N = 2304, T = 8, k = 1040, frames = 16;
    const int srcLength = frames * (k / 8) - 5;             // a short last frame
    std::vector<char> src((size_t)srcLength), out((size_t)srcLength + 1, 0);
    unsigned s = 2468u;
    for (auto &c : src) { s = s * 1664525u + 1013904223u; c = (char)(s >> 24); }

    // ---- refusals: t out of range, n beyond K, n that is no whole number of bytes, a k that is none
    Coder c(K, N, rate_1_2);
    const int plainFrames = c.getCodeSize(srcLength);
    bool refused = c.setOuterBch(0) != 0 && c.setOuterBch(13) != 0 && c.setOuterBch(T, 1160) != 0 && c.setOuterBch(T, 1148) != 0 &&
                   c.setOuterBch(T, 112) != 0 && c.setOuterBch(T, 0) != 0;
    refused = refused && c.getCodeSize(srcLength) == plainFrames;           // a refused call changes nothing
    refused = refused && c.setOuterBch(12) == 0 && c.setOuterBch(T, 1024) == 0 && c.setOuterBch(T) == 0;
    refused = refused && c.setTransportBlock(1024) == LDPC_ERR_STATE;       // the second of the two calls
    Coder other(K, N, rate_1_2);
    refused = refused && other.setTransportBlock(1128) == 0 && other.setOuterBch(T) == LDPC_ERR_STATE &&
              other.getCodeSize(141 * 3) == 3;
    const bool lengths = plainFrames == (srcLength + K / 8 - 1) / (K / 8) && c.getCodeSize(srcLength) == frames &&
                         c.getCodeSize(frames * (k / 8)) == frames && c.getCodeSize(frames * (k / 8) + 1) == frames + 1 &&
                         c.getPriorCodeLength(srcLength) == frames * (N / 8) && c.getPostCodeLength(srcLength) == frames * N &&
                         c.bchStatus(0) == -2 && c.bchCounts().failed == 0;
    if (argc > 1) {
        printf("refused=%s lengths=%s\n", refused ? "ok" : "bad", lengths ? "ok" : "bad");
        return 0;
    }

    const int priorLength = c.getPriorCodeLength(srcLength);
    std::vector<char> prior((size_t)priorLength);
    std::vector<float> rx((size_t)c.getPostCodeLength(srcLength));
    srand(1);
    if (c.forEncoder() || c.encode(src.data(), prior.data(), srcLength) || c.forDecoder(frames) ||
        c.test(prior.data(), rx.data(), priorLength, 0.4f) || c.addDecodeType(DecodeTDMPCL) ||
        c.decode(rx.data(), out.data(), srcLength, DecodeTDMPCL)) { printf("chain: %s\n", c.lastError()); return 1; }
    if (out[(size_t)srcLength] != 0) { printf("decode wrote behind srcCode\n"); return 1; }
    long err = 0;
    for (int i = 0; i < srcLength; ++i) err += src[i] != out[i];
    bool clean = c.bchCounts().failed == 0 && c.bchCounts().corrected == 0 && c.bchCounts().bits == 0;
    for (int f = 0; f < frames; ++f) clean = clean && c.bchStatus(f) == 0;
    clean = clean && c.bchStatus(frames) == -2 && c.bchStatus(-1) == -2;

    // ---- wrong bits in the source rows, encoded again by a plain Coder
    std::vector<char> rows((size_t)frames * (K / 8)), prior2((size_t)priorLength);
    for (int f = 0; f < frames; ++f) memcpy(&rows[(size_t)f * (K / 8)], &prior[(size_t)f * (N / 8)], K / 8);
    auto flip = [&](int f, int bit) { rows[(size_t)f * (K / 8) + bit / 8] ^= (char)(1 << (bit % 8)); };
    const int three[3] = {0, 519, 1151}, nine[9] = {3, 77, 200, 333, 512, 640, 800, 1039, 1040};
    for (int b : three) flip(5, b);
    for (int i = 0; i < 8; ++i) flip(9, nine[i]);
    for (int b : nine) flip(11, b);
    Coder plain(K, N, rate_1_2);
    if (plain.forEncoder() || plain.encode(rows.data(), prior2.data(), (int)rows.size())) { printf("plain: %s\n", plain.lastError()); return 1; }
    srand(2);
    if (c.test(prior2.data(), rx.data(), priorLength, 0.4f) || c.decode(rx.data(), out.data(), srcLength, DecodeTDMPCL)) {
        printf("decode: %s\n", c.lastError());
        return 1;
    }
    bool repaired = c.bchCounts().failed == 1 && c.bchCounts().corrected == 2 && c.bchCounts().bits == 11;
    for (int f = 0; f < frames; ++f) repaired = repaired && c.bchStatus(f) == (f == 5 ? 3 : f == 9 ? 8 : f == 11 ? -1 : 0);
    for (int i = 0; i < srcLength; ++i)
        if (i / (k / 8) != 11 && src[i] != out[i]) repaired = false;
    // the frame that is not decodable comes back as the inner decoder left it: eight of the nine wrong bits are payload bits
    int wrong = 0;
    for (int i = 11 * (k / 8); i < 12 * (k / 8); ++i) wrong += __builtin_popcount((unsigned char)(src[i] ^ out[i]));
    repaired = repaired && wrong == 8;

    printf("refused=%s lengths=%s ErrNum=%ld clean=%s repaired=%s\n", refused ? "ok" : "bad", lengths ? "ok" : "bad", err,
           clean ? "ok" : "bad", repaired ? "ok" : "bad");
    return 0;
}
