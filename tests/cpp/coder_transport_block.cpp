// Coder::setTransportBlock end to end: Coder(1152, 2304, rate_1_2) whose frames carry 1128 payload bits, CRC16 and eight
// zero fillers; srand(1), encode -> test(0.4) -> decode(DecodeTDMPCL) returns the payload bytes with every CRC passing; the
// same received values with frame 7 replaced by noise make exactly that frame fail its CRC; refusals of the setter.
// Prints "refused=<ok|bad> lengths=<ok|bad> ErrNum=<differing payload bytes> CrcFailures=<n> noisy=<ok|bad>"; exit 0 when the
// chain ran.  With an argument it stops after the parts that need no device and prints "refused=<ok|bad> lengths=<ok|bad>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "MyLdpc.h"

int main(int argc, char **)
{
    const int K = 1152, N = 2304, A = 1128, frames = 24, noisy = 7;
    const int srcLength = frames * (A / 8) - 5;             // a short last frame
    std::vector<char> src((size_t)srcLength), out((size_t)srcLength + 1, 0);
    unsigned s = 12345u;
    for (auto &c : src) { s = s * 1664525u + 1013904223u; c = (char)(s >> 24); }

    // ---- refusals: payload + CRC beyond K, a payload that is no whole number of bytes, a CRC length that does not exist
    Coder c(K, N, rate_1_2);
    const int plainFrames = c.getCodeSize(srcLength);
    bool refused = c.setTransportBlock(1160) != 0 && c.setTransportBlock(1124) != 0 && c.setTransportBlock(1128, 8) != 0 &&
                   c.setTransportBlock(1136, 24) != 0 && c.setTransportBlock(0) != 0;
    refused = refused && c.getCodeSize(srcLength) == plainFrames;           // a refused call changes nothing
    refused = refused && c.setTransportBlock(1128, 24) == 0 && c.setTransportBlock(1152, 0) == 0 && c.setTransportBlock(A) == 0;
    const bool lengths = plainFrames == (srcLength + K / 8 - 1) / (K / 8) && c.getCodeSize(srcLength) == frames &&
                         c.getCodeSize(frames * (A / 8)) == frames && c.getCodeSize(frames * (A / 8) + 1) == frames + 1 &&
                         c.getPriorCodeLength(srcLength) == frames * (N / 8) && c.getPostCodeLength(srcLength) == frames * N &&
                         c.lastCrcFailures() == 0 && !c.crcPassed(0);
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
    const int failures = c.lastCrcFailures();
    bool allPassed = true;
    for (int f = 0; f < frames; ++f) allPassed = allPassed && c.crcPassed(f);
    allPassed = allPassed && !c.crcPassed(frames) && !c.crcPassed(-1);

    // ---- one frame of noise
    for (int i = 0; i < N; ++i) rx[(size_t)noisy * N + i] = gaussian(0, 1.0f);
    if (c.decode(rx.data(), out.data(), srcLength, DecodeTDMPCL)) { printf("decode: %s\n", c.lastError()); return 1; }
    bool noisyOk = c.lastCrcFailures() == 1;
    for (int f = 0; f < frames; ++f) noisyOk = noisyOk && c.crcPassed(f) == (f != noisy);
    for (int i = 0; i < srcLength; ++i)
        if (i / (A / 8) != noisy && src[i] != out[i]) noisyOk = false;

    printf("refused=%s lengths=%s ErrNum=%ld CrcFailures=%d noisy=%s\n", refused ? "ok" : "bad", lengths ? "ok" : "bad", err,
           failures + (allPassed ? 0 : 1000), noisyOk ? "ok" : "bad");
    return 0;
}
