// Coder::decodeSoft end to end: Coder(1152, 2304, rate_1_2) whose frames carry 1128 payload bits, CRC16 and eight zero
// fillers (setTransportBlock) and send E = 1920 of their 2304 code bits (setRateMatch): srand(1), encode -> test(sd) ->
// decode(DecodeMS), then decodeSoft(DecodeMS) with both kinds on the same received values.  Prints
//   "refused=<ok|bad> same=<ok|bad> signs=<disagreements> checked=<n> ext=<ok|bad> crc=<failures plain>/<failures soft>"
// refused:  decodeSoft(DecodeSP) is LDPC_ERR_UNSUPPORTED with lastError() set, a NULL buffer and an unknown kind are
//           LDPC_ERR_ARG;
// same:     payload bytes, crcPassed() and lastIterations() of decodeSoft equal those of decode();
// signs:    finite non-zero posteriors among the first 1128 of each frame's N = 2304 whose sign is not the payload bit,
//           over the frames whose CRC passed (the payload is then the decoder's own first bits);
// ext:      posterior - extrinsic is finite everywhere, and zero exactly on the code bits that were not sent.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "MyLdpc.h"

int main()
{
    const int K = 1152, N = 2304, A = 1128, E = 1920, frames = 64;
    const int srcLength = frames * (A / 8);
    std::vector<char> src((size_t)srcLength), plain((size_t)srcLength, 0), dec((size_t)srcLength, 0), dec2((size_t)srcLength, 0);
    unsigned s = 4242u;
    for (auto &c : src) { s = s * 1664525u + 1013904223u; c = (char)(s >> 24); }

    Coder a(K, N, rate_1_2);
    if (a.setTransportBlock(A) || a.setRateMatch(E, 0)) { printf("set-up: %s\n", a.lastError()); return 1; }
    a.setMaxIterations(20);
    const int priorLength = a.getPriorCodeLength(srcLength);
    std::vector<char> prior((size_t)priorLength);
    std::vector<float> rx((size_t)a.getPostCodeLength(srcLength));
    if ((int)rx.size() != frames * E) { printf("getPostCodeLength\n"); return 1; }
    srand(1);
    if (a.forEncoder() || a.encode(src.data(), prior.data(), srcLength) || a.forDecoder(frames) ||
        a.test(prior.data(), rx.data(), priorLength, 0.62f) || a.addDecodeType(DecodeMS) || a.addDecodeType(DecodeSP) ||
        a.decode(rx.data(), plain.data(), srcLength, DecodeMS)) { printf("plain chain: %s\n", a.lastError()); return 1; }
    const int plainTime = a.lastIterations(), plainFail = a.lastCrcFailures();
    std::vector<char> plainOk((size_t)frames);
    for (int f = 0; f < frames; ++f) plainOk[(size_t)f] = a.crcPassed(f);

    std::vector<float> post((size_t)frames * N, NAN), ext((size_t)frames * N, NAN);
    bool refused = a.decodeSoft(rx.data(), dec.data(), srcLength, DecodeSP, post.data()) == LDPC_ERR_UNSUPPORTED &&
                   strstr(a.lastError(), "DecodeSP") != nullptr;
    refused = refused && a.decodeSoft(rx.data(), dec.data(), srcLength, DecodeMS, nullptr) == LDPC_ERR_ARG;
    refused = refused && a.decodeSoft(rx.data(), dec.data(), srcLength, DecodeMS, post.data(), 3) == LDPC_ERR_ARG;
    for (float v : post) refused = refused && std::isnan(v);          // a refused call wrote nothing

    if (a.decodeSoft(rx.data(), dec.data(), srcLength, DecodeMS, post.data())) { printf("decodeSoft: %s\n", a.lastError()); return 1; }
    bool same = memcmp(dec.data(), plain.data(), (size_t)srcLength) == 0 && a.lastIterations() == plainTime &&
                a.lastCrcFailures() == plainFail;
    long signs = 0, checked = 0;
    for (int f = 0; f < frames; ++f) {
        same = same && a.crcPassed(f) == (bool)plainOk[(size_t)f];
        if (!a.crcPassed(f)) continue;
        for (int n = 0; n < A; ++n) {
            const float p = post[(size_t)f * N + n];
            if (!std::isfinite(p) || p == 0.0f) continue;
            const int bit = ((unsigned char)dec[(size_t)f * (A / 8) + n / 8] >> (n % 8)) & 1;
            ++checked;
            signs += (p < 0.0f) != (bit != 0);
        }
    }
    if (a.decodeSoft(rx.data(), dec2.data(), srcLength, DecodeMS, ext.data(), LDPC_SOFT_EXTRINSIC)) {
        printf("decodeSoft extrinsic: %s\n", a.lastError());
        return 1;
    }
    same = same && memcmp(dec2.data(), plain.data(), (size_t)srcLength) == 0;
    // posterior - extrinsic = the channel value the decoder read, up to the rounding of two fp32 operations: finite
    // everywhere, and exactly zero where nothing was received (erasureLlr = 0: code bits [E, N) were not sent)
    bool extOk = true;
    for (int f = 0; f < frames; ++f)
        for (int n = 0; n < N; ++n) {
            const float p = post[(size_t)f * N + n], x = ext[(size_t)f * N + n];
            extOk = extOk && std::isfinite(p) && std::isfinite(x);
            if (n >= E) extOk = extOk && p == x;
        }
    printf("refused=%s same=%s signs=%ld checked=%ld ext=%s crc=%d/%d\n", refused ? "ok" : "bad", same ? "ok" : "bad", signs, checked,
           extOk ? "ok" : "bad", plainFail, a.lastCrcFailures());
    return 0;
}
