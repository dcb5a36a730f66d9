// Coder::setCrcEarlyStop.  Without an argument, end to end on Coder(1152, 2304, rate_1_2) whose frames carry 1128 payload
// bits, CRC16 and eight zero fillers: srand(1), encode -> test(sd) -> decode(DecodeMS) once without and once with
// setCrcEarlyStop(true) (two Coders, the same received values).  Prints
//   "refused=<ok|bad> same=<ok|bad> Time=<plain> TimeCrc=<with> CrcStops=<n> CrcStopsPlain=<n> CrcFailures=<plain>/<with>"
// same: the payload bytes of every frame whose CRC passed with the early stop equal those without it.
// With the argument "refusals": the parts that need no device only -- the setter before setTransportBlock and with
// crcBits = 0, and addDecodeType on DecodeMSCL and on DecodeTDMP where it follows the host-layered path (rate_5_6, every
// row of one weight); prints "refused=<ok|bad>" and the two reasons.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "MyLdpc.h"

static bool refusals()
{
    const int K = 1152, N = 2304, A = 1128;
    Coder c(K, N, rate_1_2);
    bool ok = c.setCrcEarlyStop(true) == LDPC_ERR_STATE && strstr(c.lastError(), "setTransportBlock") != nullptr;
    ok = ok && c.setCrcEarlyStop(false) == 0;
    ok = ok && c.setTransportBlock(A, 0) == 0 && c.setCrcEarlyStop(true) == LDPC_ERR_ARG && strstr(c.lastError(), "crcBits") != nullptr;
    ok = ok && c.setTransportBlock(A) == 0 && c.setCrcEarlyStop(true) == 0 && c.lastCrcStops() == 0;
    ok = ok && c.forDecoder(8) == 0;
    ok = ok && c.addDecodeType(DecodeMSCL) == LDPC_ERR_UNSUPPORTED;
    const std::string mscl = c.lastError();
    ok = ok && mscl.find("DecodeMSCL") != std::string::npos && mscl.find("setCrcEarlyStop") != std::string::npos;
    // rate 5/6: every row of H has one weight, DecodeTDMP follows the reference's host-layered path
    Coder h(480, 576, rate_5_6);
    ok = ok && h.setTransportBlock(456) == 0 && h.setCrcEarlyStop(true) == 0 && h.forDecoder(8) == 0;
    ok = ok && h.addDecodeType(DecodeTDMP) == LDPC_ERR_UNSUPPORTED;
    const std::string tdmp = h.lastError();
    ok = ok && tdmp.find("DecodeTDMP") != std::string::npos && tdmp.find("setCrcEarlyStop") != std::string::npos;
    printf("refused=%s\n%s\n%s\n", ok ? "ok" : "bad", mscl.c_str(), tdmp.c_str());
    return ok;
}

int main(int argc, char **)
{
    if (argc > 1) return refusals() ? 0 : 1;
    const int K = 1152, N = 2304, A = 1128, frames = 64;
    const int srcLength = frames * (A / 8);
    std::vector<char> src((size_t)srcLength), plain((size_t)srcLength, 0), early((size_t)srcLength, 0);
    unsigned s = 12345u;
    for (auto &c : src) { s = s * 1664525u + 1013904223u; c = (char)(s >> 24); }

    Coder a(K, N, rate_1_2), b(K, N, rate_1_2);
    if (a.setTransportBlock(A) || b.setTransportBlock(A) || b.setCrcEarlyStop(true)) { printf("set-up: %s %s\n", a.lastError(), b.lastError()); return 1; }
    a.setMaxIterations(20);
    b.setMaxIterations(20);
    const int priorLength = a.getPriorCodeLength(srcLength);
    std::vector<char> prior((size_t)priorLength);
    std::vector<float> rx((size_t)a.getPostCodeLength(srcLength));
    srand(1);
    if (a.forEncoder() || a.encode(src.data(), prior.data(), srcLength) || a.forDecoder(frames) ||
        a.test(prior.data(), rx.data(), priorLength, 0.7f) || a.addDecodeType(DecodeMS) ||
        a.decode(rx.data(), plain.data(), srcLength, DecodeMS)) { printf("plain chain: %s\n", a.lastError()); return 1; }
    if (b.forDecoder(frames) || b.addDecodeType(DecodeMS) || b.decode(rx.data(), early.data(), srcLength, DecodeMS)) {
        printf("early-stop chain: %s\n", b.lastError());
        return 1;
    }
    bool same = true;
    for (int f = 0; f < frames; ++f)
        if (b.crcPassed(f) && memcmp(plain.data() + (size_t)f * (A / 8), early.data() + (size_t)f * (A / 8), A / 8) != 0) same = false;
    printf("refused=%s same=%s Time=%d TimeCrc=%d CrcStops=%lld CrcStopsPlain=%lld CrcFailures=%d/%d\n", "ok", same ? "ok" : "bad",
           a.lastIterations(), b.lastIterations(), b.lastCrcStops(), a.lastCrcStops(), a.lastCrcFailures(), b.lastCrcFailures());
    return 0;
}
