// Coder::setEncodeOnDevice end to end.
// Usage: coder_device_encode compare <rate 0..5> <N> <srcBytes>
//            encode() of a pseudo-random payload with the device path and with the host path; exit 0 when the two
//            priorCode buffers are equal byte for byte.  Prints "host=<rc> device=<rc> frames=<n> differ=<bytes>".
//        coder_device_encode roundtrip <rate 0..5> <N> <frames> <sd>
//            device-path encode -> Coder::test at standard deviation <sd> -> decode(DecodeMS); also reports what the host
//            path's forEncoder() answers.  Prints "hostForEncoder=<rc> ParityFail=<n> ErrNum=<n>"; exit 0 when the
//            device path ran (the caller judges the numbers).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "MyLdpc.h"

static const int kMb[6] = {12, 8, 8, 6, 6, 4};

static void payload(std::vector<char> &v)
{
    unsigned s = 12345u;
    for (auto &c : v) { s = s * 1664525u + 1013904223u; c = (char)(s >> 24); }
}

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const enum rate_type rate = (enum rate_type)atoi(argv[2]);
    const int N = atoi(argv[3]);
    const int K = N - kMb[(int)rate] * (N / 24);
    if (!strcmp(argv[1], "compare")) {
        const int srcLength = atoi(argv[4]);
        std::vector<char> src((size_t)srcLength);
        payload(src);
        Coder host(K, N, rate), dev(K, N, rate);
        dev.setEncodeOnDevice(true);
        const int prior = host.getPriorCodeLength(srcLength);
        std::vector<char> a((size_t)prior, 0x55), b((size_t)prior, 0x55);
        int rh = host.forEncoder();
        if (!rh) rh = host.encode(src.data(), a.data(), srcLength);
        int rd = dev.forEncoder();
        if (!rd) rd = dev.encode(src.data(), b.data(), srcLength);
        if (rh) printf("host: %s\n", host.lastError());
        if (rd) printf("device: %s\n", dev.lastError());
        long differ = 0;
        for (int i = 0; i < prior; ++i) differ += a[i] != b[i];
        printf("host=%d device=%d bytes=%d differ=%ld\n", rh, rd, prior, differ);
        return (rh || rd || differ) ? 1 : 0;
    }
    if (!strcmp(argv[1], "roundtrip") && argc >= 6) {
        const int frames = atoi(argv[4]);
        const float sd = (float)atof(argv[5]);
        const int srcLength = frames * (K / 8);
        std::vector<char> src((size_t)srcLength), out((size_t)srcLength + 1, 0);
        payload(src);
        Coder host(K, N, rate);
        const int rh = host.forEncoder();
        Coder c(K, N, rate);
        c.setEncodeOnDevice(true);
        if (c.forEncoder()) { printf("forEncoder: %s\n", c.lastError()); return 1; }
        std::vector<char> prior((size_t)c.getPriorCodeLength(srcLength));
        if (c.encode(src.data(), prior.data(), srcLength)) { printf("encode: %s\n", c.lastError()); return 1; }
        long bad = 0;
        const std::vector<int> &rr = c.hRowRange(), &cc = c.hCols();
        for (int f = 0; f < frames; ++f) {
            const unsigned char *cw = (const unsigned char *)prior.data() + (size_t)f * (N / 8);
            for (size_t m = 0; m + 1 < rr.size(); ++m) {
                int par = 0;
                for (int p = rr[m]; p < rr[m + 1]; ++p) par ^= (cw[cc[p] / 8] >> (cc[p] % 8)) & 1;
                bad += par;
            }
            if (memcmp(cw, src.data() + (size_t)f * (K / 8), (size_t)(K / 8))) ++bad;
        }
        std::vector<float> post((size_t)c.getPostCodeLength(srcLength));
        srand(1);
        if (c.forDecoder(frames) || c.test(prior.data(), post.data(), (int)prior.size(), sd) || c.addDecodeType(DecodeMS) ||
            c.decode(post.data(), out.data(), srcLength, DecodeMS)) { printf("decode chain: %s\n", c.lastError()); return 1; }
        long err = 0;
        for (int i = 0; i < srcLength; ++i) err += src[i] != out[i];
        printf("hostForEncoder=%d ParityFail=%ld ErrNum=%ld\n", rh, bad, err);
        return 0;
    }
    return 2;
}
