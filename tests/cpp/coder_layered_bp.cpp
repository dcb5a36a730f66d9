// Coder with DecodeLayeredBP end to end: decodes the channel floats of <in> (frames x N float32) with the layered
// log-domain sum-product under a message type and an llr scale, writes the srcLength decoded bytes to <out> and, with a
// soft kind, the frames x N soft values to <soft out>.  <devices> > 1: setDevices with ordinal 0 that many times.
// Usage: coder_layered_bp <rate 0..5> <N> <frames> <msg dtype 0..> <llr scale> <ms scale> <ms offset> <soft kind 0|1|2>
//                         <devices> <in> <out> <soft out>
// Exit 0 on success; 3 when addDecodeType refuses (lastError() is printed); 1 on any other failure.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "MyLdpc.h"

int main(int argc, char **argv)
{
    if (argc != 13) return 2;
    const enum rate_type rate = (enum rate_type)atoi(argv[1]);
    const int N = atoi(argv[2]), frames = atoi(argv[3]);
    static const int mbs[6] = {12, 8, 8, 6, 6, 4};
    const int K = N - mbs[(int)rate] * (N / 24);
    const int kind = atoi(argv[8]), ndev = atoi(argv[9]);
    Coder c(K, N, rate);
    // several devices: each takes a contiguous range of the stream, batchSize frames per launch group
    if (c.forDecoder(ndev > 1 ? (frames + ndev - 1) / ndev : frames) != LDPC_SUCCESS) { printf("forDecoder: %s\n", c.lastError()); return 1; }
    c.setMaxIterations(20);
    c.setMessageType(atoi(argv[4]));
    c.setLlrScale((float)atof(argv[5]));
    c.setMinSumCorrection((float)atof(argv[6]), (float)atof(argv[7]));
    if (ndev > 1) {
        std::vector<int> ord((size_t)ndev, 0);
        c.setDevices(ord.data(), ndev);
    }
    if (c.addDecodeType(DecodeLayeredBP) != LDPC_SUCCESS) { printf("addDecodeType: %s\n", c.lastError()); return 3; }
    std::vector<float> post((size_t)frames * N), soft((size_t)frames * N);
    FILE *f = fopen(argv[10], "rb");
    if (!f || fread(post.data(), sizeof(float), post.size(), f) != post.size()) return 1;
    fclose(f);
    const int srcLength = frames * (K / 8);
    std::vector<char> out((size_t)srcLength + 1);
    const int rc = kind ? c.decodeSoft(post.data(), out.data(), srcLength, DecodeLayeredBP, soft.data(), kind)
                        : c.decode(post.data(), out.data(), srcLength, DecodeLayeredBP);
    if (rc != LDPC_SUCCESS) { printf("decode: %s\n", c.lastError()); return 1; }
    f = fopen(argv[11], "wb");
    if (!f || fwrite(out.data(), 1, (size_t)srcLength, f) != (size_t)srcLength) return 1;
    fclose(f);
    if (kind) {
        f = fopen(argv[12], "wb");
        if (!f || fwrite(soft.data(), sizeof(float), soft.size(), f) != soft.size()) return 1;
        fclose(f);
    }
    printf("ok\n");
    return 0;
}
