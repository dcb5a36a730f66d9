// Coder::setMessageType(LDPC_MSG_I8, bits) end to end: decodes the channel floats of <in> (frames x N float32) with one
// decode type under fixed-point messages of <bits> bits, llr scale <llr scale> (the LSBs per unit of channel value) and an
// optional min-sum correction, and writes the srcLength decoded bytes to <out>.
// Usage: coder_fixed <rate 0..5> <N> <frames> <MS|CPU|SP|TDMPCL|MSCL> <msg dtype> <bits> <llr scale> <scale> <offset> <in> <out>
// Exit 0 on success; 3 when addDecodeType (DecodeCPU: the first decode) refuses (lastError() is printed); 1 on any other failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "MyLdpc.h"

int main(int argc, char **argv)
{
    if (argc != 12) return 2;
    const enum rate_type rate = (enum rate_type)atoi(argv[1]);
    const int N = atoi(argv[2]), frames = atoi(argv[3]);
    static const int mbs[6] = {12, 8, 8, 6, 6, 4};
    const int K = N - mbs[(int)rate] * (N / 24);
    const char *mode = argv[4];
    const enum decodeType t = !strcmp(mode, "MS") ? DecodeMS : !strcmp(mode, "CPU") ? DecodeCPU : !strcmp(mode, "SP") ? DecodeSP
                              : !strcmp(mode, "TDMPCL") ? DecodeTDMPCL : DecodeMSCL;
    Coder c(K, N, rate);
    if (c.forDecoder(frames) != LDPC_SUCCESS) { printf("forDecoder: %s\n", c.lastError()); return 1; }
    c.setMaxIterations(20);
    c.setMessageType(atoi(argv[5]), atoi(argv[6]));
    c.setLlrScale((float)atof(argv[7]));
    c.setMinSumCorrection((float)atof(argv[8]), (float)atof(argv[9]));
    if (c.addDecodeType(t) != LDPC_SUCCESS) { printf("addDecodeType: %s\n", c.lastError()); return 3; }
    std::vector<float> post((size_t)frames * N);
    FILE *f = fopen(argv[10], "rb");
    if (!f || fread(post.data(), sizeof(float), post.size(), f) != post.size()) return 1;
    fclose(f);
    const int srcLength = frames * (K / 8);
    std::vector<char> out((size_t)srcLength + 1);
    if (c.decode(post.data(), out.data(), srcLength, t) != LDPC_SUCCESS) { printf("decode: %s\n", c.lastError()); return t == DecodeCPU ? 3 : 1; }
    f = fopen(argv[11], "wb");
    if (!f || fwrite(out.data(), 1, (size_t)srcLength, f) != (size_t)srcLength) return 1;
    fclose(f);
    printf("ok\n");
    return 0;
}
