// Coder with typed channel values end to end: decodes the elements of <in> (frames x N of int8 or binary16) with DecodeMS
// through decodeTyped, or with a soft kind through decodeSoftTyped, writes the srcLength decoded bytes to <out> and the
// frames x N soft values to <soft out>.
// Usage: coder_typed_input <rate 0..5> <N> <frames> <llr type 1|2> <llr unit> <soft kind 0|1|2> <in> <out> <soft out>
// Exit 0 on success; 1 on any failure (lastError() is printed).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "MyLdpc.h"

int main(int argc, char **argv)
{
    if (argc != 10) return 2;
    const enum rate_type rate = (enum rate_type)atoi(argv[1]);
    const int N = atoi(argv[2]), frames = atoi(argv[3]), type = atoi(argv[4]), kind = atoi(argv[6]);
    const float unit = (float)atof(argv[5]);
    static const int mbs[6] = {12, 8, 8, 6, 6, 4};
    const int K = N - mbs[(int)rate] * (N / 24);
    Coder c(K, N, rate);
    if (c.forDecoder(frames) != LDPC_SUCCESS) { printf("forDecoder: %s\n", c.lastError()); return 1; }
    c.setMaxIterations(20);
    if (c.addDecodeType(DecodeMS) != LDPC_SUCCESS) { printf("addDecodeType: %s\n", c.lastError()); return 1; }
    const size_t esz = type == LDPC_LLR_I8 ? 1 : type == LDPC_LLR_F16 ? 2 : 4;
    std::vector<unsigned char> post((size_t)frames * N * esz);
    std::vector<float> soft((size_t)frames * N);
    FILE *f = fopen(argv[7], "rb");
    if (!f || fread(post.data(), 1, post.size(), f) != post.size()) return 1;
    fclose(f);
    const int srcLength = frames * (K / 8);
    std::vector<char> out((size_t)srcLength + 1);
    const int rc = kind ? c.decodeSoftTyped(post.data(), type, unit, out.data(), srcLength, DecodeMS, soft.data(), kind)
                        : c.decodeTyped(post.data(), type, unit, out.data(), srcLength, DecodeMS);
    if (rc != LDPC_SUCCESS) { printf("decode: %s\n", c.lastError()); return 1; }
    // a float unit other than 1 is refused, and the handle decodes on
    std::vector<float> dummy((size_t)frames * N, 1.0f);
    std::vector<char> out2((size_t)srcLength + 1);
    if (c.decodeTyped(dummy.data(), LDPC_LLR_F32, 0.5f, out2.data(), srcLength, DecodeMS) == LDPC_SUCCESS) { printf("F32 with unit 0.5 was accepted\n"); return 1; }
    if (c.decodeTyped(dummy.data(), LDPC_LLR_F32, 1.0f, out2.data(), srcLength, DecodeMS) != LDPC_SUCCESS) { printf("decode: %s\n", c.lastError()); return 1; }
    f = fopen(argv[8], "wb");
    if (!f || fwrite(out.data(), 1, (size_t)srcLength, f) != (size_t)srcLength) return 1;
    fclose(f);
    if (kind) {
        f = fopen(argv[9], "wb");
        if (!f || fwrite(soft.data(), sizeof(float), soft.size(), f) != soft.size()) return 1;
        fclose(f);
    }
    printf("ok\n");
    return 0;
}
