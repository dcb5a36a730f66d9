// Coder with DecodeLayeredFixed and setFixedRecordKernel end to end: decodes the channel values of <in> (frames x N, float32 or int8) with the
// fixed-point layered min-sum under a message type and width, a posterior width, an llr scale and a correction, writes the
// srcLength decoded bytes to <out> and, with a soft kind, the frames x N soft values to <soft out>.
// <devices> > 1: setDevices with ordinal 0 that many times.  <int8 unit> > 0: <in> holds int8 and goes through decodeTyped /
// decodeSoftTyped.
// <record> 1: setFixedRecordKernel(true), the fixed-point record kernel; 0: the streaming layered engine.
// Usage: coder_layered_fx_record <rate 0..5> <N> <frames> <msg dtype> <msg bits> <post bits> <llr scale> <ms scale> <ms offset>
//                                <soft kind 0|1|2> <devices> <int8 unit> <in> <out> <soft out> <record 0|1>
// Exit 0 on success; 3 when addDecodeType refuses (lastError() is printed); 1 on any other failure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "MyLdpc.h"

int main(int argc, char **argv)
{
    if (argc != 17) return 2;
    const enum rate_type rate = (enum rate_type)atoi(argv[1]);
    const int N = atoi(argv[2]), frames = atoi(argv[3]);
    static const int mbs[6] = {12, 8, 8, 6, 6, 4};
    const int K = N - mbs[(int)rate] * (N / 24);
    const int kind = atoi(argv[10]), ndev = atoi(argv[11]);
    const float unit = (float)atof(argv[12]);
    Coder c(K, N, rate);
    if (c.forDecoder(ndev > 1 ? (frames + ndev - 1) / ndev : frames) != LDPC_SUCCESS) { printf("forDecoder: %s\n", c.lastError()); return 1; }
    c.setMaxIterations(20);
    c.setMessageType(atoi(argv[4]), atoi(argv[5]));
    c.setPosteriorBits(atoi(argv[6]));
    c.setFixedRecordKernel(atoi(argv[16]) != 0);
    c.setLlrScale((float)atof(argv[7]));
    c.setMinSumCorrection((float)atof(argv[8]), (float)atof(argv[9]));
    if (ndev > 1) {
        std::vector<int> ord((size_t)ndev, 0);
        c.setDevices(ord.data(), ndev);
    }
    if (c.addDecodeType(DecodeLayeredFixed) != LDPC_SUCCESS) { printf("addDecodeType: %s\n", c.lastError()); return 3; }
    const size_t count = (size_t)frames * N;
    std::vector<float> post(unit > 0 ? 0 : count), soft(count);
    std::vector<int8_t> post8(unit > 0 ? count : 0);
    FILE *f = fopen(argv[13], "rb");
    if (!f) return 1;
    if (unit > 0 ? fread(post8.data(), 1, count, f) != count : fread(post.data(), sizeof(float), count, f) != count) return 1;
    fclose(f);
    const int srcLength = frames * (K / 8);
    std::vector<char> out((size_t)srcLength + 1);
    int rc;
    if (unit > 0)
        rc = kind ? c.decodeSoftTyped(post8.data(), LDPC_LLR_I8, unit, out.data(), srcLength, DecodeLayeredFixed, soft.data(), kind)
                  : c.decodeTyped(post8.data(), LDPC_LLR_I8, unit, out.data(), srcLength, DecodeLayeredFixed);
    else
        rc = kind ? c.decodeSoft(post.data(), out.data(), srcLength, DecodeLayeredFixed, soft.data(), kind)
                  : c.decode(post.data(), out.data(), srcLength, DecodeLayeredFixed);
    if (rc != LDPC_SUCCESS) { printf("decode: %s\n", c.lastError()); return 1; }
    f = fopen(argv[14], "wb");
    if (!f || fwrite(out.data(), 1, (size_t)srcLength, f) != (size_t)srcLength) return 1;
    fclose(f);
    if (kind) {
        f = fopen(argv[15], "wb");
        if (!f || fwrite(soft.data(), sizeof(float), soft.size(), f) != soft.size()) return 1;
        fclose(f);
    }
    printf("ok\n");
    return 0;
}
