// Coder with DecodeBitFlip end to end: decodes the channel values of <in> (frames x N, float32 or int8) by hard-decision
// bit flipping and writes the srcLength decoded bytes to <out>.  <offsets>: "-" for the default schedule, else up to 16
// comma-separated round offsets for setBitFlipThresholds.  <int8 unit> > 0: <in> holds int8 and goes through decodeTyped.
// <soft> = 1: asks decodeSoft instead, which must refuse (exit 4 with lastError() printed).
// Usage: coder_bitflip <rate 0..5> <N> <frames> <max iter> <offsets> <int8 unit> <soft 0|1> <in> <out>
// Exit 0 on success; 3 when addDecodeType refuses (lastError() is printed); 4 when decodeSoft refuses; 1 on any other failure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "MyLdpc.h"

int main(int argc, char **argv)
{
    if (argc != 10) return 2;
    const enum rate_type rate = (enum rate_type)atoi(argv[1]);
    const int N = atoi(argv[2]), frames = atoi(argv[3]);
    static const int mbs[6] = {12, 8, 8, 6, 6, 4};
    const int K = N - mbs[(int)rate] * (N / 24);
    const float unit = (float)atof(argv[6]);
    const int soft_kind = atoi(argv[7]);
    Coder c(K, N, rate);
    if (c.forDecoder(frames) != LDPC_SUCCESS) { printf("forDecoder: %s\n", c.lastError()); return 1; }
    c.setMaxIterations(atoi(argv[4]));
    if (strcmp(argv[5], "-")) {
        std::vector<int> offsets;
        for (char *tok = strtok(argv[5], ","); tok; tok = strtok(nullptr, ",")) offsets.push_back(atoi(tok));
        c.setBitFlipThresholds(offsets.data(), (int)offsets.size());
    }
    if (c.addDecodeType(DecodeBitFlip) != LDPC_SUCCESS) { printf("addDecodeType: %s\n", c.lastError()); return 3; }
    const size_t count = (size_t)frames * N;
    std::vector<float> post(unit > 0 ? 0 : count);
    std::vector<int8_t> post8(unit > 0 ? count : 0);
    FILE *f = fopen(argv[8], "rb");
    if (!f) return 1;
    if (unit > 0 ? fread(post8.data(), 1, count, f) != count : fread(post.data(), sizeof(float), count, f) != count) return 1;
    fclose(f);
    const int srcLength = frames * (K / 8);
    std::vector<char> out((size_t)srcLength + 1);
    if (soft_kind) {
        std::vector<float> soft(count);
        std::vector<float> y(count, 1.0f);
        const int rc = c.decodeSoft(unit > 0 ? y.data() : post.data(), out.data(), srcLength, DecodeBitFlip, soft.data(), LDPC_SOFT_POSTERIOR);
        printf("decodeSoft: %d %s\n", rc, c.lastError());
        return rc == LDPC_ERR_UNSUPPORTED ? 4 : 1;
    }
    const int rc = unit > 0 ? c.decodeTyped(post8.data(), LDPC_LLR_I8, unit, out.data(), srcLength, DecodeBitFlip)
                            : c.decode(post.data(), out.data(), srcLength, DecodeBitFlip);
    if (rc != LDPC_SUCCESS) { printf("decode: %s\n", c.lastError()); return 1; }
    f = fopen(argv[9], "wb");
    if (!f || fwrite(out.data(), 1, (size_t)srcLength, f) != (size_t)srcLength) return 1;
    fclose(f);
    printf("ok\n");
    return 0;
}
