/*
 * MyLdpc.cpp -- class Coder of wing02/MyLdpcCppApi re-created above the MI355X
 * C ABI (include/ldpc_hip.h).  Host-side C++ only: every decode runs in the HIP
 * kernels of libldpc_hip.so.  Reference lines are cited per method.
 */
#include "../../include/MyLdpc.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "wimax_seeds.h"

namespace {
const int kSeedCols = WIMAX_NB;
}

int Coder::fail(int code, const std::string &msg)
{
    err = msg;
    return code ? code : LDPC_FAIL;
}

/* MyLdpc.cpp:20-29 */
Coder::Coder(int ldpcK, int ldpcN, enum rate_type rate)
    : times(40), llrScale(8.0f), device(0), hSeed(nullptr), seedRowLength(0), ldpcK(ldpcK),
      ldpcN(ldpcN), ldpcM(ldpcN - ldpcK), z(0), nonZeros(0), batchSize(0), rate(rate),
      isEncoder(false), isDecoder(false), lastTime(0), encX(-1), structured(false), graph(nullptr),
      cpuDecoderBatch(0)
{
    initCheckMatrix();
}

Coder::~Coder()
{
    for (auto &kv : decoders) ldpc_decoder_destroy(kv.second);
    if (osd) ldpc_osd_destroy(osd);
    if (encoder) ldpc_encoder_destroy(encoder);
    if (graph) ldpc_graph_destroy(graph);
}

/* MyLdpc.cpp:52-135.  The triplet list + Eigen setFromTriplets become a direct
 * row-major listing: within a row the blocks come in ascending block column. */
int Coder::initCheckMatrix()
{
    z = ldpcN / n_b;                                        /* :55 */
    const int r = (int)rate;
    if (r < 0 || r >= WIMAX_NUM_RATES || z <= 0 || z * n_b != ldpcN)
        return fail(LDPC_ERR_ARG, "Coder: N must be a positive multiple of 24 and rate one of the six seeds");
    hSeed = wimax_seed_table[r];
    seedRowLength = wimax_seed_rows[r];                     /* :58-83 */
    if (ldpcM != seedRowLength * z)
        return fail(LDPC_ERR_ARG, "Coder: N-K does not match the rate's seed matrix");
    shift.assign((size_t)seedRowLength * kSeedCols, -1);
    for (int i = 0; i < seedRowLength * kSeedCols; ++i) {
        int p = hSeed[i];
        if (p >= 0) shift[i] = (rate != rate_2_3_a) ? p * z / WIMAX_Z0 : p % z;   /* :89-94 */
    }
    rows.clear(); cols.clear();
    rowRange.assign((size_t)ldpcM + 1, 0);
    for (int sr = 0; sr < seedRowLength; ++sr)
        for (int pr = 0; pr < z; ++pr) {
            rowRange[(size_t)sr * z + pr] = (int)rows.size();
            for (int sc = 0; sc < kSeedCols; ++sc) {
                const int p = shift[(size_t)sr * kSeedCols + sc];
                if (p < 0) continue;
                rows.push_back(sr * z + pr);                /* (z + c - r) % z == p, :97 */
                cols.push_back(sc * z + (pr + p) % z);
            }
        }
    rowRange[ldpcM] = (int)rows.size();
    nonZeros = (int)rows.size();                            /* :109 */
    return LDPC_SUCCESS;
}

/* Length helpers, MyLdpc.cpp:620-631; with setRateMatch(): E transmitted bits per frame take the place of the N code bits. */
int Coder::getPriorCodeLength(int srcLength) { return getCodeSize(srcLength) * ((rmE ? rmE : ldpcN) / 8); }
int Coder::getPostCodeLength(int srcLength) { return getCodeSize(srcLength) * (rmE ? rmE : ldpcN); }
/* with setTransportBlock() or setOuterBch(): srcLength counts payload bytes, A / 8 or k / 8 per frame */
int Coder::getCodeSize(int srcLength)
{
    const int per = tbSpec.A ? tbSpec.A / 8 : bchK / 8;
    return per ? (srcLength + per - 1) / per : frameCount(srcLength);
}

/* ----------------------------------------------------------------- encoder */

/* forEncoder, MyLdpc.cpp:137-165.  The reference inverts dense (M-z)^2 int
 * matrices (Richardson-Urbanke with gap z), which cannot scale past a few
 * thousand bits.  A systematic codeword is unique once H's parity part is
 * nonsingular, so any exact solver of H [s p]^T = 0 gives the same bytes.  The
 * 802.16e seeds have a weight-3 parity block column (rows 0, x, mb-1; equal
 * outer shifts, middle shift 0) followed by a dual diagonal, which solves in
 * O(E): p1 = sum of all block rows of A s, then forward substitution. */
void Coder::setEncodeOnDevice(bool on) { encodeOnDevice = on; }

/* Rate matching (the "rate matching" section of ldpc_hip.h) around encode() and decode(): host buffers through
 * ldpc_rate_match / ldpc_rate_recover; the fast path is the device chain of the C ABI. */
int Coder::setRateMatch(int E, int k0, int punctured, int fillerLo, int fillerHi, float erasureLlr)
{
    if (osdOrder >= 0) return fail(LDPC_ERR_STATE, "setRateMatch: setOsd() is in force: the two are not combined");
    ldpc_rate_spec spec;
    ldpc_rate_spec_init(&spec, ldpcN);
    spec.punctured = punctured;
    spec.filler_lo = fillerLo;
    spec.filler_hi = fillerHi;
    spec.erasure_llr = erasureLlr;
    int32_t Ncb = 0, L = 0;
    if (int rc = ldpc_rate_lengths(&spec, &Ncb, &L)) return fail(rc, ldpc_last_error());
    if (E < 8 || E % 8) return fail(LDPC_ERR_ARG, "setRateMatch: E must be a positive multiple of 8 (encode() writes whole bytes)");
    if (k0 < 0 || k0 >= Ncb) return fail(LDPC_ERR_ARG, "setRateMatch: k0 outside the circular buffer [0, N - punctured)");
    rmSpec = spec;
    rmE = E;
    rmK0 = k0;
    return LDPC_SUCCESS;
}

/* Modulation of test() (the "modem" section of ldpc_hip.h) */
int Coder::setModulation(int Qm, bool interleave)
{
    ldpc_modem_spec spec;
    ldpc_modem_spec_init(&spec, Qm);
    spec.interleave = interleave ? 1 : 0;
    const int bits = rmE ? rmE : ldpcN;
    if (ldpc_modem_symbol_floats(&spec, bits) == 0) return fail(LDPC_ERR_ARG, std::string("setModulation: ") + ldpc_last_error());
    modSpec = spec;
    return LDPC_SUCCESS;
}

/* Transport blocks of one code block each (the "transport block" section of ldpc_hip.h) around encode() and decode() */
int Coder::setTransportBlock(int payloadBits, int crcBits)
{
    ldpc_tb_spec spec;
    ldpc_tb_spec_init(&spec, payloadBits, ldpcK);
    if (crcBits >= 0) spec.tb_crc = crcBits;
    spec.C = 1;
    spec.cb_crc = 0;
    int32_t lay[6];
    if (bchK) return fail(LDPC_ERR_STATE, "setTransportBlock: setOuterBch() is in force: a frame carries one of the two");
    if (int rc = ldpc_tb_layout(&spec, lay)) return fail(rc, std::string("setTransportBlock: ") + ldpc_last_error());
    tbSpec = spec;
    crcOk.clear();
    crcFailures = 0;
    return LDPC_SUCCESS;
}

/* The outer BCH code (the "outer code" section of ldpc_hip.h) around encode() and decode(): n code bits in front of zero
 * fillers up to K */
int Coder::setOuterBch(int t, int n)
{
    if (tbSpec.A) return fail(LDPC_ERR_STATE, "setOuterBch: setTransportBlock() is in force: a frame carries one of the two");
    if (ldpcK % 8) return fail(LDPC_ERR_ARG, "setOuterBch: K must be a multiple of 8 (rows of K / 8 bytes)");
    ldpc_bch_spec spec;
    ldpc_bch_spec_init(&spec, n < 0 ? ldpcK : n, t, ldpcK / 8);
    int32_t lay[4];
    if (int rc = ldpc_bch_layout(&spec, lay)) return fail(rc, std::string("setOuterBch: ") + ldpc_last_error());
    bchSpec = spec;
    bchK = lay[0];
    bchStatusOfFrame.clear();
    bchFailed = bchCorrected = bchBits = 0;
    return LDPC_SUCCESS;
}

/* Ordered-statistics post-processing (the section of that name in ldpc_hip.h) behind the decoders addDecodeType makes
 * from here on */
int Coder::setOsd(int order)
{
    if (order < -1 || order > 1) return fail(LDPC_ERR_ARG, "setOsd: order must be -1 (off), 0 or 1");
    if (order >= 0 && rmE) return fail(LDPC_ERR_STATE, "setOsd: setRateMatch() is in force: the two are not combined");
    if (order >= 0 && ldpcK % 8) return fail(LDPC_ERR_ARG, "setOsd: K must be a multiple of 8 (rows of K / 8 bytes)");
    if (!decoders.empty()) return fail(LDPC_ERR_STATE, "setOsd: call it before addDecodeType()");
    osdOrder = order;
    osdProcessed = osdFlipped = 0;
    return LDPC_SUCCESS;
}

/* CRC-aided early termination of the decoders addDecodeType makes from here on */
int Coder::setCrcEarlyStop(bool on)
{
    if (!on) { crcEarlyStop = false; return LDPC_SUCCESS; }
    if (!tbSpec.A) return fail(LDPC_ERR_STATE, "setCrcEarlyStop: call setTransportBlock() first: without it the frames carry no CRC");
    int32_t kind = 0, bits = 0;
    if (int rc = ldpc_tb_frame_crc(&tbSpec, &kind, &bits)) return fail(rc, std::string("setCrcEarlyStop: setTransportBlock() with crcBits = 0: ") + ldpc_last_error());
    crcEarlyStop = true;
    return LDPC_SUCCESS;
}

/* the two config fields of a decoder made while setCrcEarlyStop is on */
int Coder::applyCrcEarlyStop(ldpc_decoder_config &cfg)
{
    if (!crcEarlyStop) return LDPC_SUCCESS;
    int32_t kind = 0, bits = 0;
    if (int rc = ldpc_tb_frame_crc(&tbSpec, &kind, &bits)) return fail(rc, std::string("setCrcEarlyStop: ") + ldpc_last_error());
    cfg.crc_kind = kind;
    cfg.crc_bits = bits;
    return LDPC_SUCCESS;
}

int Coder::makeGraph()
{
    if (graph) return LDPC_SUCCESS;
    int rc = ldpc_graph_create(rows.data(), cols.data(), nonZeros, ldpcM, ldpcN, &graph);
    return rc ? fail(rc, ldpc_last_error()) : LDPC_SUCCESS;
}

int Coder::forEncoder()
{
    if (!hSeed) return fail(LDPC_ERR_STATE, "Coder was not constructed");
    if (encodeOnDevice) {
        /* the device encoder recognises the parity structure from the graph (any middle shift of the weight-3
         * column): no host precompute.  4096 frames per launch group */
        if (int rc = makeGraph()) return rc;
        if (!encoder) {
            int rc = ldpc_encoder_create(graph, ldpcK, z, 4096, device, &encoder);
            if (rc) return fail(rc, ldpc_last_error());
        }
        isEncoder = true;
        return LDPC_SUCCESS;
    }
    const int mb = seedRowLength, kb = kSeedCols - mb;
    structured = true;
    encX = -1;
    int cnt = 0;
    for (int i = 0; i < mb; ++i) {
        const int p = shift[(size_t)i * kSeedCols + kb];
        if (p < 0) continue;
        ++cnt;
        if (i != 0 && i != mb - 1) { if (p != 0 || encX >= 0) structured = false; encX = i; }
    }
    if (cnt != 3 || encX < 0 || shift[kb] < 0 || shift[(size_t)(mb - 1) * kSeedCols + kb] != shift[kb])
        structured = false;
    for (int j = 0; j < mb - 1 && structured; ++j)
        for (int i = 0; i < mb; ++i) {
            const int p = shift[(size_t)i * kSeedCols + kb + 1 + j];
            const bool want = (i == j || i == j + 1);
            if (want ? (p != 0) : (p >= 0)) { structured = false; break; }
        }
    if (!structured) {
        /* generic fallback: bit-packed Gauss-Jordan inverse of the M x M parity part */
        const int M = ldpcM;
        if (M > 8192) return fail(LDPC_ERR_UNSUPPORTED, "forEncoder: unstructured parity part too large");
        const size_t W = ((size_t)2 * M + 63) / 64;
        std::vector<unsigned long long> a((size_t)M * W, 0ull);
        for (int e = 0; e < nonZeros; ++e)
            if (cols[e] >= ldpcK) {
                const int c = cols[e] - ldpcK;
                a[(size_t)rows[e] * W + c / 64] |= 1ull << (c % 64);
            }
        for (int i = 0; i < M; ++i) a[(size_t)i * W + (M + i) / 64] |= 1ull << ((M + i) % 64);
        for (int c = 0; c < M; ++c) {
            int piv = -1;
            for (int r2 = c; r2 < M; ++r2)
                if (a[(size_t)r2 * W + c / 64] >> (c % 64) & 1ull) { piv = r2; break; }
            if (piv < 0) return fail(LDPC_ERR_UNSUPPORTED, "forEncoder: parity part of H is singular");
            if (piv != c)
                for (size_t w = 0; w < W; ++w) std::swap(a[(size_t)piv * W + w], a[(size_t)c * W + w]);
            for (int r2 = 0; r2 < M; ++r2)
                if (r2 != c && (a[(size_t)r2 * W + c / 64] >> (c % 64) & 1ull))
                    for (size_t w = 0; w < W; ++w) a[(size_t)r2 * W + w] ^= a[(size_t)c * W + w];
        }
        denseInv.assign((size_t)M * M, 0);
        for (int i = 0; i < M; ++i)
            for (int j = 0; j < M; ++j)
                denseInv[(size_t)i * M + j] = (unsigned char)(a[(size_t)i * W + (M + j) / 64] >> ((M + j) % 64) & 1ull);
    }
    isEncoder = true;
    return LDPC_SUCCESS;
}

/* encode, MyLdpc.cpp:554-569, index for index: frame f reads srcCode + f*K/8 (integer division
 * of the PRODUCT, as the decoders write frame f at (f*K)/8, decodeCL.c:191-192) and writes
 * priorCode + f*N/8; the last frame may be short (zero-padded, :639-650).  For K % 8 != 0 --
 * e.g. Coder(324, 648, rate_1_2) -- frames therefore start at bytes 0, 40, 81, 121, ...: every
 * other frame skips one source byte, exactly as in the reference. */
int Coder::encode(char *srcCode, char *priorCode, int srcLength)
{
    if (!isEncoder) return fail(LDPC_ERR_STATE, "encode: call forEncoder() first");
    if (!srcCode || !priorCode || srcLength <= 0) return fail(LDPC_ERR_ARG, "encode: bad arguments");
    if (bchK) {
        /* payload (the last frame zero-padded) -> K / 8 source bytes per frame: payload, parity, zero fillers */
        const int frames = getCodeSize(srcLength);
        std::vector<char> payload((size_t)frames * (bchK / 8), 0), source((size_t)frames * (ldpcK / 8));
        memcpy(payload.data(), srcCode, (size_t)srcLength);
        if (int rc = ldpc_bch_encode(&bchSpec, (const uint8_t *)payload.data(), frames, (uint8_t *)source.data(), (int64_t)source.size(), device))
            return fail(rc, ldpc_last_error());
        return encodeSource(source.data(), priorCode, (int)source.size());
    }
    if (!tbSpec.A) return encodeSource(srcCode, priorCode, srcLength);
    /* payload (the last frame zero-padded) -> K / 8 source bytes per frame: payload, CRC, zero fillers */
    const int frames = getCodeSize(srcLength);
    std::vector<char> payload((size_t)frames * (tbSpec.A / 8), 0), source((size_t)frames * (ldpcK / 8));
    memcpy(payload.data(), srcCode, (size_t)srcLength);
    if (int rc = ldpc_tb_attach(&tbSpec, (const uint8_t *)payload.data(), frames, (uint8_t *)source.data(), (int64_t)source.size(), device))
        return fail(rc, ldpc_last_error());
    return encodeSource(source.data(), priorCode, (int)source.size());
}

/* srcLength bytes of K / 8 per frame */
int Coder::encodeSource(char *srcCode, char *priorCode, int srcLength)
{
    if (!rmE) return encodeFrames(srcCode, priorCode, srcLength);
    /* the mother codewords go to a buffer of their own, the caller receives E / 8 bytes per frame */
    const int frames = frameCount(srcLength);
    std::vector<char> mother((size_t)frames * (ldpcN / 8));
    if (int rc = encodeFrames(srcCode, mother.data(), srcLength)) return rc;
    const int rc = ldpc_rate_match(&rmSpec, (const uint8_t *)mother.data(), LDPC_CODE_PACKED, frames, rmK0, rmE,
                                   (uint8_t *)priorCode, (int64_t)frames * (rmE / 8), LDPC_CODE_PACKED, device);
    return rc ? fail(rc, ldpc_last_error()) : LDPC_SUCCESS;
}

/* whole codewords: N / 8 bytes per frame */
int Coder::encodeFrames(char *srcCode, char *priorCode, int srcLength)
{
    if (encodeOnDevice && encoder) {
        int rc = ldpc_encode(encoder, (const uint8_t *)srcCode, srcLength, (uint8_t *)priorCode, (int64_t)frameCount(srcLength) * (ldpcN / 8));
        return rc ? fail(rc, ldpc_last_error()) : LDPC_SUCCESS;
    }
    /* frames [0, last]: frame `offset` starts at byte offset*K/8 and is the last one once (offset+1)*K/8 >= srcLength
     * (:557-565).  The frames are independent and encodeOnce only reads the object: large payloads are spread over host
     * threads, contiguous frame ranges each (4096 frames of the (64800, 32400) code: 41 ms on one core). */
    long long last = 0;
    while ((last + 1) * (long long)ldpcK / 8 < srcLength) ++last;
    auto one = [&](long long offset) {
        const int at = (int)(offset * ldpcK / 8);
        encodeOnce(&srcCode[at], &priorCode[offset * ldpcN / 8], offset < last ? ldpcK / 8 : srcLength - at);
    };
    const long long frames = last + 1;
    const unsigned hw = std::thread::hardware_concurrency();
    const long long threads = std::min<long long>(std::min<long long>(hw ? hw : 1, 16), frames * (long long)ldpcN / (1 << 21));
    if (threads <= 1) {
        for (long long offset = 0; offset < frames; ++offset) one(offset);
        return LDPC_SUCCESS;
    }
    std::vector<std::thread> pool;
    for (long long t = 0; t < threads; ++t) {
        const long long lo = frames * t / threads, hi = frames * (t + 1) / threads;
        pool.emplace_back([&one, lo, hi] { for (long long offset = lo; offset < hi; ++offset) one(offset); });
    }
    for (auto &th : pool) th.join();
    return LDPC_SUCCESS;
}

/* ---- z-bit vectors as 64-bit words (bit r of a block = bit r % 64 of word r / 64), each followed by one
 *      zero word so that a 64-bit window may start at any bit ---------------------------------------- */
namespace {

inline unsigned long long window64(const unsigned long long *v, long long bit)
{
    const long long w = bit >> 6;
    const int b = (int)(bit & 63);
    return b ? (v[w] >> b) | (v[w + 1] << (64 - b)) : v[w];
}

/* acc[dst .. dst + count) ^= v[src .. src + count) */
inline void xor_bits(unsigned long long *acc, long long dst, const unsigned long long *v, long long src, long long count)
{
    while (count > 0) {
        const long long dw = dst >> 6;
        const int db = (int)(dst & 63);
        const int n = (int)(count < 64 - db ? count : 64 - db);
        const unsigned long long bits = window64(v, src) & (n == 64 ? ~0ull : ((1ull << n) - 1ull));
        acc[dw] ^= bits << db;
        dst += n; src += n; count -= n;
    }
}

/* acc[r] ^= v[(r + p) mod z] for r < z: the action of a circulant with shift p (row r has its one at
 * column (r + p) mod z, initCheckMatrix above) */
inline void xor_rotated(unsigned long long *acc, const unsigned long long *v, int p, int z)
{
    xor_bits(acc, 0, v, p, z - p);
    if (p) xor_bits(acc, z - p, v, 0, p);
}

}  // namespace

/* encodeOnce, MyLdpc.cpp:633-682.  Output layout [K info | z p1 | M-z p2],
 * LSB-first bits (:661-680).  The structured solve works on whole z-bit vectors, 64 bits per operation
 * (the bit-at-a-time form it replaces spent 0.29 ms per frame at N = 64800; this one about 10 us); the
 * dense fallback for an unstructured parity part stays bit-wise. */
int Coder::encodeOnce(const char *src, char *code, int srcLength)
{
    const int mb = seedRowLength, kb = kSeedCols - mb;
    if (srcLength < 0) srcLength = 0;
    if (srcLength > ldpcK / 8) srcLength = ldpcK / 8;
    /* the reference copies the source with strncpy (:661), which stops at a NUL
     * byte; the intent -- and this code -- is a plain copy */
    memcpy(code, src, (size_t)srcLength);
    memset(code + srcLength, 0, (size_t)(ldpcN / 8 - srcLength));
    if (structured) {
        const int W = (z + 63) / 64 + 1;                      /* words per block incl. the zero word */
        /* information bits: the first K/8 whole bytes of the frame (:641-650), zero beyond srcLength -- exactly
         * the bytes just written to `code`; as words with slack for the 64-bit windows */
        const size_t infoWords = ((size_t)ldpcK + 63) / 64 + 2;
        std::vector<unsigned long long> info(infoWords, 0ull), lam((size_t)mb * W, 0ull), par((size_t)mb * W, 0ull), blk((size_t)W, 0ull);
        memcpy(info.data(), code, (size_t)srcLength);
        /* lambda_i = (A s) restricted to block row i */
        for (int j = 0; j < kb; ++j) {
            std::fill(blk.begin(), blk.end(), 0ull);
            xor_bits(blk.data(), 0, info.data(), (long long)j * z, z);
            bool any = false;
            for (int w = 0; w + 1 < W; ++w) any = any || blk[w];
            if (!any) continue;
            for (int i = 0; i < mb; ++i) {
                const int p = shift[(size_t)i * kSeedCols + j];
                if (p >= 0) xor_rotated(&lam[(size_t)i * W], blk.data(), p, z);
            }
        }
        unsigned long long *p1 = &par[0];
        for (int i = 0; i < mb; ++i)
            for (int w = 0; w + 1 < W; ++w) p1[w] ^= lam[(size_t)i * W + w];
        const int h0 = shift[kb];
        /* v_1 = lambda_0 + P(h0) p1 ; v_{i+1} = lambda_i + v_i (+ p1 at row x) */
        for (int w = 0; w + 1 < W; ++w) par[(size_t)W + w] = lam[w];
        xor_rotated(&par[(size_t)W], p1, h0, z);
        for (int i = 1; i <= mb - 2; ++i)
            for (int w = 0; w + 1 < W; ++w)
                par[(size_t)(i + 1) * W + w] = lam[(size_t)i * W + w] ^ par[(size_t)i * W + w] ^ ((i == encX) ? p1[w] : 0ull);
        /* parity block b goes to code bits [K + b z, K + (b + 1) z): assembled in words, then ORed in bytewise */
        const long long nbits = (long long)ldpcM;
        std::vector<unsigned long long> out(((size_t)ldpcN + 63) / 64 + 2, 0ull);
        for (int b = 0; b < mb; ++b) xor_bits(out.data(), (long long)ldpcK + (long long)b * z, &par[(size_t)b * W], 0, z);
        const unsigned char *ob = reinterpret_cast<const unsigned char *>(out.data());
        for (long long byte = ldpcK / 8; byte < (ldpcK + nbits + 7) / 8 && byte < ldpcN / 8; ++byte) code[byte] |= (char)ob[byte];
        return LDPC_SUCCESS;
    }
    std::vector<unsigned char> s((size_t)ldpcK, 0), par((size_t)ldpcM, 0);
    for (int c = 0; c < ldpcK / 8 && c < srcLength; ++c)         /* :641-650 */
        for (int b = 0; b < 8; ++b) s[(size_t)8 * c + b] = ((unsigned char)src[c] >> b) & 1;
    /* lambda_i = (A s) restricted to block row i */
    std::vector<unsigned char> lam((size_t)ldpcM, 0);
    for (int i = 0; i < mb; ++i)
        for (int j = 0; j < kb; ++j) {
            const int p = shift[(size_t)i * kSeedCols + j];
            if (p < 0) continue;
            for (int r = 0; r < z; ++r) lam[(size_t)i * z + r] ^= s[(size_t)j * z + (r + p) % z];
        }
    for (int i = 0; i < ldpcM; ++i) {
        unsigned char acc = 0;
        for (int j = 0; j < ldpcM; ++j) acc ^= denseInv[(size_t)i * ldpcM + j] & lam[j];
        par[i] = acc;
    }
    for (int i = 0; i < ldpcM; ++i)
        if (par[i]) {
            const int off = ldpcK + i;
            code[off / 8] |= (char)(1 << (off % 8));
        }
    return LDPC_SUCCESS;
}

/* ----------------------------------------------------------------- decoder */

/* forDecoder, MyLdpc.cpp:167-305: the adjacency lists become an ldpc_graph; the
 * OpenCL context/program/buffers become decoder handles made in addDecodeType. */
int Coder::forDecoder(int batchSize)
{
    if (!hSeed) return fail(LDPC_ERR_STATE, "Coder was not constructed");
    if (batchSize <= 0) return fail(LDPC_ERR_ARG, "forDecoder: batchSize must be positive");
    this->batchSize = batchSize;
    if (int rc = makeGraph()) return rc;
    isDecoder = true;
    return LDPC_SUCCESS;
}

/* one device (setDevice) or a device list (setDevices) behind the handle */
int Coder::makeDecoder(const ldpc_decoder_config &cfg0, ldpc_decoder **out)
{
    ldpc_decoder_config cfg = cfg0;
    cfg.host_input = hostInput;
    if (devices.empty()) return ldpc_decoder_create(graph, &cfg, out);
    return ldpc_decoder_create_multi(graph, &cfg, devices.data(), (int)devices.size(), out);
}

/* addDecodeType, MyLdpc.cpp:307-552. */
int Coder::addDecodeType(enum decodeType deType)
{
    if (!isDecoder) return fail(LDPC_ERR_STATE, "addDecodeType: call forDecoder() first");
    if (decoders.count((int)deType)) return LDPC_SUCCESS;
    if (osdOrder >= 0) {
        if (deType == DecodeSP)
            return fail(LDPC_ERR_UNSUPPORTED, "addDecodeType: DecodeSP has no soft output for setOsd() (see decodeSoft); the min-sum "
                        "decode types, DecodeBP and DecodeLayeredBP have");
        if (deType == DecodeBitFlip)
            return fail(LDPC_ERR_UNSUPPORTED, "addDecodeType: DecodeBitFlip is a hard-decision decoder and has no soft output for setOsd()");
        if (deType == DecodeCPU)
            return fail(LDPC_ERR_UNSUPPORTED, "addDecodeType: DecodeCPU packs its bytes at bit offsets; setOsd() works on rows of K / 8 bytes");
        if (!osd)
            if (int rc = ldpc_osd_create(graph, ldpcK, batchSize, device, &osd)) return fail(rc, std::string("addDecodeType: ") + ldpc_last_error());
    }
    if (deType == DecodeCPU) return LDPC_SUCCESS;   /* made on first use: needs the stream length (:438-439 is a no-op too) */
    ldpc_decoder_config cfg;
    ldpc_decoder_config_init(&cfg);
    cfg.K = ldpcK;
    cfg.max_batch = batchSize;
    cfg.max_iter = times;
    cfg.llr_scale = llrScale;
    cfg.device = device;
    cfg.early_term = 1;
    cfg.poll_interval = 4;
    cfg.pack_mode = LDPC_PACK_BYTES;
    cfg.layer_rows = z;
    cfg.msg_dtype = msgType;                           /* setMessageType(): ldpc_decoder_create refuses what it does not carry */
    cfg.msg_bits = msgBits;
    cfg.algo = (deType == DecodeSP) ? LDPC_ALGO_SP : (deType == DecodeMS) ? LDPC_ALGO_MS
               : (deType == DecodeMSCL) ? LDPC_ALGO_MS_FUSED : (deType == DecodeBP) ? LDPC_ALGO_BP
               : (deType == DecodeLayeredBP) ? LDPC_ALGO_LAYERED_BP
               : (deType == DecodeLayeredFixed) ? LDPC_ALGO_LAYERED_FX
               : (deType == DecodeLayeredBPFixed) ? LDPC_ALGO_LAYERED_BP_FX
               : (deType == DecodeBitFlip) ? LDPC_ALGO_BITFLIP : LDPC_ALGO_LAYERED;
    if (deType == DecodeLayeredFixed || deType == DecodeLayeredBPFixed) cfg.post_bits = postBits;     /* setPosteriorBits(); the circulant size as DecodeTDMPCL */
    if (deType == DecodeLayeredBPFixed) cfg.bp_frac_bits = fracBits;    /* setLlrFractionBits() */
    if (deType == DecodeBitFlip && !bfThreshold.empty()) {             /* setBitFlipThresholds(): the last offset repeats */
        if (bfThreshold.size() > 16) return fail(LDPC_ERR_ARG, "addDecodeType: setBitFlipThresholds takes at most 16 round offsets");
        for (size_t j = 0; j < 16; ++j) cfg.bf_threshold[j] = bfThreshold[j < bfThreshold.size() ? j : bfThreshold.size() - 1];
    }
    if (deType == DecodeLayeredFixed && fxRecord) cfg.tune_flags |= LDPC_TUNE_ON(LDPC_TUNE_FX_RECORD);   /* setFixedRecordKernel() */
    if (deType == DecodeTDMP) {
        /* The reference's host-layered path (MyLdpc.cpp:889-976) sizes layer l as
         * hRowRange[l + z] - hRowRange[l] (:907, :958): right only when all rows of H have one weight
         * (rates 2/3A and 5/6).  There DecodeTDMP follows it operation for operation
         * (LDPC_ALGO_LAYERED_HOST); for the other seeds the reference's result is not a decode of H,
         * and DecodeTDMP runs the layered schedule with the fused kernel's semantics instead. */
        bool uniform = true;
        for (int m = 1; m < ldpcM && uniform; ++m)
            uniform = (rowRange[m + 1] - rowRange[m]) == (rowRange[1] - rowRange[0]);
        if (uniform) cfg.algo = LDPC_ALGO_LAYERED_HOST;
    }
    if (deType == DecodeMSCL) cfg.max_iter = 120;      /* hard-coded in the reference kernel, decodeCL.c:479 */
    if (msScale != 0.0f || msOffset != 0.0f) {
        if (cfg.algo == LDPC_ALGO_MS_FUSED)
            return fail(LDPC_ERR_UNSUPPORTED, "addDecodeType: DecodeMSCL reproduces the reference's fused min-sum "
                        "kernel and takes no min-sum correction (setMinSumCorrection)");
        if (cfg.algo == LDPC_ALGO_LAYERED_HOST)
            return fail(LDPC_ERR_UNSUPPORTED, "addDecodeType: DecodeTDMP follows the reference's host-layered path on "
                        "this code and takes no min-sum correction (setMinSumCorrection); DecodeTDMPCL does");
        if (cfg.algo != LDPC_ALGO_SP) { cfg.ms_scale = msScale; cfg.ms_offset = msOffset; }   /* DecodeSP: ignored; DecodeBP, DecodeLayeredBP: refused by ldpc_decoder_create */
    }
    if (crcEarlyStop) {
        if (cfg.algo == LDPC_ALGO_MS_FUSED)
            return fail(LDPC_ERR_UNSUPPORTED, "addDecodeType: DecodeMSCL reproduces the reference's fused min-sum "
                        "kernel, which stops on the syndrome alone (setCrcEarlyStop)");
        if (cfg.algo == LDPC_ALGO_LAYERED_HOST)
            return fail(LDPC_ERR_UNSUPPORTED, "addDecodeType: DecodeTDMP follows the reference's host-layered path on "
                        "this code, which stops on the syndrome alone (setCrcEarlyStop); DecodeTDMPCL takes the CRC");
        if (int rc = applyCrcEarlyStop(cfg)) return rc;
    }
    ldpc_decoder *d = nullptr;
    int rc = makeDecoder(cfg, &d);
    if (rc) return fail(rc, ldpc_last_error());
    decoders[(int)deType] = d;
    return LDPC_SUCCESS;
}

/* decode, MyLdpc.cpp:571-618: the frame stream is cut into batchSize groups by
 * ldpc_decode.  srcLength bytes are written. */
int Coder::decode(float *postCode, char *srcCode, int srcLength, enum decodeType deType)
{
    return decodeFrames(postCode, LDPC_LLR_F32, 1.0f, srcCode, srcLength, deType, nullptr, 0);
}

/* decode() on int8 / fp16 channel values (ldpc_decode_typed): the decoder reads y = x * llrUnit */
int Coder::decodeTyped(const void *postCode, int llrType, float llrUnit, char *srcCode, int srcLength, enum decodeType deType)
{
    return decodeFrames(postCode, llrType, llrUnit, srcCode, srcLength, deType, nullptr, 0);
}

int Coder::decodeSoftTyped(const void *postCode, int llrType, float llrUnit, char *srcCode, int srcLength, enum decodeType deType,
                           float *soft, int kind)
{
    if (!soft) return fail(LDPC_ERR_ARG, "decodeSoftTyped: soft is NULL");
    if (kind != LDPC_SOFT_POSTERIOR && kind != LDPC_SOFT_EXTRINSIC) return fail(LDPC_ERR_ARG, "decodeSoftTyped: unknown kind");
    if (deType == DecodeSP) return fail(LDPC_ERR_UNSUPPORTED, "decodeSoftTyped: DecodeSP has no soft output (see decodeSoft)");
    return decodeFrames(postCode, llrType, llrUnit, srcCode, srcLength, deType, soft, kind);
}

int Coder::decodeSoft(float *postCode, char *srcCode, int srcLength, enum decodeType deType, float *soft, int kind)
{
    if (!soft) return fail(LDPC_ERR_ARG, "decodeSoft: soft is NULL");
    if (kind != LDPC_SOFT_POSTERIOR && kind != LDPC_SOFT_EXTRINSIC) return fail(LDPC_ERR_ARG, "decodeSoft: unknown kind");
    if (deType == DecodeSP)
        return fail(LDPC_ERR_UNSUPPORTED, "decodeSoft: DecodeSP works in the probability domain, where the posterior has "
                    "saturated by the time a frame stops; the min-sum decode types, DecodeBP and DecodeLayeredBP carry soft output");
    return decodeFrames(postCode, LDPC_LLR_F32, 1.0f, srcCode, srcLength, deType, soft, kind);
}

/* soft != nullptr: ldpc_decode_soft, N floats per frame of the mother code.  (llrType, llrUnit): the element type of
 * postCode, LDPC_LLR_F32 with unit 1 for decode() and decodeSoft() */
int Coder::decodeFrames(const void *postCode, int llrType, float llrUnit, char *srcCode, int srcLength, enum decodeType deType,
                        float *soft, int kind)
{
    if (!isDecoder) return fail(LDPC_ERR_STATE, "decode: call forDecoder() first");
    if (!postCode || !srcCode || srcLength <= 0) return fail(LDPC_ERR_ARG, "decode: bad arguments");
    const int codeSize = getCodeSize(srcLength);
    /* with setTransportBlock() or setOuterBch() the decoders write whole frames of K / 8 bytes to a buffer of their own */
    char *const payloadOut = srcCode;
    const int payloadLength = srcLength;
    std::vector<char> decoded;
    if (tbSpec.A || bchK) {
        decoded.resize((size_t)codeSize * (ldpcK / 8));
        srcCode = decoded.data();
        srcLength = (int)decoded.size();
    }
    ldpc_decoder *d = nullptr;
    if (deType == DecodeCPU) {
        /* decodeCPU, MyLdpc.cpp:684-784: one pass over the whole stream, bit-offset packing */
        if (!decoders.count((int)DecodeCPU) || cpuDecoderBatch < codeSize) {
            if (decoders.count((int)DecodeCPU)) ldpc_decoder_destroy(decoders[(int)DecodeCPU]);
            decoders.erase((int)DecodeCPU);
            ldpc_decoder_config cfg;
            ldpc_decoder_config_init(&cfg);
            cfg.K = ldpcK; cfg.max_batch = codeSize; cfg.max_iter = times; cfg.device = device;
            cfg.algo = LDPC_ALGO_MS; cfg.pack_mode = LDPC_PACK_BITS; cfg.early_term = 1; cfg.poll_interval = 4;
            cfg.layer_rows = z;                              /* circulant size: lets the record / one-launch kernels apply
                                                                (with a correction: the record kernel or the streaming ones) */
            cfg.ms_scale = msScale; cfg.ms_offset = msOffset;
            cfg.msg_dtype = msgType; cfg.msg_bits = msgBits;
            if (msgType == LDPC_MSG_I8) cfg.llr_scale = llrScale;    /* the LSBs per unit of channel value; min-sum reads it in no other case */
            if (int rc = applyCrcEarlyStop(cfg)) return rc;
            int rc = makeDecoder(cfg, &d);
            if (rc) return fail(rc, ldpc_last_error());
            decoders[(int)DecodeCPU] = d;
            cpuDecoderBatch = codeSize;
        }
        d = decoders[(int)DecodeCPU];
        memset(srcCode, 0, (size_t)srcLength);               /* :685 */
    } else {
        auto it = decoders.find((int)deType);
        if (it == decoders.end()) return fail(LDPC_ERR_STATE, "decode: addDecodeType() was not called for this type");
        d = it->second;
    }
    /* setOsd(): the decode's soft form, then the frames with a dirty syndrome through ldpc_osd_run */
    const bool withOsd = osdOrder >= 0 && !soft && osd && deType != DecodeCPU;
    std::vector<float> posterior;
    if (withOsd) {
        posterior.resize((size_t)codeSize * ldpcN);
        soft = posterior.data();
        kind = LDPC_SOFT_POSTERIOR;
    }
    std::vector<float> recovered;
    if (rmE && llrType != LDPC_LLR_F32)
        return fail(LDPC_ERR_UNSUPPORTED, "decodeTyped: rate recovery (setRateMatch) sums float values; quantise behind it "
                    "(ldpc_rate_recover_device, ldpc_llr_quantize_device, ldpc_decode_typed_device)");
    if (rmE) {
        /* E received values per frame -> the N channel values the decoder reads */
        recovered.resize((size_t)codeSize * ldpcN);
        int rm = ldpc_rate_recover(&rmSpec, static_cast<const float *>(postCode), codeSize, rmK0, rmE, nullptr, 0, recovered.data(), device);
        if (rm) return fail(rm, ldpc_last_error());
        postCode = recovered.data();
    }
    /* LDPC_LLR_F32 with unit 1: these are ldpc_decode_soft and ldpc_decode */
    int rc = soft ? ldpc_decode_soft_typed(d, postCode, llrType, llrUnit, codeSize, (uint8_t *)srcCode, srcLength, nullptr, soft,
                                           (int64_t)codeSize * ldpcN, kind)
                  : ldpc_decode_typed(d, postCode, llrType, llrUnit, codeSize, (uint8_t *)srcCode, srcLength, nullptr);
    if (rc) return fail(rc, ldpc_last_error());
    ldpc_decode_stats st;
    if (ldpc_decoder_stats(d, &st) == LDPC_OK) lastTime = st.batch_time;
    int64_t stops = 0;
    crcStops = ldpc_decoder_crc_stops(d, &stops) == LDPC_OK ? (long long)stops : 0;
    if (withOsd) {
        std::vector<uint8_t> rowsOut((size_t)codeSize * (ldpcK / 8));
        std::vector<int32_t> status((size_t)codeSize, 0);
        rc = ldpc_osd_run(osd, posterior.data(), codeSize, osdOrder, 256.0f, rowsOut.data(), (int64_t)rowsOut.size(), nullptr, status.data(),
                          nullptr);
        if (rc) return fail(rc, ldpc_last_error());
        memcpy(srcCode, rowsOut.data(), std::min((size_t)srcLength, rowsOut.size()));
        osdProcessed = osdFlipped = 0;
        for (int32_t st : status) {
            osdProcessed += st > 0;
            osdFlipped += st == 2;
        }
    }
    if (tbSpec.A) {
        std::vector<char> payload((size_t)codeSize * (tbSpec.A / 8));
        crcOk.assign((size_t)codeSize, 0);
        rc = ldpc_tb_check(&tbSpec, (const uint8_t *)decoded.data(), codeSize, (uint8_t *)payload.data(), nullptr, crcOk.data(), device);
        if (rc) return fail(rc, ldpc_last_error());
        memcpy(payloadOut, payload.data(), (size_t)payloadLength);
        crcFailures = 0;
        for (unsigned char ok : crcOk) crcFailures += !ok;
    }
    if (bchK) {
        std::vector<char> payload((size_t)codeSize * (bchK / 8));
        bchStatusOfFrame.assign((size_t)codeSize, 0);
        rc = ldpc_bch_decode(&bchSpec, (const uint8_t *)decoded.data(), codeSize, (uint8_t *)payload.data(), bchStatusOfFrame.data(), device);
        if (rc) return fail(rc, ldpc_last_error());
        memcpy(payloadOut, payload.data(), (size_t)payloadLength);
        bchFailed = bchCorrected = bchBits = 0;
        for (int32_t st : bchStatusOfFrame) {
            bchFailed += st < 0;
            bchCorrected += st > 0;
            bchBits += st > 0 ? st : 0;
        }
    }
    return LDPC_SUCCESS;
}

/* ------------------------------------------------------------ test channel */

/* gaussian, MyLdpc.cpp:1093-1105.  C++ overloads: sqrt/log/cos on float. */
float gaussian(float ave, float sd)
{
    const float pi = 3.1415926f;
    const float s1 = (float)((1.0 + rand()) / (RAND_MAX + 1.0));
    const float s2 = (float)((1.0 + rand()) / (RAND_MAX + 1.0));
    const float r = std::sqrt(-2 * std::log(s2));
    const float t = 2 * pi * s1;
    const float zz = r * std::cos(t);
    return ave + zz * sd;
}

/* test, MyLdpc.cpp:1061-1078 */
int Coder::test(char *priorCode, float *postCode, int priorCodeLength, float rate)
{
    if (!priorCode || !postCode || priorCodeLength < 0) return fail(LDPC_ERR_ARG, "test: bad arguments");
    if (modSpec.Qm) {
        /* symbols through the modem stage on the device; the demapped values take the place of the +-1 samples */
        const int bits = rmE ? rmE : ldpcN;
        const int64_t row = ldpc_modem_symbol_floats(&modSpec, bits);
        if (row == 0) return fail(LDPC_ERR_ARG, std::string("test: ") + ldpc_last_error());
        if (priorCodeLength % (bits / 8)) return fail(LDPC_ERR_ARG, "test: priorCodeLength is not a whole number of frames");
        const int64_t frames = priorCodeLength / (bits / 8);
        const uint64_t hi = (uint64_t)(unsigned)rand(), lo = (uint64_t)(unsigned)rand();
        std::vector<float> sym((size_t)(frames * row));
        int rc = ldpc_modem_transmit(&modSpec, (const uint8_t *)priorCode, LDPC_CODE_PACKED, frames, bits, rate, (hi << 32) | lo, 0,
                                     sym.data(), (int64_t)sym.size(), device);
        if (!rc) rc = ldpc_modem_demap(&modSpec, sym.data(), frames, bits, postCode, device);
        return rc ? fail(rc, ldpc_last_error()) : LDPC_SUCCESS;
    }
    for (int c = 0; c < priorCodeLength; ++c)
        for (int b = 0; b < 8; ++b)
            postCode[c * 8 + b] = (priorCode[c] & (1 << b)) ? -1.0f : 1.0f;
    for (int i = 0; i < priorCodeLength * 8; ++i) postCode[i] += gaussian(0, rate);
    return LDPC_SUCCESS;
}
