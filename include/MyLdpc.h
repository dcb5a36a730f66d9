/*
 * MyLdpc.h -- the reference's public C++ API (class Coder, MyLdpc.h:104-238 of
 * wing02/MyLdpcCppApi) re-created on top of the MI355X C ABI (ldpc_hip.h).
 *
 * Same names, argument meaning, call order and data conventions as the
 * reference (Test.cpp:28-104 compiles against this header unchanged apart from
 * its `#include "cl.hpp"`):
 *     Coder c(K, N, rate); c.forEncoder(); c.forDecoder(batch);
 *     c.encode(src, prior, srcLen); c.test(prior, post, priorLen, sd);
 *     c.addDecodeType(DecodeSP); c.decode(post, out, srcLen, DecodeSP);
 *
 * Deliberate differences (all listed in INTEGRATION.md):
 *   - no Eigen, no OpenCL: the public Eigen member `checkMatrix` (MyLdpc.h:128)
 *     becomes the CSR view hRowRange()/hCols(); `kernelSourceCode` and the
 *     run-time dependency on ./decodeCL.c (MyLdpc.cpp:237) are gone.
 *   - methods return 0 on success as before, but failures return a non-zero
 *     ldpc_status and never exit() (reference: MyLdpc.cpp:243-254); lastError().
 *   - several decode types may be added to one Coder (the reference shares its
 *     kernel objects between SP/MS/TDMP, MyLdpc.cpp:334,397,450).
 *   - DecodeCPU runs the same min-sum arithmetic on the GPU (bit-identical to
 *     decodeCPU, MyLdpc.cpp:684-784, including its bit-offset packing); there is
 *     no CPU decode path in this library.
 *   - DecodeTDMPCL runs the layered schedule with the semantics of the fused kernel
 *     (decodeCL.c:307-426).  DecodeTDMP follows the reference's HOST-driven layered path
 *     (MyLdpc.cpp:889-976 over decodeCL.c:203-300) operation for operation on the seeds where
 *     that path is a decode of H -- every row of one weight: rates 2/3A and 5/6; the reference
 *     sizes layer l as hRowRange[l+z]-hRowRange[l], :907,958 -- and falls back to the fused
 *     kernel's semantics on the other four.  DecodeMSCL runs the fused flooding kernel's
 *     arithmetic (decodeCL.c:432-567, 120 iterations as there).
 *   - `times` (MyLdpc.cpp:24) and the SP channel scale 8 (decodeCL.c:9) stay the
 *     defaults and can be changed with setMaxIterations()/setLlrScale().
 *   - setDevices(): one Coder over several GPUs (the reference uses devices[0] only).
 *   - setEncodeOnDevice(): encode() on the GPU (the "encoder" section of ldpc_hip.h) instead of the host.
 *   - setRateMatch(): puncturing, filler bits and a circular-buffer transmission of E bits per frame around
 *     encode() / decode() (the "rate matching" section of ldpc_hip.h).
 *   - setModulation(): test() sends QPSK / 16- / 64- / 256-QAM symbols through the "modem" section of ldpc_hip.h.
 *   - setTransportBlock(): every frame carries payload bits plus a CRC ("transport block" section of ldpc_hip.h), which
 *     decode() checks: crcPassed() / lastCrcFailures().
 *   - setOuterBch(): every frame carries payload bits plus the parity of a BCH code ("outer code" section of ldpc_hip.h),
 *     with which decode() repairs up to t wrong bits per frame: bchStatus() / bchCounts().
 *   - setOsd(): decode() passes the frames a decoder leaves with a dirty syndrome through ordered-statistics decoding
 *     ("ordered-statistics post-processing" section of ldpc_hip.h): osdCounts().
 */
#ifndef MYLDPC_H_
#define MYLDPC_H_

#include <map>
#include <string>
#include <vector>

#include "ldpc_hip.h"

#define LDPC_SUCCESS 0
#define LDPC_FAIL 1

enum rate_type { rate_1_2, rate_2_3_a, rate_2_3_b, rate_3_4_a, rate_3_4_b, rate_5_6 };

enum decodeType { DecodeCPU, DecodeMS, DecodeSP, DecodeTDMP, DecodeTDMPCL, DecodeMSCL,
                  DecodeBP, /* not in the reference: log-domain sum-product, LDPC_ALGO_BP (include/ldpc_hip.h) */
                  DecodeLayeredBP, /* not in the reference: the layered schedule of DecodeTDMPCL (same circulant size) with
                                     DecodeBP's check node, LDPC_ALGO_LAYERED_BP (include/ldpc_hip.h); fp32 messages only */
                  DecodeLayeredFixed, /* not in the reference: the layered schedule of DecodeTDMPCL (same circulant size) in
                                     fixed point, LDPC_ALGO_LAYERED_FX (include/ldpc_hip.h): setMessageType(LDPC_MSG_I8,
                                     bits) gives the message width, setPosteriorBits() the width of the saturating
                                     posterior memory, setLlrScale() the LSBs per unit of channel value; it takes
                                     setMinSumCorrection, setCrcEarlyStop, decodeSoft (values in LSBs) and decodeTyped */
                  DecodeLayeredBPFixed /* not in the reference: DecodeLayeredFixed with DecodeLayeredBP's check node computed as
                                     hardware does, min plus a correction from a table, LDPC_ALGO_LAYERED_BP_FX
                                     (include/ldpc_hip.h): setMessageType(LDPC_MSG_I8, bits), setPosteriorBits() and
                                     setLlrFractionBits() give the widths, setLlrScale() the LSBs per unit of channel value,
                                     chosen so that llrScale * y is the LLR in LSBs of 2^-fractionBits; it takes
                                     setCrcEarlyStop, decodeSoft (values in LSBs) and decodeTyped, and no
                                     setMinSumCorrection (LDPC_ERR_UNSUPPORTED: there is no minimum to correct) */,
                  DecodeBitFlip /* not in the reference: hard-decision parallel bit flipping, LDPC_ALGO_BITFLIP
                                     (include/ldpc_hip.h): only the sign of a channel value is read, setLlrScale() is ignored,
                                     setBitFlipThresholds() gives the round offsets; it takes setCrcEarlyStop and
                                     decodeTyped, and no decodeSoft, setMinSumCorrection or message type other than
                                     LDPC_MSG_F32 (LDPC_ERR_UNSUPPORTED) */ };

const int n_b = 24;

class Coder {
public:
    Coder(int ldpcK, int ldpcN, enum rate_type rate);
    ~Coder();
    Coder(const Coder &) = delete;
    Coder &operator=(const Coder &) = delete;

    int forEncoder();
    int forDecoder(int batchSize);
    int addDecodeType(enum decodeType deType);

    int encode(char *srcCode, char *priorCode, int srcLength);
    /* postCode: getPostCodeLength(srcLength) floats; srcCode: srcLength bytes out */
    int decode(float *postCode, char *srcCode, int srcLength, enum decodeType deType);
    /* decode() with soft output (ldpc_hip.h: ldpc_decode_soft): soft takes N floats per frame over the MOTHER code --
     * also under setRateMatch(), where postCode holds E per frame --, per frame the posterior of the round the frame
     * stopped in (kind LDPC_SOFT_POSTERIOR: positive <-> bit 0, its sign is the decoded bit) or that minus the channel
     * value the decoder read (LDPC_SOFT_EXTRINSIC).  Everything else as decode(), the transport-block check included.
     * DecodeSP returns LDPC_ERR_UNSUPPORTED with lastError() set: sum-product has no usable soft value in the probability
     * domain; DecodeBP and DecodeLayeredBP, the log-domain sum-products, give LLRs (y_n = llrScale * y). */
    int decodeSoft(float *postCode, char *srcCode, int srcLength, enum decodeType deType, float *soft, int kind = LDPC_SOFT_POSTERIOR);
    /* decode() / decodeSoft() on channel values as receivers deliver them (ldpc_hip.h: enum ldpc_llr_type, ldpc_decode_typed):
     * postCode holds getPostCodeLength(srcLength) elements of llrType -- LDPC_LLR_I8 (int8_t), LDPC_LLR_F16 (binary16) or
     * LDPC_LLR_F32 (llrUnit exactly 1: the call is decode()) -- and the decoder reads y = x * llrUnit, one fp32 multiply,
     * then does exactly what decode() does with that y.  A quarter (half) of the bytes cross the bus.  Not under
     * setRateMatch(), whose recovery sums floats: LDPC_ERR_UNSUPPORTED. */
    int decodeTyped(const void *postCode, int llrType, float llrUnit, char *srcCode, int srcLength, enum decodeType deType);
    int decodeSoftTyped(const void *postCode, int llrType, float llrUnit, char *srcCode, int srcLength, enum decodeType deType,
                        float *soft, int kind = LDPC_SOFT_POSTERIOR);

    /* BPSK + AWGN of standard deviation `rate` on libc rand() (MyLdpc.cpp:1061-1105) */
    int test(char *priorCode, float *postCode, int priorCodeLength, float rate);

    int getPriorCodeLength(int srcLength);
    int getPostCodeLength(int srcLength);
    int getCodeSize(int srcLength);

    /* ---- additions ------------------------------------------------------ */
    void setMaxIterations(int times) { this->times = times; }   /* before addDecodeType */
    void setLlrScale(float s) { llrScale = s; }                 /* DecodeSP, DecodeBP and DecodeLayeredBP (2 / sd^2 for BPSK in noise sd); with LDPC_MSG_I8 the LSBs per unit; before addDecodeType */
    void setDevice(int ordinal) { device = ordinal; devices.clear(); }
    /* Several HIP devices behind one Coder (the reference opens devices[0] only, MyLdpc.cpp:235):
     * decode() then cuts the frame stream into one contiguous range per entry and decodes the
     * ranges side by side, batchSize frames per device and launch group; bytes identical to the
     * single-device result.  Before addDecodeType(). */
    void setDevices(const int *ordinals, int count) { devices.assign(ordinals, ordinals + (count > 0 ? count : 0)); }
    /* How decode() moves the caller's (pageable) postCode to the devices: LDPC_HOST_INPUT_STAGED (default:
     * through the library's own pinned ring) or LDPC_HOST_INPUT_LOCK_PAGES (page-locks the caller's pages
     * for the call; include/ldpc_hip.h).  Before addDecodeType(). */
    void setHostInput(int mode) { hostInput = mode; }
    /* Normalized / offset min-sum for DecodeMS, DecodeCPU and DecodeTDMPCL: each check row's two smallest
     * magnitudes m become fmaxf(m - offset, 0) * scale (scale 0 = 1; offset in units of postCode, include/ldpc_hip.h:
     * ms_scale / ms_offset).  DecodeSP ignores it.  DecodeTDMP on a code whose rows differ in weight runs the
     * layered schedule of DecodeTDMPCL and takes the correction too; where it follows the reference's host-layered
     * path (every row of one weight) it fails in addDecodeType while a correction is set, as DecodeMSCL always
     * does (both reproduce reference kernels), and as DecodeBP and DecodeLayeredBP do (LDPC_ERR_UNSUPPORTED: there is no minimum to
     * correct).  (0, 0) = off.  Before addDecodeType(). */
    void setMinSumCorrection(float scale, float offset) { msScale = scale; msOffset = offset; }
    /* How the decoders addDecodeType makes from here on store their messages (include/ldpc_hip.h: enum ldpc_msg_dtype):
     * LDPC_MSG_F32 (the default, the reference's arithmetic), LDPC_MSG_F16 or LDPC_MSG_F8 (one E4M3 byte per message).
     * DecodeMS and DecodeCPU take all three, DecodeBP takes F32 and F16 (DecodeLayeredBP, like every layered type, F32 only), and give the bytes of the C ABI decoder with that
     * msg_dtype; with any other decode type a type other than LDPC_MSG_F32 makes addDecodeType fail as ldpc_decoder_create does
     * (LDPC_ERR_UNSUPPORTED; an unknown value: LDPC_ERR_ARG).  LDPC_MSG_I8 (DecodeMS and DecodeCPU only) stores saturating
     * integers of `bits` = 4, 5, 6 or 8 bits (0 = 8; with any other type bits must be 0); setLlrScale() is then the number
     * of LSBs per unit of channel value.  Before addDecodeType(). */
    void setMessageType(int msgDtype, int bits = 0) { msgType = msgDtype; msgBits = bits; }
    /* DecodeLayeredFixed and DecodeLayeredBPFixed: the posterior memory holds `bits` bits, message bits <= bits <= 16 (0 = 16;
     * include/ldpc_hip.h: post_bits); anything else makes addDecodeType fail as ldpc_decoder_create does.  Read by no other
     * decode type.  Before addDecodeType(). */
    void setPosteriorBits(int bits) { postBits = bits; }
    /* DecodeLayeredFixed: true runs the same rule, bit for bit, on the fixed-point record kernel (include/ldpc_hip.h:
     * LDPC_TUNE_FX_RECORD) where the code fits it, and on the streaming layered engine where it does not; with
     * setCrcEarlyStop addDecodeType then fails as ldpc_decoder_create does.  Off by default.  Read by no other decode type.
     * Before addDecodeType(). */
    void setFixedRecordKernel(bool on) { fxRecord = on; }
    /* DecodeLayeredBPFixed: one LSB of a message is 2^-bits LLR units, 0 <= bits <= 4 (include/ldpc_hip.h: bp_frac_bits);
     * anything else makes addDecodeType fail as ldpc_decoder_create does.  Read by no other decode type.  Before
     * addDecodeType(). */
    void setLlrFractionBits(int bits) { fracBits = bits; }
    /* DecodeBitFlip: off(i) of rounds 1 .. count, count <= 16, the last one also for every later round (include/ldpc_hip.h:
     * bf_threshold; each in [0, 62], all zero or count = 0: the default off(i) = i - 1); anything else makes addDecodeType
     * fail as ldpc_decoder_create does.  Read by no other decode type.  Before addDecodeType(). */
    void setBitFlipThresholds(const int *offsets, int count)
    {
        bfThreshold.assign(offsets, offsets + (count > 0 ? count : 0));
    }
    /* encode() on the GPU `setDevice` names (ldpc_encode, include/ldpc_hip.h) instead of the host: same bytes.
     * forEncoder() then creates the device encoder and skips the host precompute, so it also serves the seed whose
     * parity part the host solves by dense elimination only (rate_3_4_b: any N, where the host path stops at
     * M > 8192).  Off by default.  Before forEncoder(). */
    void setEncodeOnDevice(bool on);
    /* Rate matching (ldpc_hip.h, "rate matching"): code bits [0, punctured) are never sent, code bits
     * [fillerLo, fillerHi) are known zeros (the caller keeps those source bits zero) and are not sent either, and each
     * frame sends E bits of the circular buffer from position k0 on (E above the buffer's length repeats).  Then
     * encode() writes E / 8 bytes per frame (E % 8 == 0), test() and decode() take E floats per frame, and
     * getPriorCodeLength / getPostCodeLength follow; getCodeSize is the frame count as before.  erasureLlr: what
     * decode() feeds the decoder at positions that were not received -- 0, or the distinct-value rule of ldpc_hip.h:
     * pass 1e-6 with DecodeTDMP / DecodeTDMPCL, whose layered min-sum arithmetic cannot take an exact 0 (DecodeLayeredBP can).  Host buffers go
     * through ldpc_rate_match / ldpc_rate_recover on the GPU `setDevice` names.  Off by default: without this call every
     * byte and length is as in the reference.  Before forEncoder() and forDecoder().  Returns 0 or an ldpc_status. */
    int setRateMatch(int E, int k0, int punctured = 0, int fillerLo = 0, int fillerHi = 0, float erasureLlr = 0);
    /* Modulation of test() (ldpc_hip.h, "modem"): Qm = 1 (BPSK), 2 (QPSK), 4, 6 or 8 (16-, 64-, 256-QAM) bits per symbol,
     * with or without the bit interleaver of TS 38.212.  test() then maps each frame's bits -- E per frame with
     * setRateMatch(), N otherwise; they must be a multiple of Qm -- to symbols of unit mean energy, adds noise of standard
     * deviation `rate` PER REAL DIMENSION from the counter-based generator (its seed is drawn from two rand() calls, so
     * srand() still governs it) and writes the max-log demapped values into postCode: same length as without the call, so
     * decode(), getPostCodeLength() and callers are unchanged.  Runs on the GPU `setDevice` names (ldpc_modem_transmit +
     * ldpc_modem_demap).  DecodeSP reads values of very unequal reliability then: setLlrScale(2 / (rate * rate)).
     * Off by default: without this call every byte is as in the reference.  Returns 0 or an ldpc_status. */
    int setModulation(int Qm, bool interleave = true);
    /* Transport blocks (ldpc_hip.h, "transport block"), one code block each: a frame carries payloadBits payload bits
     * (a multiple of 8) followed by their CRC -- crcBits 0, 16 or 24 (CRC24A); -1 = the rule of TS 38.212: 24 above 3824
     * payload bits, else 16 -- and zero filler bits up to K; payloadBits + crc <= K.  Then encode() reads payloadBits / 8
     * source bytes per frame, decode() writes payloadBits / 8 bytes per frame and checks every frame's CRC, srcLength
     * counts payload bytes in both, and getCodeSize / getPriorCodeLength / getPostCodeLength follow.  lastCrcFailures()
     * and crcPassed(frame) report the check of the last decode().  Composes with setEncodeOnDevice, setRateMatch and
     * setModulation; a caller who does not want the fillers [payloadBits + crc, K) sent passes them to setRateMatch.
     * Runs on the GPU `setDevice` names (ldpc_tb_attach / ldpc_tb_check).  Off by default: without this call every byte and
     * length is as in the reference.  Before encode() and decode().  Returns 0 or an ldpc_status. */
    int setTransportBlock(int payloadBits, int crcBits = -1);
    /* Outer BCH code ("outer code" section of ldpc_hip.h), as a DVB-S2 frame has one around its LDPC information bits:
     * every frame carries k = n - r payload bits, the r parity bits of the BCH code that corrects t errors (1 .. 12;
     * GF(2^14) up to n = 16383, else GF(2^16); r = 14 t or 16 t there) and zero fillers up to K.  n = -1 means K; n % 8 == 0,
     * n <= K, K % 8 == 0 and k % 8 == 0 are required.  Then encode() reads k / 8 source bytes per frame, decode() writes
     * the k / 8 payload bytes per frame after the outer decoder has repaired up to t wrong bits, srcLength counts
     * payload bytes in both, and getCodeSize / getPriorCodeLength / getPostCodeLength follow.  bchStatus(frame) of the
     * last decode(): 0 clean, 1 .. t bits repaired, -1 not decodable (the payload is then what the inner decoder left),
     * -2 no such frame; bchCounts(): {frames failed, frames repaired, bits repaired}.  Composes with setEncodeOnDevice,
     * setRateMatch and setModulation.  Mutually exclusive with setTransportBlock(): the second of the two calls returns
     * LDPC_ERR_STATE.  Runs on the GPU `setDevice` names (ldpc_bch_encode / ldpc_bch_decode).  Off by default.  Before
     * encode() and decode().  Returns 0 or an ldpc_status. */
    int setOuterBch(int t, int n = -1);
    int bchStatus(int frame) const { return frame >= 0 && (size_t)frame < bchStatusOfFrame.size() ? bchStatusOfFrame[(size_t)frame] : -2; }
    struct BchCounts { int failed, corrected, bits; };
    BchCounts bchCounts() const { return BchCounts{bchFailed, bchCorrected, bchBits}; }
    /* Ordered-statistics post-processing ("ordered-statistics post-processing" section of ldpc_hip.h): order 0 or 1 turns
     * it on, -1 (the default) off.  decode() and decodeTyped() then run the soft form of the decode (posterior values) and
     * ldpc_osd_run behind it with weight_scale 256: a frame whose hard decision has a dirty syndrome leaves as the codeword
     * the rule picks, every other frame as the decoder wrote it.  The transport-block CRC and the outer BCH code see the
     * result.  decodeSoft() and decodeSoftTyped() are unchanged: they return the decoder's own bytes and values.
     * osdCounts() of the last decode(): {frames processed, frames where a flip was chosen}.  Call it before
     * addDecodeType() (LDPC_ERR_STATE once a decoder exists).  Decode types without soft output (DecodeSP, and DecodeCPU,
     * whose bytes are bit-packed) and codes that are not eligible fail in addDecodeType with the library's code and message.
     * Not to be combined with setRateMatch(): the second of the two calls returns LDPC_ERR_STATE.  K % 8 == 0 is required.
     * Returns 0 or an ldpc_status. */
    int setOsd(int order);
    struct OsdCounts { int processed, flipped; };
    OsdCounts osdCounts() const { return OsdCounts{osdProcessed, osdFlipped}; }
    /* CRC-aided early termination (ldpc_hip.h: crc_kind / crc_bits): with setTransportBlock() every frame carries a CRC,
     * and a frame then also stops in the first round in which its payload and CRC bits pass it -- usually a round before
     * its syndrome is clean.  Needs setTransportBlock() with crcBits != 0 first (LDPC_ERR_STATE otherwise).  DecodeSP,
     * DecodeMS, DecodeCPU, DecodeBP, DecodeLayeredBP and DecodeTDMPCL take it, and DecodeTDMP where it runs the layered schedule of DecodeTDMPCL; on
     * DecodeMSCL, and on DecodeTDMP where it follows the reference's host-layered path, addDecodeType fails while it is
     * on, as with setMinSumCorrection (both reproduce reference kernels).  The decoders then run the streaming kernels.
     * lastCrcStops(): frames of the last decode() that stopped in a round in which their syndrome was not clean.  A frame
     * stopped with wrong bits that pass the CRC is the undetected error crcPassed() cannot see either; its chance grows
     * with the rounds tested (ldpc_hip.h).  Off by default: without this call every byte is as without it.  Before
     * addDecodeType().  Returns 0 or an ldpc_status. */
    int setCrcEarlyStop(bool on);
    long long lastCrcStops() const { return crcStops; }
    int lastCrcFailures() const { return crcFailures; }
    bool crcPassed(int frame) const { return frame >= 0 && (size_t)frame < crcOk.size() && crcOk[(size_t)frame] != 0; }
    int lastIterations() const { return lastTime; }             /* the reference's "Time=" */
    const char *lastError() const { return err.c_str(); }
    int getNonZeros() const { return nonZeros; }
    int getZ() const { return z; }
    /* H in CSR form, row-major edge order (replaces the Eigen checkMatrix member) */
    const std::vector<int> &hRowRange() const { return rowRange; }
    const std::vector<int> &hRows() const { return rows; }
    const std::vector<int> &hCols() const { return cols; }

private:
    int initCheckMatrix();
    int encodeOnce(const char *src, char *code, int srcLength);
    int decodeFrames(const void *postCode, int llrType, float llrUnit, char *srcCode, int srcLength, enum decodeType deType,
                     float *soft, int kind);
    int fail(int code, const std::string &msg);

    int times;
    float llrScale;
    int device;
    std::vector<int> devices;        /* setDevices(); empty: `device` alone */
    int hostInput = 0;               /* setHostInput() */
    float msScale = 0.0f, msOffset = 0.0f; /* setMinSumCorrection() */
    int msgType = 0;                 /* setMessageType(): LDPC_MSG_F32 */
    int msgBits = 0;                 /* setMessageType(): bits per message with LDPC_MSG_I8 */
    int postBits = 0;                /* setPosteriorBits(): DecodeLayeredFixed, DecodeLayeredBPFixed */
    int fracBits = 0;                /* setLlrFractionBits(): DecodeLayeredBPFixed */
    std::vector<int> bfThreshold;    /* setBitFlipThresholds(): DecodeBitFlip */
    bool fxRecord = false;           /* setFixedRecordKernel(): DecodeLayeredFixed */
    int makeDecoder(const ldpc_decoder_config &cfg, ldpc_decoder **out);
    const signed char *hSeed;
    int seedRowLength;
    int ldpcK, ldpcN, ldpcM, z, nonZeros, batchSize;
    enum rate_type rate;
    bool isEncoder, isDecoder;
    int lastTime;
    std::string err;

    std::vector<int> rows, cols, rowRange;

    /* encoder (structured, replaces the dense Richardson-Urbanke precompute) */
    std::vector<int> shift;          /* [seedRowLength*24] scaled shifts, -1 = empty */
    int encX;                        /* block row of the weight-3 parity column's middle entry */
    std::vector<unsigned char> denseInv; /* fallback: bit-packed inverse of the parity part */
    bool structured;

    bool encodeOnDevice = false;     /* setEncodeOnDevice() */
    int rmE = 0, rmK0 = 0;           /* setRateMatch(); rmE = 0: off */
    ldpc_rate_spec rmSpec = {};
    ldpc_modem_spec modSpec = {};    /* setModulation(); Qm = 0: off */
    ldpc_tb_spec tbSpec = {};        /* setTransportBlock(); A = 0: off */
    ldpc_bch_spec bchSpec = {};      /* setOuterBch(); bchK = 0: off */
    int bchK = 0;                    /* payload bits per frame */
    std::vector<int32_t> bchStatusOfFrame;   /* per frame of the last decode() */
    int bchFailed = 0, bchCorrected = 0, bchBits = 0;
    std::vector<unsigned char> crcOk;/* per frame of the last decode() */
    int crcFailures = 0;
    bool crcEarlyStop = false;       /* setCrcEarlyStop() */
    long long crcStops = 0;
    int applyCrcEarlyStop(ldpc_decoder_config &cfg);
    int frameCount(int kBytes) const { return (kBytes + (ldpcK / 8) - 1) / (ldpcK / 8); }   /* frames of K/8-byte rows */
    int encodeSource(char *srcCode, char *priorCode, int srcLength);
    int encodeFrames(char *srcCode, char *priorCode, int srcLength);
    ldpc_encoder *encoder = nullptr; /* forEncoder() with encodeOnDevice */
    int makeGraph();

    ldpc_graph *graph;
    std::map<int, ldpc_decoder *> decoders; /* decodeType -> handle */
    int cpuDecoderBatch;
    int osdOrder = -1;               /* setOsd(); -1: off */
    ldpc_osd *osd = nullptr;         /* made by the first addDecodeType() while setOsd() is in force */
    int osdProcessed = 0, osdFlipped = 0;
};

float gaussian(float ave, float sd);

#endif /* MYLDPC_H_ */
