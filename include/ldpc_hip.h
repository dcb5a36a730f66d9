/*
 * ldpc_hip.h -- C ABI of libldpc_hip.so: batched LDPC belief-propagation decoding
 * on AMD MI355X (gfx950), hand-written HIP kernels.
 *
 * This is the drop-in boundary for the decode hot path of wing02/MyLdpcCppApi.
 * The reference has no FFI layer: its boundary is the C++ class `Coder`
 * (MyLdpc.h:104-238) whose decode() (MyLdpc.cpp:571-618) drives OpenCL kernels
 * (decodeCL.c).  Each entry point below names the reference interface it
 * replaces.  include/MyLdpc.h + csrc/MyLdpc.cpp re-create `Coder` on top of this
 * ABI; INTEGRATION.md shows the binding.
 *
 * Conventions (all taken from the reference):
 *   - H is given as its nonzeros in ROW-MAJOR order; edge id = rank in that
 *     order (MyLdpc.cpp:186-219).  fp32 reductions follow the reference's
 *     orders: ascending edge id along a row and along a column.
 *   - channel values `llr`: N floats per frame, frame-major, +1 <-> bit 0,
 *     -1 <-> bit 1 (MyLdpc.cpp:1066-1069).
 *   - output: the first K hard bits of every frame, LSB-first
 *     (decodeCL.c:188-199 / MyLdpc.cpp:765-774).
 *   - every function returns 0 on success (LDPC_SUCCESS == 0, MyLdpc.h:24) and
 *     a positive LDPC_ERR_* code otherwise; it never exits the process
 *     (the reference calls exit(0), MyLdpc.cpp:243-254).  ldpc_last_error()
 *     returns the message of the calling thread's last failure.
 *   - a decoder handle is not re-entrant (neither is Coder, MyLdpc.h:184-236):
 *     one handle per host thread / stream.
 *
 * There is no CPU fallback: without a usable HIP device every compute entry
 * point fails with LDPC_ERR_HIP.
 */
#ifndef LDPC_HIP_H_
#define LDPC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_HIP_ABI_VERSION 3   /* 2: tuning fields in the config (were reserved[8]), device lists;
                                    3: host_input / host_copy_threads replace the experimental `streams` */

enum ldpc_status {
    LDPC_OK = 0,
    LDPC_ERR_ARG = 1,         /* bad argument (message says which)            */
    LDPC_ERR_HIP = 2,         /* HIP runtime error / no device                */
    LDPC_ERR_NOMEM = 3,
    LDPC_ERR_UNSUPPORTED = 4, /* valid request this build cannot serve        */
    LDPC_ERR_STATE = 5        /* call order / handle misuse                   */
};

/* decodeType of the reference (MyLdpc.h:37-39) maps as:
 *   DecodeSP                 -> LDPC_ALGO_SP       (decodeCL.c:3-108)
 *   DecodeMS, DecodeCPU      -> LDPC_ALGO_MS       (decodeCL.c:113-186, MyLdpc.cpp:684-784)
 *   DecodeTDMPCL             -> LDPC_ALGO_LAYERED  (the fused kernel, decodeCL.c:307-426)
 *   DecodeTDMP               -> LDPC_ALGO_LAYERED_HOST where the reference's host-layered path is
 *                               well defined (all rows of H of one weight), else LDPC_ALGO_LAYERED
 *   DecodeMSCL               -> LDPC_ALGO_MS_FUSED (decodeCL.c:432-567) */
enum ldpc_algo {
    LDPC_ALGO_SP = 0,      /* flooding sum-product, probability domain, fp32     */
    LDPC_ALGO_MS = 1,      /* flooding min-sum, fp32                             */
    LDPC_ALGO_LAYERED = 2, /* layered (TDMP) min-sum                             */
    LDPC_ALGO_MS_FUSED = 3,/* flooding min-sum with the arithmetic of the fused kernel
                              decodeOnceMS (DecodeMSCL, decodeCL.c:432-567): short
                              quasi-cyclic codes only, whole decode in LDS; the reference
                              hard-codes max_iter = 120 there                            */
    LDPC_ALGO_LAYERED_HOST = 4,/* layered min-sum as the reference's HOST drives it (DecodeTDMP,
                              MyLdpc.cpp:889-976 over decodeCL.c:203-300): check node of the MS
                              kernel chain, three-way hard decision once per iteration.  The
                              reference mis-sizes its layers unless every row of H has the same
                              weight (MyLdpc.cpp:907,958): any other H is LDPC_ERR_UNSUPPORTED.
                              fp32, one launch per layer                                    */
    LDPC_ALGO_BP = 5,      /* flooding sum-product in the LOG domain (box-plus check node): this library's own
                              definition, below; streaming kernels, fp32 or LDPC_MSG_F16 messages              */
    LDPC_ALGO_LAYERED_BP = 6,/* layered (TDMP) schedule with LDPC_ALGO_BP's box-plus check node: this library's own
                              definition, below; the streaming layered engine, fp32, one launch per layer    */
    /* The value 7 is not assigned and stays "unknown algo" (LDPC_ERR_ARG): callers and tests of the library have used it as
     * their example of an unknown algorithm since LDPC_ALGO_LAYERED_BP, and what was refused stays refused. */
    LDPC_ALGO_LAYERED_FX = 8,/* layered (TDMP) min-sum in fixed point: q-bit messages (LDPC_MSG_I8, msg_bits) and a
                              posterior MEMORY of post_bits bits that saturates: this library's own definition, below;
                              the streaming layered engine, one byte per R and two per P, one launch per layer */
    LDPC_ALGO_LAYERED_BP_FX = 9,/* LDPC_ALGO_LAYERED_FX's schedule, widths and storage with a box-plus check node in integers:
                              min plus a correction read from a table of bp_frac_bits fractional bits, as hardware box-plus
                              decoders compute it: this library's own definition, below */
    LDPC_ALGO_BITFLIP = 10  /* hard-decision parallel bit flipping: one bit per code bit in, one bit per variable and per
                              check as state, frames bit-sliced 64 to a word: this library's own definition, below */
};

/* LDPC_ALGO_BP, bit for bit.  The reference's sum-product (LDPC_ALGO_SP) works on probabilities in fp32 and saturates at
 * practical SNRs; this is the same algorithm on log-likelihood ratios, which does not, with a one-line stand-in for the
 * exact correction term.  It is min-sum's variable node with another check node.  Every operation is fp32, one at a
 * time, no contraction.
 *   Channel:      chan[n] = llr_scale * y[n], one multiply (rounded to binary16 with LDPC_MSG_F16).  It is the y_n of the
 *                 posterior and of the soft-output rule.  exp(llr_scale * y) is SP's likelihood ratio, so llr_scale * y is
 *                 the LLR: for BPSK +-1 in noise of standard deviation sd, llr_scale = 2 / sd^2.  Padding frames read
 *                 y = 1.  llr_scale NaN, inf or <= 0: LDPC_ERR_ARG.
 *   Row inputs:   x_0 .. x_{D-1}, the variable->check messages of the row in ascending edge id, are read as
 *                     a_j = fminf(|x_j|, 1000.0f),  s_j = (x_j < 0),  t_j = s_j ? -a_j : a_j
 *                 so NaN reads +1000 (fminf drops it, its sign is +), -0 reads +0 and +-inf read +-1000 (min-sum's start
 *                 value).
 *   Correction:   c(x) = fmaxf(0.6931472f - 0.25f * x, 0.0f)       (the float nearest ln 2, 0x3F317218)
 *   Box-plus:     m = fminf(|u|, |v|),  S = |u| + |v|,  D = fabsf(|u| - |v|),
 *                 g = fmaxf((m + c(S)) - c(D), 0.0f),  u [+] v = ((u < 0) != (v < 0)) ? -g : g
 *                 It is bitwise commutative and |u [+] v| <= min(|u|, |v|); it is NOT associative, so the association is
 *                 part of the definition:
 *   Row, D >= 3:  forward  f_0 = t_0,          f_j = f_{j-1} [+] t_j   for j = 1 .. D-2
 *                 backward b_{D-1} = t_{D-1},  b_j = t_j [+] b_{j+1}   for j = D-2 .. 1
 *                 out_0 = b_1,  out_{D-1} = f_{D-2},  out_k = f_{k-1} [+] b_{k+1} otherwise.
 *   Short rows:   D = 2: out_0 = t_1, out_1 = t_0.  D = 1: out_0 = +1000.0f.
 *   Rounding:     R_k = out_k, with LDPC_MSG_F16 rounded to binary16 where it is PRODUCED (in registers too).
 *   Everything else is LDPC_ALGO_MS's: the posterior chan + R_e1 + R_e2 + ... in ascending edge id, bit = !(P > 0),
 *   Q = P - R rounded where stored, freezing, iters, the CRC rule, both soft kinds.  With c == 0 the definition is
 *   flooding min-sum.
 * It always runs the streaming flooding engine: layer_rows is accepted and ignored for the choice, the one-launch and
 * record kernels are never selected (LDPC_TUNE_ON(FUSED) or LDPC_TUNE_ON(LDSP): LDPC_ERR_UNSUPPORTED), as are
 * LDPC_MSG_F8 and a non-zero ms_scale / ms_offset (there is no minimum to correct). */

/* LDPC_ALGO_LAYERED_BP, bit for bit: the schedule and the bookkeeping of LDPC_ALGO_LAYERED with the row of LDPC_ALGO_BP.
 * Every operation is fp32, one at a time, no contraction.
 *   Channel:      chan[n] = llr_scale * y[n], one multiply.  Padding frames read y = 1.  llr_scale NaN, inf or <= 0:
 *                 LDPC_ERR_ARG.
 *   Start:        P = chan, R = 0; the initial bits are chan < 0.
 *   Row update:   for a row of layer l with edges e0 .. e0+D-1 in ascending edge id
 *                     q_k = P[col_k] - R_k
 *                     out = the row of LDPC_ALGO_BP (above) applied to x_k = q_k: the clamp t_k on input, the same
 *                           forward / backward association, D = 2 and D = 1 as there, no storage rounding
 *                     R_k = out_k,  P[col_k] = q_k + R_k          (q_k as formed, not clamped)
 *   Rounds:       layers in order; the rows of a layer are independent (a layer whose rows share a column is refused).
 *   After the last layer of round i: bit = (P < 0), kept current with every write of P; syndrome, freeze rule, iters and
 *                 the CRC rule exactly as for LDPC_ALGO_LAYERED.
 *   Soft output:  posterior = P after the last layer of the round the frame stopped in (an LLR); extrinsic = that minus
 *                 chan[n], where chan[n] is the fp32 product formed first, then one subtraction (never one fma).
 *   Debug taps:   0 = R, 2 = P, 3 = bits.
 * A row takes its sign from (x < 0) and never multiplies messages, so -- unlike LDPC_ALGO_LAYERED, whose running fp32
 * sign product one exact 0 kills -- it takes exact zeros as the flooding decoders do (see erasure_llr below).
 * Refusals: layer_rows is required (<= 0 or not dividing M: LDPC_ERR_ARG, as for LAYERED).  LDPC_MSG_F16 and LDPC_MSG_F8
 * are LDPC_ERR_UNSUPPORTED (the layered engine is fp32), as is a non-zero ms_scale / ms_offset.  It always runs the
 * streaming layered engine: the LDS-resident and record kernels are never selected (the 16-byte check record holds two
 * minima and cannot hold D independent messages); LDPC_TUNE_ON(FUSED) or LDPC_TUNE_ON(LDSP) is LDPC_ERR_UNSUPPORTED.
 * crc_kind, early termination on and off, both pack modes, ldpc_decode, ldpc_decode_soft and ldpc_decoder_create_multi
 * work as for LDPC_ALGO_LAYERED. */

/* LDPC_ALGO_LAYERED_FX, bit for bit, in integers: the layered decoder a hardware team builds for a QC code.  In the
 * flooding rule of LDPC_MSG_I8 (below) the posterior is recomputed every round in an accumulator that never saturates; in
 * the layered schedule the posterior IS the state: it lives in a memory of p bits and saturates, and P - R_old is formed
 * from the saturated P.
 *   Configuration: msg_dtype = LDPC_MSG_I8 (any other: LDPC_ERR_ARG); msg_bits = q one of 4, 5, 6, 8 (0 = 8),
 *                 L = 2^(q-1) - 1; post_bits = p with q <= p <= 16 (0 = 16), LP = 2^(p-1) - 1, anything else
 *                 LDPC_ERR_ARG; layer_rows required and dividing M, layers column-disjoint, as for LDPC_ALGO_LAYERED;
 *                 llr_scale finite and > 0 (LDPC_ERR_ARG otherwise): the LSBs per unit of channel value.  sq is the store
 *                 rule of LDPC_MSG_I8: sq(x) = clamp(rintf(x), -L, L), ties to even, NaN gives 0, +-inf give +-L.
 *   Start:        c[n] = sq(llr_scale * y[n]), one fp32 multiply; padding frames read y = 1.  The channel has q bits, as
 *                 in flooding.  P[n] = c[n], R = 0, bit = (c < 0).
 *   Row of a layer, edges e0 .. e0+D-1 in ascending edge id:
 *                 t_k = P[col_k] - R_k                         exact, not clamped
 *                 x_k = clamp(t_k, -L, L)                      the variable->check message
 *                 the check row of LDPC_MSG_I8 on x_0 .. x_{D-1}: sign = XOR of (x_k < 0), so a zero counts as positive
 *                   and does not kill the row; the two smallest |x_k| from the start value 1000, which reads L (a
 *                   degree-1 row gives L); with ms_scale / ms_offset each of the two candidates, the start value
 *                   among them as in LDPC_MSG_I8, becomes
 *                   m' = fminf(truncf(fmaxf(m - ms_offset, 0) * ms_scale), L), fp32, in this order (ms_scale 0 meaning 1;
 *                   ms_scale = 0.75 is exactly (3m) >> 2); edge k takes the second minimum iff it holds the first
 *                 R_k = that message
 *                 P[col_k] = clamp(t_k + R_k, -LP, LP)         from the UNCLAMPED t_k: only the posterior memory saturates
 *                 bit = (P[col_k] < 0), kept current with every write; frozen frames keep theirs.
 *   Rounds:       rounds, syndrome, freezing, iters, the CRC rule and both pack modes are LDPC_ALGO_LAYERED's, with
 *                 early_term 0 or 1.
 *   Soft output:  P after the last layer of the round the frame stopped in, in LSBs as fp32; extrinsic: P - c.
 *   Debug taps:   0 = R, 2 = P, 3 = bits, as floats.
 * Properties: with p = 16 and (1 + column degree) * 127 <= 32767 the posterior never saturates, and the rule is the
 * plain layered schedule on integers.  The kernels compute in fp32 on integers far below 2^24, which is exact.
 * Refusals, all before the device is touched: the LDPC_ERR_ARG cases above, and LDPC_TUNE_ON(FUSED) or LDPC_TUNE_ON(LDSP)
 * is LDPC_ERR_UNSUPPORTED: it runs the streaming layered engine unless LDPC_TUNE_FX_RECORD is on (below).  post_bits != 0
 * with any other algorithm is LDPC_ERR_ARG.  LDPC_ALGO_LAYERED with LDPC_MSG_I8 stays LDPC_ERR_UNSUPPORTED: a different rule with different state is an
 * algorithm of its own here, as LAYERED_HOST and LAYERED_BP are.  ldpc_decode, ldpc_decode_device, ldpc_decode_soft*,
 * ldpc_decode_typed*, ldpc_decoder_create_multi, the debug taps, crc_kind and kernel times (spans named lfx) work as
 * for LDPC_ALGO_LAYERED.
 *   LDPC_TUNE_ON(LDPC_TUNE_FX_RECORD): the same rule, bit for bit, in one launch on the record organisation of
 *                 LDPC_ALGO_LAYERED (layered_ldsp_fx_kernel): a persistent workgroup per frame, the posteriors of the block
 *                 columns met by two or more layers as int16 in LDS, and per row and layer one 8-byte record that only the
 *                 row's own lane reads and writes:
 *                   word 0: signs of R_0 .. R_{D-1} in bits 0 .. 23, argmin in bits 24 .. 28
 *                   word 1: m1' in bits 0 .. 7, m2' in bits 8 .. 15 (the two magnitudes after correction and the clamp to
 *                           L), the int16 posterior of the row's single-layer column in bits 16 .. 31
 *                 R_k = (sign_k ? -1 : 1) * (k == argmin ? m2' : m1').  A magnitude of 0 makes the sign immaterial; among
 *                 entries that tie for the minimum m1' = m2', so the argmin kept does not matter.
 *                 Off by default; the automatic choice stays the streaming engine.  Refusals, before the device is touched:
 *                 with LDPC_ALGO_LAYERED_BP_FX it is LDPC_ERR_UNSUPPORTED (a box-plus row sends D independent messages,
 *                 which two minima cannot hold); with crc_kind != 0 it is LDPC_ERR_UNSUPPORTED.  A code the kernel cannot
 *                 serve -- not quasi-cyclic at layer_rows, a row of more than 24 entries, posteriors beyond the LDS limit,
 *                 LDPC_PACK_BITS with K % 8 != 0 -- decodes on the streaming engine with the same result.  Every entry
 *                 point, early_term 0 or 1, soft output and the debug taps work as without it; the kernel time is one span
 *                 named layered_ldsp_fx_kernel[grid x block, frames per workgroup].  tune_ldsp_grid, the per-CU and waves
 *                 fields of tune_ldsp_shape and LDPC_TUNE_LDSP_EXT act as on the float record kernel; LDPC_TUNE_LDSP_PACK
 *                 is ignored (circulants of <= 32 rows run one frame per one-wave workgroup). */

/* LDPC_ALGO_LAYERED_BP_FX, bit for bit, in integers: LDPC_ALGO_LAYERED_FX with the check node of LDPC_ALGO_LAYERED_BP, the
 * way a hardware box-plus decoder computes it: the minimum plus a small correction read from a table.
 *   Configuration: as for LDPC_ALGO_LAYERED_FX -- msg_dtype = LDPC_MSG_I8, msg_bits = q one of 4, 5, 6, 8 (0 = 8),
 *                 L = 2^(q-1) - 1, post_bits = p with q <= p <= 16 (0 = 16), LP = 2^(p-1) - 1, layer_rows required and
 *                 dividing M, layers column-disjoint, llr_scale finite and > 0, each LDPC_ERR_ARG otherwise -- and one
 *                 field more: bp_frac_bits = f, 0 <= f <= 4 (anything else: LDPC_ERR_ARG).  One LSB is 2^-f LLR units, and
 *                 the caller chooses llr_scale so that llr_scale * y is the channel LLR in LSBs: for BPSK +-1 in noise of
 *                 standard deviation sd, llr_scale = 2^f * 2 / sd^2.
 *   Table:        T_f[d] = (int)floor(2^f * log(1 + exp(-d / 2^f)) + 0.5) for d = 0, 1, ..., computed in double on the host
 *                 once per decoder and cut at the first d where it is 0; T_f[d] = 0 beyond.  T_0 = {1, 0}; T_4 has 57
 *                 entries, the largest is T_4[0] = 11.  ldpc_bp_fx_table() returns the table the kernels use.
 *   Box-plus:     for integers a, b in [-L, L]
 *                     s = (a < 0) XOR (b < 0)                      a zero counts as positive, as in LDPC_ALGO_LAYERED_FX
 *                     m = min(|a|, |b|)
 *                     g = max(0, m + T[|a| + |b|] - T[||a| - |b||])
 *                     a [+] b = s ? -g : g
 *                 T does not increase, so g <= m <= L: nothing needs clamping.  It is commutative and not associative, so
 *                 the association is part of the definition:
 *   Row, D >= 2:  on x_0 .. x_{D-1} in ascending edge id
 *                     forward  F_0 = x_0,          F_k = F_{k-1} [+] x_k
 *                     backward B_{D-1} = x_{D-1},  B_k = x_k [+] B_{k+1}
 *                     R_0 = B_1,  R_{D-1} = F_{D-2},  R_k = F_{k-1} [+] B_{k+1} otherwise
 *                 (D = 2: R_0 = x_1, R_1 = x_0.)
 *   Row, D = 1:   R_0 = +L.  LDPC_ALGO_LAYERED_BP gives a degree-1 row +1000.0f, min-sum's start value; here it reads L, as
 *                 the start value does in LDPC_ALGO_LAYERED_FX.
 *   Schedule:     LDPC_ALGO_LAYERED_FX's: c = sq(llr_scale * y), P = c, R = 0; t_k = P[col_k] - R_k exact;
 *                 x_k = clamp(t_k, -L, L); R_k from the row above; P[col_k] = clamp(t_k + R_k, -LP, LP) from the unclamped
 *                 t_k; bit = (P[col_k] < 0) kept current with every write.  Rounds, syndrome, freezing, iters, the CRC rule,
 *                 both pack modes, typed input, soft output (P, or P - c, in LSBs as fp32), the debug taps, the host path
 *                 and device lists are LDPC_ALGO_LAYERED_FX's.
 * Properties: a [+] 0 = 0, and with an all-zero table the row is LDPC_ALGO_LAYERED_FX's plain min-sum row.  The sign of
 * every non-zero R_k is the XOR of (x_j < 0) over j != k, as in min-sum.
 * Refusals, all before the device is touched: the LDPC_ERR_ARG cases of LDPC_ALGO_LAYERED_FX and bp_frac_bits outside
 * 0 .. 4; a non-zero ms_scale or ms_offset is LDPC_ERR_UNSUPPORTED (there is no minimum to correct), as is
 * LDPC_TUNE_ON(FUSED) or LDPC_TUNE_ON(LDSP).  bp_frac_bits != 0 with any other algorithm is LDPC_ERR_ARG.  Kernel times
 * name its spans lbfx. */

/* LDPC_ALGO_BITFLIP, bit for bit, in integers: the hard-decision decoder a storage controller or an optical link runs
 * first.  Nothing in it is a float after the first comparison.
 *   Input:        r_n = (y_n < 0): NaN and -0 read 0.  With typed input the test is on y = (float)x * llr_unit, so the sign
 *                 of the stored value decides.  llr_scale is ignored.  Padding frames read y = 1.
 *   State:        x_n, starting as r_n; r_n is kept.  d_n is the degree of column n.
 *   Round i = 1 .. max_iter:
 *                 s_m = XOR of x over row m.
 *                 A frame whose s is all zero is done: frozen, iters = i - 1 (a frame that arrives as a codeword has
 *                 iters = 0).  This is the freeze rule of the other decoders; early_term = 0 launches every round on every
 *                 tile and changes no bit, iteration count or done flag: a done frame stays frozen either way.
 *                 Otherwise, for every column: u_n = sum of s_m over the rows m of column n, E_n = u_n + (x_n != r_n),
 *                 hit_n = (E_n >= T(d_n, i)).
 *                 A frame with a hit in some column flips x_n in exactly its hit columns.  A frame without a hit flips the
 *                 columns whose E_n is the frame's largest, if that largest E is >= 2.  All flips of a round are decided
 *                 from the same s: parallel flipping.
 *   Threshold:    T(d, i) = max(floor((d + 1) / 2) + 1, d + 1 - off(i)): of the d + 1 votes on a bit (its d checks and the
 *                 received bit) all must disagree at off = 0, one fewer per unit of off, never fewer than a strict
 *                 majority.  With bf_threshold (config field below) all zero, off(i) = i - 1.  Otherwise
 *                 off(i) = bf_threshold[i - 1] for i <= 16 and bf_threshold[15] for every later round: entry j is the
 *                 offset of round j + 1.  Entries must lie in [0, 62] (LDPC_ERR_ARG otherwise, as is a non-zero entry
 *                 with any other algorithm); bf_threshold = {62, 62, ...} is strict majority from round 1.
 *   After the last round: iters = max_iter for the frames not done (the bits of round max_iter are not tested again), the
 *                 output bits are x, frames_converged counts the done frames.
 *   crc_kind:     in round i a running frame whose x[0 .. crc_bits) passes the CRC is done as if its s were zero
 *                 (iters = i - 1); ldpc_decoder_crc_stops counts those whose s was not.  Needs early_term = 1, as always.
 *   Debug taps:   3 = x after the tapped round, 0 = the syndrome words s of the tapped round, M values per frame as
 *                 floats 0 / 1 (ldpc_decoder_dump with count = frames * M).
 * Why the fall-back: on the 802.16e rate-1/2 codes over a binary symmetric channel the thresholds alone leave 86 of 512
 * frames at N = 576 and crossover 0.01 (strict majority from round 1: 85; only the largest E in every round: 28); with the
 * fall-back 29 are left, in fewer rounds than the largest-E rule needs (DESIGN.md section 8v has the table).
 * Served: both pack modes, ldpc_decode, ldpc_decode_device, the typed entry points, crc_kind, ldpc_decoder_create_multi.
 * Refusals, all before the device is touched: soft output (ldpc_decode_soft*: there is none) is LDPC_ERR_UNSUPPORTED, as
 * are a msg_dtype other than LDPC_MSG_F32 (there are no messages), a non-zero ms_scale / ms_offset and
 * LDPC_TUNE_ON(FUSED) or LDPC_TUNE_ON(LDSP); LDPC_TUNE_FX_RECORD is LDPC_ERR_ARG as with every algorithm it does not belong
 * to.  A column of degree above 62 is LDPC_ERR_UNSUPPORTED (E must fit six bits).  frames_per_lane is accepted and ignored: tiles
 * are 64 frames.  Hand-over and tail compaction are switched off for this algorithm (poll_interval and tune_compact are
 * accepted and ignored): a round is too cheap to be worth moving frames for.  Kernel times name bitflip_check_kernel,
 * bitflip_vote_kernel and bitflip_flip_kernel. */

/* How the streaming flooding min-sum decoder (LDPC_ALGO_MS) stores its messages; the arithmetic is fp32 in one
 * operation order for all four.  F16 and F8 are this library's own definitions (the reference is fp32 only) and are
 * LDPC_ERR_UNSUPPORTED with every other algorithm (LDPC_ALGO_LAYERED_BP included: the layered engine is fp32) -- except that LDPC_ALGO_BP takes F16 (not F8); the one-launch and record kernels are fp32 and are never selected
 * for them (F8 with LDPC_TUNE_FUSED / LDPC_TUNE_LDSP forced on: LDPC_ERR_UNSUPPORTED).  An unknown value: LDPC_ERR_ARG.
 *   LDPC_MSG_F16: channel values and variable->check messages are rounded to binary16 (nearest even) where they are
 *     stored, a corrected check->variable magnitude (ms_scale / ms_offset) where it is produced.
 *   LDPC_MSG_F8: one byte per message, OCP E4M3 ("e4m3fn": 1-4-3, bias 7, subnormals down to 2^-9, no infinities).
 *     s8(x) for fp32 x: NaN stays NaN; anything else is clamped to [-448, 448] and then rounded to the nearest E4M3
 *     value, ties to the even code, the sign of zero kept (so 464, 1000 and +inf give 448, 2^-10 gives 0, 1.5 * 2^-10
 *     gives 2^-9, -1e-8 gives -0).  Loads widen exactly.  s8 is applied to the channel values where they are stored
 *     (y8 = s8(y); round 1 reads them as Q), to the variable->check messages where they are stored, and to the
 *     check->variable message where it is PRODUCED, in registers too: corrected, s8(fmaxf(m - ms_offset, 0) * ms_scale);
 *     plain, every |q| is an E4M3 value already and only the start value 1000 is affected, which reads 448.  The
 *     posterior -- hard decision and soft output alike -- is y8 + R_e1 + R_e2 + ... in fp32, ascending edge id.
 *   LDPC_MSG_I8: fixed point, the datapath of a hardware decoder: saturating q-bit integers, q = msg_bits (config field
 *     below) one of 4, 5, 6, 8; 0 means 8, any other value is LDPC_ERR_ARG, as is a non-zero msg_bits with another
 *     msg_dtype.  L = 2^(q-1) - 1, that is 7, 15, 31 or 127.  A message is a two's-complement byte holding an integer in
 *     [-L, L]; the code -128 is never produced; the zero message is the byte 0x00.  LDPC_ALGO_MS, and LDPC_ALGO_LAYERED_FX
 *     and LDPC_ALGO_LAYERED_BP_FX with the rules of their own above (every other algorithm: LDPC_ERR_UNSUPPORTED); the one-launch and record kernels are never selected (forcing them:
 *     LDPC_ERR_UNSUPPORTED, as for F8).  The kernels compute in fp32, which on integers below 2^24 is exact integer
 *     arithmetic, so the rule can be restated in integers alone:
 *       Store rule:  sq(x) = clamp(rintf(x), -L, L): ties go to even, NaN gives 0, +-inf gives +-L.
 *       Channel:     c[n] = sq(llr_scale * y[n]), one fp32 multiply.  llr_scale is here the number of LSBs per unit of
 *                    channel value; it must be finite and > 0, else LDPC_ERR_ARG.  With typed input (ldpc_decode_typed),
 *                    y = (float)x * llr_unit as always, so int8 input with llr_unit = 1 and llr_scale = 1 goes straight
 *                    through.  Padding frames read y = 1.  Round 1 reads c as Q, as fp8 does.
 *       Check row, plain:  min-sum on the stored integers; the start value 1000 reads L, so a degree-1 row gives L.
 *       Check row, corrected (ms_scale / ms_offset): each of the two candidates becomes
 *                    m' = fminf(truncf(fmaxf(m - ms_offset, 0) * ms_scale), L), in fp32 and in this order, where the value
 *                    is PRODUCED, in registers too.  With ms_scale = 0.75 this is exactly (3m) >> 2.  ms_offset is in
 *                    LSBs and need not be an integer.
 *       Posterior:   P = c + R_e1 + R_e2 + ... in ascending edge id: exact, an accumulator wide enough never to saturate.
 *       Bits and messages out:  bit = !(P > 0);  Q = sq(P - R) where stored (only the clamp acts).
 *       Soft output: P, or P - c, in LSBs as fp32.
 *     Freezing, iters, the CRC rule, both pack modes and the debug taps are LDPC_ALGO_MS's. */
/* The value 3 is not assigned and stays LDPC_ERR_ARG: callers and tests of the library have used it as their example of
 * an unknown msg_dtype since LDPC_MSG_F8, and what was refused stays refused. */
enum ldpc_msg_dtype { LDPC_MSG_F32 = 0, LDPC_MSG_F16 = 1, LDPC_MSG_F8 = 2, LDPC_MSG_I8 = 4 };

/* ldpc_decode() and the caller's input buffer (the reference copies it with a blocking
 * enqueueWriteBuffer, MyLdpc.cpp:796 / :988).
 *   STAGED (the default): the library never hands the caller's pageable memory to the HIP runtime and
 *     never changes its page state.  Worker threads owned by the handle copy each launch group, 8 MiB
 *     at a time, into a ring of the library's own pinned buffers, from which it is DMA-copied to the
 *     device while the previous group decodes.
 *   LOCK_PAGES (opt-in): groups larger than 4 MiB are page-locked where they lie (hipHostRegister) for the
 *     duration of the call and DMA-read in place: no CPU copy (worth it for long streams of cheap
 *     decodes, where the CPU copy is slower than the decode).  Whole pages strictly inside the call's
 *     own byte range only; every range is recorded process-wide, released before the call returns, and a
 *     range that cannot be released makes the call -- and ldpc_decoder_destroy -- fail.  A group whose
 *     pages cannot be locked (another call of this library holds them) is staged instead.
 * In both modes groups of up to 4 MiB are copied by the calling thread into pinned scratch. */
enum ldpc_host_input { LDPC_HOST_INPUT_AUTO = 0, LDPC_HOST_INPUT_STAGED = 1, LDPC_HOST_INPUT_LOCK_PAGES = 2 };

enum ldpc_pack_mode {
    LDPC_PACK_BYTES = 0, /* toChar, decodeCL.c:188-199: K/8 whole bytes per frame at (frame*K)/8 */
    LDPC_PACK_BITS = 1   /* decodeCPU, MyLdpc.cpp:765-774: bit i of frame b at bit b*K+i         */
};

typedef struct ldpc_graph ldpc_graph;
typedef struct ldpc_decoder ldpc_decoder;

typedef struct ldpc_decoder_config {
    uint32_t struct_size;   /* = sizeof(ldpc_decoder_config); ABI guard                    */
    int32_t K;              /* information bits per frame (ldpcK)                          */
    int32_t max_batch;      /* frames per launch group (forDecoder's batchSize)            */
    int32_t algo;           /* enum ldpc_algo                                              */
    int32_t msg_dtype;      /* enum ldpc_msg_dtype                                         */
    int32_t max_iter;       /* `times`, MyLdpc.cpp:24 (reference: 40)                      */
    float llr_scale;        /* SP: q = exp(llr_scale*y)..., decodeCL.c:9 (reference: 8); BP: chan = llr_scale * y, the
                               LLR (> 0 and finite, else LDPC_ERR_ARG); ignored by the min-sum algorithms -- except with
                               LDPC_MSG_I8: the LSBs per unit of channel value, c = sq(llr_scale * y) (> 0 and finite) */
    int32_t early_term;     /* 1: frames freeze when their syndrome is clean (reference
                               behaviour, decodeCL.c:27,48-49); 0: always run max_iter      */
    int32_t device;         /* HIP device ordinal                                          */
    int32_t layer_rows;     /* rows per layer = circulant size z.  Required for LDPC_ALGO_LAYERED / LAYERED_BP / MS_FUSED; with
                               SP / MS it lets the one-launch kernels for quasi-cyclic codes apply (0: streaming) */
    int32_t pack_mode;      /* enum ldpc_pack_mode                                         */
    int32_t frames_per_lane;/* tuning: 0 = auto, else 1, 2 or 4 (tile = 64*frames_per_lane) */
    int32_t poll_interval;  /* early_term: host checks "all frames done" every this many
                               iterations (0 = never; finished tiles still skip on device).
                               With polling on, the last running frames of a multi-tile batch
                               (at most a quarter of it, and <= 1024 frames for max_batch >=
                               4096, <= 512 otherwise) are handed to a small child decoder
                               (tail compaction)                                              */
    /* ---- tuning (was reserved[8]): 0 = automatic everywhere.  Kernel selection and launch
     *      shapes only -- results never depend on these (the parity tests run the alternatives
     *      against each other).  The library reads NO environment variables. ---------------- */
    int32_t tune_flags;         /* LDPC_TUNE_* two-bit fields below: 0 auto, 1 force on, 2 force off */
    int32_t tune_rows_per_wave; /* check kernels: rows per wave                                   */
    int32_t tune_cols_per_wave; /* variable kernels: columns per wave                             */
    int32_t tune_link_rows;     /* rows per wave of the column-fused check kernel (default 16; 4 for a
                                   single tile); -1 = column-local fusion off                     */
    int32_t tune_compact;       /* tail compaction: hand over when <= this many frames still run
                                   (default and maximum: 1024 for max_batch >= 4096, 512
                                   otherwise); -1 = off                                           */
    int32_t tune_ldsp_grid;     /* record kernels (ldsp_kernels.hpp): persistent workgroups        */
    int32_t tune_ldsp_shape;    /* workgroups per CU | waves per workgroup << 8                    */
    int32_t tune_place;         /* streaming flooding decoders: fresh allocations tried for the check->variable and for
                                   the variable->check array when the decoder is created (one message round is timed with
                                   each; the fastest combination is kept, the others are released).  WHICH allocations
                                   lie behind these two arrays decides between speeds of the streaming check kernel that
                                   differ by up to 19 % and last as long as the allocations.
                                   0 = automatic (up to 6 per array when the arrays hold at least 256 MiB and memory
                                   allows; after four measurements a stage stops once it has seen the fast speed next to the slow one), 1 = take the first allocations
                                   as they come, 2..8 = that many per array                              */
    int32_t host_input;         /* enum ldpc_host_input: how ldpc_decode() moves the caller's pageable channel
                                   values to the device (memory the caller has page-locked itself is always
                                   copied from directly)                                               */
    int32_t host_copy_threads;  /* LDPC_HOST_INPUT_STAGED: CPU threads that copy a launch group into the
                                   library's pinned ring (0 = automatic: 4; 1..16).  They belong to the
                                   handle: started on its first large host-buffer call, joined when it is
                                   destroyed                                                           */
    int32_t tune_q_order;       /* streaming flooding decoders: the variable->check array is stored in the order its
                                   writers produce it (variable-node kernels column by column), so that every store
                                   of a round streams and the check kernels gather their inputs instead
                                   (0 = automatic: on; 1 = on; -1 = off: edge order, as the check->variable array) */
    /* ---- normalized / offset min-sum (appended; a struct_size of offsetof(ldpc_decoder_config, ms_scale), the
     *      size before these fields, is accepted and means both off).  Each of a check row's two magnitude
     *      candidates m (the two smallest |q|) becomes
     *          m' = fmaxf(m - ms_offset, 0) * ms_scale        (fp32, in this order)
     *      once per row and frame, before the per-edge selection and sign; with LDPC_MSG_F16 the result is
     *      rounded to fp16 where it is produced.  ms_offset is in the units of the channel values passed to
     *      ldpc_decode (with the reference's convention, BPSK +-1 plus noise: units of y, not of LLRs): offset
     *      min-sum depends on the scale of the input, normalized min-sum does not.
     *      LDPC_ALGO_MS and LDPC_ALGO_LAYERED only (others, LDPC_ALGO_BP and LDPC_ALGO_LAYERED_BP among them: LDPC_ERR_UNSUPPORTED when either is
     *      non-zero).  The
     *      record kernels and the streaming kernels carry the correction; the LDS-resident one-launch kernels do
     *      not and are not selected (forcing them, LDPC_TUNE_ON(FUSED) with LDPC_TUNE_OFF(LDSP):
     *      LDPC_ERR_UNSUPPORTED).  NaN, inf or a value out of range: LDPC_ERR_ARG. ----------------------------- */
    float ms_scale;             /* alpha: 0 = off (factor 1), else 0 < alpha <= 1                            */
    float ms_offset;            /* beta: 0 = off, else 0 < beta < 1000                                        */
    /* ---- CRC-aided early termination (appended; a struct_size of offsetof(ldpc_decoder_config, crc_kind), the size
     *      before these fields, is accepted and means off).  A receiver whose frames carry a CRC (ldpc_tb_frame_crc) can
     *      stop a frame as soon as its information bits pass it, usually a round before the syndrome is clean: parity
     *      and punctured columns converge last.  With crc_kind != 0, after the variable-node phase of round i = 1, 2, ...
     *      (layered: after the last layer) has produced the hard bits b_i(f, .) of every running frame f:
     *          clean_i(f): the syndrome of b_i(f, .) is zero                                   (the rule without a CRC)
     *          crc_i(f):   b_i(f, 0 .. crc_bits-1) leave remainder zero under the polynomial of crc_kind, conventions of
     *                      ldpc_crc_bits: zero register, no reflection, bit 0 first
     *      a running frame freezes at the first i with clean_i(f) OR crc_i(f): iters[f] = i, its output is b_i.  A frame
     *      that never freezes gets iters = max_iter and the last round's bits, as without a CRC.  frames_converged counts
     *      frames frozen by either rule; ldpc_decoder_crc_stops those frozen in a round where clean_i was false.
     *      Needs early_term = 1 (LDPC_ERR_ARG otherwise, as for an unknown kind or crc_bits out of range).
     *      Streaming kernels only: LDPC_ALGO_SP, LDPC_ALGO_MS (fp32 and LDPC_MSG_F16, with or without ms_scale /
     *      ms_offset), LDPC_ALGO_BP (fp32 and LDPC_MSG_F16), and LDPC_ALGO_LAYERED and LDPC_ALGO_LAYERED_BP with one launch per layer; one more launch per round (crc_term_kernel).
     *      LDPC_ALGO_MS_FUSED and LDPC_ALGO_LAYERED_HOST reproduce reference kernels: LDPC_ERR_UNSUPPORTED.  The
     *      LDS-resident one-launch kernels and the record kernels do not carry the rule and are not selected (forcing
     *      them, LDPC_TUNE_ON(FUSED) or LDPC_TUNE_ON(LDSP): LDPC_ERR_UNSUPPORTED).
     *      Two facts.  An all-zero prefix passes every one of these CRCs; that is harmless, it is the all-zero payload
     *      (padding frames are born frozen and are never counted).  And every round tested is one more chance in 2^16 or
     *      2^24 that wrong bits pass: a frame stopped that way is the same undetected error ldpc_tb_check_device would
     *      report, so the undetected-error rate of a transport block can grow by up to the number of rounds tested. --- */
    int32_t crc_kind;           /* 0 = off, else enum ldpc_crc_kind: LDPC_CRC16, LDPC_CRC24A, LDPC_CRC24B             */
    int32_t crc_bits;           /* the CRC covers hard bits [0, crc_bits) of every frame, parity included:
                                   24 < crc_bits <= K (16 < for LDPC_CRC16)                                           */
    /* ---- fixed-point messages (appended; a struct_size of offsetof(ldpc_decoder_config, msg_bits), the size before
     *      these fields, is accepted and means 0, as the two shorter sizes do).  The struct grows by 16 bytes, not 4: a
     *      struct_size 4 or 8 bytes past the previous full size has always been refused as an ABI mismatch and stays
     *      refused, so no caller's wrong size turns into a read behind its struct. ------------------------------------ */
    int32_t msg_bits;           /* LDPC_MSG_I8: q = 4, 5, 6 or 8 bits per message (0 = 8), enum ldpc_msg_dtype above;
                                   with any other msg_dtype it must be 0 (LDPC_ERR_ARG)                                */
    int32_t post_bits;          /* LDPC_ALGO_LAYERED_FX: p bits of posterior memory, msg_bits <= p <= 16 (0 = 16); with any
                                   other algorithm it must be 0 (LDPC_ERR_ARG).  The first of the three words that were
                                   msg_reserved[3]: size and offsets are unchanged                                     */
    int32_t bp_frac_bits;       /* LDPC_ALGO_LAYERED_BP_FX: f fractional bits of an LSB, 0 <= f <= 4; with any other algorithm
                                   it must be 0 (LDPC_ERR_ARG).  The first of the two words that were msg_reserved2[2]: size
                                   and offsets are unchanged                                                           */
    int32_t msg_reserved3;      /* must be 0 (LDPC_ERR_ARG otherwise)                                                  */
    /* ---- bit-flipping thresholds (appended; a struct_size of offsetof(ldpc_decoder_config, bf_threshold), the size before
     *      this field, is accepted and means all zero, as the shorter sizes do).  Sixteen words do not fit the one reserved
     *      word left, so the struct grows; LDPC_HIP_ABI_VERSION stays 3 because nothing a caller built against version 3
     *      passes is read differently: its struct_size says which fields it has. ------------------------------------------ */
    int32_t bf_threshold[16];   /* LDPC_ALGO_BITFLIP: off(i) of rounds 1 .. 16 (the last entry also for every later round),
                                   each in [0, 62]; all zero = the default off(i) = i - 1.  With any other algorithm every
                                   entry must be 0 (LDPC_ERR_ARG)                                                       */
} ldpc_decoder_config;

/* two-bit fields of tune_flags: LDPC_TUNE_ON(f) forces the choice on, LDPC_TUNE_OFF(f) off */
enum ldpc_tune_field {
    LDPC_TUNE_FUSED = 0,        /* LDS-resident one-launch kernels (fused_kernels.hpp)              */
    LDPC_TUNE_LDSP = 2,         /* record kernels: posteriors in LDS, check records in cache        */
    LDPC_TUNE_LDSP_EXT = 4,     /* single-layer columns travel with the records (off: all in LDS)   */
    LDPC_TUNE_LDSP_PACK = 6,    /* several frames per wave for circulants of <= 32 rows             */
    LDPC_TUNE_LINK_NARROW = 8,  /* column-fused check kernel in narrow waves (1 value per lane) or wide
                                   (V per lane); default: both -- and LINK_HALF -- are timed when a
                                   decoder with 2 or 4 frames per lane is created and the fastest is kept          */
    LDPC_TUNE_CHECK_WIDE = 10,  /* check kernels move V floats per lane (default off)               */
    LDPC_TUNE_SYN_XCD = 12,     /* XCD-aware syndrome grid (default on)                             */
    LDPC_TUNE_FUSED_PACK = 14,  /* fused layered kernel: several frames per wave (default on)       */
    LDPC_TUNE_FUSED_LOOP = 16,  /* fused kernels: run-time row loops instead of unrolled (default off) */
    LDPC_TUNE_DEVICE_TAIL = 18, /* device-side early exit + tail compaction without host polling
                                   (default: on when early_term && poll_interval == 0)              */
    LDPC_TUNE_MERGE = 20,       /* degree classes of one bucket share a launch (default on)         */
    LDPC_TUNE_LINK_DEEP = 22,   /* column-fused check kernel requests its inputs two rows ahead     */
    LDPC_TUNE_LINK_HALF = 24,   /* column-fused check kernel with 2 values per lane (tiles of 256)  */
    LDPC_TUNE_LINK_GUIDED = 26, /* column-fused check kernel: its launch ends with shorter row chunks
                                   (default on from 4 tiles)                                         */
    LDPC_TUNE_TILES_FIRST = 28, /* flooding launches as grids of (tiles, blocks): the blocks in flight
                                   are spread over all tiles of the batch (default: the column-fused
                                   check launch only; on: all; off: none)                               */
    LDPC_TUNE_FX_RECORD = 30    /* LDPC_ALGO_LAYERED_FX on the fixed-point record kernel (layered_ldsp_fx_kernel).
                                   Values: 0 (off, the default) and LDPC_TUNE_ON(LDPC_TUNE_FX_RECORD); LDPC_TUNE_OFF
                                   is not defined for it (it does not fit an int32_t; a negative tune_flags is
                                   LDPC_ERR_ARG), and with any algorithm other than LDPC_ALGO_LAYERED_FX /
                                   LDPC_ALGO_LAYERED_BP_FX the bit is LDPC_ERR_ARG                         */
};
#define LDPC_TUNE_ON(field) (1 << (field))
#define LDPC_TUNE_OFF(field) (2 << (field))

/* Counts (iterations, frames, converged frames, frame_rounds) cover the last call -- every launch group of an
 * ldpc_decode() call; the times are those of its last launch group. */
typedef struct ldpc_decode_stats {
    int32_t iterations_launched; /* check/variable rounds enqueued by the last call (maximum over its launch groups) */
    int32_t batch_time;          /* the reference's `Time=` (MyLdpc.cpp:838,1048): max iters  */
    int64_t frames;              /* frames of the last call                                  */
    int64_t frames_converged;    /* frames whose syndrome was clean                          */
    float ms_total;              /* HIP-event time of the whole decode on its stream         */
    float ms_check;              /* summed check-node kernels (needs timing enabled)         */
    float ms_var;                /* summed variable-node kernels                             */
    float ms_other;              /* init / pack / bookkeeping kernels                        */
    int32_t launches_check;      /* kernel launches behind ms_check                          */
    int32_t launches_var;
    int64_t frame_rounds;        /* streaming flooding kernels: sum over the rounds of the frames in tiles that
                                    still did work (tile size x tiles with a running frame when the round began;
                                    finished tiles leave at kernel entry): what a round's traffic is priced at
                                    under early termination.  0 for the one-launch and layered kernels    */
} ldpc_decode_stats;

/* ---- library -------------------------------------------------------------- */
int ldpc_abi_version(void);
const char *ldpc_last_error(void);
/* Number of HIP devices (0 and LDPC_ERR_HIP if the runtime is unusable). */
int ldpc_device_count(int *count);

/* ---- graph: replaces Coder::forDecoder's adjacency build, MyLdpc.cpp:171-222 ---- */
/* rows/cols: the E nonzeros of the M x N parity-check matrix in row-major order
 * (strictly ascending (row, col)).  Host-only; no device is touched. */
int ldpc_graph_create(const int32_t *rows, const int32_t *cols, int64_t E, int32_t M, int32_t N,
                      ldpc_graph **out);
int ldpc_graph_destroy(ldpc_graph *g);
int ldpc_graph_info(const ldpc_graph *g, int32_t *M, int32_t *N, int64_t *E, int32_t *max_row_deg,
                    int32_t *max_col_deg);

/* ---- decoder: replaces Coder::forDecoder's device setup + addDecodeType,
 *      MyLdpc.cpp:226-305, 307-552 -------------------------------------------- */
/* Reference defaults.  The caller says how large its struct is, so that the call never writes behind it:
 * ldpc_decoder_config_init_sized fills the first struct_size bytes -- one of the five sizes ldpc_decoder_create accepts:
 * offsetof(ms_scale), offsetof(crc_kind), offsetof(msg_bits), offsetof(bf_threshold), sizeof -- and stores struct_size itself; any other size is LDPC_ERR_ARG and
 * nothing is written.  The exported function ldpc_decoder_config_init is what callers built against the header before
 * crc_kind / crc_bits call with their shorter struct: it fills offsetof(ldpc_decoder_config, crc_kind) bytes and stores
 * that as struct_size (CRC off).  Code compiled against THIS header gets its own struct's size through the macro below,
 * so `ldpc_decoder_config_init(&cfg)` keeps meaning "all of cfg, struct_size = sizeof cfg". */
void ldpc_decoder_config_init(ldpc_decoder_config *cfg);
int ldpc_decoder_config_init_sized(ldpc_decoder_config *cfg, uint32_t struct_size);
#define ldpc_decoder_config_init(cfg) ((void)ldpc_decoder_config_init_sized((cfg), (uint32_t)sizeof(ldpc_decoder_config)))
int ldpc_decoder_create(const ldpc_graph *g, const ldpc_decoder_config *cfg, ldpc_decoder **out);
/* The reference uses devices[0] of its context only (MyLdpc.cpp:226-235).  Here one handle may
 * span several HIP devices: ldpc_decode() cuts the caller's frame stream into n_devices contiguous
 * ranges (ldpc_shard_range), and one host thread per entry of devices[] runs that range through
 * its own device decoder -- own stream, own pinned staging, results copied straight to the
 * caller's buffers at the range's offsets; no exchange between devices (frames are independent).
 * Bytes and iteration counts equal the single-device result.  An ordinal may appear more than
 * once (two decoders sharing one GPU).  cfg->device is ignored; cfg->max_batch is per device.
 * Device-pointer entry points (ldpc_decode_device, taps, dumps) need a single-device handle. */
int ldpc_decoder_create_multi(const ldpc_graph *g, const ldpc_decoder_config *cfg, const int32_t *devices,
                              int32_t n_devices, ldpc_decoder **out);
/* Waits for this handle's own work only (its streams), not for the device; joins the handle's worker
 * threads.  Returns LDPC_ERR_STATE (after freeing the handle all the same) if a page-locked block of a
 * caller's buffer could not be released by an earlier LDPC_HOST_INPUT_LOCK_PAGES call. */
int ldpc_decoder_destroy(ldpc_decoder *d);
/* Frames [*lo, *hi) of part `part` of `parts` when `frames` frames are cut into contiguous, balanced
 * ranges whose boundaries are multiples of `unit` frames (earlier parts take the remainder).  The
 * same arithmetic shards frames over ranks in the benchmark (one process per GPU). */
int ldpc_shard_range(int64_t frames, int32_t part, int32_t parts, int32_t unit, int64_t *lo, int64_t *hi);

/* ---- decode: replaces Coder::decode + decodeOnceSP/MS/TDMP*, MyLdpc.cpp:571-618,
 *      786-1059.  Host buffers; chunks `frames` into max_batch groups; blocking.
 *      out must hold ldpc_out_bytes(K, frames, pack_mode) bytes.
 *      iters (nullable): per frame, the iteration at which its syndrome first was
 *      clean, or max_iter. ------------------------------------------------------- */
int ldpc_decode(ldpc_decoder *d, const float *llr_host, int64_t frames, uint8_t *out_host,
                int64_t out_bytes, int32_t *iters);

/* Same, on buffers already resident in this decoder's device memory; enqueued on
 * `stream` (a hipStream_t, NULL = default stream), returns without waiting unless
 * poll_interval > 0.  0 <= frames <= max_batch (frames == 0 enqueues nothing).
 *   llr_dev:   frames * N floats; rows behind them (up to max_batch) are not part of the call.
 *   out_dev:   nullable: iteration counts and stats only.  Otherwise out_bytes bytes, of which the first
 *              min(out_bytes, ldpc_out_bytes(K, frames, pack_mode)) are written (LDPC_PACK_BYTES: a short buffer
 *              truncates, bytes from out_bytes on stay as they were; the bits between frames with K % 8 != 0
 *              read 0.  LDPC_PACK_BITS: a short buffer is LDPC_ERR_ARG).  out_bytes < 0 is LDPC_ERR_ARG, with or
 *              without out_dev.
 *   iters_dev: nullable; frames counts.  Written by every engine whether or not out_dev is given.
 *   With out_dev == NULL the call still decodes: it writes iters_dev (if given) and what ldpc_decoder_stats
 *   reports (iterations, batch_time, frames, frames_converged, frame_rounds); with out_dev == NULL and
 *   iters_dev == NULL the stats alone.
 *   A call refused with LDPC_ERR_ARG has enqueued nothing.
 * Device pointers, here and in every *_device entry point below:
 *   - float and int32 buffers (llr_dev, iters_dev, the rate matcher's rx_dev / soft_dev / y_dev) need their natural
 *     4-byte alignment and no more: the kernels take their 16-byte paths only where the address allows;
 *   - byte buffers (out_dev, bits_dev, ref_dev, src_dev, code_dev, tx_dev) may have any alignment;
 *   - a call reads and writes nothing outside [ptr, ptr + size) of the buffers it is given, size being what the call
 *     states for `frames` frames -- not for max_batch. */
int ldpc_decode_device(ldpc_decoder *d, const float *llr_dev, int64_t frames, uint8_t *out_dev,
                       int64_t out_bytes, int32_t *iters_dev, void *stream);

int64_t ldpc_out_bytes(int32_t K, int64_t frames, int32_t pack_mode);

/* The correction table of LDPC_ALGO_LAYERED_BP_FX at f = bp_frac_bits fractional bits, T_f[0 .. *count - 1], the last entry
 * being its first 0 -- the very numbers a decoder created with this f hands to its kernels.  *count is set whenever f is
 * valid; out may be NULL to ask for the count alone, otherwise cap >= *count entries are needed (LDPC_ERR_ARG if fewer, as
 * for f outside 0 .. 4 or count NULL).  No entry lies near a rounding tie (tests/test_layered_bp_fx_cpu.py), so the table
 * does not depend on the host's libm.  Needs no device. */
int ldpc_bp_fx_table(int32_t f, int32_t *out, int32_t cap, int32_t *count);

/* ---- soft output: the decode above plus one fp32 value per frame and code bit --------------------------------
 * The rule, per frame.  Let i_f = iters[f] be the round in which frame f froze (its syndrome first was clean, or its
 * CRC passed), or max_iter; with early_term = 0 it is max_iter for every frame.  Then
 *   LDPC_SOFT_POSTERIOR:  soft[f * N + n] = p_{i_f}(f, n), the fp32 posterior bit n of the frame's output was decided
 *     from, in the units of the channel values, positive <-> bit 0:
 *       LDPC_ALGO_MS, every form (fp32, LDPC_MSG_F16, ms_scale / ms_offset): p = y_n + R_e1 + R_e2 + ... in fp32, one add
 *         at a time, R = the check->variable messages of round i_f on the column's edges in ascending edge id; y_n is the
 *         channel value as the decoder read it (rounded to fp16 with LDPC_MSG_F16).  This is the very sum the variable
 *         node forms for the hard decision.
 *       LDPC_ALGO_BP, fp32 and LDPC_MSG_F16: the same sum with y_n = chan[n] = llr_scale * y[n] as the decoder stored it
 *         (one fp32 multiply, rounded to fp16 with LDPC_MSG_F16): the value is an LLR.
 *       LDPC_ALGO_LAYERED, LDPC_ALGO_LAYERED_HOST, LDPC_ALGO_MS_FUSED: P[n] after the last layer (MS_FUSED: after the
 *         posterior update) of round i_f.
 *       LDPC_ALGO_LAYERED_BP: P[n] after the last layer of round i_f, an LLR; y_n = chan[n] = llr_scale * y[n], the fp32
 *         product formed first (the extrinsic value is never one fma).
 *   LDPC_SOFT_EXTRINSIC:  soft = p - y_n, one fp32 subtraction, the same y_n.
 * Consequence: wherever the posterior is finite and not zero, its sign is the output bit.
 * The value is that of round i_f and no later one: a frozen frame's messages keep evolving unread inside the streaming
 * decoders, so it is caught when the frame freezes (0 ulp against the CPU oracle's `post` tap of that round).
 *
 * LDPC_ALGO_SP has no soft output (LDPC_ERR_UNSUPPORTED; LDPC_ALGO_BP and LDPC_ALGO_LAYERED_BP are the sum-products that have one): the reference's
 * sum-product runs in the probability domain in
 * fp32, and its normalised posterior (f0 - f1) / (f0 + f1) carries nothing by the time a frame stops -- on the
 * BG1-profile test code (N = 1088, 64 frames, llr_scale 8) it is exactly +-1 on 68210 of 69632 values at 3.0 dB, and 0/0
 * on 20690 of them at 1.5 dB.
 *
 * ldpc_decode_soft_device follows ldpc_decode_device in everything the two share (out_dev and iters_dev stay nullable).
 *   soft_dev:    soft_floats floats, 4-byte aligned and no more; exactly frames * N are written, nothing else -- not the
 *                rows behind them, not for the padding frames of a ragged tile.  Must not overlap llr_dev.
 *   LDPC_ERR_ARG (nothing enqueued): soft_dev NULL, soft_floats < frames * N, an unknown soft_kind, an overlap with
 *                llr_dev.  LDPC_ERR_STATE: a debug tap is set.  LDPC_ERR_UNSUPPORTED: LDPC_ALGO_SP, on any engine.
 * It works on whichever engine the handle was created with, through both hand-overs of the stragglers, and leaves
 * nothing behind: the plain entry points launch and move exactly what they did before and after a soft call.
 * ldpc_decode_soft: the same on host buffers, as ldpc_decode (launch groups, device lists); soft_host holds
 * frames * N floats.  The handle's first soft call allocates the staging buffers for it. */
enum ldpc_soft_kind { LDPC_SOFT_POSTERIOR = 1, LDPC_SOFT_EXTRINSIC = 2 };
int ldpc_decode_soft_device(ldpc_decoder *d, const float *llr_dev, int64_t frames, uint8_t *out_dev, int64_t out_bytes,
                            int32_t *iters_dev, float *soft_dev, int64_t soft_floats, int32_t soft_kind, void *stream);
int ldpc_decode_soft(ldpc_decoder *d, const float *llr_host, int64_t frames, uint8_t *out_host, int64_t out_bytes,
                     int32_t *iters, float *soft_host, int64_t soft_floats, int32_t soft_kind);

/* ---- typed channel values: int8 and fp16 input for every decode entry point -------------------------------------
 * Receivers deliver int8 (sometimes fp16) soft bits; widened to fp32 on the host they cost four (two) times the bytes on
 * every bus in front of a decoder whose first kernel rounds them to fp16 or E4M3 again.  A typed call names the element
 * type of its channel buffer and a unit.  The rule, bit for bit: for element x[f * N + n] the decoder reads
 *       y = (float)x * llr_unit          one fp32 multiply; the widening is exact
 * and everything else is exactly what the handle does when ldpc_decode_device is given that y: SP forms
 * exp(llr_scale * y), BP and LAYERED_BP form chan = llr_scale * y, min-sum stores y; with LDPC_MSG_F16 / LDPC_MSG_F8 the
 * value is rounded where it is stored, with LDPC_MSG_I8 it is sq(llr_scale * y), a second multiply of its own.  Two roundings, never one: the product x * llr_unit is a value of its own, never
 * folded with llr_scale and never contracted into the conversion to fp16.  Padding frames read y = +1.0f exactly, not
 * 1 * llr_unit.  Soft output, extrinsic kind: the y_n of the rule above is this product (BP, LAYERED_BP: llr_scale * y).
 *   LDPC_LLR_I8:  all 256 codes are legal; -128 reads -128 * llr_unit.  Any alignment.
 *   LDPC_LLR_F16: binary16; infinities and NaN widen as they are.  Two-byte alignment and no more (an odd address:
 *                 LDPC_ERR_ARG).
 *   LDPC_LLR_F32: llr_unit must be exactly 1.0f, and the call IS ldpc_decode_device / ldpc_decode.
 *   LDPC_ERR_ARG (nothing enqueued): an unknown type; llr_unit NaN, infinite or <= 0; what the plain entry points refuse.
 *   The soft forms refuse a soft buffer that overlaps the BYTES of the typed buffer.
 * A call reads nothing outside [ptr, ptr + frames * N * element size).  The kernels take 16-byte loads (16 int8 or 8 fp16
 * values) only where the address and the row stride N * element size both allow them -- int8 rows of N = 648 do not --
 * and read element by element otherwise.
 * Every handle takes typed calls: every algorithm, message type and engine; early termination, polling, both hand-overs
 * of the stragglers, the CRC stop and the debug taps behave as with float input.  The streaming engines read the
 * caller's rows themselves; the one-launch and record kernels get one widening pass (llr_widen_kernel) into max_batch * N
 * floats the handle owns, allocated by its first typed call and released with it.  The plain entry points launch and
 * move exactly what they did, before and after a typed call.
 * ldpc_decode_typed / ldpc_decode_soft_typed: host buffers, as ldpc_decode (launch groups, device lists).  Launch groups,
 *   the pinned ring and the copies are sized in bytes of the element type and the device staging slots hold the narrow
 *   elements.  Narrow channel values are always STAGED (or copied directly from memory the caller page-locked itself):
 *   LDPC_HOST_INPUT_LOCK_PAGES is treated as LDPC_HOST_INPUT_STAGED for them.  The rule that cuts a single-group call in
 *   two keeps its threshold of 256 MiB of input, so a narrow call is cut later (at 4x the frames with int8).
 * ldpc_llr_quantize_device: the sender's side of the rule, for chains that stay in HBM and for sweeps of the quantisation
 *   itself.  t = y / llr_unit, one IEEE fp32 divide; then
 *     LDPC_LLR_I8:  NaN -> 0; otherwise rintf(t), ties to even, clamped to [-127, 127] (+-inf give +-127; -128 is never
 *                   produced);
 *     LDPC_LLR_F16: NaN stays NaN; otherwise t is clamped to +-65504 and rounded to binary16, nearest even;
 *     LDPC_LLR_F32: LDPC_ERR_ARG.
 *   count values; y_dev and out_dev must not overlap (LDPC_ERR_ARG); enqueued on `stream`, returns without waiting. */
enum ldpc_llr_type { LDPC_LLR_F32 = 0, LDPC_LLR_F16 = 1, LDPC_LLR_I8 = 2 };
int ldpc_decode_typed_device(ldpc_decoder *d, const void *llr_dev, int32_t llr_type, float llr_unit, int64_t frames,
                             uint8_t *out_dev, int64_t out_bytes, int32_t *iters_dev, void *stream);
int ldpc_decode_soft_typed_device(ldpc_decoder *d, const void *llr_dev, int32_t llr_type, float llr_unit, int64_t frames,
                                  uint8_t *out_dev, int64_t out_bytes, int32_t *iters_dev, float *soft_dev,
                                  int64_t soft_floats, int32_t soft_kind, void *stream);
int ldpc_decode_typed(ldpc_decoder *d, const void *llr_host, int32_t llr_type, float llr_unit, int64_t frames,
                      uint8_t *out_host, int64_t out_bytes, int32_t *iters);
int ldpc_decode_soft_typed(ldpc_decoder *d, const void *llr_host, int32_t llr_type, float llr_unit, int64_t frames,
                           uint8_t *out_host, int64_t out_bytes, int32_t *iters, float *soft_host, int64_t soft_floats,
                           int32_t soft_kind);
int ldpc_llr_quantize_device(const float *y_dev, int64_t count, int32_t llr_type, float llr_unit, void *out_dev,
                             int32_t device, void *stream);

/* Per-kernel HIP-event timing of subsequent decode calls (two event records per
 * launch on the decode stream; off by default).  enable = 1: every call; enable = k > 1:
 * every k-th ldpc_decode_device call, starting with the next one (the events cost about 2 %
 * of a 4096-frame step, so a benchmark times a sample of its steps).  Enabling (again)
 * clears what was gathered; times then accumulate over all following timed calls.
 * ldpc_decoder_stats: stats of the last call (ms_check/ms_var/ms_other: everything
 * gathered since timing was enabled); blocks until that call has finished. */
int ldpc_decoder_set_timing(ldpc_decoder *d, int enable);
int ldpc_decoder_stats(ldpc_decoder *d, ldpc_decode_stats *stats);
/* CRC-aided early termination (crc_kind != 0): *frames = frames of the last call that froze in a round in which their
 * syndrome was not clean -- stopped by the CRC alone.  Summed over the launch groups of an ldpc_decode() call, the
 * decoders the stragglers were handed to and the devices of a multi-device handle; 0 with crc_kind = 0.  Blocks until
 * the call has finished, as ldpc_decoder_stats does. */
int ldpc_decoder_crc_stops(ldpc_decoder *d, int64_t *frames);

/* One line per distinct kernel launched since timing was enabled. */
typedef struct ldpc_kernel_time {
    int32_t phase;         /* 0 check node, 1 variable node, 2 layer, 3 other          */
    int32_t degree;        /* row / column degree the kernel is specialised for        */
    int32_t launches;
    float ms_total;        /* sum of HIP-event durations of those launches             */
    int64_t bytes_total;   /* ALGORITHMIC bytes of those launches in the two-kernel formulation
                              (16 E + 4 N per frame-iteration over all kernels): 4 B per message
                              read or written + 4 B per channel value read, per frame    */
    char name[64];         /* e.g. "check_link_kernel<sp,7,4>" (algo, degree, frames/lane), the
                              kernel's name in a rocprofv3 trace up to the spelling of the
                              template arguments; the one-launch record kernels carry their
                              launch shape instead: "layered_ldsp_kernel[768x384,1]" =
                              [persistent grid x workgroup size, frames per workgroup]  */
    int64_t bytes_moved;   /* bytes those launches' own loads and stores move: = bytes_total except
                              for the column-fused check kernel, whose fused columns' messages
                              never travel through HBM (the figure the PMC counters confirm)  */
} ldpc_kernel_time;
int ldpc_decoder_kernel_times(ldpc_decoder *d, ldpc_kernel_time *out, int32_t capacity,
                              int32_t *count);

/* Which form of the column-fused check kernel this decoder runs (0 wide: V values per lane, 1 narrow: one,
 * 2 half: two) and, if it was chosen by the creation-time measurement, what each candidate took per launch
 * on the decoder's own arrays (ms[0..2] in that order, 0 = not a candidate / not measured; *calibrated = 0 when
 * the form was fixed by the tuning fields or the code has no column-fused rows). */
int ldpc_decoder_link_form(ldpc_decoder *d, int32_t *form, int32_t *calibrated, float ms[3]);

/* The placement search of tune_place: how many combinations were timed (*candidates, 0 = no search; the first is the
 * decoder's original allocations, then fresh R arrays, then fresh Q arrays), which was kept (*kept) and the time of one
 * message round with each (ms[0 .. *candidates), at most 15). */
int ldpc_decoder_placement(ldpc_decoder *d, int32_t *candidates, int32_t *kept, float ms[16]);
/* Measurement aid: device addresses of a streaming decoder's arrays, out[0..3] = Q, R, channel term, hard-bit masks. */
int ldpc_decoder_array_addresses(ldpc_decoder *d, uint64_t out[4]);

/* ---- debug taps (tolerance checks against the oracle) ------------------------
 * Stop the NEXT decode call after `iter` check/variable rounds (0 = off) and keep
 * its messages.  ldpc_decoder_dump then copies them out in the reference's layout
 * [frame][E] / [frame][N] (decodeCL.c: q/r at b*nonZeros+e, posteriors at b*N+n).
 * which: 0 = check->variable messages R (SP: r0-r1), 1 = variable->check
 * messages Q (SP: q0-q1), 2 = channel term (SP: exp(scale*y), MS: y, BP: scale*y; layered:
 * posterior P), 3 = hard bits as floats 0/1 [frame][N]. */
int ldpc_decoder_set_tap(ldpc_decoder *d, int32_t iter);
int ldpc_decoder_dump(ldpc_decoder *d, int32_t which, float *host_out, int64_t count);

/* ---- test channel and error count on the device: replace Coder::test / gaussian
 *      (MyLdpc.cpp:1061-1105: BPSK, bit 0 -> +1.0, bit 1 -> -1.0, plus N(0, sd^2)) and the
 *      comparison loop of Test.cpp:105-110, for data that never leaves HBM.
 * ldpc_awgn_device: llr_dev[f*N + n] = (bits ? 1 - 2*bits[f*N + n] : +1) + sd * z(seed, first_frame + f, n)
 *      for f < frames; bits_dev: one byte per code bit (0/1), NULL = the all-zero codeword.  z is
 *      the counter-based standard normal of csrc/ldpc_channel.h (Philox4x32-10 + Box-Muller in
 *      IEEE double; identical on host and device, any frame range reproducible anywhere), NOT
 *      the reference's rand()-based gaussian().  Enqueued on `stream`, returns without waiting.
 * ldpc_count_errors_device: compares two packed outputs of `frames` x `bytes_per_frame` bytes
 *      (ref_dev NULL = all zero); blocks; errors[0] = differing bits, [1] = differing bytes (the
 *      reference's ErrNum), [2] = frames with at least one difference. */
int ldpc_awgn_device(float *llr_dev, int64_t frames, int32_t N, const uint8_t *bits_dev, float sd,
                     uint64_t seed, int64_t first_frame, int32_t device, void *stream);
int ldpc_count_errors_device(const uint8_t *out_dev, const uint8_t *ref_dev, int64_t frames,
                             int64_t bytes_per_frame, int64_t errors[3], int32_t device, void *stream);

/* ---- encoder: replaces Coder::forEncoder / encode / encodeOnce (MyLdpc.cpp:137-165, 554-569, 633-682) for whole
 *      batches on the device, so that encode -> channel -> decode -> count can stay in HBM.
 * Systematic: the codeword is [K information bits | M = N - K parity bits], the unique solution of H c = 0.  The
 * parity part H[:, K..N) must have one of two structures, recognised from the graph alone:
 *   LDPC_PARITY_DUAL_DIAGONAL (needs block_rows = z > 0): circulant blocks of z rows; the first parity block column
 *     has three blocks, in block rows 0, x, c-1 with shifts (a, b, a), any b; parity block columns 1 .. c-1 are the
 *     zero-shift dual diagonal; block rows c .. M/z - 1 ("extension", possibly none) each own one zero-shift
 *     identity parity column and otherwise touch information and core parity columns only.  802.16e: c = M/z for
 *     all six seeds; codes.nr_bg1_profile_edges: c = 4, x = 1, 42 extension block rows.
 *   LDPC_PARITY_STAIRCASE: parity column K + m has its ones in rows m and m + 1 only (codes.dvbs2_profile_edges).
 * Anything else is LDPC_ERR_UNSUPPORTED from ldpc_parity_structure / ldpc_encoder_create, with a message that names the
 * condition that failed; any other H is served by ldpc_encoder_create_dense (LDPC_PARITY_DENSE, below).
 * ldpc_parity_structure (host only, no device is touched): out[0] = enum ldpc_parity_kind, out[1] = c, out[2] = x,
 *   out[3] = a, out[4] = b, out[5] = extension block rows, out[6] = z, out[7] = 0 (all 0 but out[0] for a staircase).
 * Data (Coder::encode's): frame f reads the K/8 WHOLE source bytes from byte (f*K)/8 on (the product first: for
 *   K % 8 != 0 frames start at 0, 40, 81, 121, ... for K = 324); bytes at index >= src_bytes read as zero;
 *   information bits K - K%8 .. K-1 are zero; bits LSB first.  Code formats: enum ldpc_code_format.
 * ldpc_encode_device: buffers in the encoder's device memory, frames <= max_frames, every frame's first byte inside
 *   src_bytes; enqueued on `stream` (a hipStream_t, NULL = default stream), returns without waiting; allocates
 *   nothing (the handle owns scratch for max_frames frames: N bits per frame plus the row sums).
 * ldpc_encode: host buffers, LDPC_CODE_PACKED, blocking, in chunks of max_frames; the frame count follows from
 *   src_bytes as in Coder::encode (the last frame is the first one with (f+1)*K/8 >= src_bytes).
 * An encoder handle is not re-entrant: one per host thread / stream. */
typedef struct ldpc_encoder ldpc_encoder;
enum ldpc_code_format {
    LDPC_CODE_PACKED = 0, /* N/8 bytes per frame at byte f*N/8, LSB first (Coder::encode's priorCode); N % 8 == 0 */
    LDPC_CODE_BITS = 1    /* N bytes per frame, 0/1: what ldpc_awgn_device takes as bits_dev                      */
};
enum ldpc_parity_kind { LDPC_PARITY_DUAL_DIAGONAL = 1, LDPC_PARITY_STAIRCASE = 2, LDPC_PARITY_DENSE = 3 /* below */ };
int ldpc_parity_structure(const ldpc_graph *g, int32_t K, int32_t block_rows, int32_t out[8]);
int ldpc_encoder_create(const ldpc_graph *g, int32_t K, int32_t block_rows, int32_t max_frames, int32_t device,
                        ldpc_encoder **out);
int ldpc_encoder_destroy(ldpc_encoder *e);
int ldpc_encode_device(ldpc_encoder *e, const uint8_t *src_dev, int64_t src_bytes, int64_t frames, uint8_t *code_dev,
                       int64_t code_bytes, int32_t format, void *stream);
int ldpc_encode(ldpc_encoder *e, const uint8_t *src_host, int64_t src_bytes, uint8_t *code_host, int64_t code_bytes);
/* bytes of `frames` codewords in `format` (0 for an unknown format, or LDPC_CODE_PACKED with N % 8 != 0) */
int64_t ldpc_code_bytes(int32_t N, int64_t frames, int32_t format);

/* ---- encoder for any H: LDPC_PARITY_DENSE, a dense GF(2) parity solve on the device.  The reference's forEncoder solved
 *      a dense system for every code; here this is the path of the matrices that have neither structure above (MacKay,
 *      Gallager, PEG, anything from an alist file).  ldpc_parity_structure never returns LDPC_PARITY_DENSE and
 *      ldpc_encoder_create keeps refusing what it refuses.
 * Dense structure: given H (M x N) and K with N - M <= K < N (and K >= 1), put rho = N - K, H_s = H[:, 0..K) and
 *   H_p = H[:, K..N) (M x rho).  The code is encodable in this column order iff
 *     rank(H_p) = rho  (the parity bits are determined), and
 *     rank(H)   = rho  (every information word has a codeword; rows beyond the rank are redundant, not contradictory).
 *   Then for every u the parity bits p are the unique solution of H_p p = H_s u, and the codeword is [u | p].  The
 *   solution is unique, so the result does not depend on how an implementation eliminates.  Refusals
 *   (LDPC_ERR_UNSUPPORTED, the message names the condition and the numbers): rank(H_p) < rho ("parity part is singular:
 *   rank r of rho"); rank(H) > rho ("information bits are not free"); M > 16384.  K outside [N - M, N) is LDPC_ERR_ARG.
 *   The data rules of ldpc_encode_device hold unchanged: frame f reads K/8 whole source bytes from byte (f*K)/8,
 *   information bits K - K%8 .. K-1 are zero, LDPC_CODE_PACKED needs N % 8 == 0.
 * Systematic order (ldpc_graph_systematic_order; host only, no device is touched): scan the columns N-1, N-2, ..., 0; a
 *   column joins the pivot set iff it is linearly independent over GF(2) of the columns already in it (the construction
 *   of step 4 of the OSD rule with the index in place of the reliability).  rho = |pivot set| = rank(H) -> *rank;
 *   perm[0 .. N-rho) = the non-pivot columns in ascending order, perm[N-rho .. N) = the pivot columns in ascending
 *   order; column perm[i] of H is column i of the re-ordered H'.  H' with K = N - rho is always encodable.  If
 *   H[:, N-M..N) is nonsingular already (all six 802.16e seeds, both profile codes) perm is the identity.  A pure
 *   function of H.
 * ldpc_parity_dense (host only): out = {rho, rank(H_p), M, 64-bit words per row of T = ceil(M / 64)}; returns what
 *   ldpc_encoder_create_dense would return before it looks for a device, out filled as far as it was computed.
 * ldpc_parity_dense_rows (host only, a diagnostic like ldpc_host_block_plan): rows [first, first + rows) of the solve
 *   matrix T (rho x M bits; bit j of a row = bit j % 64 of word j / 64, tail bits zero) with T H_p = I_rho over GF(2),
 *   so that p = T (H_s u); `words` = the 64-bit words t_out holds, at least rows * ceil(M / 64).
 * ldpc_encoder_create_dense: checks, in this order, the arguments, the M limit, the host analysis (bit-packed
 *   Gauss-Jordan on [H_p | I_M]; the combinations of rows with an empty parity part are applied to the sparse H_s), and
 *   only then the device (LDPC_ERR_HIP last).  It returns an ordinary ldpc_encoder: ldpc_encode_device, ldpc_encode and
 *   ldpc_encoder_destroy serve it as they serve the structured kinds (same argument checks, stream semantics, chunking by
 *   max_frames, no allocation per call).  The handle owns, besides the N bits per frame, M row sums per frame and T.
 * Limits (fixed): M <= 16384 for the dense encoder (T is at most 32 MiB); M * N <= 2^27 bits for
 *   ldpc_graph_systematic_order.  Larger inputs are LDPC_ERR_UNSUPPORTED with the numbers in the message.
 *   Creation is the host elimination, at most M^2 (M + rho) / 128 word operations on one thread, far fewer on sparse H.
 *   Measured (tools/encoder_measure.py --dense --cap, the host of an MI355X): 1 ms at M = 1152 and 0.06 s at M = 8064
 *   (802.16e rate 1/2), 1.9 s at the limit M = 16384 (a shuffled triangular parity part with random fill, 98 k edges);
 *   a random column-weight-3 H of 8192 x 16384 in its systematic order: 1.2 s, after 0.35 s for the order itself. */
int ldpc_graph_systematic_order(const ldpc_graph *g, int32_t *perm /* N */, int32_t *rank);
int ldpc_parity_dense(const ldpc_graph *g, int32_t K, int64_t out[4]);
int ldpc_parity_dense_rows(const ldpc_graph *g, int32_t K, int32_t first, int32_t rows, uint64_t *t_out, int64_t words);
int ldpc_encoder_create_dense(const ldpc_graph *g, int32_t K, int32_t max_frames, int32_t device, ldpc_encoder **out);

/* ---- rate matching: puncturing, shortening (filler bits), repetition and HARQ soft combining between the encoder and
 *      the decoders, for data that stays in HBM.  The reference has no counterpart: it sends whole mother codewords.
 * Spec: plain parameters -- no handle, no device state; the index map is closed-form.
 * Buffer: the circular buffer is code bits [P, N) in order, Ncb = N - P positions, fillers included (TS 38.212
 *   section 5.4.2.1 without the bit interleaver and without a limited buffer).  L = Ncb - (hi - lo) >= 1 of them can be
 *   sent.  A transmission is (k0, E), 0 <= k0 < Ncb, E >= 1: walk the buffer from position k0, wrap at Ncb, skip
 *   fillers (a k0 on a filler starts at the next non-filler), emit E bits; E > L repeats.  In closed form
 *       r0 = k0 - clamp(k0 - (lo - P), 0, hi - lo),  rank(e) = (r0 + e) mod L,
 *       index(e) = P + rank + (rank >= lo - P ? hi - lo : 0).
 *   filler_lo == filler_hi means no fillers (the common value is then ignored).
 * Match:   tx[f][e] = code[f][index(e)].
 * Recover: for every frame f and code bit n
 *       s = accumulate ? soft[f][n] : 0.0f;  s += rx[f][e] for every e with index(e) = n, in ASCENDING e
 *       (fp32, no reassociation: the result is bit-defined; a gather, no atomics);  fillers: s = 0;
 *       soft[f][n] = s                                             (if a soft buffer is given)
 *       y[f][n] = fill_llr at fillers, else s if s != 0.0f, else
 *                 erasure_llr > 0 ? erasure_llr * (1.0f + (float)n / (float)N) : 0.0f      (fp32, IEEE divide)
 *   `soft` holds pure sums of everything received so far (HARQ: first transmission accumulate = 0, retransmissions
 *   accumulate = 1 with their own k0 / E; the sums stay exact because the erasure values never enter them); `y` is
 *   what a decoder reads.  soft and y must not overlap.  Conventions of the channel values as for ldpc_decode:
 *   positive <-> bit 0, so a filler (a known zero) reads +fill_llr.
 * The erasure rule -- why erasure_llr exists.  A position that was never received (punctured, or not reached by a
 *   short transmission) carries no information: 0.  The layered MIN-SUM arithmetic the project reproduces from the
 *   reference (LDPC_ALGO_LAYERED, LDPC_ALGO_LAYERED_HOST) cannot take an exact 0: a check row's sign is the running product of its inputs (a *= tmp with the message sign
 *   taken from tmp), so one input of exactly 0 zeroes every message of its row for good, and two erased columns of
 *   EQUAL tiny magnitude cancel back to exactly 0 in the layered update.  With erased = 0 LDPC_ALGO_LAYERED fails on
 *   every frame that has a punctured column; the flooding decoders (LDPC_ALGO_SP, LDPC_ALGO_MS, LDPC_ALGO_BP) handle zeros, and so
 *   does LDPC_ALGO_LAYERED_BP, whose rows take their sign from (x < 0): on the 64 frames of the BG1-profile test scenario with
 *   punctured columns and erasure_llr = 0 it gets all 64 right where LDPC_ALGO_LAYERED gets none.  Small,
 *   pairwise DISTINCT positive values repair the layered min-sum decoders completely (DESIGN.md has the figures):
 *   erasure_llr = 1e-6 is the recommended value whenever a layered min-sum decoder reads y; it is harmless for SP, MS, BP
 *   and LAYERED_BP.
 *   With LDPC_MSG_F16 messages the values collapse to a few fp16 levels and stop being distinct -- the flooding
 *   decoders, the only ones with fp16 messages, do not need the rule.  erasure_llr > 0 needs N <= 2^22 (beyond that
 *   the values are no longer pairwise distinct in fp32): LDPC_ERR_ARG.
 * Formats are enum ldpc_code_format for code and tx alike: LDPC_CODE_PACKED needs N % 8 == 0 on the code side and
 *   E % 8 == 0 on the tx side (E/8 bytes per frame, LSB first); tx in LDPC_CODE_BITS is exactly what
 *   ldpc_awgn_device(..., N = E, ...) takes as bits_dev, and rx is what it writes.
 * The *_device calls enqueue on `stream` (a hipStream_t, NULL = default stream), return without waiting and allocate
 *   nothing.  ldpc_rate_match / ldpc_rate_recover take host buffers, block, and run the same kernels over chunks of
 *   frames (device scratch is allocated and released inside the call).  There is no CPU path.
 * ldpc_rate_index is host-only arithmetic (no device is touched): index_out[e] = index(e) for e < E.
 * Every argument error is LDPC_ERR_ARG with a message that names the field. */
typedef struct ldpc_rate_spec {
    uint32_t struct_size;          /* = sizeof(ldpc_rate_spec); ABI guard                                              */
    int32_t  N;                    /* mother code length (columns of H)                                                */
    int32_t  punctured;            /* P: code bits [0, P) are never transmitted (NR: 2Z)                               */
    int32_t  filler_lo, filler_hi; /* code bits [lo, hi) are known zeros, never transmitted; P <= lo <= hi <= N       */
    float    fill_llr;             /* decoder input at fillers (init: 10; SP needs llr_scale * fill_llr < 88)          */
    float    erasure_llr;          /* eps: 0 = erased positions read 0.0f; > 0 = the distinct-value rule above         */
} ldpc_rate_spec;
void ldpc_rate_spec_init(ldpc_rate_spec *spec, int32_t N);   /* no puncturing, no fillers, fill_llr 10, erasure_llr 0 */
int ldpc_rate_lengths(const ldpc_rate_spec *spec, int32_t *Ncb, int32_t *L);
int ldpc_rate_index(const ldpc_rate_spec *spec, int32_t k0, int32_t E, int32_t *index_out);
int ldpc_rate_match_device(const ldpc_rate_spec *spec, const uint8_t *code_dev, int32_t code_format, int64_t frames, int32_t k0,
                           int32_t E, uint8_t *tx_dev, int64_t tx_bytes, int32_t tx_format, int32_t device, void *stream);
/* soft_dev: nullable, read when accumulate != 0, written; y_dev: nullable; at least one of the two; accumulate needs soft_dev */
int ldpc_rate_recover_device(const ldpc_rate_spec *spec, const float *rx_dev, int64_t frames, int32_t k0, int32_t E, float *soft_dev,
                             int32_t accumulate, float *y_dev, int32_t device, void *stream);
int ldpc_rate_match(const ldpc_rate_spec *spec, const uint8_t *code_host, int32_t code_format, int64_t frames, int32_t k0, int32_t E,
                    uint8_t *tx_host, int64_t tx_bytes, int32_t tx_format, int32_t device);
int ldpc_rate_recover(const ldpc_rate_spec *spec, const float *rx_host, int64_t frames, int32_t k0, int32_t E, float *soft_host,
                      int32_t accumulate, float *y_host, int32_t device);

/* ---- modem: bit interleaver, Gray mapper, AWGN channel and max-log demapper for QPSK and 16-, 64-, 256-QAM (and the
 *      reference's BPSK), between ldpc_rate_match_device and ldpc_rate_recover_device, for data that stays in HBM.  The
 *      reference has no counterpart: Coder::test sends one real +-1 sample per code bit.
 * Spec: plain parameters -- no handle, no device state.  Qm in {1, 2, 4, 6, 8} bits per symbol; a transmission of E bits
 *   per frame needs E % Qm == 0 and has S = E / Qm symbols.  A frame's row of symbols holds ldpc_modem_symbol_floats
 *   floats: E real samples for Qm = 1, else 2 S (I0 Q0 I1 Q1 ...).  ldpc_modem_spec_init sets interleave = (Qm >= 2).
 * Interleaver (TS 38.212 section 5.4.2.2): bit i (0 <= i < Qm) of symbol j is tx bit
 *       e(i, j) = interleave ? i * S + j : j * Qm + i
 *   (Qm = 1: e = j either way).  ldpc_modem_index is host-only arithmetic: index_out[j * Qm + i] = e(i, j).
 * Mapper (TS 38.211 section 5.1, Gray): with m = Qm / 2 the I axis takes the symbol's bits c0, c1, ... = b0, b2, ...,
 *   the Q axis b1, b3, ....  The integer level of an axis is
 *       amp_0 = 0,  amp_k(c0, c1, ...) = (1 - 2 c0) * (2^(k-1) - amp_(k-1)(c1, ...))         level = amp_m
 *   ((1 - 2 b0) [2 - (1 - 2 b2)] for 16-QAM, and so on): the odd integers in +-(2^m - 1), neighbours differ in one bit.
 *       x = (float)amp * A,  A = (float)(1.0 / sqrt((double)norm)),  norm = 2, 10, 42, 170 for Qm = 2, 4, 6, 8
 *   (one fp32 multiply).  Qm = 1: x = 1 - 2 b exactly, one real sample per bit -- the reference's BPSK.
 *   ldpc_modem_points is host-only: the 2^Qm points, the one of label v = sum b_i 2^(Qm-1-i) at iq[2v], iq[2v+1]
 *   (Qm = 1: (1, 0) and (-1, 0)).
 * Channel: real sample n of frame f (n = 2 j for I and 2 j + 1 for Q of symbol j; n = e for Qm = 1) is
 *       r = (float)((double)x + (double)sd * z(seed, first_frame + f, n))
 *   with z the counter-based normal of csrc/ldpc_channel.h: component n % 4 of ldpc_ch_normal4(seed, frame, n / 4).  With
 *   Qm = 1 this is ldpc_ch_sample: the call reproduces ldpc_awgn_device bit for bit.  sd == 0 writes x itself and does not
 *   run the generator; sd < 0, NaN or inf is LDPC_ERR_ARG.  For Qm >= 2 the symbols have unit mean energy and sd is the
 *   standard deviation PER REAL DIMENSION, so Es/N0 = 1 / (2 sd^2); for Qm = 1 (one real dimension of energy 1) the
 *   reference's convention holds, Es/N0 = 1 / (2 sd^2) as well.
 * Demapper (max-log; fp32, no contraction, no knowledge of sd): per axis value r and axis bit k
 *       D_b = min over the 2^(m-1) levels x_j whose bit k is b of (r - x_j) * (r - x_j),     y = (D_1 - D_0) * 0.25f
 *   written to rx[f][e(i, j)], i.e. de-interleaved.  The x_j are the mapper's fp32 values; min is exact, so the result is
 *   bit-defined whatever order the minima are taken in.  Qm = 1: y = r.  y is in the decoders' units of channel values:
 *   positive <-> bit 0, the true max-log LLR is 2 y / sd^2 (for QPSK y = r A).  It is what ldpc_rate_recover_device takes
 *   as rx_dev, and what a decoder takes directly when E = N.  The values of one symbol's bits differ widely in
 *   reliability: LDPC_ALGO_SP then wants llr_scale = 2 / sd^2 instead of the reference's constant 8 (DESIGN.md has the
 *   figures), with llr_scale * |y| below the fp32 exp limit of 88.  Inputs must be finite (not checked).  sym and rx
 *   must not overlap (LDPC_ERR_ARG); neither may tx and sym.
 * tx_format is LDPC_CODE_BITS or LDPC_CODE_PACKED, the two forms ldpc_rate_match_device writes (packed: E % 8 == 0).
 *   sym_floats is the capacity of sym; less than frames * ldpc_modem_symbol_floats is LDPC_ERR_ARG.
 * The *_device calls enqueue on `stream` (a hipStream_t, NULL = default stream), return without waiting and allocate
 *   nothing; frames == 0 enqueues nothing.  ldpc_modem_transmit / ldpc_modem_demap take host buffers, block, and run the
 *   same kernels over chunks of frames (device scratch is allocated and released inside the call).  There is no CPU path.
 *   The pointer rules of ldpc_decode_device apply: sym_dev and rx_dev need 4-byte alignment and no more, tx_dev none.
 * Every argument error is LDPC_ERR_ARG with a message that names the field. */
typedef struct ldpc_modem_spec {
    uint32_t struct_size;          /* = sizeof(ldpc_modem_spec); ABI guard                                              */
    int32_t  Qm;                   /* bits per symbol: 1 (BPSK, real), 2 (QPSK), 4, 6, 8 (16-, 64-, 256-QAM)            */
    int32_t  interleave;           /* 1: the bit interleaver of TS 38.212 section 5.4.2.2; 0: a symbol takes Qm consecutive bits */
} ldpc_modem_spec;
void ldpc_modem_spec_init(ldpc_modem_spec *spec, int32_t Qm);
/* floats per frame of symbols; 0 (and a message) for a spec or E the other calls refuse */
int64_t ldpc_modem_symbol_floats(const ldpc_modem_spec *spec, int32_t E);
int ldpc_modem_index(const ldpc_modem_spec *spec, int32_t E, int32_t *index_out);
int ldpc_modem_points(int32_t Qm, float *iq);
int ldpc_modem_transmit_device(const ldpc_modem_spec *spec, const uint8_t *tx_dev, int32_t tx_format, int64_t frames, int32_t E,
                               float sd, uint64_t seed, int64_t first_frame, float *sym_dev, int64_t sym_floats, int32_t device,
                               void *stream);
int ldpc_modem_demap_device(const ldpc_modem_spec *spec, const float *sym_dev, int64_t frames, int32_t E, float *rx_dev,
                            int32_t device, void *stream);
int ldpc_modem_transmit(const ldpc_modem_spec *spec, const uint8_t *tx_host, int32_t tx_format, int64_t frames, int32_t E, float sd,
                        uint64_t seed, int64_t first_frame, float *sym_host, int64_t sym_floats, int32_t device);
int ldpc_modem_demap(const ldpc_modem_spec *spec, const float *sym_host, int64_t frames, int32_t E, float *rx_host, int32_t device);

/* ---- transport block: CRC attachment, segmentation into code blocks and filler bits in front of ldpc_encode_device; the
 *      CRC checks and the reassembly behind ldpc_decode_device (TS 38.212 sections 5.1 and 5.2.2), for data that stays in
 *      HBM.  The reference has no counterpart: it pushes K raw bits per frame and compares with the bytes it sent.
 * Bit order: the project's, LSB first -- bit i of a row is bit i % 8 of byte i / 8.
 * CRC (TS 38.212 section 5.1): g24A = 0x1864CFB, g24B = 0x1800063, g16 = 0x11021.  For bits a_0 .. a_(n-1) the parity
 *   p_0 .. p_(L-1) makes a_0 x^(n+L-1) + ... + a_(n-1) x^L + p_0 x^(L-1) + ... + p_(L-1) divisible by g: register zero, no
 *   reflection, no final XOR; the parity follows the data, p_0 first.  The nine ASCII bytes "123456789", each taken MSB
 *   first, give 0xCDE703 (24A), 0x23EF52 (24B) and 0x31C3 (16), p_0 being the top bit of the value.
 * Spec: plain parameters -- no handle, no device state.
 *       B = A + tb_crc,  B % C == 0,  S = B / C,  Kp = S + cb_crc <= K
 *   The stream of a transport block is its A payload bits followed by the tb_crc parity bits of those A bits (24: CRC24A).
 *   Code block c takes stream bits [c S, (c + 1) S) -- S % 8 need not be 0, a code block may start in the middle of a
 *   byte --, then the cb_crc parity bits of those S bits (CRC24B), then zeros: the filler bits [Kp, K) of every frame,
 *   known zeros, the filler_lo / filler_hi a caller passes to ldpc_rate_spec.
 *   ldpc_tb_spec_init applies the rule of section 5.2.2 with the code's K in place of Kcb: tb_crc = A > 3824 ? 24 : 16;
 *   B <= K: C = 1, cb_crc = 0; otherwise cb_crc = 24 and C = ceil(B / (K - 24)).  If B % C != 0 afterwards the spec is
 *   left as computed and the other calls refuse it.
 * ldpc_tb_layout (host only): out = {B, S, Kp, filler_lo = Kp, filler_hi = K, C}.
 * ldpc_crc_bits (host only): the CRC of the first nbits bits of a byte row, by long division.
 * ldpc_tb_attach_device: payload_dev holds tbs rows of A/8 bytes, src_dev receives tbs * C rows of K/8 bytes -- what
 *   ldpc_encode_device takes as src_dev with frames = tbs * C.  Frame t C + c is code block c of transport block t; every
 *   byte of every row is written.  src_bytes < tbs * C * K/8 is LDPC_ERR_ARG.
 * ldpc_tb_check_device: dec_dev holds tbs * C rows of K/8 bytes, as a decoder writes them with LDPC_PACK_BYTES.  The three
 *   outputs are nullable, at least one must be given.
 *       cb_ok_dev[f] = 1 if cb_crc == 0 or the first Kp bits of frame f leave remainder zero, else 0
 *       payload_dev  = the first A bits of the reassembled stream, tbs rows of A/8 bytes
 *       tb_ok_dev[t] = 1 if (tb_crc == 0 or the B reassembled bits leave remainder zero) and all C code blocks are ok
 *   Decoded filler bits are ignored.
 * ldpc_tb_tally_device: blocks, as ldpc_count_errors_device does; ref_dev NULL = all zero.  counts[0] = transport blocks
 *   with tb_ok == 0, [1] = blocks whose bytes_per_tb payload bytes differ from the reference, [2] = blocks that differ
 *   although tb_ok == 1 (undetected errors), [3] = blocks with tb_ok == 0 although the payload is equal (the damage is in
 *   parity bits only).
 * The *_device calls enqueue on `stream` (a hipStream_t, NULL = default stream), return without waiting and allocate
 *   nothing; byte buffers may have any alignment; nothing outside the stated sizes is read or written; overlapping input
 *   and output is LDPC_ERR_ARG; a refused call has enqueued nothing; tbs == 0 enqueues nothing.  ldpc_tb_attach /
 *   ldpc_tb_check take host buffers, block, and run the same kernels over chunks of whole transport blocks.  There is no
 *   CPU path.  Every argument error is LDPC_ERR_ARG with a message that names the field. */
enum ldpc_crc_kind { LDPC_CRC16 = 16, LDPC_CRC24A = 24, LDPC_CRC24B = 25 };
typedef struct ldpc_tb_spec {
    uint32_t struct_size;          /* = sizeof(ldpc_tb_spec); ABI guard                                                 */
    int32_t  A;                    /* payload bits per transport block; A % 8 == 0, A >= 8                              */
    int32_t  tb_crc;               /* CRC on the transport block: 0, 16 or 24 (CRC24A)                                  */
    int32_t  C;                    /* code blocks per transport block, >= 1                                             */
    int32_t  cb_crc;               /* CRC on each code block: 0 or 24 (CRC24B)                                          */
    int32_t  K;                    /* information bits of the code; K % 8 == 0                                          */
} ldpc_tb_spec;
void ldpc_tb_spec_init(ldpc_tb_spec *spec, int32_t A, int32_t K);
int ldpc_tb_layout(const ldpc_tb_spec *spec, int32_t out[6]);
int ldpc_crc_bits(int32_t kind, const uint8_t *bytes, int64_t nbits, uint32_t *crc);
/* Host only.  ldpc_crc_weights: w[n], n < nbits, is the ldpc_crc_bits of the unit vector e_n of nbits bits; the CRC is
 *   linear, so the XOR of the weights of a row's set bits is the row's CRC (what the decoders' CRC test computes).
 * ldpc_tb_frame_crc: the CRC every FRAME of a spec carries, as the decoder config's (crc_kind, crc_bits):
 *   cb_crc == 24: (LDPC_CRC24B, Kp); C == 1 with tb_crc 16 or 24: (LDPC_CRC16 or LDPC_CRC24A, Kp); otherwise LDPC_ERR_ARG
 *   -- the frames have no CRC of their own (the transport block's CRC spans several frames, or there is none). */
int ldpc_crc_weights(int32_t kind, int32_t nbits, uint32_t *w);
int ldpc_tb_frame_crc(const ldpc_tb_spec *spec, int32_t *kind, int32_t *bits);
int ldpc_tb_attach_device(const ldpc_tb_spec *spec, const uint8_t *payload_dev, int64_t tbs, uint8_t *src_dev, int64_t src_bytes,
                          int32_t device, void *stream);
int ldpc_tb_check_device(const ldpc_tb_spec *spec, const uint8_t *dec_dev, int64_t tbs, uint8_t *payload_dev, uint8_t *cb_ok_dev,
                         uint8_t *tb_ok_dev, int32_t device, void *stream);
int ldpc_tb_tally_device(const uint8_t *tb_ok_dev, const uint8_t *payload_dev, const uint8_t *ref_dev, int64_t tbs,
                         int64_t bytes_per_tb, int64_t counts[4], int32_t device, void *stream);
int ldpc_tb_attach(const ldpc_tb_spec *spec, const uint8_t *payload_host, int64_t tbs, uint8_t *src_host, int64_t src_bytes,
                   int32_t device);
int ldpc_tb_check(const ldpc_tb_spec *spec, const uint8_t *dec_host, int64_t tbs, uint8_t *payload_host, uint8_t *cb_ok_host,
                  uint8_t *tb_ok_host, int32_t device);

/* ---- outer code: a binary BCH code around the information bits of a frame, in front of ldpc_encode_device and behind a
 *      decoder, as a DVB-S2 frame is BCH o LDPC: it removes the few wrong bits a decoder leaves at its round budget and tells
 *      the receiver whether a frame is good without the sent bytes.  A plain parameter set and a row layout, as
 *      ldpc_tb_spec is: no handle, no device state visible to the caller (the library caches derived plans; the cache is
 *      thread-safe).  "DVB-S2-profile": the generator is computed from the field polynomial, it has not been compared
 *      with the polynomials the standard prints.
 *
 * The rule, bit for bit (project bit order: bit i of a row is bit i % 8 of byte i / 8):
 *   Field GF(2^m) = GF(2)[x] / prim, alpha = x.  g(x) = lcm of the minimal polynomials over GF(2) of alpha^j,
 *   j = 1 .. 2t; r = deg g, k = n - r.  n <= 2^m - 1 (a shortened code), n % 8 == 0, k >= 8 and k % 8 == 0.
 *   ldpc_bch_spec_init: m = 14, prim = 0x402B (x^14+x^5+x^3+x+1) for n <= 16383, else m = 16, prim = 0x1002D
 *   (x^16+x^5+x^3+x^2+1); callers may overwrite m and prim.  r = 168 / 140 / 112 and 192 / 160 / 128 at t = 12 / 10 / 8.
 *   Polynomials as in the CRC section: bit i of the n code bits is the coefficient of x^(n-1-i).  The message
 *   a_0 .. a_(k-1) is followed by the parity p_0 .. p_(r-1), p(x) = x^r a(x) mod g(x) with a(x) = sum a_i x^(k-1-i) and
 *   p(x) = sum p_j x^(r-1-j): register zero, no reflection, no final XOR.
 *   Encode: row f of src receives bits [0, k) = payload row f (k/8 bytes), bits [k, n) the parity, bits
 *   [n, 8 row_bytes) zeros; every byte of every row is written.  With row_bytes = K/8 the result is what
 *   ldpc_encode_device takes as src_dev.
 *   Syndromes of received bits v_i: S_j = v(alpha^j), j = 1 .. 2t, v(x) = sum v_i x^(n-1-i); an error at bit i has
 *   locator alpha^(n-1-i).
 *   Decode, a bounded-distance decoder defined by its result: all S_j = 0: status 0.  Else, if a set P of bit positions
 *   in [0, n) with 1 <= |P| <= t exists whose flipping makes all 2t syndromes zero (it is unique, d >= 2t + 1): the
 *   bits are flipped and status = |P|.  Otherwise status = -1 and no bit is changed.  Positions >= n never count as
 *   error positions (a locator polynomial with a root outside [0, n) is a failure); bits [n, 8 row_bytes) of the input
 *   are ignored.  Outputs, each nullable, at least one given: payload_dev, frames * k/8 bytes, the first k bits after
 *   the flips; status_dev, one int32 per frame.
 *   Tally (blocks, as ldpc_tb_tally_device; ref_dev NULL = all zero): counts[0] = frames with status -1, [1] = frames
 *   whose payload differs from ref, [2] = frames that differ although status >= 0 (miscorrected or undetected),
 *   [3] = frames with status > 0, [4] = sum of the positive statuses (bits corrected), [5] = frames with status -1
 *   although the payload is equal.
 *
 * ldpc_bch_layout (host only): out = {k, r, number of distinct minimal polynomials, m}.
 * ldpc_bch_generator (host only): the coefficients g_0 .. g_r (one byte each, 0 or 1) of any valid (m, prim, t), without
 *   the byte rules on n and k; *r receives the degree; g may be NULL (then only *r), cap < r + 1 is LDPC_ERR_ARG.
 * The pointer rules of ldpc_decode_device apply to the *_device calls, which enqueue on `stream`, return without waiting
 *   and allocate nothing: byte buffers may have any alignment, status_dev needs its natural 4-byte alignment; nothing
 *   outside the stated sizes is read or written (dec: frames * row_bytes bytes; src_bytes < frames * row_bytes is
 *   LDPC_ERR_ARG); overlapping input and output is LDPC_ERR_ARG; a refused call has enqueued nothing; frames == 0 enqueues
 *   nothing.  ldpc_bch_encode / ldpc_bch_decode take host buffers, block, and run the same kernels over chunks of
 *   frames.  There is no CPU path.  Every argument error -- m outside 4 .. 16, a prim that is not primitive, t outside
 *   1 .. 12 or 2t >= 2^m - 1, n, k, row_bytes, struct_size -- is LDPC_ERR_ARG with a message that names the field. */
typedef struct ldpc_bch_spec {
    uint32_t struct_size;          /* = sizeof(ldpc_bch_spec); ABI guard                                                 */
    int32_t  m;                    /* field GF(2^m) = GF(2)[x] / prim, alpha = x; 4 <= m <= 16                          */
    uint32_t prim;                 /* field polynomial, bit i = coefficient of x^i, x^m term included; must be primitive */
    int32_t  t;                    /* designed correction capability, 1 <= t <= 12, 2t < 2^m - 1                        */
    int32_t  n;                    /* code bits per frame (message + parity), n <= 2^m - 1 (shortened), n % 8 == 0       */
    int32_t  row_bytes;            /* bytes per frame row on the encoder/decoder side, 8 * row_bytes >= n (e.g. K / 8)   */
} ldpc_bch_spec;
void ldpc_bch_spec_init(ldpc_bch_spec *spec, int32_t n, int32_t t, int32_t row_bytes);
int ldpc_bch_layout(const ldpc_bch_spec *spec, int32_t out[4]);
int ldpc_bch_generator(int32_t m, uint32_t prim, int32_t t, uint8_t *g, int32_t cap, int32_t *r);
int ldpc_bch_encode_device(const ldpc_bch_spec *spec, const uint8_t *payload_dev, int64_t frames, uint8_t *src_dev, int64_t src_bytes,
                           int32_t device, void *stream);
int ldpc_bch_decode_device(const ldpc_bch_spec *spec, const uint8_t *dec_dev, int64_t frames, uint8_t *payload_dev, int32_t *status_dev,
                           int32_t device, void *stream);
int ldpc_bch_tally_device(const int32_t *status_dev, const uint8_t *payload_dev, const uint8_t *ref_dev, int64_t frames,
                          int64_t bytes_per_frame, int64_t counts[6], int32_t device, void *stream);
int ldpc_bch_encode(const ldpc_bch_spec *spec, const uint8_t *payload_host, int64_t frames, uint8_t *src_host, int64_t src_bytes,
                    int32_t device);
int ldpc_bch_decode(const ldpc_bch_spec *spec, const uint8_t *dec_host, int64_t frames, uint8_t *payload_host, int32_t *status_host,
                    int32_t device);

/* ---- ordered-statistics post-processing (OSD, orders 0 and 1) behind a decoder with soft output: the frames whose hard
 *      decision has a dirty syndrome are re-encoded from their most reliable independent positions, optionally with every
 *      single flip among them tried.  The output of a processed frame is always a codeword.  For short codes, where belief
 *      propagation stops well short of maximum likelihood; the reference has no counterpart.
 *
 * The rule, bit for bit.  ldpc_osd_device is a pure function of the graph H (M x N), the soft values, `order` and
 * `weight_scale`.  Input: frame f's row p_0 .. p_(N-1) of fp32 posteriors, as ldpc_decode_soft_device(...,
 * LDPC_SOFT_POSTERIOR) writes them; positive <-> bit 0.
 *   1. Hard bits.  h_n = (p_n < 0): zeros and NaN read as bit 0.  The stage takes its own hard decision, so it does not
 *      depend on which decoder produced p.
 *   2. Weights, integers, so that every sum below is exact and order-free:
 *        t = fabsf(p_n) * weight_scale                               one fp32 multiply
 *        w_n = (p_n != p_n) ? 0 : (int32)floorf(fminf(t, 65535.0f))
 *      weight_scale must be finite and > 0, else LDPC_ERR_ARG.  A good default is 256: LLR units for the sum-product
 *      decoders, a resolution of 1/256 of a channel unit for min-sum posteriors.
 *   3. Order.  Position n precedes n' iff (w_n, n) < (w_n', n') lexicographically: the least reliable first, ties to the
 *      index.
 *   4. Least reliable basis.  Scan the positions in that order; a position joins the pivot set P iff its column of H is
 *      linearly independent over GF(2) of the columns already in P.  |P| = rank(H) = rho <= M; the free set F is the other
 *      N - rho positions.  For any bits on F there is exactly one codeword, so the result does not depend on which rows an
 *      implementation pivots on.
 *   5. Metric.  D(c) = sum of w_n over the n with c_n != h_n.  It fits int32: N <= 4096 and w <= 65535.
 *   6. Order 0.  c0 is the codeword that agrees with h on F.
 *   7. Order 1.  For every j in F, c^j is the codeword that agrees with h on F except at j.  The result is the candidate of
 *      the smallest D among c0 and all c^j; on a tie c0 wins, then the smallest position j.
 *   8. Which frames.  A frame whose h has a zero syndrome is left alone; every other frame is processed.
 *   9. Outputs per frame, each nullable, at least one given:
 *        code_dev    N bytes, 0 or 1 (LDPC_CODE_BITS layout): the chosen codeword, or h for an untouched frame;
 *        out_dev     the first K bits of that row, packed as the decoders' LDPC_PACK_BYTES does for K % 8 == 0: K/8 bytes
 *                    at byte f * K/8, LSB first; K % 8 != 0 with out_dev given is LDPC_ERR_ARG; every frame's bytes are
 *                    written;
 *        status_dev  int32: 0 = the frame was clean and untouched, 1 = c0 was chosen, 2 = a flip was chosen;
 *        metric_dev  int32: D of the chosen codeword, 0 for an untouched frame.
 *
 * The handle owns the dense bit image of H (built from the graph on the host, uploaded once), the graph's rows for the
 *   syndrome and one dirty flag per frame.  Eligibility is a fixed rule -- both N <= 4096 and M * ceil(N / 32) <= 28672
 *   32-bit words (112 KiB of the 160 KiB of LDS a workgroup can have; the rest holds keys, weights, pivot bookkeeping and
 *   the candidate search) -- anything larger is LDPC_ERR_UNSUPPORTED with both numbers in the message.  802.16e (576, 288),
 *   (1152, 576), (1152, 960) and the BG1-profile test code (1088, M = 736) fit; (2304, 1152) does not.
 * ldpc_osd_create: K outside (0, N], max_frames <= 0 are LDPC_ERR_ARG.  On a machine without a device the handle is still
 *   made (host analysis only), so that the argument checks of the compute calls answer everywhere; the compute calls then
 *   give LDPC_ERR_HIP after their argument checks.  There is no CPU path.
 * ldpc_osd_device: enqueues on `stream` (a hipStream_t, NULL = default stream), returns without waiting and allocates
 *   nothing; no host round trip decides which frames are dirty.  The pointer rules of ldpc_decode_device apply: soft_dev,
 *   status_dev and metric_dev need 4-byte alignment and no more, byte buffers any; nothing outside the sizes stated for
 *   `frames` frames is read or written; frames == 0 enqueues nothing; a refused call has enqueued nothing.  LDPC_ERR_ARG,
 *   with a message that names the field: order outside {0, 1}, a bad weight_scale, frames > max_frames, out_bytes <
 *   frames * K/8, no output given, an output that overlaps soft_dev or another output.
 * ldpc_osd_run: the same on host buffers, blocking, in chunks of max_frames (frames is not limited); its first call
 *   allocates the staging buffers.
 * ldpc_osd_info: out = {M, N, words per row = ceil(N / 32), LDS bytes of one workgroup}.
 * A handle is not re-entrant: one per host thread / stream. */
typedef struct ldpc_osd ldpc_osd;
int ldpc_osd_create(const ldpc_graph *g, int32_t K, int32_t max_frames, int32_t device, ldpc_osd **out);
int ldpc_osd_destroy(ldpc_osd *o);
int ldpc_osd_device(ldpc_osd *o, const float *soft_dev, int64_t frames, int32_t order, float weight_scale, uint8_t *out_dev,
                    int64_t out_bytes, uint8_t *code_dev, int32_t *status_dev, int32_t *metric_dev, void *stream);
int ldpc_osd_run(ldpc_osd *o, const float *soft_host, int64_t frames, int32_t order, float weight_scale, uint8_t *out_host,
                 int64_t out_bytes, uint8_t *code_host, int32_t *status_host, int32_t *metric_host);
int ldpc_osd_info(const ldpc_osd *o, int32_t out[4]);

/* ---- measurement aid: the rate a plain float4 copy of `bytes` bytes (read + write counted)
 *      sustains on `device` right now, best of `reps` launches each with the default cache policy
 *      and with non-temporal loads and stores (the streaming kernels' policy), HIP-event timed on
 *      a stream of its own.  *copy_gbs = the better of the two; by_policy (may be NULL) receives
 *      {default, non-temporal}.  The benchmark reports it next to its roofline figures so that a kernel's fraction of
 *      the 8 TB/s specification can also be read against what the box at hand delivers. */
int ldpc_hbm_probe_device(int32_t device, int64_t bytes, int32_t reps, double *copy_gbs, double *by_policy);
/* The non-temporal copy back to back for `milliseconds` (the first third untimed): the rate the box SUSTAINS.
 * The boxes of this pool drop to about 5.2 TB/s under load at times while a burst still shows 6.4. */
int ldpc_hbm_sustained_device(int32_t device, int64_t bytes, int32_t milliseconds, double *copy_gbs);

/* ---- diagnostics of the host-buffer path (no device is touched) --------------------------------
 * ldpc_host_block_plan: the page arithmetic of LDPC_HOST_INPUT_LOCK_PAGES for launch group `group` of a
 *      call over `frames` frames of N floats, `max_batch` frames per group, first byte at address `base`:
 *      out[0..1] = the group's bytes [s0, s1); out[2..3] = the page-locked block [b0, b1) (equal: none);
 *      out[4] = end of the DMA-read body [b0, body_end); out[5] = 1 if the CPU copies the whole group.
 * ldpc_host_locked_ranges: ranges of caller memory this library holds page-locked right now (*live,
 *      0 between calls) and ranges it failed to release (*stale, 0 unless hipHostUnregister failed). */
int ldpc_host_block_plan(uint64_t base, int64_t frames, int32_t N, int32_t max_batch, int64_t group, uint64_t out[6]);
int ldpc_host_locked_ranges(int64_t *live, int64_t *stale);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_HIP_H_ */
