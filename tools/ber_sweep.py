#!/usr/bin/env python3
"""BER / FER versus SNR on the GPU, in the reference's convention (Test.cpp:56-57):
BPSK +-1, sd = 10^(-SNR_dB/20), all-zero codeword (valid for every linear code; --payload random: random source
bytes drawn on the device and encoded there by ldpc_encode_device, which also sees a decoder that is biased towards 0), channel values
generated in HBM by ldpc_awgn_device (counter-based noise, csrc/ldpc_channel.h: frame f of batch
b is frame b*frames + f of the seed's stream, so a point can be extended or re-run on any rank)
and errors counted by ldpc_count_errors_device; nothing crosses PCIe but the counts.  The
reference counts differing BYTES (Test.cpp:105-110); this prints byte errors too.

    python tools/ber_sweep.py [--code dvbs2_12|dvbs2_910|bg1|wimax:<rate>:<N> | --alist PATH] [--algo sp|ms|layered|bp|layered_bp|layered_fx|layered_bp_fx|bitflip]
                              [--payload zero|random] [--rate-match P,FLO,FHI,E[,K0]] [--erasure-llr X]
                              [--modulation bpsk|qpsk|qam16|qam64|qam256] [--no-interleave] [--transport-block A[,C]] [--crc-stop] [--bch T[,N]]
                              [--msg-dtype f32|f16|f8|i8 [--msg-bits Q --llr-scale S]] [--post-bits P] [--fx-record] [--frac-bits F] [--soft-check] [--osd 0|1 [--osd-scale S]]
                              [--snr=1.0,1.5,...]  (write --snr=-0.5,0 for a list that starts with a minus) [--frames 4096] [--iters 50]
--rate-match: code bits [0, P) punctured, [FLO, FHI) filler bits (known zeros; multiples of 8, inside the information part),
E bits per frame sent from circular-buffer position K0 (default 0): ldpc_rate_match_device between the encoder and the
channel, ldpc_rate_recover_device between the channel and the decoder -- the whole chain stays in HBM.  --erasure-llr 1e-6
whenever --algo layered reads punctured or unsent positions (include/ldpc_hip.h, "the erasure rule").
--modulation: the ldpc_awgn_device step becomes ldpc_modem_transmit_device + ldpc_modem_demap_device (include/ldpc_hip.h,
"modem"): the bits of a frame (E with --rate-match, else N; a multiple of the bits per symbol) travel as symbols of unit
mean energy, sd = 10^(-SNR_dB/20) is the noise PER REAL DIMENSION, and every point also prints Es/N0 = 1/(2 sd^2) and
Eb/N0 = Es/N0 / (bits per symbol x rate).  --no-interleave switches the bit interleaver of TS 38.212 off.  With --algo sp
the decoder's llr_scale follows the noise, 2 / sd^2 per point (and the fillers read min(10, 80 / llr_scale)), unless
--llr-scale is given.  From 16-QAM up use --payload random: the all-zero codeword sends one corner point only, and the
bits of a QAM symbol are not equally protected.
--algo bp (the log-domain sum-product, include/ldpc_hip.h: LDPC_ALGO_BP) reads LLRs: its llr_scale follows the noise, 2 / sd^2
per point, with any modulation and with none, unless --llr-scale is given; --msg-dtype f16, --soft-check and --crc-stop apply.
--algo layered_bp (LDPC_ALGO_LAYERED_BP: the layered schedule with bp's check node) reads LLRs in the same way; like --algo
layered it needs a code with a circulant size (bg1, wimax:...), it is fp32 only, and it takes exact zeros (no --erasure-llr).
--algo layered_fx (LDPC_ALGO_LAYERED_FX: the layered schedule in fixed point) takes --msg-bits Q, --post-bits P (the
saturating posterior memory) and --llr-scale S, the LSBs per unit of channel value; --ms-offset is in LSBs; --fx-record runs it
on the fixed-point record kernel (one launch, same results; not with --crc-stop).
--algo layered_bp_fx (LDPC_ALGO_LAYERED_BP_FX: layered_fx with box-plus rows from a correction table) takes --msg-bits Q,
--post-bits P, --frac-bits F (one LSB is 2^-F LLR units, 0 ... 4) and --llr-scale S, the LSBs per unit of channel value;
without --llr-scale it follows the noise, 2^F * 2 / sd^2 per point: the channel LLR in LSBs.  No --ms-scale / --ms-offset.
--transport-block A[,C] (with --payload random): the random bytes are transport blocks of A payload bits; ldpc_tb_attach_device
in front of the encoder adds the transport block's CRC, cuts it into C code blocks with CRC24B each (C omitted: the rule of
ldpc_tb_spec_init) and fills up to K with zeros; ldpc_tb_check_device and ldpc_tb_tally_device behind the decoder judge the
blocks as a receiver does, without the bytes that were sent (include/ldpc_hip.h, "transport block").  --frames must be a
multiple of C.  Every point also prints the block error rate (blocks whose payload is wrong), the blocks whose CRCs failed
(detected), the wrong blocks whose CRCs passed (undetected) and the right blocks whose CRCs failed (parity only).  The
fillers [Kp, K) are sent unless --rate-match names them.
--bch T[,N] (with --payload random; not with --transport-block): the random bytes are the k = N - r message bits of a BCH code
that corrects T errors (N omitted: K; include/ldpc_hip.h, "outer code"); ldpc_bch_encode_device in front of the encoder adds the
parity (and zero fillers up to K), ldpc_bch_decode_device behind the decoder repairs up to T wrong bits per frame.  Every point
also prints the frames with a wrong bit among the N code bits after the LDPC decoder and the frames whose payload is wrong
after the outer code, the frames it repaired, could not decode (status -1) and miscorrected, the bits it repaired, and
residual_hist: how many frames the LDPC decoder left with 0, 1 .. T and more than T wrong bits (T + 2 bins).

--crc-stop (with --transport-block whose frames carry a CRC of their own: C = 1, or C > 1 with CRC24B): the decoder also stops
a frame in the first round in which its first Kp bits pass that CRC (include/ldpc_hip.h: crc_kind / crc_bits; the streaming
kernels then run).  Every point of a --transport-block run prints crc_stops, the frames stopped in a round in which their
syndrome was not clean (0 without --crc-stop), next to the block counts -- blocks_undetected is where a false pass would show.
--soft-check (not with --algo sp): every batch is decoded a second time through ldpc_decode_soft_device; every point prints
soft_checked, the posteriors of the K output bits that are finite and not zero, soft_sign_disagreements, those whose sign is
not the output bit, and soft_bytes_differ against the plain call -- the last two must be 0, the run fails otherwise.
--osd 0|1 (not with --algo sp; short codes: N <= 4096 and M * ceil(N / 32) <= 28672, e.g. wimax:0:576): the batch is decoded
through ldpc_decode_soft_device and the frames whose posterior has a dirty syndrome go through ordered-statistics decoding of
that order (include/ldpc_hip.h, "ordered-statistics post-processing"; ldpc_osd_device, weight_scale --osd-scale, default 256).
Every point also prints frame_errors_before_osd / frame_errors_after_osd (frames whose K information bits are wrong),
osd_processed (frames with a dirty syndrome), osd_flipped (frames where a flip was chosen) and osd_ms_per_batch (HIP events
around ldpc_osd_device).  fer, ber and the error counts are those of the decoder alone.
--alist PATH (in place of --code): any parity-check matrix in MacKay's alist format (codes.load_alist).  Its columns are put into
the systematic order of ldpc_graph_systematic_order (include/ldpc_hip.h, "encoder for any H"; rho = rank(H), K = N - rho and
whether the order was the identity are printed), the decoder runs on the re-ordered matrix, and --payload random encodes with the
dense encoder (ldpc_encoder_create_dense).  Flooding algorithms only (--algo sp, ms or bp; no circulant size is known).  K % 8 != 0
is fine: the bits between the frames of the byte stream are zero on both sides and the frame errors are counted per frame's bytes.
--algo bitflip (LDPC_ALGO_BITFLIP: hard-decision parallel bit flipping) reads only the sign of a channel value: the
hard-decision baseline of a code.  --bf-threshold O1,O2,... gives up to 16 round offsets (the last one repeats).  No --soft-check,
--osd, --ms-scale / --ms-offset or --msg-dtype.
--channel bsc --crossover P1,P2,... (in place of --snr; BPSK without --modulation or --rate-match): a binary symmetric channel.
Every value is the SIGN (+-1) of the ldpc_awgn_device value at sd = 1 / Qinv(P), the noise at which a hard decision on BPSK
is wrong with probability P: the same counter-based generator, identical on the host, and no second channel kernel.  Every
point prints crossover and the sd it used; snr_db is that sd's.  Any --algo takes it: a soft decoder then sees what bitflip sees.
The DVB-S2 / BG1 codes are PROFILE SURROGATES (codes.py): the numbers are not the standards'."""
import argparse, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import myldpccppapi_amd as L
from myldpccppapi_amd import codes

ap = argparse.ArgumentParser()
ap.add_argument("--code", default="dvbs2_12")
ap.add_argument("--alist", default=None, metavar="PATH", help="in place of --code: H from an alist file, re-ordered to be systematic; flooding algorithms only")
ap.add_argument("--algo", default="sp")
ap.add_argument("--snr", default="2.5,3.0,3.5,4.0,4.5,5.0")
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--llr-scale", type=float, default=None, help="channel scale of sp and bp (sp: default 8, with --modulation 2 / sd^2 per point; bp: 2 / sd^2 per point); "
                                                                  "with --msg-dtype i8 the LSBs per unit of channel value (default 8)")
ap.add_argument("--batches", type=int, default=1, help="batches of --frames per SNR point")
ap.add_argument("--seed", type=int, default=20260101)
ap.add_argument("--ms-scale", type=float, default=0.0, help="normalized min-sum factor (ms / layered; 0 = off)")
ap.add_argument("--ms-offset", type=float, default=0.0, help="offset min-sum offset, units of y -- with --msg-dtype i8: LSBs (0 = off)")
ap.add_argument("--payload", choices=("zero", "random"), default="zero",
                help="random: source bytes drawn on the device, encoded by ldpc_encode_device, errors counted against them")
ap.add_argument("--rate-match", default=None, metavar="P,FLO,FHI,E[,K0]", help="puncture [0,P), fillers [FLO,FHI), send E bits from K0")
ap.add_argument("--erasure-llr", type=float, default=0.0, help="decoder input at positions that were not received (0, or 1e-6 for layered)")
ap.add_argument("--modulation", choices=("bpsk", "qpsk", "qam16", "qam64", "qam256"), default=None,
                help="send symbols through ldpc_modem_transmit_device + ldpc_modem_demap_device instead of ldpc_awgn_device")
ap.add_argument("--no-interleave", action="store_true", help="with --modulation: no bit interleaver")
ap.add_argument("--transport-block", default=None, metavar="A[,C]",
                help="with --payload random: A payload bits per transport block, C code blocks (default: the rule of ldpc_tb_spec_init)")
ap.add_argument("--bch", default=None, metavar="T[,N]",
                help="with --payload random: outer BCH code that corrects T errors over N code bits (default: K)")
ap.add_argument("--msg-dtype", choices=("f32", "f16", "f8", "i8"), default="f32",
                help="message storage (f16: --algo ms and bp; f8: --algo ms; i8: --algo ms, layered_fx and layered_bp_fx, saturating "
                     "integers of --msg-bits bits, channel c = sq(--llr-scale * y), --ms-offset in LSBs; --algo layered_fx and "
                     "layered_bp_fx imply i8)")
ap.add_argument("--msg-bits", type=int, default=0, help="with --msg-dtype i8: 4, 5, 6 or 8 bits per message (0 = 8)")
ap.add_argument("--fx-record", action="store_true", help="--algo layered_fx: the fixed-point record kernel (LDPC_TUNE_FX_RECORD), same results")
ap.add_argument("--post-bits", type=int, default=0, help="--algo layered_fx and layered_bp_fx: bits of the saturating posterior memory, --msg-bits ... 16 (0 = 16)")
ap.add_argument("--frac-bits", type=int, default=0, help="--algo layered_bp_fx: fractional bits of an LSB, 0 ... 4 (one LSB = 2^-F LLR units)")
ap.add_argument("--bf-threshold", default=None, metavar="O1,O2,...", help="--algo bitflip: up to 16 round offsets in [0, 62], the last one repeats (default: off(i) = i - 1)")
ap.add_argument("--channel", choices=("awgn", "bsc"), default="awgn", help="bsc: the sign of the AWGN value at the sd whose hard decision errs with --crossover")
ap.add_argument("--crossover", default="0.01,0.02,0.03", help="with --channel bsc: the crossover probabilities, in place of --snr")
ap.add_argument("--llr-type", choices=("f32", "f16", "i8"), default="f32",
                help="quantise the channel values on the device (ldpc_llr_quantize_device) behind the channel / rate-recover step "
                     "and decode them through ldpc_decode_typed_device")
ap.add_argument("--llr-unit", type=float, default=None, help="with --llr-type f16 / i8: the decoder reads y = x * unit (default: "
                                                             "i8 0.05, f16 1/256)")
ap.add_argument("--crc-stop", action="store_true", help="with --transport-block: frames also stop once their CRC passes")
ap.add_argument("--soft-check", action="store_true",
                help="every batch is decoded once more with soft output (not --algo sp): prints the finite non-zero posteriors whose sign "
                     "disagrees with the output bit -- must be 0")
ap.add_argument("--osd", type=int, choices=(0, 1), default=None, help="ordered-statistics decoding of that order behind the decoder (not --algo sp)")
ap.add_argument("--osd-scale", type=float, default=256.0, help="with --osd: weight_scale")
args = ap.parse_args()
if args.algo in ("layered_fx", "layered_bp_fx"):
    args.msg_dtype = "i8"           # the algorithm is defined on fixed-point messages alone
assert args.algo != "bitflip" or (args.osd is None and not args.soft_check), "--algo bitflip has no soft output (include/ldpc_hip.h)"
assert args.channel == "awgn" or not (args.modulation or args.rate_match), "--channel bsc: BPSK without --modulation or --rate-match"
assert args.osd is None or args.algo != "sp", "--osd: sum-product has no soft output (include/ldpc_hip.h)"
assert not (args.soft_check and args.algo == "sp"), "--soft-check: sum-product has no soft output (include/ldpc_hip.h)"
assert not args.transport_block or args.payload == "random", "--transport-block needs --payload random"
assert args.transport_block or not args.crc_stop, "--crc-stop needs --transport-block"
assert not args.bch or args.payload == "random", "--bch needs --payload random"
assert not (args.bch and args.transport_block), "--bch and --transport-block exclude one another: a frame carries one of the two"
assert args.modulation or not args.no_interleave, "--no-interleave needs --modulation"
QM = {None: 0, "bpsk": 1, "qpsk": 2, "qam16": 4, "qam64": 6, "qam256": 8}[args.modulation]
# llr_scale = 2 / sd^2 per SNR point: sp behind a demapper, bp always (its messages are LLRs)
matched = ((bool(QM) and args.algo == "sp") or args.algo in ("bp", "layered_bp", "layered_bp_fx")) and args.llr_scale is None
# the matched scale in the decoder's units: LLR units, for layered_bp_fx LSBs of 2^-F LLR units
llr_unit_scale = float(1 << args.frac_bits) if args.algo == "layered_bp_fx" else 1.0

layer = 0
if args.alist:
    if args.algo not in ("sp", "ms", "bp"):
        ap.error("--alist: flooding algorithms only (--algo sp, ms or bp): an alist file names no circulant size for --algo %s" % args.algo)
    rows, cols, M0, N = codes.load_alist(args.alist)
    perm, rho = L.systematic_order(L.Graph(rows, cols, M0, N))
    rows, cols = codes.permute_columns(rows, cols, perm)
    K = N - rho
    args.code = "alist:" + os.path.basename(args.alist)
    print("alist %s: M=%d N=%d rho=rank(H)=%d K=%d (%d redundant rows) column order %s" % (
        args.alist, M0, N, rho, K, M0 - rho, "is the identity" if np.array_equal(perm, np.arange(N)) else "re-ordered"))
elif args.code == "dvbs2_12":
    N, K = 64800, 32400
    rows, cols = codes.dvbs2_profile_edges(N, K)
elif args.code == "dvbs2_910":
    N, K = 64800, 58320
    rows, cols = codes.dvbs2_profile_edges(N, K)
elif args.code == "bg1":
    Z = 384
    N, K, layer = 68 * Z, 22 * Z, Z
    rows, cols = codes.nr_bg1_profile_edges(Z)
else:
    _, rate, N = args.code.split(":")
    rate, N = int(rate), int(N)
    K, M, layer = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
M = M0 if args.alist else N - K
assert layer or args.algo not in ("layered", "layered_bp", "layered_fx", "layered_bp_fx"), "--algo %s needs the code's circulant size z: --code bg1 or wimax:<rate>:<N>" % args.algo
g = L.Graph(rows, cols, M, N)
B = args.frames
tb = None
if args.transport_block:
    tbv = [int(x) for x in args.transport_block.split(",")]
    tb = L.TransportBlock(tbv[0], K, C=tbv[1] if len(tbv) > 1 else None)
crc_kind, crc_bits = tb.frame_crc() if args.crc_stop else (0, 0)
bch = None
if args.bch:
    bv = [int(x) for x in args.bch.split(",")]
    bch = L.BchCode(bv[1] if len(bv) > 1 else K, bv[0], row_bytes=K // 8)


def make_decoder(llr_scale):
    return L.Decoder(g, K, max_batch=B, algo=args.algo, max_iter=args.iters, llr_scale=llr_scale,
                     layer_rows=layer, poll_interval=2, ms_scale=args.ms_scale, ms_offset=args.ms_offset,
                     crc_kind=crc_kind, crc_bits=crc_bits, msg_dtype=args.msg_dtype, msg_bits=args.msg_bits, post_bits=args.post_bits,
                     bp_frac_bits=args.frac_bits, tune={"fx_record": True} if args.fx_record else None,
                     bf_threshold=[int(v) for v in args.bf_threshold.split(",")] if args.bf_threshold else None)


dec = None if matched else make_decoder(8.0 if args.llr_scale is None else args.llr_scale)
out = torch.empty(L.out_bytes(K, B), dtype=torch.uint8, device="cuda")
it = torch.empty(B, dtype=torch.int32, device="cuda")
from myldpccppapi_amd import channel
import time
y = torch.empty((B, N), dtype=torch.float32, device="cuda")
enc = src = code = None
if args.payload == "random":
    assert K % 8 == 0 or args.alist, "--payload random compares whole bytes per frame: K % 8 must be 0"
    enc = L.DenseEncoder(g, K, max_frames=B) if args.alist else L.Encoder(g, K, layer, max_frames=B)
    src = torch.empty(L.out_bytes(K, B), dtype=torch.uint8, device="cuda")
    code = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
# K % 8 != 0 (--alist): frame f owns the K/8 bytes from byte (f K)/8 on; the bytes between frames are zero on both sides
frame_bytes = between = None
if K % 8:
    frame_bytes = (torch.arange(B, dtype=torch.int64, device="cuda") * K // 8)[:, None] + torch.arange(K // 8, dtype=torch.int64, device="cuda")
    between = torch.ones(L.out_bytes(K, B), dtype=torch.bool, device="cuda")
    between[frame_bytes.reshape(-1)] = False


def count_errors(out_t):
    """(bit, byte, frame) errors of the decoded bytes against the source (all zero without --payload random)"""
    if frame_bytes is None:
        return channel.count_errors_device(out_t, src, B)
    bits, byts, _ = channel.count_errors_device(out_t, src, 1)
    diff = out_t if src is None else out_t ^ src
    return bits, byts, int((diff[frame_bytes] != 0).any(dim=1).sum())


pay = back = cb_ok = tb_ok = None
if tb is not None:
    assert B % tb.C == 0, "--frames must be a multiple of the %d code blocks of a transport block" % tb.C
    TBS = B // tb.C
    pay = torch.empty((TBS, tb.A // 8), dtype=torch.uint8, device="cuda")
    back = torch.empty_like(pay)
    cb_ok = torch.empty(B, dtype=torch.uint8, device="cuda")
    tb_ok = torch.empty(TBS, dtype=torch.uint8, device="cuda")
bpay = bback = bstatus = popcount = None
if bch is not None:
    bpay = torch.empty((B, bch.k // 8), dtype=torch.uint8, device="cuda")
    bback = torch.empty_like(bpay)
    bstatus = torch.empty(B, dtype=torch.int32, device="cuda")
    popcount = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int64, device="cuda")
rm = tx = rx = None
rate = K / N
if args.rate_match:
    rmv = [int(x) for x in args.rate_match.split(",")]
    P, FLO, FHI, E = rmv[:4]
    K0 = rmv[4] if len(rmv) > 4 else 0
    assert FLO % 8 == 0 and FHI % 8 == 0 and FLO <= FHI <= K, "--rate-match: FLO and FHI are multiples of 8 inside the information part"
    assert tb is None or FLO == FHI or (tb.filler_lo <= FLO and FHI <= tb.filler_hi), \
        "--rate-match: with --transport-block the fillers lie inside [%d, %d)" % (tb.filler_lo if tb else 0, tb.filler_hi if tb else 0)
    rm = L.RateMatcher(N, punctured=P, filler=(FLO, FHI), erasure_llr=args.erasure_llr)
    rx = torch.empty((B, E), dtype=torch.float32, device="cuda")
    if enc is not None:
        tx = torch.empty((B, E), dtype=torch.uint8, device="cuda")
    rate = (K - (FHI - FLO)) / E
md = sym = zeros = None
if QM:
    sent = E if rm is not None else N                              # bits per frame on the air
    assert sent % QM == 0, "--modulation: the %d bits of a frame do not fill symbols of %d bits" % (sent, QM)
    md = L.Modem(QM, interleave=not args.no_interleave)
    sym = torch.empty((B, md.symbol_floats(sent)), dtype=torch.float32, device="cuda")
    if enc is None:
        zeros = torch.zeros((B, sent), dtype=torch.uint8, device="cuda")


def channel_batch(first, sd, seed):
    """Channel values of one batch into y (channel_values), and with --channel bsc their signs in their place."""
    channel_values(first, sd, seed)
    if args.channel == "bsc":
        torch.sign(y, out=y)


def channel_values(first, sd, seed):
    """Channel values of one batch into y; with a random payload: fresh source bytes -> code bits -> BPSK + noise."""
    stream = torch.cuda.current_stream().cuda_stream
    if enc is not None:
        if tb is not None:
            pay.random_(0, 256, generator=gen)
            tb.attach_device(pay.data_ptr(), TBS, src.data_ptr(), src.numel(), stream)   # payload, CRCs, zero fillers
        elif bch is not None:
            bpay.random_(0, 256, generator=gen)
            bch.encode_device(bpay.data_ptr(), B, src.data_ptr(), src.numel(), stream)   # payload, parity, zero fillers
        else:
            src.random_(0, 256, generator=gen)
            if between is not None:
                src[between] = 0
            if rm is not None:
                src.view(B, K // 8)[:, FLO // 8:FHI // 8] = 0      # filler bits are known zeros
        enc.encode_device(src.data_ptr(), src.numel(), B, code.data_ptr(), code.numel(), "bits", stream)
    if rm is None:
        if md is None:
            channel.awgn_device(N, first, B, sd, seed=seed, codewords=code, out=y)
        else:
            modem_batch(code if enc is not None else zeros, N, first, sd, seed, y, stream)
        return
    if enc is not None:
        rm.match_device(code.data_ptr(), B, K0, E, tx.data_ptr(), tx.numel(), "bits", "bits", stream)
    if md is None:
        channel.awgn_device(E, first, B, sd, seed=seed, codewords=tx, out=rx)
    else:
        modem_batch(tx if enc is not None else zeros, E, first, sd, seed, rx, stream)
    rm.recover_device(rx.data_ptr(), B, K0, E, None, False, y.data_ptr(), stream)


def quantise_batch():
    """--llr-type: the float values in y become int8 / fp16 elements in yq, which is what the decoder is given"""
    if yq is not None:
        L.quantize_device(y.data_ptr(), y.numel(), args.llr_type, llr_unit, yq.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)


def decode_batch(out_t, it_t, **kw):
    if yq is None:
        dec.decode_device(y.data_ptr(), B, out_t.data_ptr(), out_t.numel(), it_t.data_ptr() if it_t is not None else None, None, **kw)
    else:
        dec.decode_device(yq.data_ptr(), B, out_t.data_ptr(), out_t.numel(), it_t.data_ptr() if it_t is not None else None, None,
                          llr_type=args.llr_type, llr_unit=llr_unit, **kw)


def modem_batch(bits, n, first, sd, seed, dst, stream):
    """bits uint8 [B, n] -> symbols + noise -> demapped values float32 [B, n] in dst."""
    md.transmit_device(bits.data_ptr(), B, n, sd, seed, sym.data_ptr(), sym.numel(), first, "bits", stream)
    md.demap_device(sym.data_ptr(), B, n, dst.data_ptr(), stream)


def point_decoder(sd):
    """The decoder of one SNR point: with the matched scale a new one per point (llr_scale is fixed at creation)."""
    global dec
    if not matched:
        return
    if dec is not None:
        dec.close()
    scale = llr_unit_scale * 2.0 / (sd * sd)
    if rm is not None and args.algo == "sp":                         # exp(llr_scale * fill_llr) must stay finite
        rm.spec.fill_llr = min(10.0, 80.0 / scale)
    dec = make_decoder(scale)


soft = out2 = shifts = None
if args.soft_check:
    assert K % 8 == 0, "--soft-check compares whole bytes per frame: K % 8 must be 0"
    soft = torch.empty((B, N), dtype=torch.float32, device="cuda")
    out2 = torch.empty_like(out)
    shifts = torch.arange(8, dtype=torch.int32, device="cuda")


def soft_check():
    """The batch in y once more through ldpc_decode_soft_device: (posteriors of the K output bits that are finite and not
    zero, those among them whose sign is not the output bit, bytes that differ from the plain call's)."""
    decode_batch(out2, None, soft_ptr=soft.data_ptr(), soft_floats=soft.numel(), soft="posterior")
    bits = ((out2.view(B, K // 8).to(torch.int32)[:, :, None] >> shifts) & 1).reshape(B, K)
    p = soft[:, :K]
    ok = torch.isfinite(p) & (p != 0)
    return int(ok.sum()), int((ok & ((p < 0) != (bits != 0))).sum()), int((out2 != out).sum())


osd = osd_soft = osd_out = osd_status = None
if args.osd is not None:
    assert K % 8 == 0, "--osd compares whole bytes per frame: K % 8 must be 0"
    osd = L.Osd(g, K, max_frames=B)
    osd_soft = torch.empty((B, N), dtype=torch.float32, device="cuda")
    osd_out = torch.empty_like(out)
    osd_status = torch.empty(B, dtype=torch.int32, device="cuda")


def osd_batch():
    """The posteriors of the batch just decoded through ldpc_osd_device: (ms, frame errors after, processed, flipped)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    osd.run_device(osd_soft.data_ptr(), B, args.osd, args.osd_scale, osd_out.data_ptr(), osd_out.numel(), None, osd_status.data_ptr(), None,
                   torch.cuda.current_stream().cuda_stream)
    e1.record()
    e1.synchronize()
    after = channel.count_errors_device(osd_out, src, B)[2]
    return e0.elapsed_time(e1), after, int((osd_status > 0).sum()), int((osd_status == 2).sum())


yq, llr_unit = None, 1.0
if args.llr_type != "f32":
    llr_unit = args.llr_unit if args.llr_unit is not None else (0.05 if args.llr_type == "i8" else 1.0 / 256)
    yq = torch.empty((B, N), dtype=torch.int8 if args.llr_type == "i8" else torch.float16, device="cuda")
    print("typed input: llr_type=%s llr_unit=%g (%d bytes per frame instead of %d)" % (args.llr_type, llr_unit, N * yq.element_size(), 4 * N))
if rm is not None:
    print("rate matching: punctured=%d fillers=[%d,%d) E=%d k0=%d erasure_llr=%g effective rate (K - fillers)/E = %.4f" % (
        P, FLO, FHI, E, K0, args.erasure_llr, rate))
if tb is not None:
    print("transport block: A=%d tb_crc=%d C=%d cb_crc=%d, %d bits per code block, Kp=%d of K=%d, %d blocks per batch" % (
        tb.A, tb.tb_crc, tb.C, tb.cb_crc, tb.S, tb.Kp, K, TBS))
if bch is not None:
    print("outer code: BCH over GF(2^%d), t=%d n=%d k=%d r=%d, fillers [%d, %d)" % (bch.m, bch.t, bch.n, bch.k, bch.r, bch.n, K))
if md is not None:
    print("modulation: %s (%d bits per symbol) interleave=%d llr_scale=%s" % (
        args.modulation, QM, md.spec.interleave, "2/sd^2 per point" if matched else "%g" % (8.0 if args.llr_scale is None else args.llr_scale)))
if args.crc_stop:
    print("crc stop: crc_kind=%d over the first %d bits of every frame" % (crc_kind, crc_bits))
print("code=%s algo=%s payload=%s ms_scale=%g ms_offset=%g frames=%d x %d max_iter=%d (info bits per point: %d)" % (
    args.code, args.algo, args.payload, args.ms_scale, args.ms_offset, B, args.batches, args.iters, B * K * args.batches))
crossover = {}
if args.channel == "bsc":           # a hard decision on BPSK +-1 in noise sd errs with probability Q(1 / sd)
    from statistics import NormalDist
    for p in (float(x) for x in args.crossover.split(",")):
        assert 0.0 < p < 0.5, "--crossover: probabilities inside (0, 0.5)"
        snr = 20.0 * np.log10(NormalDist().inv_cdf(1.0 - p))
        crossover[snr] = p
    points = list(crossover)
else:
    points = [float(x) for x in args.snr.split(",")]
# one untimed batch first: the first launch of every kernel (the library's and torch's) pays one-time costs
point_decoder(10.0 ** (-points[-1] / 20.0))
channel_batch(0, 10.0 ** (-points[-1] / 20.0), args.seed + 1)
quantise_batch()
decode_batch(out, it)
count_errors(out)
float(it.float().sum())
torch.cuda.synchronize()
for snr in points:
    sd = 10.0 ** (-snr / 20.0)
    point_decoder(sd)
    tot = [0, 0, 0]
    blocks = [0, 0, 0, 0]
    it_sum, conv, stops, rounds, dec_ms = 0.0, 0, 0, 0, 0.0
    soft_tot = [0, 0, 0]
    outer = [0] * 6
    osd_tot = [0.0, 0, 0, 0]
    hist = [0] * (bch.t + 2) if bch is not None else None
    t0 = time.perf_counter()
    for b in range(args.batches):
        channel_batch(b * B, sd, args.seed)
        quantise_batch()
        if osd is None:
            decode_batch(out, it)
        else:
            decode_batch(out, it, soft_ptr=osd_soft.data_ptr(), soft_floats=osd_soft.numel(), soft="posterior")
        e = count_errors(out)
        tot = [t + x for t, x in zip(tot, e)]
        if osd is not None:
            osd_tot = [t + x for t, x in zip(osd_tot, osd_batch())]
        if tb is not None:
            tb.check_device(out.data_ptr(), TBS, back.data_ptr(), cb_ok.data_ptr(), tb_ok.data_ptr(), None)
            blocks = [t + x for t, x in zip(blocks, tb.tally_device(tb_ok.data_ptr(), back.data_ptr(), pay.data_ptr(), TBS, None))]
        if bch is not None:
            wrong = popcount[((out.view(B, K // 8) ^ src.view(B, K // 8))[:, :bch.n // 8]).long()].sum(dim=1)
            hist = [h + int(x) for h, x in zip(hist, torch.bincount(wrong.clamp(max=bch.t + 1), minlength=bch.t + 2).tolist())]
            bch.decode_device(out.data_ptr(), B, bback.data_ptr(), bstatus.data_ptr(), None)
            outer = [t + x for t, x in zip(outer, bch.tally_device(bstatus.data_ptr(), bback.data_ptr(), bpay.data_ptr(), B, None))]
        it_sum += float(it.float().sum())
        st = dec.stats()
        conv += st["frames_converged"]
        rounds += st["frame_rounds"]
        dec_ms += st["ms_total"]
        if tb is not None:
            stops += dec.crc_stops()
        if args.soft_check:
            soft_tot = [t + x for t, x in zip(soft_tot, soft_check())]
    dt = time.perf_counter() - t0
    frames = B * args.batches
    res = {"snr_db": snr, "sd": round(sd, 4), "ber": tot[0] / (frames * K), "bit_errors": tot[0],
           "byte_errors": tot[1], "fer": tot[2] / frames, "avg_iters": round(it_sum / frames, 2),
           "frames_converged": conv, "frames": frames, "frame_rounds": rounds, "decode_ms_per_batch": round(dec_ms / args.batches, 3),
           "end_to_end_Mbit_s": round(frames * K / dt / 1e6, 1)}
    if args.channel == "bsc":
        res["crossover"] = crossover[snr]
    if md is not None:
        es_n0 = 1.0 / (2.0 * sd * sd)
        res.update({"es_n0_db": round(10.0 * np.log10(es_n0), 3), "eb_n0_db": round(10.0 * np.log10(es_n0 / (QM * rate)), 3),
                    "llr_scale": round(llr_unit_scale * 2.0 / (sd * sd), 3) if matched else (8.0 if args.llr_scale is None else args.llr_scale)})
    if md is None and args.algo in ("bp", "layered_bp", "layered_bp_fx"):
        res["llr_scale"] = round(llr_unit_scale * 2.0 / (sd * sd), 3) if matched else args.llr_scale
    if tb is not None:
        n = TBS * args.batches
        res.update({"blocks": n, "bler": blocks[1] / n, "blocks_crc_failed": blocks[0], "blocks_undetected": blocks[2],
                    "blocks_parity_only": blocks[3], "crc_stops": stops})
    if bch is not None:
        res.update({"frame_errors_after_ldpc": frames - hist[0], "frame_errors_after_bch": outer[1], "bch_repaired_frames": outer[3],
                    "bch_failed_frames": outer[0], "bch_miscorrected_frames": outer[2], "bch_repaired_bits": outer[4],
                    "residual_hist": hist})
    if osd is not None:
        res.update({"osd_order": args.osd, "frame_errors_before_osd": tot[2], "frame_errors_after_osd": osd_tot[1], "osd_processed": osd_tot[2],
                    "osd_flipped": osd_tot[3], "osd_ms_per_batch": round(osd_tot[0] / args.batches, 3)})
    if args.soft_check:
        res.update({"soft_checked": soft_tot[0], "soft_sign_disagreements": soft_tot[1], "soft_bytes_differ": soft_tot[2]})
    print(json.dumps(res), flush=True)
    assert soft_tot[1] == 0 and soft_tot[2] == 0, "soft output disagrees with the decoded bytes"
