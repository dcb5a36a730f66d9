"""Inputs and expectations of tests/test_gpu_crc_term.py beyond the chain scenario (a helper, not a test module): frames of
the BG1-profile code of ratematch_util (Z = 16, N = 1088, K = 352) that carry a CRC, sent whole over BPSK + AWGN, with the
noise chosen per frame range.  Everything here runs on the CPU and comes from tb_ref, codes.py and the oracle (through
crc_term_ref), never from the library under test; computed once per process and handed out read-only."""
import functools
import os
import subprocess

import numpy as np

import oracle
from myldpccppapi_amd import codes

import crc_term_ref as CR
import ratematch_util as U
import tb_ref

MAXIT = 20
#: name -> (A, C, tb_crc): frames of TransportBlock(A, K = 352, C, tb_crc) -- their (crc kind, crc bits, Kp)
BLOCKS = {"chain": (312, 1, 16),        # CRC16 over 328 bits, fillers [328, 352)
          "cb": (632, 2, 24),           # CRC24B over 352 = K bits: S = 328, no fillers
          "cb348": (632, 2, 16),        # CRC24B over 348 bits (no multiple of 8 or 64), fillers [348, 352)
          "a24": (304, 1, 24)}          # CRC24A over 328 bits


def frame_crc(block):
    A, C, tb_crc = BLOCKS[block]
    spec = tb_ref.Spec(A, U.K, C=C, tb_crc=tb_crc)
    assert spec.valid
    return (25 if spec.cb_crc else tb_crc), spec.Kp, spec


@functools.lru_cache(maxsize=None)
def codewords(block, tbs=32):
    """(payload uint8 [tbs, A/8], codewords uint8 [tbs * C, N]) of random payloads via tb_ref.attach and
    codes.nr_bg1_profile_encode."""
    spec = frame_crc(block)[2]
    payload = np.random.default_rng(11).integers(0, 256, (tbs, spec.A // 8), dtype=np.uint8)
    info = tb_ref.bits_of(tb_ref.attach(spec, payload))
    base = codes.nr_bg1_profile_base(Z=U.Z)
    code = np.stack([codes.nr_bg1_profile_encode(base, U.Z, info[f]) for f in range(info.shape[0])]).astype(np.uint8)
    for a in (payload, code):
        a.setflags(write=False)
    return payload, code


@functools.lru_cache(maxsize=None)
def received(block, frames, sd_easy, sd_hard, hard_every, seed=5):
    """float32 [frames, N]: frame f carries codeword f % (number of codewords); every hard_every-th frame (0: none) sees
    noise of sd_hard, the others of sd_easy."""
    code = codewords(block)[1]
    cw = code[np.arange(frames) % code.shape[0]]
    y = oracle.awgn(U.N, 0, frames, sd_easy, seed=seed, codewords=cw)
    if hard_every:
        hard = np.arange(hard_every // 2, frames, hard_every)
        y[hard] = oracle.awgn(U.N, 100000, hard.size, sd_hard, seed=seed + 1, codewords=cw[hard])
    y.setflags(write=False)
    return y


def _decoder(algo, variant=""):
    rows, cols, g = U.bg1()
    return CR.oracle_decoder(g, algo, llr_scale=U.LLR_SCALE, layer_rows=U.Z, msg_f16=variant == "f16")


@functools.lru_cache(maxsize=None)
def want(block, algo, frames, sd_easy, sd_hard, hard_every, variant=""):
    """crc_rule() on received(...)."""
    kind, bits, _ = frame_crc(block)
    rows, cols, _ = U.bg1()
    r = CR.crc_rule(_decoder(algo, variant), received(block, frames, sd_easy, sd_hard, hard_every), rows, cols, U.M, U.N, U.K,
                    kind, bits, MAXIT)
    for v in r.values():
        v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def want_syndrome(block, algo, frames, sd_easy, sd_hard, hard_every):
    """oracle.decode with the syndrome rule alone: (out, iters)."""
    r = oracle.decode(U.bg1()[2], received(block, frames, sd_easy, sd_hard, hard_every), algo, max_iter=MAXIT,
                      llr_scale=U.LLR_SCALE, layer_rows=U.Z)
    return r["out"], r["iters"]


# the mixtures of the hand-over tests: (block, algo, frames, sd_easy, sd_hard, hard_every)
POLLED = ("chain", "ms", 256, 0.60, 0.98, 6)          # 4 tiles of 64: hand-over once <= 64 frames run
TAIL = ("chain", "ms", 2048, 0.60, 0.98, 20)          # 32 tiles of 64 = 4 x the 8 overflow tiles: hand-over at <= 512


def handover_round(iters, frames, threshold):
    """The first round after which 0 < running <= threshold and 4 * running <= frames (both hand-overs' rule), or None."""
    iters = np.asarray(iters)
    for rnd in range(1, MAXIT):
        run = int((iters > rnd).sum())
        if run == 0:
            return None
        if run <= threshold and 4 * run <= frames:
            return rnd
    return None


def crc_stops_after_handover(case, threshold):
    """(hand-over round, frames that stop by the CRC alone in a later round) by the helper's counts."""
    r = want(*case)
    rnd = handover_round(r["iters"], case[2], threshold)
    assert rnd is not None
    late = r["by_crc"][r["iters"][r["by_crc"]] > rnd]
    return rnd, late


def coder_crc_early_stop_exe(tmp_path):
    """tests/cpp/coder_crc_early_stop.cpp built against the in-tree libraries."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "coder_crc_early_stop")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "coder_crc_early_stop.cpp"), "-o", exe,
                           "-L" + os.path.join(root, "myldpccppapi_amd"), "-lmyldpc", "-lldpc_hip",
                           "-Wl,-rpath," + os.path.join(root, "myldpccppapi_amd")])
    return exe
