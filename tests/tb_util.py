"""Shared set-up of the transport-block tests: the shapes, the program of tests/cpp/coder_transport_block.cpp, and the
chain scenario -- the BG1-profile code of ratematch_util (Z = 16, N = 1088, K = 352, P = 32, fillers
[328, 352), one transmission (k0, E) = (0, 1032) over 64 frames, erasure_llr 1e-6, max_iter 20, noise seed 100) carrying
TransportBlock(A = 312, K = 352): CRC16 and Kp = 328, exactly the filler start.  Everything here comes from tb_ref,
ratematch_ref, codes.py and the oracle, never from the library under test; the expensive parts are computed once per
process and handed out read-only."""
import functools
import os
import subprocess

import numpy as np

import oracle
from myldpccppapi_amd import codes

import ratematch_ref as rref
import ratematch_util as U
import tb_ref

#: (A, tb_crc, C, cb_crc, K)
SHAPES = [(8, 16, 1, 0, 24),            # three bytes, far fewer than lanes
          (8, 24, 1, 0, 64),            # fillers [32, 64)
          (312, 16, 1, 0, 352),         # the chain scenario
          (1000, 24, 1, 0, 1024),       # two bytes per lane
          (4056, 24, 1, 0, 4080),       # 510 bytes, ragged last lanes
          (8424, 24, 1, 0, 8448),       # largest block size used here
          (1000, 24, 2, 24, 544),       # S = 512, byte aligned
          (1008, 24, 2, 24, 544),       # S = 516, S % 8 = 4, filler start off a byte boundary
          (1008, 24, 4, 24, 288),       # S = 258
          (1008, 24, 8, 24, 160),       # S = 129
          (1024, 16, 16, 24, 96),       # S = 65, odd offset, shorter than a wave
          (2016, 24, 17, 24, 144),      # C = 17
          (5176, 24, 65, 24, 104),      # C = 65, more segments than lanes
          (1000, 24, 2, 0, 512),        # no code-block CRC
          (1024, 0, 2, 24, 536)]        # no transport-block CRC


def ref_spec(shape):
    A, tb_crc, C, cb_crc, K = shape
    return tb_ref.Spec(A, K, C=C, tb_crc=tb_crc, cb_crc=cb_crc)


def coder_transport_block_exe(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "coder_transport_block")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "coder_transport_block.cpp"), "-o", exe,
                           "-L" + os.path.join(root, "myldpccppapi_amd"), "-lmyldpc", "-lldpc_hip",
                           "-Wl,-rpath," + os.path.join(root, "myldpccppapi_amd")])
    return exe


# ---- the chain scenario ------------------------------------------------------------------------------------------
A, K0, E, SEED, ERASURE = 312, 0, 1032, 100, 1e-6
CLEAN_DB = 3.0
#: algo -> (hard point in dB, llr_scale)
HARD = {"layered": (0.0, U.LLR_SCALE), "ms": (0.0, U.LLR_SCALE), "sp": (1.5, 8.0)}
WINDOW = (8, 56)          # failing blocks of 64 the oracle must leave at the hard point


def chain_spec():
    spec = tb_ref.Spec(A, U.K)
    assert (spec.tb_crc, spec.C, spec.cb_crc, spec.Kp) == (16, 1, 0, U.FILLER[0]) and spec.K == U.FILLER[1]
    return spec


@functools.lru_cache(maxsize=None)
def chain_payload():
    """(payload uint8 [64, 39], source rows uint8 [64, 44] by tb_ref.attach, codewords uint8 [64, N]).  The payload is
    the scenario's own: the first 312 information bits of every frame of ratematch_util.payload(), so that the codewords
    differ from those of section 8e in the 16 CRC bits and the parity they cause only."""
    payload = tb_ref.bytes_of(U.payload()[0][:, :A])
    src = tb_ref.attach(chain_spec(), payload)
    info = tb_ref.bits_of(src)
    assert not info[:, U.FILLER[0]:U.FILLER[1]].any()
    base = codes.nr_bg1_profile_base(Z=U.Z)
    code = np.stack([codes.nr_bg1_profile_encode(base, U.Z, info[f]) for f in range(U.FRAMES)]).astype(np.uint8)
    for a in (payload, src, code):
        a.setflags(write=False)
    return payload, src, code


@functools.lru_cache(maxsize=None)
def chain_received(snr_db):
    """(tx uint8 [64, E], rx float32 [64, E], y float32 [64, N], sd)."""
    sd = 10.0 ** (-snr_db / 20.0)
    tx = rref.match(U.scenario_spec(0.0), chain_payload()[2], K0, E)
    rx = oracle.awgn(E, 0, U.FRAMES, sd, seed=SEED, codewords=tx)
    y = rref.recover(U.scenario_spec(ERASURE), rx, K0, E)[1]
    for a in (tx, rx, y):
        a.setflags(write=False)
    return tx, rx, y, sd


@functools.lru_cache(maxsize=None)
def chain_oracle(algo, snr_db):
    """(decoded bytes uint8 [64 * 44], iters, payload, cb_ok, tb_ok, counts) of oracle.decode and tb_ref.check."""
    r = oracle.decode(U.bg1()[2], chain_received(snr_db)[2], algo, max_iter=U.MAX_ITER, llr_scale=HARD[algo][1], layer_rows=U.Z)
    out = np.asarray(r["out"], np.uint8).reshape(-1)
    payload, cb_ok, tb_ok = tb_ref.check(chain_spec(), out)
    return out, np.asarray(r["iters"]), payload, cb_ok, tb_ok, tb_ref.tally(tb_ok, payload, chain_payload()[0])


def chain_points(algo):
    return (CLEAN_DB, HARD[algo][0])
