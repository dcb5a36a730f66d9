"""Inputs and expectations of tests/test_gpu_fixed.py (a helper, not a test module): the codes and frames of fp16_cases.py
under the fixed-point rule (tests/fixed_ref.py), an overlay of channel values at the edges of the store rule sq, and the
hand-over batch.  Everything here runs on the CPU, is computed once per process and handed out read-only;
tests/test_fixed_cpu.py checks that every case reaches what it is there for."""
import functools
import os
import subprocess

import numpy as np

from myldpccppapi_amd import channel
from util import converged_frames

import fp16_cases as fc
import fixed_ref as RI

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# LSBs per unit of channel value (BPSK +-1 plus noise): the clean value 1 sits at a quarter of the range, L / 4 rounded up to
# a power of two, so that noise of a few sigma saturates and a product with it is exact.  Not at 4 bits: with the clean
# value at 2 LSBs a truncating correction ((3 * 2) >> 2 = 1, 2 - 1 = 1) halves every message and no frame of the d = 7 and
# d = 16 staircase codes converges at all, so nothing there would stop at distinct rounds; the clean value sits at 4
LLR_SCALE = {4: 4.0, 5: 4.0, 6: 8.0, 8: 32.0}
# (d, q) of the column-fused cases: every linked degree at q = 6, one of them at the narrowest and one at the widest width
FUSED_CASES = tuple((d, 6) for d in fc.DEGREES) + ((7, 4), (3, 8))
TWO_TILES = 300                                     # frames of the run with two tiles of 256 (the second ragged)


def _freeze(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def as_float(a):
    """an int32 message / posterior array as the float32 values the library reports"""
    return np.asarray(a).astype(f32)


@functools.lru_cache(maxsize=None)
def want(d, q, kind="ride", setting=None):
    """fixed_ref.flood on staircase(d, kind): plain (setting None) or corrected, taps after round fc.TAP"""
    c = fc.staircase(d, kind)
    return _freeze(RI.flood(c["code"], c["y"], fc.MAXIT, *(setting or (0.0, 0.0)), q=q, llr_scale=LLR_SCALE[q], tap_iter=fc.TAP))


@functools.lru_cache(maxsize=None)
def want_registers_raw(d, q, setting):
    """The model of a wrong kernel on the ride code: the staircase columns see R before MsgRound (the corrected product
    neither truncated nor saturated)"""
    c = fc.staircase(d, "ride")
    return _freeze(RI.flood(c["code"], c["y"], fc.MAXIT, *(setting or (0.0, 0.0)), q=q, llr_scale=LLR_SCALE[q], tap_iter=fc.TAP,
                            raw_cols=fc.fused_columns(c)))


def repeat_frames(a, frames):
    """rows 0 .. frames-1 of a per-frame array continued periodically (frames decode independently)"""
    a = np.asarray(a)
    return a[np.arange(frames) % a.shape[0]]


# ---- the degenerate overlay -----------------------------------------------------------------------------------------

OVERLAY_FRAMES = 14
SATURATING_FRAME = 13


def overlay(y, q, seed=29):
    """Writes 14 degenerate frames over y[:14] (in place) and returns y; the values are given in LSBs and written divided by
    LLR_SCALE[q] (a power of two: the product in the decoder is exact).  Frame by frame: zeros on N/5 positions; a frame of
    zeros; 40 values each of +L, -L, L + 1, 1000; 20 +inf; 20 -inf; 5 NaN; on a sixth of the positions each the ties +-0.5
    (to 0), +-1.5 (to +-2), +-2.5 (to +-2); L + 0.49 and L + 0.5 on a quarter each; -0 and an fp32 denormal on a quarter each;
    and a frame in which every value is +-(L - 1), a quarter negative: every R of round 1 is +-(L - 1) or its corrected value
    and P - R leaves [-L, L] in the columns of degree 3 and more."""
    N = y.shape[1]
    assert y.shape[0] >= OVERLAY_FRAMES
    rng = np.random.default_rng(seed)
    L, S = RI.limit(q), f32(LLR_SCALE[q])

    def pick(n):
        return rng.choice(N, n, replace=False)

    def lsb(v):
        return f32(v) / S

    y[0, pick(N // 5)] = 0.0
    y[1, :] = 0.0
    y[2, pick(40)] = lsb(L)
    y[3, pick(40)] = lsb(-L)
    y[4, pick(40)] = lsb(L + 1)
    y[5, pick(40)] = lsb(1000)
    y[6, pick(20)] = np.inf
    y[7, pick(20)] = -np.inf
    y[8, pick(5)] = np.nan
    p = pick(N)
    for i, v in enumerate((0.5, -0.5, 1.5, -1.5, 2.5, -2.5)):
        y[9, p[i * (N // 6):(i + 1) * (N // 6)]] = lsb(v)
    y[10, p[:N // 4]] = lsb(L + 0.49)
    y[10, p[N // 4:N // 2]] = lsb(L + 0.5)
    y[11, p[:N // 4]] = -0.0
    y[11, p[N // 4:N // 2]] = 1e-41
    y[12, :] = lsb(1)
    y[13, :] = lsb(L - 1)
    y[13, pick(N // 4)] = lsb(-(L - 1))
    return y


@functools.lru_cache(maxsize=None)
def degenerate_inputs(name, q):
    """24 frames over AWGN (as the fp16 test), the overlay on the first 14"""
    N = fc.degenerate_code(name)["N"]
    y = overlay(channel.awgn_frames(N, 0, fc.DEGENERATE_FRAMES, 0.7, seed=21), q)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def degenerate_want(name, q, corrected):
    c, y = fc.degenerate_code(name), degenerate_inputs(name, q)
    setting = fc.DEGENERATE_SETTING if corrected else (0.0, 0.0)
    return _freeze(RI.flood(c["code"], y, fc.DEGENERATE_MAXIT, *setting, q=q, llr_scale=LLR_SCALE[q], tap_iter=fc.TAP))


@functools.lru_cache(maxsize=None)
def conversion_inputs(N, frames, q):
    """frames x N values: the conversion test's edge inputs (fixed_ref.edge_inputs), repeated to fill"""
    x = RI.edge_inputs(q)
    y = np.resize(x, frames * N).reshape(frames, N).astype(f32)
    y.setflags(write=False)
    return y


# ---- hand-over, soft output -----------------------------------------------------------------------------------------

HANDOVER_Q = 6


@functools.lru_cache(maxsize=None)
def handover_want(B, setting=None):
    """fp16_cases.handover_inputs(B) under the fixed-point rule at q = 6; with post / c for the soft-output test"""
    c, y = fc.staircase(7, "ride"), fc.handover_inputs(B)
    r = RI.flood(c["code"], y, fc.HANDOVER_MAXIT, *(setting or (0.0, 0.0)), q=HANDOVER_Q, llr_scale=LLR_SCALE[HANDOVER_Q])
    r["n_conv"] = int(converged_frames(c["rows"], c["cols"], c["M"], r["hard"]).sum())
    return _freeze(r)


def soft_of(w, kind):
    """float32 [frames, N]: the stop-round posterior, or that minus the stored channel value, in LSBs"""
    return as_float(w["post"] if kind == "posterior" else w["post"] - w["c"])


def coder_fixed_exe(tmp_path):
    """Builds tests/cpp/coder_fixed.cpp (Coder::setMessageType with a bit width, end to end) against the in-tree libraries."""
    exe = str(tmp_path / "coder_fixed")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "coder_fixed.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "myldpccppapi_amd"), "-lmyldpc", "-lldpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myldpccppapi_amd")])
    return exe
