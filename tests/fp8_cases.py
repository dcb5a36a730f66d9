"""Inputs and expectations of tests/test_gpu_fp8.py (a helper, not a test module): the codes and frames of fp16_cases.py
under the fp8 rule (tests/fp8_ref.py), an overlay of channel values at the edges of the E4M3 conversion, and the hand-over
batch.  Everything here runs on the CPU, is computed once per process and handed out read-only; tests/test_fp8_cpu.py
checks that every case reaches what it is there for."""
import functools

import numpy as np

from myldpccppapi_amd import channel
from util import converged_frames

import fp16_cases as fc
import fp8_ref as R8

f32 = np.float32


def _freeze(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def want(d, kind="ride", setting=None):
    """fp8_ref.flood on staircase(d, kind): plain (setting None) or corrected, taps after round fc.TAP"""
    c = fc.staircase(d, kind)
    return _freeze(R8.flood(c["code"], c["y"], fc.MAXIT, *(setting or (0.0, 0.0)), tap_iter=fc.TAP))


@functools.lru_cache(maxsize=None)
def want_registers_unrounded(d, setting):
    """The model of a wrong kernel on the ride code: the staircase columns see R before s8 (for plain min-sum: the start
    value 1000 instead of 448)"""
    c = fc.staircase(d, "ride")
    return _freeze(R8.flood(c["code"], c["y"], fc.MAXIT, *(setting or (0.0, 0.0)), tap_iter=fc.TAP, raw_cols=fc.fused_columns(c)))


# ---- the degenerate overlay -----------------------------------------------------------------------------------------

OVERLAY_FRAMES = 18
SATURATING_FRAME = 17


def overlay(y, seed=23):
    """Writes 18 degenerate frames over y[:18] (in place) and returns y.  Frame by frame: zeros on N/5 positions; a frame of
    zeros; 40 values each of +448, -448, 464 (beyond the largest code: clamps), 1000; 20 +inf; 20 -inf; 5 NaN; on a
    quarter of the positions each: the smallest subnormal 2^-9, 5 * 2^-9, the tie 2^-10 (to the even code 0), the tie
    3 * 2^-10 (to the even code 2^-8), -1e-8 (to -0), the normal-range ties 1.0625 (to 1) and 1.1875 (to 1.25), 1e-41 (an
    fp32 denormal, to 0); a frame of +1; and a frame in which every value is +-400 (a quarter negative): every R of
    round 1 is +-400 or its corrected value and Q = y8 + sum of R leaves E4M3's range in the columns of degree 3 and more."""
    N = y.shape[1]
    assert y.shape[0] >= OVERLAY_FRAMES
    rng = np.random.default_rng(seed)

    def pick(n):
        return rng.choice(N, n, replace=False)

    y[0, pick(N // 5)] = 0.0
    y[1, :] = 0.0
    y[2, pick(40)] = 448.0
    y[3, pick(40)] = -448.0
    y[4, pick(40)] = 464.0
    y[5, pick(40)] = 1000.0
    y[6, pick(20)] = np.inf
    y[7, pick(20)] = -np.inf
    y[8, pick(5)] = np.nan
    y[9, pick(N // 4)] = 2.0 ** -9
    y[10, pick(N // 4)] = 5 * 2.0 ** -9
    y[11, pick(N // 4)] = 2.0 ** -10
    y[12, pick(N // 4)] = 3 * 2.0 ** -10
    y[13, pick(N // 4)] = -1e-8
    q = pick(N // 2)
    y[14, q[:N // 4]] = 1.0625
    y[14, q[N // 4:]] = 1.1875
    y[15, pick(N // 4)] = 1e-41
    y[16, :] = 1.0
    y[17, :] = 400.0
    y[17, pick(N // 4)] = -400.0
    return y


@functools.lru_cache(maxsize=None)
def degenerate_inputs(name):
    """24 frames over AWGN (as the fp16 test), the overlay on the first 18"""
    N = fc.degenerate_code(name)["N"]
    y = overlay(channel.awgn_frames(N, 0, fc.DEGENERATE_FRAMES, 0.7, seed=21))
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def degenerate_want(name, corrected):
    c, y = fc.degenerate_code(name), degenerate_inputs(name)
    setting = fc.DEGENERATE_SETTING if corrected else (0.0, 0.0)
    return _freeze(R8.flood(c["code"], y, fc.DEGENERATE_MAXIT, *setting, tap_iter=fc.TAP))


@functools.lru_cache(maxsize=None)
def conversion_inputs(N, frames):
    """frames x N values: the conversion test's edge inputs (fp8_ref.edge_inputs), repeated to fill"""
    x = R8.edge_inputs()
    y = np.resize(x, frames * N).reshape(frames, N).astype(f32)
    y.setflags(write=False)
    return y


# ---- hand-over, soft output, CRC ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def handover_want(B, setting=None):
    """fp16_cases.handover_inputs(B) under the fp8 rule; with post / y8 for the soft-output test"""
    c, y = fc.staircase(7, "ride"), fc.handover_inputs(B)
    r = R8.flood(c["code"], y, fc.HANDOVER_MAXIT, *(setting or (0.0, 0.0)))
    r["n_conv"] = int(converged_frames(c["rows"], c["cols"], c["M"], r["hard"]).sum())
    return _freeze(r)


def soft_of(w, kind):
    """float32 [frames, N]: the stop-round posterior, or that minus the stored channel value (one fp32 subtraction)"""
    with np.errstate(invalid="ignore"):
        return w["post"] if kind == "posterior" else (w["post"] - w["y8"]).astype(f32)
