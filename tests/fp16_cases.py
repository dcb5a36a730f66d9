"""Codes, inputs and expectations for tests/test_gpu_fp16.py (a helper, not a test module).

msg_dtype = f16 is this repository's own definition (the reference is fp32 only): channel values and variable->check
messages are rounded to binary16 where they are stored, the arithmetic is fp32, and a corrected min-sum magnitude is
rounded where the check->variable message is produced.  Three things are put together here: staircase (IRA) codes whose
linked class has a degree the column-fused check kernels exist for (3, 7, 16), with frames that stop at many different
rounds; an overlay of channel values at the edges of the binary16 conversion; and a batch with scattered stragglers for
the hand-over on a staircase code.  Everything here runs on the CPU -- the C oracle for plain min-sum, the numpy
restatement (ms_correction_ref.py) for the corrected one -- and tests/test_fp16_cpu.py checks from these results alone
that every case reaches what it is there for."""
import ctypes
import functools

import numpy as np

import oracle
from myldpccppapi_amd import channel, codes
import kernel_matrix as km
from ms_correction_ref import Code, flood_ms
from util import converged_frames

f32 = np.float32
SETTINGS = ((0.75, 0.0), (0.0, 0.15), (0.8, 0.05))          # pure scale, pure offset, both (test_gpu_ms_correction.py)
DEGREES = (3, 7, 16)
LINKED_ROWS = 400
FRAMES = 133                                                # two tiles of 64 and a ragged third; one ragged tile at V = 4
MAXIT = 25
TAP = 2
# unlinked rows: <= 64 of them ride along in the column-fused launch (link_extra_rows), more get launches of their own
# (plan_launches in engine_flood.hip; 72 here, two classes of which share a bucket launch, as the fp32 codes of
# test_gpu_kernel_matrix.py)
EXTRA = {"ride": {5: 20, 20: 2}, "own": {5: 50, 6: 20, 20: 2}}
CASES = tuple((d, "ride") for d in DEGREES) + ((7, "own"),)
# noise range of the frames per linked degree: frames stop at many different rounds, and some never do
NOISE = {3: (0.5, 0.9), 7: (0.45, 0.75), 16: (0.3, 0.6)}


def _freeze(r):
    for v in list(r.values()) + list(r.get("taps", {}).values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def f16_round(x):
    """The oracle's binary16 round trip (oracle/ldpc_oracle.c: f16_round), float32 in and out."""
    f = oracle.lib().oracle_f16_round
    f.restype = None
    f.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.c_int64]
    x = np.ascontiguousarray(x, f32)
    out = np.empty_like(x)
    f(x.ctypes.data_as(f.argtypes[0]), out.ctypes.data_as(f.argtypes[1]), x.size)
    return out


def noisy_frames(N, frames, lo, hi, seed):
    """All-zero codeword over AWGN, the noise level of each frame drawn from [lo, hi] (as _channel of
    test_gpu_kernel_matrix.py)."""
    y = channel.awgn_frames(N, 0, frames, 1.0, seed=seed)
    sd = np.random.default_rng(seed).uniform(lo, hi, frames).astype(f32)[:, None]
    return (f32(1) + (y - f32(1)) * sd).astype(f32)


@functools.lru_cache(maxsize=None)
def staircase(d, kind="ride"):
    """dict(rows, cols, M, N, K, og, code, y): the IRA code with LINKED_ROWS rows of degree d and its FRAMES frames"""
    rows, cols, M, N, K = km.ira_code(d, LINKED_ROWS, EXTRA[kind], seed=d)
    K = K // 8 * 8
    y = noisy_frames(N, FRAMES, *NOISE[d], seed=100 + d)
    y.setflags(write=False)
    return dict(rows=rows, cols=cols, M=M, N=N, K=K, og=oracle.Graph(rows, cols, M, N, K), code=Code(rows, cols, M, N, K), y=y)


@functools.lru_cache(maxsize=None)
def wimax():
    """WiMAX rate 1/2, N = 960: the code of test_gpu_parity.py::test_degenerate_channel_values"""
    rate, N = codes.RATE_1_2, 960
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    return dict(rows=rows, cols=cols, M=M, N=N, K=K, z=z, og=oracle.Graph(rows, cols, M, N, K), code=Code(rows, cols, M, N, K))


def fused_columns(c):
    """bool [N]: the staircase parity columns of degree 2 (each joins two consecutive linked rows)"""
    cd = np.bincount(c["cols"], minlength=c["N"])
    m = np.zeros(c["N"], bool)
    m[c["N"] - LINKED_ROWS:] = True
    return m & (cd == 2)


# ---- the degenerate overlay -----------------------------------------------------------------------------------------

OVERLAY_FRAMES = 19
# the values overlay() writes, in the order of the frames they go to
OVERLAY_VALUES = dict(just_finite=65519.0, to_inf=65520.0, far_out=-70000.0, erasure_llr=1e-6, tie_to_zero=2.0 ** -25,
                      tie_to_even=3 * 2.0 ** -25, to_minus_zero=-1e-8, tie_11th_bit=1 + 2.0 ** -11, near_max=64500.0,
                      fp32_denormal=1e-41)


def overlay(y, seed=21):
    """Writes the 19 degenerate frames over y[:19] (in place) and returns y.  Frame by frame: erasures on N/5 positions;
    a frame of zeros; 40 values that round to the largest binary16 number, 40 that round to +inf, 40 far beyond; 20 +inf,
    20 -inf, 5 NaN; on a quarter of the positions each: the rate matcher's erasure value (a binary16 subnormal), the tie
    at 2^-25 (to 0), the tie at 3 * 2^-25 (to even: 2^-23), -1e-8 (to -0); a frame of +1, one of -1 (all ties in min-sum);
    N/3 values times 400 (beyond the 1000 clip; some beyond 65504); a quarter at 1 + 2^-11 (a tie at the 11th mantissa
    bit, to even: 1), at 64500, at 1e-41 (an fp32 denormal, to 0).  The quarter at 64500 sits among values around 1, so the
    R it receives are around 1 and Q stays finite; in the last frame every value is +-64500 (a quarter negative), every R is
    +-1000 or its corrected value, and Q = y + sum of R leaves binary16's range in the columns of degree 3 and more."""
    N = y.shape[1]
    assert y.shape[0] >= OVERLAY_FRAMES
    rng = np.random.default_rng(seed)
    v = OVERLAY_VALUES

    def pick(n):
        return rng.choice(N, n, replace=False)

    y[0, pick(N // 5)] = 0.0
    y[1, :] = 0.0
    y[2, pick(40)] = v["just_finite"]
    y[3, pick(40)] = v["to_inf"]
    y[4, pick(40)] = v["far_out"]
    y[5, pick(20)] = np.inf
    y[6, pick(20)] = -np.inf
    y[7, pick(5)] = np.nan
    y[8, pick(N // 4)] = v["erasure_llr"]
    y[9, pick(N // 4)] = v["tie_to_zero"]
    y[10, pick(N // 4)] = v["tie_to_even"]
    y[11, pick(N // 4)] = v["to_minus_zero"]
    y[12, :] = 1.0
    y[13, :] = -1.0
    y[14, pick(N // 3)] *= f32(400.0)
    y[15, pick(N // 4)] = v["tie_11th_bit"]
    y[16, pick(N // 4)] = v["near_max"]
    y[17, pick(N // 4)] = v["fp32_denormal"]
    y[18, :] = v["near_max"]
    y[18, pick(N // 4)] = -v["near_max"]
    return y


DEGENERATE_FRAMES = 24
DEGENERATE_MAXIT = 15
DEGENERATE_SETTING = (0.8, 0.05)


def degenerate_code(name):
    return wimax() if name == "wimax" else staircase(7, "ride")


@functools.lru_cache(maxsize=None)
def degenerate_inputs(name):
    """24 frames over AWGN (as the fp32 test), the overlay on the first 19"""
    N = degenerate_code(name)["N"]
    y = overlay(channel.awgn_frames(N, 0, DEGENERATE_FRAMES, 0.7, seed=21))
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def degenerate_want(name, corrected):
    c, y = degenerate_code(name), degenerate_inputs(name)
    if corrected:
        return _freeze(flood_ms(c["code"], y, DEGENERATE_MAXIT, *DEGENERATE_SETTING, f16=True, tap_iter=TAP))
    return _freeze(as_ref(oracle.decode(c["og"], y, "ms", max_iter=DEGENERATE_MAXIT, tap_iter=TAP, msg_f16=True)))


# ---- expectations ---------------------------------------------------------------------------------------------------

def as_ref(r):
    """an oracle.decode result under the keys of ms_correction_ref.flood_ms"""
    return dict(out=r["out"], iters=r["iters"], hard=r["hard"], r_tap=r["taps"].get("r"), q_tap=r["taps"].get("q"))


@functools.lru_cache(maxsize=None)
def want(d, kind="ride", setting=None, f16=True):
    """Plain min-sum (setting None): the C oracle; corrected: the numpy restatement.  Keys out, iters, hard, r_tap,
    q_tap (the messages after round TAP)."""
    c = staircase(d, kind)
    if setting is None:
        return _freeze(as_ref(oracle.decode(c["og"], c["y"], "ms", max_iter=MAXIT, tap_iter=TAP, msg_f16=f16)))
    return _freeze(flood_ms(c["code"], c["y"], MAXIT, *setting, f16=f16, tap_iter=TAP))


@functools.lru_cache(maxsize=None)
def want_registers_unrounded(d, setting):
    """The model of a wrong kernel (flood_ms: raw_cols) on the ride code: the staircase columns see unrounded R"""
    c = staircase(d, "ride")
    return _freeze(flood_ms(c["code"], c["y"], MAXIT, *setting, f16=True, tap_iter=TAP, raw_cols=fused_columns(c)))


def tap_frames(iters):
    """(frames whose R tap is compared, frames whose Q tap is compared)"""
    iters = np.asarray(iters)
    return np.nonzero(iters >= TAP)[0], np.nonzero(iters > TAP)[0]


def same_floats(got, ref):
    """bit patterns where the expectation is a number (signs of zeros and infinities included), NaN where it is NaN"""
    got, ref = np.ascontiguousarray(got, f32), np.ascontiguousarray(ref, f32)
    num = ~np.isnan(ref)
    return bool(np.array_equal(got.view(np.uint32)[num], ref.view(np.uint32)[num]) and np.isnan(got[~num]).all())


# ---- hand-over on a staircase code ----------------------------------------------------------------------------------

HANDOVER_MAXIT = 30
HANDOVER_BATCHES = (700, 2100)
HANDOVER_STRAGGLERS = 90


@functools.lru_cache(maxsize=None)
def handover_inputs(B):
    """B frames that converge within a few rounds, 90 scattered ones replaced by frames that never do"""
    N = staircase(7, "ride")["N"]
    y = channel.awgn_frames(N, 0, B, 0.45, seed=41)
    where = np.random.default_rng(40).choice(B, HANDOVER_STRAGGLERS, replace=False)
    y[where] = channel.awgn_frames(N, 5000, HANDOVER_STRAGGLERS, 1.05, seed=42)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def handover_want(B, setting=None, f16=True):
    c, y = staircase(7, "ride"), handover_inputs(B)
    if setting is None:
        r = as_ref(oracle.decode(c["og"], y, "ms", max_iter=HANDOVER_MAXIT, msg_f16=f16))
    else:
        r = flood_ms(c["code"], y, HANDOVER_MAXIT, *setting, f16=f16)
    r["n_conv"] = int(converged_frames(c["rows"], c["cols"], c["M"], r["hard"]).sum())
    return _freeze(r)
