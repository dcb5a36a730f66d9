"""Inputs and expectations of tests/test_gpu_layered_fx.py (a helper, not a test module): the BG1-profile test code, the
irregular matrix code with every row a layer of its own, the saturation overlay on WiMAX (576, 288) and the staircase code,
a star code whose centre column outgrows 16 bits, the CRC frames of bp_cases and typed inputs, all under the fixed-point
layered rule (tests/layered_fx_ref.py).  Everything here runs on the CPU, is computed once per process and handed out
read-only; tests/test_layered_fx_cpu.py checks that every case reaches what it is there for."""
import functools

import numpy as np

from myldpccppapi_amd import channel, codes

import bp_cases as bc
import fixed_cases as fxc
import fp16_cases as fc
import layered_bp_cases as lc
import layered_fx_ref as FX
from ms_correction_ref import Code

f32 = np.float32
TAP = fc.TAP                        # the round whose R, P and bits are compared
LLR_SCALE = fxc.LLR_SCALE           # LSBs per unit of channel value at every width (fixed_cases.py says why)
CORRECTED = (0.75, 1.0)             # (3 (m - 1)) >> 2: scale and a one-LSB offset together
PLAIN = (0.0, 0.0)
WIDTHS = ((6, 8), (8, 16))          # (q, p) of the BG1 and matrix cases
SATURATION_WIDTHS = ((4, 4), (6, 8), (8, 16))      # p = q, p = q + 2, p = 16


def _freeze(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def setting(corrected):
    return CORRECTED if corrected else PLAIN


def as_float(a):
    """an int32 message / posterior array as the float32 values the library reports"""
    return np.asarray(a).astype(f32)


# ---- the BG1-profile test code (N = 1088, z = 16, row degrees 3 ... 19) ----------------------------------------------

BG1_MAXIT = lc.BG1_MAXIT            # 12
BG1_TWO_TILES = lc.BG1_TWO_TILES    # 262 = V = 4: a full tile and a ragged second one
bg1_code = lc.bg1_code
bg1_inputs = lc.bg1_inputs          # noise level drawn per frame from [0.4, 1.3]


@functools.lru_cache(maxsize=None)
def bg1_want(frames, q, p, corrected, tap=TAP, early_term=True, pack_mode=0):
    c = bg1_code()
    return _freeze(FX.layered_fx(c["code"], bg1_inputs(frames), c["z"], BG1_MAXIT, *setting(corrected), q=q, p=p,
                                 llr_scale=LLR_SCALE[q], tap_iter=tap, early_term=early_term, pack_mode=pack_mode))


# ---- every degree class: the irregular matrix code, every row a layer ------------------------------------------------

MATRIX_MAXIT = lc.MATRIX_MAXIT      # 5: about 135 launches per round with layer_rows = 1
matrix = bc.matrix


@functools.lru_cache(maxsize=None)
def matrix_want(q, p, corrected):
    m = matrix()
    return _freeze(FX.layered_fx(m["code"], m["y"], 1, MATRIX_MAXIT, *setting(corrected), q=q, p=p, llr_scale=LLR_SCALE[q],
                                 tap_iter=TAP))


# ---- saturation and degenerate channel values ------------------------------------------------------------------------

SATURATION_FRAMES = fc.DEGENERATE_FRAMES            # 24, the overlay of fixed_cases.py on the first 14
SATURATION_MAXIT = {"wimax": 10, "ira": 4}          # ira: one row per layer, 422 launches per round


@functools.lru_cache(maxsize=None)
def saturation_code(name):
    """WiMAX (576, 288), layered by its circulant size; the staircase code, whose consecutive rows share a column: one row
    per layer"""
    if name == "ira":
        c = fc.staircase(7, "ride")
        return dict(rows=c["rows"], cols=c["cols"], M=c["M"], N=c["N"], K=c["K"], z=1, code=c["code"])
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    return dict(rows=rows, cols=cols, M=M, N=N, K=K, z=z, code=Code(rows, cols, M, N, K))


@functools.lru_cache(maxsize=None)
def saturation_inputs(name, q):
    """24 frames over AWGN with fixed_cases.overlay on the first 14: zeros, +-L, L + 1, 1000, +-inf, NaN, the ties of sq,
    -0, a denormal, and the frame of +-(L - 1) whose messages push t beyond L and P to +-LP"""
    y = fxc.overlay(channel.awgn_frames(saturation_code(name)["N"], 0, SATURATION_FRAMES, 0.7, seed=21), q)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def saturation_want(name, q, p, corrected=False):
    c = saturation_code(name)
    return _freeze(FX.layered_fx(c["code"], saturation_inputs(name, q), c["z"], SATURATION_MAXIT[name], *setting(corrected),
                                 q=q, p=p, llr_scale=LLR_SCALE[q], tap_iter=TAP))


# ---- a posterior that outgrows 16 bits -------------------------------------------------------------------------------
# With p = 16 the posterior cannot saturate unless (1 + column degree) * 127 > 32767, so none of the codes above gets there.
# The star code has one column in every one of its 300 rows, each row a layer of its own: row m = (column 0, column 1 + m).

STAR_ROWS = 300
STAR_FRAMES = 8
STAR_TAP = 1                        # the all-positive and the all-negative frame stop in round 1


@functools.lru_cache(maxsize=None)
def star_code():
    M, N, K = STAR_ROWS, STAR_ROWS + 1, 8
    rows = np.repeat(np.arange(M), 2).astype(np.int32)
    cols = np.stack([np.zeros(M, np.int64), 1 + np.arange(M)], axis=1).reshape(-1).astype(np.int32)
    return dict(rows=rows, cols=cols, M=M, N=N, K=K, z=1, code=Code(rows, cols, M, N, K))


@functools.lru_cache(maxsize=None)
def star_inputs():
    """frame 0: every value +127 LSB; frame 1: every value -127 LSB (every row of two ones is satisfied); the rest AWGN"""
    y = channel.awgn_frames(STAR_ROWS + 1, 0, STAR_FRAMES, 0.7, seed=23)
    y[0, :] = f32(127) / f32(LLR_SCALE[8])
    y[1, :] = f32(-127) / f32(LLR_SCALE[8])
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def star_want():
    c = star_code()
    return _freeze(FX.layered_fx(c["code"], star_inputs(), 1, 2, q=8, p=16, llr_scale=LLR_SCALE[8], tap_iter=STAR_TAP))


# ---- CRC stop --------------------------------------------------------------------------------------------------------

CRC_WIDTH = (6, 8)


@functools.lru_cache(maxsize=None)
def crc_case():
    """(kind, bits, y, want): bp_cases.crc_case's frames under the fixed-point layered rule with the CRC as a second stop
    predicate"""
    import crc_term_cases as CC
    import crc_term_ref as CR
    kind, bits, y, _ = bc.crc_case()
    c = bg1_code()
    q, p = CRC_WIDTH
    w = FX.layered_fx(c["code"], y, c["z"], CC.MAXIT, q=q, p=p, llr_scale=LLR_SCALE[q],
                      stop=lambda h: CR.crc_passes(kind, h[:, :bits]))
    return kind, bits, y, _freeze(w)


# ---- typed input -----------------------------------------------------------------------------------------------------

TYPED_UNIT = {"i8": 0.125, "f16": 1.0}


@functools.lru_cache(maxsize=None)
def typed_inputs(kind):
    """the 70 BG1 frames as the sender would quantise them: int8 with unit 1/8 (rint, clamped to +-127), or binary16"""
    y = bg1_inputs(70)
    if kind == "i8":
        x = np.clip(np.rint(y / f32(TYPED_UNIT["i8"])), -127, 127).astype(np.int8)
    else:
        x = y.astype(np.float16)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def typed_want(kind, q, p):
    """y = (float)x * unit, one fp32 multiply, then the rule"""
    c = bg1_code()
    y = (typed_inputs(kind).astype(f32) * f32(TYPED_UNIT[kind])).astype(f32)
    return _freeze(FX.layered_fx(c["code"], y, c["z"], BG1_MAXIT, q=q, p=p, llr_scale=LLR_SCALE[q]))
