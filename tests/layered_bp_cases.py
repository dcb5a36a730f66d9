"""Inputs and expectations of tests/test_gpu_layered_bp.py (a helper, not a test module): the BG1-profile test code, the
irregular matrix code with every row a layer of its own, the degenerate frames, the CRC frames of bp_cases and the
punctured-column scenario of ratematch_util under the layered log-domain sum-product rule (tests/layered_bp_ref.py).
Everything here runs on the CPU, is computed once per process and handed out read-only; tests/test_layered_bp_cpu.py
checks that every case reaches what it is there for."""
import functools

import numpy as np

import bp_cases as bc
import fp16_cases as fc
import layered_bp_ref as LB
import ratematch_util as U
from ms_correction_ref import Code

f32 = np.float32
TAP = fc.TAP                        # the round whose R, P and bits are compared
SCALES = bc.SCALES                  # 4.0, and 1.7: no power of two, so the product llr_scale * y rounds


def _freeze(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


# ---- the BG1-profile test code (N = 1088, z = 16, row degrees 3 ... 19) ----------------------------------------------

BG1_MAXIT = 12
BG1_TWO_TILES = 64 * 4 + 6          # V = 4: a full tile and a ragged second one


@functools.lru_cache(maxsize=None)
def bg1_code():
    rows, cols, _ = U.bg1()
    return dict(rows=rows, cols=cols, M=U.M, N=U.N, K=U.K, z=U.Z, code=Code(rows, cols, U.M, U.N, U.K))


@functools.lru_cache(maxsize=None)
def bg1_inputs(frames):
    """frames of the all-zero codeword whose noise level is drawn from [0.4, 1.3]: they stop in round 1, 2, 3, ..., some never"""
    y = fc.noisy_frames(U.N, frames, 0.4, 1.3, seed=20261020 + frames)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def bg1_want(frames, scale=SCALES[0], tap=TAP, early_term=True, maxit=BG1_MAXIT):
    c = bg1_code()
    return _freeze(LB.layered_bp(c["code"], bg1_inputs(frames), c["z"], maxit, llr_scale=scale, tap_iter=tap,
                                 early_term=early_term))


# ---- every degree class: the irregular matrix code, every row a layer ------------------------------------------------

MATRIX_MAXIT = 5                    # about 135 launches per round with layer_rows = 1


@functools.lru_cache(maxsize=None)
def matrix_want(scale=SCALES[0]):
    m = bc.matrix()
    return _freeze(LB.layered_bp(m["code"], m["y"], 1, MATRIX_MAXIT, llr_scale=scale, tap_iter=TAP))


# ---- degenerate inputs -----------------------------------------------------------------------------------------------

def degenerate_layer_rows(name):
    """the WiMAX code is layered by its circulant size; the staircase code's consecutive rows share a column: one row per layer"""
    return fc.wimax()["z"] if name == "wimax" else 1


DEGENERATE_MAXIT = {"wimax": fc.DEGENERATE_MAXIT, "ira": 4}     # ira: 472 launches per round


@functools.lru_cache(maxsize=None)
def degenerate_want(name):
    c, y = fc.degenerate_code(name), fc.degenerate_inputs(name)
    return _freeze(LB.layered_bp(c["code"], y, degenerate_layer_rows(name), DEGENERATE_MAXIT[name],
                                 llr_scale=bc.DEGENERATE_SCALE, tap_iter=TAP))


# ---- CRC stop --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def crc_case():
    """(kind, bits, y, want): bp_cases.crc_case's frames under the layered rule with the CRC as a second stop predicate"""
    import crc_term_cases as CC
    import crc_term_ref as CR
    kind, bits, y, _ = bc.crc_case()
    c = bg1_code()
    w = LB.layered_bp(c["code"], y, c["z"], CC.MAXIT, llr_scale=bc.SCALE, stop=lambda h: CR.crc_passes(kind, h[:, :bits]))
    return kind, bits, y, _freeze(w)


# ---- erasures: scenario S1 of ratematch_util with erasure_llr = 0 ----------------------------------------------------

ERASURE_SCENARIO = "S1"


def erasure_scale():
    """2 / sd^2 of the scenario's noise, as a float32"""
    sd = U.received(ERASURE_SCENARIO)[1]
    return float(f32(2.0 / (sd * sd)))


@functools.lru_cache(maxsize=None)
def erasure_want():
    """the layered BP reference on the scenario's decoder input with exact zeros at the punctured columns"""
    c = bg1_code()
    y = U.recovered(ERASURE_SCENARIO, 0.0, 1)
    return _freeze(LB.layered_bp(c["code"], y, c["z"], U.MAX_ITER, llr_scale=erasure_scale()))


def frames_right(out):
    """frames whose information bytes are the payload's"""
    out = np.asarray(out).reshape(U.FRAMES, U.K // 8)
    return int((out == U.payload()[1].reshape(U.FRAMES, U.K // 8)).all(axis=1).sum())
