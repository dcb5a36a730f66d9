"""Inputs and expectations of tests/test_gpu_layered_bp_fx.py (a helper, not a test module): the codes and the channel values of
tests/layered_fx_cases.py -- the BG1-profile test code, the irregular matrix code with every row a layer of its own, the
saturation overlay on WiMAX (576, 288), the CRC frames and the typed inputs -- under the fixed-point layered box-plus rule
(tests/layered_bp_fx_ref.py), with the correction table the library hands out (ldpc_bp_fx_table, which needs no device).
Everything here runs on the CPU, is computed once per process and handed out read-only; tests/test_layered_bp_fx_cpu.py checks
that every case reaches what it is there for."""
import functools

import numpy as np

import myldpccppapi_amd as L

import layered_bp_fx_ref as BX
import layered_fx_cases as xc

f32 = np.float32
TAP = xc.TAP
LLR_SCALE = xc.LLR_SCALE            # LSBs per unit of channel value at every width: with FRAC below, llr_scale * y = 2 y LLR units
WIDTHS = ((6, 8, 2), (8, 16, 4))    # (q, p, f) of the BG1 and matrix cases
SATURATION_WIDTHS = ((4, 4, 0), (6, 8, 2), (8, 16, 3))      # p = q, p = q + 2, p = 16; f = 0 is the table {1, 0}

_freeze = xc._freeze
as_float = xc.as_float


@functools.lru_cache(maxsize=None)
def table(f):
    """T_f from the library, read-only"""
    t = L.bp_fx_table(f)
    t.setflags(write=False)
    return t


# ---- the BG1-profile test code (N = 1088, z = 16, row degrees 3 ... 19) ----------------------------------------------

BG1_MAXIT = xc.BG1_MAXIT
BG1_TWO_TILES = xc.BG1_TWO_TILES
bg1_code = xc.bg1_code
bg1_inputs = xc.bg1_inputs


@functools.lru_cache(maxsize=None)
def bg1_want(frames, q, p, f, tap=TAP, early_term=True, pack_mode=0):
    c = bg1_code()
    return _freeze(BX.layered_bp_fx(c["code"], bg1_inputs(frames), c["z"], BG1_MAXIT, table(f), q=q, p=p, llr_scale=LLR_SCALE[q],
                                    tap_iter=tap, early_term=early_term, pack_mode=pack_mode))


# ---- every degree class: the irregular matrix code, every row a layer ------------------------------------------------

MATRIX_MAXIT = xc.MATRIX_MAXIT
matrix = xc.matrix


@functools.lru_cache(maxsize=None)
def matrix_want(q, p, f):
    m = matrix()
    return _freeze(BX.layered_bp_fx(m["code"], m["y"], 1, MATRIX_MAXIT, table(f), q=q, p=p, llr_scale=LLR_SCALE[q], tap_iter=TAP))


# ---- saturation and degenerate channel values: WiMAX (576, 288) ------------------------------------------------------

SATURATION_MAXIT = xc.SATURATION_MAXIT["wimax"]


def saturation_code():
    return xc.saturation_code("wimax")


def saturation_inputs(q):
    return xc.saturation_inputs("wimax", q)


@functools.lru_cache(maxsize=None)
def saturation_want(q, p, f):
    c = saturation_code()
    return _freeze(BX.layered_bp_fx(c["code"], saturation_inputs(q), c["z"], SATURATION_MAXIT, table(f), q=q, p=p,
                                    llr_scale=LLR_SCALE[q], tap_iter=TAP))


# ---- CRC stop --------------------------------------------------------------------------------------------------------

CRC_WIDTH = (6, 8, 2)


@functools.lru_cache(maxsize=None)
def crc_case():
    """(kind, bits, y, want): bp_cases.crc_case's frames under this rule with the CRC as a second stop predicate"""
    import bp_cases as bc
    import crc_term_cases as CC
    import crc_term_ref as CR
    kind, bits, y, _ = bc.crc_case()
    c = bg1_code()
    q, p, f = CRC_WIDTH
    w = BX.layered_bp_fx(c["code"], y, c["z"], CC.MAXIT, table(f), q=q, p=p, llr_scale=LLR_SCALE[q],
                         stop=lambda h: CR.crc_passes(kind, h[:, :bits]))
    return kind, bits, y, _freeze(w)


# ---- typed input -----------------------------------------------------------------------------------------------------

TYPED_UNIT = xc.TYPED_UNIT
typed_inputs = xc.typed_inputs


@functools.lru_cache(maxsize=None)
def typed_want(kind, q, p, f):
    """y = (float)x * unit, one fp32 multiply, then the rule"""
    c = bg1_code()
    y = (typed_inputs(kind).astype(f32) * f32(TYPED_UNIT[kind])).astype(f32)
    return _freeze(BX.layered_bp_fx(c["code"], y, c["z"], BG1_MAXIT, table(f), q=q, p=p, llr_scale=LLR_SCALE[q]))
