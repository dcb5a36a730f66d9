"""Inputs and expectations of tests/test_gpu_bp.py (a helper, not a test module): the codes and frames of
kernel_matrix.py and fp16_cases.py under the log-domain sum-product rule (tests/bp_ref.py).  Everything here runs on the
CPU, is computed once per process and handed out read-only; tests/test_bp_cpu.py checks that every case reaches what it
is there for."""
import functools

import numpy as np

from myldpccppapi_amd import channel
from util import converged_frames

import bp_ref as RB
import fp16_cases as fc
import kernel_matrix as km
from ms_correction_ref import Code

f32 = np.float32
# the channel values of the cases are BPSK +-1 in noise of standard deviation around 0.7: 2 / sd^2 is about 4
SCALE = 4.0
SCALES = (4.0, 1.7)                 # the second one: no power of two, so the product llr_scale * y rounds
RND = {"f32": RB.identity, "f16": RB.f16}


def _freeze(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


# ---- every degree class: the irregular matrix code ------------------------------------------------------------------

MATRIX_FRAMES = 70
MATRIX_MAXIT = 20


@functools.lru_cache(maxsize=None)
def matrix():
    """dict(rows, cols, M, N, K, code, y): kernel_matrix.matrix_code() -- rows of every degree 0 ... 33 and 40 -- and 70
    frames whose noise level is drawn from [0.15, 0.8]"""
    rows, cols, M, N = km.matrix_code()
    K = (N - M) // 8 * 8
    y = fc.noisy_frames(N, MATRIX_FRAMES, 0.15, 0.8, seed=20261019)
    y.setflags(write=False)
    return dict(rows=rows, cols=cols, M=M, N=N, K=K, code=Code(rows, cols, M, N, K), y=y)


@functools.lru_cache(maxsize=None)
def matrix_want(storage, scale=SCALE):
    m = matrix()
    return _freeze(RB.flood(m["code"], m["y"], MATRIX_MAXIT, rnd=RND[storage], llr_scale=scale, tap_iter=fc.TAP))


# ---- the column-fused forms: staircase codes ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def want(d, kind="ride", storage="f32"):
    c = fc.staircase(d, kind)
    return _freeze(RB.flood(c["code"], c["y"], fc.MAXIT, rnd=RND[storage], llr_scale=SCALE, tap_iter=fc.TAP))


@functools.lru_cache(maxsize=None)
def want_registers_unrounded(d):
    """The model of a wrong fp16 kernel on the ride code: the staircase columns see R before its rounding to binary16"""
    c = fc.staircase(d, "ride")
    return _freeze(RB.flood(c["code"], c["y"], fc.MAXIT, rnd=RB.f16, llr_scale=SCALE, tap_iter=fc.TAP, raw_cols=fc.fused_columns(c)))


# ---- degenerate inputs ----------------------------------------------------------------------------------------------

DEGENERATE_SCALE = 1.0              # the overlay's values are at the edges of binary16 as they are


@functools.lru_cache(maxsize=None)
def degenerate_want(name, storage):
    c, y = fc.degenerate_code(name), fc.degenerate_inputs(name)
    return _freeze(RB.flood(c["code"], y, fc.DEGENERATE_MAXIT, rnd=RND[storage], llr_scale=DEGENERATE_SCALE, tap_iter=fc.TAP))


# ---- hand-over, soft output -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def handover_want(B, storage="f32"):
    """fp16_cases.handover_inputs(B) under the BP rule; with post / chan for the soft-output test"""
    c, y = fc.staircase(7, "ride"), fc.handover_inputs(B)
    r = RB.flood(c["code"], y, fc.HANDOVER_MAXIT, rnd=RND[storage], llr_scale=SCALE)
    r["n_conv"] = int(converged_frames(c["rows"], c["cols"], c["M"], r["hard"]).sum())
    return _freeze(r)


# ---- the premise of the feature -------------------------------------------------------------------------------------

def wimax_frames(N, frames, snr_db, seed):
    """(y, sd): the all-zero codeword, reference convention sd = 10^(-SNR / 20)"""
    sd = 10.0 ** (-snr_db / 20.0)
    return channel.awgn_frames(N, 0, frames, sd, seed=seed), sd


# ---- CRC stop -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def crc_case():
    """(kind, bits, y, want): 150 frames of the BG1-profile code that carry a CRC16, every third at the hard noise, under the
    BP rule with the CRC as a second stop predicate"""
    import crc_term_cases as CC
    import crc_term_ref as CR
    import ratematch_util as U
    kind, bits, _ = CC.frame_crc("chain")
    rows, cols, _ = U.bg1()
    y = CC.received("chain", 150, 0.75, 0.98, 3)
    w = RB.flood(Code(rows, cols, U.M, U.N, U.K), y, CC.MAXIT, llr_scale=SCALE, stop=lambda h: CR.crc_passes(kind, h[:, :bits]))
    return kind, bits, y, _freeze(w)
