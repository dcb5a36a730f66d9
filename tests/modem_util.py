"""Shared set-up of the modem tests: the host build of the noise generator, and the scenario of DESIGN.md section 8f
(the BG1-profile code and payload of ratematch_util, one transmission (k0, E) = (0, 1032), noise seed 100).  Everything
here comes from modem_ref, ratematch_ref, codes.py and the oracle, never from the library under test; the expensive parts
are computed once per process and handed out read-only."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import oracle

import modem_ref as mref
import ratematch_ref as rref
import ratematch_util as U
import util

K0, E, SEED, ERASURE = 0, 1032, 100, 1e-6
#: Qm -> sd per real dimension
POINTS = {2: 0.5, 4: 0.3, 6: 0.2, 8: 0.12}
S_GRID = (1, 2, 3, 64, 65, 257)

_keep = []


@functools.lru_cache(maxsize=None)
def chlib():
    d = tempfile.TemporaryDirectory()
    _keep.append(d)
    return util.host_channel_lib(d.name)


def matched_scale(sd):
    """(llr_scale, fill_llr) of a sum-product decoder that reads demapped values: 2 / sd^2 and min(10, 80 / scale)."""
    scale = 2.0 / (sd * sd)
    return scale, min(10.0, 80.0 / scale)


@functools.lru_cache(maxsize=None)
def tx_bits():
    tx = rref.match(U.scenario_spec(0.0), U.payload()[2], K0, E)
    tx.setflags(write=False)
    return tx


@functools.lru_cache(maxsize=None)
def received(Qm, interleave):
    """(symbols float32 [64, symbol_floats], demapped rx float32 [64, E]) by modem_ref alone."""
    sym = mref.transmit(Qm, interleave, tx_bits(), POINTS[Qm], SEED, 0, chlib())
    rx = mref.demap(Qm, interleave, sym, E)
    for a in (sym, rx):
        a.setflags(write=False)
    return sym, rx


@functools.lru_cache(maxsize=None)
def recovered(Qm, interleave, fill_llr):
    spec = rref.Spec(U.N, U.P, U.FILLER, fill_llr, ERASURE)
    y = rref.recover(spec, received(Qm, interleave)[1], K0, E)[1]
    y.setflags(write=False)
    return y


def decoder_settings(Qm, algo):
    """(llr_scale, fill_llr): the matched scale for sp, the defaults of the rate-matching scenarios otherwise."""
    return matched_scale(POINTS[Qm]) if algo == "sp" else (U.LLR_SCALE, 10.0)


@functools.lru_cache(maxsize=None)
def oracle_decode(Qm, interleave, algo):
    """(out bytes, iters, frames with a wrong information bit) of oracle.decode on recovered(...)."""
    scale, fill = decoder_settings(Qm, algo)
    r = oracle.decode(U.bg1()[2], recovered(Qm, interleave, fill), algo, max_iter=U.MAX_ITER, llr_scale=scale, layer_rows=U.Z)
    wrong = (np.asarray(r["out"]).reshape(U.FRAMES, U.K // 8) != U.payload()[1].reshape(U.FRAMES, U.K // 8)).any(axis=1)
    return r["out"], r["iters"], int(wrong.sum())


def raw_ber(Qm, interleave):
    return float(((received(Qm, interleave)[1] < 0) != (tx_bits() != 0)).mean())


def coder_modulation_exe(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "coder_modulation")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "coder_modulation.cpp"), "-o", exe,
                           "-L" + os.path.join(root, "myldpccppapi_amd"), "-lmyldpc", "-lldpc_hip",
                           "-Wl,-rpath," + os.path.join(root, "myldpccppapi_amd")])
    return exe
