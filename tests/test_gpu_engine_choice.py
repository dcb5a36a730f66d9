"""Which engine a configuration runs on, seen from outside: the kernel-time labels of one timed decode per case, and the
decoded bytes and iteration counts against the same algorithm with LDPC_TUNE_FUSED and LDPC_TUNE_LDSP forced off (the
streaming kernels; the engines agree bit for bit).

The label sets below were recorded on an MI355X from the library of the commit in front of the one that put the engine
choice into csrc/decoder_config_host.hpp (engine_candidates) and a single engine tag on the handle; they pin that the
choice did not move.  The (576, 288) WiMAX code, layer_rows = 24, 64 frames, 5 rounds.  LDPC_ALGO_LAYERED_HOST is
refused on that code (its rows have weights 6 and 7), so its case runs the (576, 480) code of the same circulant size,
whose rows all have weight 20.
"""
import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes

pytestmark = pytest.mark.gpu

N, FRAMES, MAX_ITER = 576, 64, 5
OFF = {"fused": False, "ldsp": False}

# name -> (Decoder arguments, label prefixes: the text in front of `<` or `[`)
FLOODING = {"check_group_kernel", "var_group_kernel", "var_kernel", "other"}      # the streaming flooding kernels of this code
CASES = {
    "sp": (dict(algo="sp"), {"fused_sp_kernel"}),
    "ms": (dict(algo="ms"), {"flood_ldsp_kernel"}),
    "layered": (dict(algo="layered"), {"layered_ldsp_kernel"}),
    "ms_fused": (dict(algo="ms_fused"), {"flood_ldsp_kernel"}),
    "layered_host": (dict(algo="layered_host"), {"layer_kernel"}),
    "bp": (dict(algo="bp"), FLOODING),
    "layered_bp": (dict(algo="layered_bp"), {"layer_kernel"}),
    "layered_fx": (dict(algo="layered_fx", msg_dtype="i8"), {"layer_kernel"}),
    "layered_bp_fx": (dict(algo="layered_bp_fx", msg_dtype="i8"), {"layer_kernel"}),
    "bitflip": (dict(algo="bitflip"), {"bitflip_check_kernel", "bitflip_vote_kernel", "bitflip_flip_kernel", "other"}),
    "ms scaled": (dict(algo="ms", ms_scale=0.75), {"flood_ldsp_corr_kernel"}),
    "layered scaled": (dict(algo="layered", ms_scale=0.75), {"layered_ldsp_corr_kernel"}),
    "ms ldsp off": (dict(algo="ms", tune={"ldsp": False}), {"fused_flood_kernel"}),
    "layered ldsp off": (dict(algo="layered", tune={"ldsp": False}), {"fused_layered_kernel"}),
    "ms fused off": (dict(algo="ms", tune={"fused": False}), FLOODING),
    "layered_fx fx_record": (dict(algo="layered_fx", msg_dtype="i8", tune={"fx_record": True}), {"layered_ldsp_fx_kernel"}),
    "ms crc": (dict(algo="ms", crc_kind=16, crc_bits=288), FLOODING),
}


def _code(algo):
    rate = codes.RATE_5_6 if algo == "layered_host" else codes.RATE_1_2
    K, M, z = codes.wimax_dims(rate, N)
    assert z == 24
    return rate, K, M


_shared = {}


def _graph(rate, M):
    if rate not in _shared:
        _shared[rate] = L.Graph(*codes.wimax_edges(rate, N), M, N)
    return _shared[rate]


def _llr():
    if "llr" not in _shared:
        y = channel.awgn_frames(N, 0, FRAMES, 0.85, seed=20261021)
        y.setflags(write=False)
        _shared["llr"] = y
    return _shared["llr"]


def run(kw, timing):
    """(label prefixes or None, bytes, iteration counts) of one decode"""
    rate, K, M = _code(kw["algo"])
    dec = L.Decoder(_graph(rate, M), K, max_batch=FRAMES, max_iter=MAX_ITER, layer_rows=24, **kw)
    try:
        if timing:
            dec.set_timing(True)
        out, iters = dec.decode(_llr())
        labels = None
        if timing:
            labels = {t["name"].split("<")[0].split("[")[0] for t in dec.kernel_times()}
        return labels, out, iters
    finally:
        dec.close()


def _streaming(kw):
    """the same algorithm on the streaming kernels: decoded once per configuration"""
    plain = {k: v for k, v in kw.items() if k != "tune"}
    key = tuple(sorted(plain.items()))
    if key not in _shared:
        _shared[key] = run(dict(plain, tune=OFF), timing=False)[1:]
    return _shared[key]


@pytest.mark.parametrize("name", list(CASES))
def test_engine_and_result(built, name):
    kw, want = CASES[name]
    labels, out, iters = run(kw, timing=True)
    print(name, sorted(labels), "iterations", np.bincount(iters, minlength=MAX_ITER + 1).tolist())
    assert labels == want
    ref_out, ref_iters = _streaming(kw)
    assert np.array_equal(out, ref_out) and np.array_equal(iters, ref_iters)
