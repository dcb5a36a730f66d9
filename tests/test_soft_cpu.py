"""Soft output without a GPU: the expectation helper (tests/soft_ref.py) checked against itself on the chain scenario, and
the two new symbols of the C ABI."""
import ctypes
import re
import os

import numpy as np
import pytest

from myldpccppapi_amd import _lib

import ratematch_util as U
import soft_ref as SR
import tb_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("point", [0, 1], ids=["clean", "hard"])
@pytest.mark.parametrize("algo", ["ms", "layered"])
def test_expectation_is_consistent_on_the_chain_scenario(algo, point):
    """64 frames at 3.0 and 0.0 dB: no NaN, every frame's row supplied by exactly one of the per-round runs, the sign of
    every non-zero posterior is the oracle's hard bit, no undefined frame, extrinsic + y == posterior wherever that sum
    is exact."""
    snr = TU.chain_points(algo)[point]
    y = TU.chain_received(snr)[2]
    w = SR.expected(U.bg1()[2], y, algo, U.MAX_ITER, layer_rows=U.Z)
    want = TU.chain_oracle(algo, snr)
    assert np.array_equal(w["out"], want[0]) and np.array_equal(w["iters"], want[1])
    distinct = np.unique(w["iters"]).size
    print(algo, snr, "distinct iteration counts", distinct, "exact zeros", int((w["post"] == 0).sum()))
    assert distinct >= 3
    assert np.array_equal(w["filled"], np.ones(U.FRAMES, np.int32))
    assert not np.isnan(w["post"]).any() and not np.isnan(w["ext"]).any()
    assert not w["undefined"].any()
    assert SR.sign_disagreements(w["post"], w["hard"]) == 0
    assert np.array_equal(w["ext"], (w["post"] - y).astype(np.float32))


def test_expectation_of_the_variants_differs_where_it_should():
    """fp16 storage and the normalisation change the values, not the rule: both still decide their own hard bits."""
    y = TU.chain_received(TU.CLEAN_DB)[2]
    g = U.bg1()
    import ms_correction_ref as MC
    code = MC.Code(g[0], g[1], U.M, U.N, U.K)
    plain = SR.expected(g[2], y, "ms", U.MAX_ITER)
    half = SR.expected(g[2], y, "ms", U.MAX_ITER, f16=True)
    scaled = SR.expected(g[2], y, "ms", U.MAX_ITER, scale=0.75, code=code)
    # the helper's own sum over ms_correction_ref's R equals the oracle's post tap where both exist (scale 1 = off)
    unit = SR.expected(g[2], y, "ms", U.MAX_ITER, scale=1.0, code=code)
    SR.assert_same_bits(unit["post"], plain["post"], what="y + sum R against the oracle's post tap")
    for w in (half, scaled):
        assert SR.sign_disagreements(w["post"], w["hard"]) == 0 and not np.isnan(w["post"]).any()
        assert np.array_equal(w["filled"], np.ones(U.FRAMES, np.int32))
        assert not np.array_equal(SR.bits(w["post"]), SR.bits(plain["post"]))
    assert np.array_equal(half["ext"], (half["post"] - SR.f16_round(y)).astype(np.float32))


def test_symbols_are_exported_with_the_declared_signatures(built):
    """ldpc_decode_soft_device / ldpc_decode_soft: in the header, in the library, and declared to ctypes argument by
    argument as the header has them."""
    L = _lib.load()
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    ctype_of = {"ldpc_decoder *": vp, "const float *": vp, "float *": vp, "uint8_t *": vp, "int32_t *": vp, "void *": vp,
                "int64_t": i64, "int32_t": i32}
    for name in ("ldpc_decode_soft_device", "ldpc_decode_soft"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        m = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            typ = arg[:arg.rindex("*") + 1] if "*" in arg else arg.rsplit(" ", 1)[0]
            want.append(ctype_of[typ.replace(" *", " *").strip()])
        assert list(getattr(L, name).argtypes) == want, (name, want)
    assert "LDPC_SOFT_POSTERIOR = 1" in header and "LDPC_SOFT_EXTRINSIC = 2" in header
    from myldpccppapi_amd import capi
    assert capi.SOFT_KINDS == {"posterior": 1, "extrinsic": 2}
