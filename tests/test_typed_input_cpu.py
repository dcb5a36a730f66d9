"""Typed channel values (int8 / fp16 input) without a GPU: the quantiser rule on hand cases, the premises of the GPU cases
of tests/test_gpu_typed_input.py, and the bindings.

The quantiser and premise tests depend on the numpy reference of tests/typed_input_ref.py alone -- they pass with or
without the feature and are there so that a seed, a unit or a scale that tests nothing fails here instead of passing
silently on the GPU.  The binding tests need the new symbols."""
import numpy as np

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib

import typed_input_ref as T

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_quantiser_rule_on_hand_cases():
    """int8: ties at +-0.5, +-1.5, 2.5 and +-126.5 go to the even code, +-127.4, 127.5, +-200 and +-inf clamp to +-127, -128
    is never produced, NaN gives 0, -0 gives 0.  fp16: 65519 (finite in fp16 by rounding) and 65520 (would round to inf)
    both give 65504, 1e-8 underflows to 0, NaN stays NaN, ties go to the even mantissa."""
    t = np.array([v for v, _ in T.I8_HAND], F32)
    got = T.quantize(t, 1.0, "i8")
    assert got.dtype == np.int8 and np.array_equal(got, np.array([c for _, c in T.I8_HAND], np.int8)), got
    t = np.array([v for v, _ in T.F16_HAND], F32)
    got = T.quantize(t, 1.0, "f16")
    want = np.array([c for _, c in T.F16_HAND], np.float16)
    assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), want.view(np.uint16)), got
    # the divide is a rounding of its own: 0.5 * unit / unit need not be 0.5, but the rule is stated on t = y / unit
    y = (F32(0.0371) * np.arange(-140, 141, dtype=F32)).astype(F32)
    q = T.quantize(y, 0.0371, "i8")
    assert q.min() == -127 and q.max() == 127 and np.array_equal(q[13:268], np.arange(-127, 128, dtype=np.int8))


def test_dequantised_values_are_exact_widenings_times_the_unit():
    """all 256 int8 codes and all 65536 binary16 patterns: y = float32(x) * float32(unit) with one rounding, in float64
    terms fl32(x * unit); infinities and NaN pass through"""
    unit = T.UNITS["i8"]
    x = np.arange(-128, 128).astype(np.int8)
    want = (x.astype(np.float64) * np.float64(F32(unit))).astype(F32)
    assert np.array_equal(_bits(T.dequantize(x, unit)), _bits(want))
    h = np.arange(65536, dtype=np.uint16).view(np.float16)
    y = T.dequantize(h, T.UNITS["f16"])
    fin = np.isfinite(h)
    with np.errstate(over="ignore"):
        want = (h[fin].astype(np.float64) * np.float64(F32(T.UNITS["f16"]))).astype(F32)
    assert np.array_equal(_bits(y[fin]), _bits(want))
    assert np.isnan(y[np.isnan(h)]).all() and np.array_equal(y[np.isinf(h)], h[np.isinf(h)].astype(F32))


def test_two_roundings_differ_from_the_folded_product_on_the_cases_inputs():
    """The premise of the GPU cases: with the cases' units and their scales that are no power of two -- BP's 1.7 and the
    second sum-product scale 6.3 -- fl(fl(x * unit) * scale) differs from fl(x * fl(unit * scale)) for int8 codes that ARE
    in the inputs, so a kernel that folds llr_unit into llr_scale fails them; for SP the exp taps of such codes differ as
    well."""
    codes8 = np.arange(-128, 128).astype(np.int8)
    for cname in T.FLOOD_CODES:
        present = np.isin(codes8, T.inputs(cname, "i8"))
        assert present[0] and present[255], cname                      # -128 and +127 are in the inputs
        for unit in (T.UNITS["i8"], T.UNITS["f16"]):
            assert np.log2(unit) != np.round(np.log2(unit))
            for scale in (T.BP_SCALES[1], T.SP_SCALE_2):
                a, b = T.two_step(codes8, unit, scale), T.folded(codes8, unit, scale)
                differ = (_bits(a) != _bits(b)) & present
                assert differ.any(), (cname, unit, scale)
                if scale == T.SP_SCALE_2:
                    assert (_bits(T.expf(a[differ])) != _bits(T.expf(b[differ]))).any(), (cname, unit)


def test_power_of_two_scales_commute_with_the_rounding():
    """The plan for this feature asked for the same premise under SP's scale 8 and BP's 4.0.  It cannot hold there: multiplying by a power of
    two is exact (no overflow or underflow in range), so fl(fl(x * unit) * 8) == fl(x * fl(unit * 8)) for every code, and
    likewise for 4.  That is why the GPU cases also run SP at 6.3 and BP at 1.7; this test pins the fact."""
    codes8 = np.arange(-128, 128).astype(np.int8)
    for unit in T.UNITS.values():
        for scale in (T.SP_SCALE, T.BP_SCALES[0]):
            assert np.array_equal(_bits(T.two_step(codes8, unit, scale)), _bits(T.folded(codes8, unit, scale))), (unit, scale)


def test_cases_stop_in_several_rounds_and_some_never():
    """every flooding and layered case: frames stop in at least four distinct rounds before the last, and some never stop"""
    for cname in T.FLOOD_CODES:
        for kind in ("i8", "f16"):
            for algo, storage in T.FLOOD_ARITH:
                it = T.flood_want(cname, kind, algo, storage)["iters"]
                early = np.unique(it[it < T.MAXIT])
                assert early.size >= 4 and (it == T.MAXIT).sum() >= 5, (cname, kind, algo, storage, np.bincount(it))
                # every tile width's head has both kinds of frames too
                for V in (1, 2, 4):
                    h = it[:64 * V + 5]
                    assert (h < T.MAXIT).any() and (h == T.MAXIT).any(), (cname, kind, algo, storage, V)
    for algo in ("layered", "layered_host", "layered_bp"):
        for kind in ("i8", "f16"):
            w = T.layered_want(algo, kind)
            it = w["iters"]
            assert np.unique(it[it < T.MAXIT]).size >= 4 and (it == T.MAXIT).sum() >= 5, (algo, kind, np.bincount(it))
            assert (it >= T.TAP).sum() > 0


def test_int8_inputs_hold_both_end_codes_and_rows_that_are_no_16_byte_multiples():
    for cname in T.FLOOD_CODES + ("bg1", "h576"):
        x = T.inputs(cname, "i8", T.FLOOD_FRAMES if cname in T.FLOOD_CODES else T.LAYERED_FRAMES)
        assert x.dtype == np.int8 and x.min() == -128 and x.max() == 127, cname
    assert T.code("w576")["N"] % 16 == 0 and (2 * T.code("w648")["N"]) % 16 == 0     # the 16-byte path: both types / fp16 only
    assert T.code("w648")["N"] % 16 != 0 and T.code("matrix")["N"] % 8 != 0          # the per-element path


def test_bindings_export_the_typed_entry_points():
    lib = _lib.load()
    for name in ("ldpc_decode_typed_device", "ldpc_decode_soft_typed_device", "ldpc_decode_typed", "ldpc_decode_soft_typed",
                 "ldpc_llr_quantize_device"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.ldpc_abi_version() == 3
    assert (L.capi.LLR_F32, L.capi.LLR_F16, L.capi.LLR_I8) == (0, 1, 2)
    assert callable(L.quantize_device)


def test_decode_without_a_unit_still_converts_to_float32(monkeypatch):
    """Decoder.decode(int8 array) without llr_unit is the old call: the array is converted to float32 and ldpc_decode gets
    it; with llr_unit the array's own dtype names the element type of ldpc_decode_typed.  No device is needed: the C entry
    points are replaced by recorders."""
    calls = []

    class Lib:
        def ldpc_decode(self, h, ptr, frames, *rest):
            calls.append(("plain", frames))
            return 0

        def ldpc_decode_typed(self, h, ptr, ty, unit, frames, *rest):
            calls.append(("typed", ty, unit, frames))
            return 0

    dec = L.Decoder.__new__(L.Decoder)
    dec._h, dec.K, dec.N = None, 8, 16
    dec.cfg = _lib.DecoderConfigCrc()
    seen = {}
    real = np.ascontiguousarray

    def spy(a, dtype=None, **kw):
        r = real(a, dtype, **kw)
        seen.setdefault("dtypes", []).append(r.dtype)
        return r

    monkeypatch.setattr(_lib, "load", lambda: Lib())
    monkeypatch.setattr(L.capi, "out_bytes", lambda K, frames, pack_mode=0: frames * K // 8)
    monkeypatch.setattr(L.capi.np, "ascontiguousarray", spy)
    x = np.arange(32, dtype=np.int8).reshape(2, 16)
    dec.decode(x)
    assert calls == [("plain", 2)] and seen["dtypes"][0] == np.float32
    dec.decode(x, llr_unit=0.25)
    dec.decode(x.astype(np.float16), llr_unit=0.5)
    dec.decode(x.astype(np.float32), llr_unit=1.0)
    assert calls[1:] == [("typed", 2, 0.25, 2), ("typed", 1, 0.5, 2), ("typed", 0, 1.0, 2)]
    try:
        dec.decode(x.astype(np.int16), llr_unit=1.0)
    except TypeError:
        pass
    else:
        raise AssertionError("an int16 array with llr_unit must be refused")
    dec._h = None
