"""CPU side of fp8 (E4M3) messages: the rounding s8 against a rounding built independently from the table of the 256
codes, the numpy restatement (tests/fp8_ref.py) against the references that exist for fp32 and fp16 messages, the
premises of the GPU cases (tests/test_gpu_fp8.py), and that the definition decodes.  No test here touches the library
under test.  Every test prints the counts it found (pytest -s shows them)."""
import functools

import numpy as np
import pytest

import oracle
from myldpccppapi_amd import channel, codes

import fp16_cases as fc
import fp8_cases as f8c
import fp8_ref as R8
from ms_correction_ref import Code, flood_ms

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def table_round(x):
    """s8 without s8's arithmetic: the nearest of the 254 finite code values (beyond +-448: the nearest is +-448), of two
    equally near ones the one whose code byte is even; the sign of the input where the result is zero; NaN for NaN."""
    t = R8.e4m3_table()
    codes_pos = np.arange(127)                                # 0x00 ... 0x7e: ascending values 0 ... 448
    vals = t[codes_pos]
    x = np.asarray(x, f32)
    a = np.abs(x.astype(np.float64))
    out = np.empty(x.shape, np.float64)
    for i, ai in enumerate(a.reshape(-1)):
        if np.isnan(ai):
            out.reshape(-1)[i] = np.nan
            continue
        d = np.abs(vals - min(ai, 448.0))                    # beyond the largest value (infinity included) it is the nearest
        best = np.nonzero(d == d.min())[0]
        pick = best[0] if best.size == 1 else best[best % 2 == 0][0]
        out.reshape(-1)[i] = vals[pick]
    return np.copysign(out, x.astype(np.float64)).astype(f32)


def test_s8_is_nearest_code_ties_to_even_code():
    """All 256 code values, the midpoint of every neighbouring pair and its two fp32 neighbours, the edge list of the
    definition: s8 equals the table rounding as bits (signs of zeros included), NaN for NaN; code values are fixed points."""
    x = R8.edge_inputs()
    assert fc.same_floats(R8.s8(x), table_round(x))
    t = R8.e4m3_table()
    fin = t[~np.isnan(t)].astype(f32)
    assert fin.size == 254 and np.array_equal(_bits(R8.s8(fin)), _bits(fin))
    want = {464: 448, 1000: 448, np.inf: 448, -np.inf: -448, 2.0 ** -10: 0, 1.5 * 2.0 ** -10: 2.0 ** -9, 3 * 2.0 ** -10: 2.0 ** -8,
            1.0625: 1, 1.1875: 1.25, 15.5: 16, 1e-6: 0, 1e-41: 0}
    for k, v in want.items():
        assert R8.s8(f32(k)) == f32(v), (k, v)
    assert _bits(R8.s8(f32(-1e-8)))[()] == 0x80000000
    assert np.isnan(R8.s8(f32(np.nan)))


def test_s8_on_a_million_random_floats():
    """10^6 floats, log-uniform magnitudes over 2^-14 ... 2^11 and both signs, in vectorised form: nearest finite code
    value by binary search over the sorted table, ties to the even code."""
    rng = np.random.default_rng(8)
    x = (np.exp2(rng.uniform(-14, 11, 10 ** 6)) * rng.choice([-1.0, 1.0], 10 ** 6)).astype(f32)
    vals = R8.e4m3_table()[:127]
    a = np.minimum(np.abs(x.astype(np.float64)), 448.0)
    hi = np.clip(np.searchsorted(vals, a), 1, 126)
    lo = hi - 1
    dl, dh = a - vals[lo], vals[hi] - a
    pick = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    want = np.copysign(vals[pick], x).astype(f32)
    assert np.array_equal(_bits(R8.s8(x)), _bits(want))
    print("ties among the random inputs:", int((dl == dh).sum()))


@functools.lru_cache(maxsize=None)
def _anchor_case():
    c = fc.staircase(7, "ride")
    return c, c["y"][:40]


def test_identity_rounding_is_the_oracle():
    """rnd = identity: bytes, iteration counts, hard bits and both taps of oracle.decode(..., "ms"), and the corrected form
    equals ms_correction_ref.flood_ms."""
    c, y = _anchor_case()
    got = R8.flood(c["code"], y, fc.MAXIT, rnd=R8.identity, tap_iter=fc.TAP)
    want = fc.as_ref(oracle.decode(c["og"], y, "ms", max_iter=fc.MAXIT, tap_iter=fc.TAP))
    run_r, run_q = fc.tap_frames(want["iters"])
    assert run_q.size >= 10
    for key in ("out", "iters", "hard"):
        assert np.array_equal(got[key], want[key]), key
    assert fc.same_floats(got["r_tap"][run_r], want["r_tap"][run_r]) and fc.same_floats(got["q_tap"][run_q], want["q_tap"][run_q])
    for setting in fc.SETTINGS:
        got = R8.flood(c["code"], y, fc.MAXIT, *setting, rnd=R8.identity, tap_iter=fc.TAP)
        want = flood_ms(c["code"], y, fc.MAXIT, *setting, tap_iter=fc.TAP)
        for key in ("out", "iters", "hard"):
            assert np.array_equal(got[key], want[key]), (setting, key)
        assert fc.same_floats(got["r_tap"], want["r_tap"]) and fc.same_floats(got["q_tap"], want["q_tap"]), setting


def test_binary16_rounding_is_flood_ms_f16():
    """rnd = binary16: flood_ms(f16=True), plain and corrected, on the staircase frames and on the fp16 degenerate inputs"""
    c, y = _anchor_case()
    for yy, cc in ((y, c["code"]), (fc.degenerate_inputs("wimax"), fc.wimax()["code"])):
        for setting in ((0.0, 0.0),) + fc.SETTINGS:
            got = R8.flood(cc, yy, fc.DEGENERATE_MAXIT, *setting, rnd=R8.f16, tap_iter=fc.TAP)
            want = flood_ms(cc, yy, fc.DEGENERATE_MAXIT, *setting, f16=True, tap_iter=fc.TAP)
            for key in ("out", "iters", "hard"):
                assert np.array_equal(got[key], want[key]), (setting, key)
            assert fc.same_floats(got["r_tap"], want["r_tap"]) and fc.same_floats(got["q_tap"], want["q_tap"]), setting


@pytest.mark.parametrize("d", fc.DEGREES)
def test_premises_of_the_gpu_cases(d):
    """On staircase(d), 133 frames, 25 rounds, under the fp8 rule, plain and with each correction: frames stop at many
    distinct rounds, some never do for d = 7 and 16, the iteration counts differ from the fp16 expectation in at least
    one frame (a kernel that silently ran fp16 would fail), at least one frame compares its Q tap, and -- corrected
    min-sum -- the model of a kernel that left R unrounded in registers changes the Q tap of at least one compared frame."""
    c = fc.staircase(d, "ride")
    for setting in (None,) + fc.SETTINGS:
        w = f8c.want(d, "ride", setting)
        it = w["iters"]
        never = int((it == fc.MAXIT).sum()) - int(c["code"].syndrome_ok(w["hard"][it == fc.MAXIT]).sum())
        differ16 = int((it != fc.want(d, "ride", setting)["iters"]).sum())
        run_r, run_q = fc.tap_frames(it)
        print("d=%d %s: %d distinct rounds, %d frames never converge, iterations differ from fp16 in %d frames, %d compare Q"
              % (d, setting, np.unique(it).size, never, differ16, run_q.size))
        assert np.unique(it).size >= 2 and differ16 >= 1 and run_q.size >= 1, (d, setting)
        if d in (7, 16):
            assert never >= 1, (d, setting)
        if setting is None:          # plain: R is +-|q| of stored messages, there is nothing to leave unrounded
            continue
        bad = f8c.want_registers_unrounded(d, setting)
        q_frames = [f for f in run_q if not fc.same_floats(bad["q_tap"][f], w["q_tap"][f])]
        print("    R unrounded in registers: Q tap differs in %d of %d compared frames" % (len(q_frames), run_q.size))
        assert len(q_frames) >= 1, (d, setting)


def test_premises_of_degenerate_and_handover_cases():
    """The degenerate frames keep their NaN and saturated values in what is compared, the frame of +-400 saturates Q after
    round 1, and the hand-over batch has stragglers that run all rounds."""
    for name in ("wimax", "ira"):
        y = f8c.degenerate_inputs(name)
        y8 = R8.s8(y)
        assert np.isnan(y8).sum() == 5 and (np.abs(y8) == 448).sum() >= 100 and (_bits(y8) == 0x80000000).sum() >= 1
        for corrected in (False, True):
            w = f8c.degenerate_want(name, corrected)
            sat = np.abs(w["q_tap"][f8c.SATURATING_FRAME])
            print(name, corrected, "saturated Q in the +-400 frame:", int((sat == 448).sum()))
            if w["iters"][f8c.SATURATING_FRAME] > fc.TAP:
                assert (sat == 448).sum() >= 1
    w = f8c.handover_want(fc.HANDOVER_BATCHES[0])
    full = int((w["iters"] == fc.HANDOVER_MAXIT).sum())
    print("hand-over: %d of %d frames run all rounds" % (full, w["iters"].size))
    assert 20 <= full <= fc.HANDOVER_STRAGGLERS + 10


def test_the_definition_decodes():
    """WiMAX (2304, 1152), 256 frames at 2.5 dB, 20 rounds: every frame is error-free under fp8 messages."""
    rate, N = codes.RATE_1_2, 2304
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    y = channel.awgn_frames(N, 0, 256, 10.0 ** (-2.5 / 20.0), seed=7)
    r = R8.flood(Code(rows, cols, M, N, K), y, 20)
    errors = int(r["hard"].any(axis=1).sum())
    print("frame errors: %d of 256, mean rounds %.2f" % (errors, r["iters"].mean()))
    assert errors == 0
