"""CPU side of tests/test_gpu_fp16.py: the premises of its cases (fp16_cases.py), from the oracle and the numpy restatement
alone.  A seed under which a GPU test would compare nothing -- no frame still running at the tap, no linked class, no
straggler -- fails here instead of passing silently there.  Every test prints the counts it found (pytest -s shows them)."""
import numpy as np
import pytest

import fp16_cases as fc
import kernel_matrix as km

IDS = ["d%d_%s" % c for c in fc.CASES]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("d,kind", fc.CASES, ids=IDS)
def test_staircase_frames_stop_at_many_rounds(d, kind):
    """At least 60 of the 133 frames are still running after round 2 (their Q is compared), frames stop at five or more
    distinct rounds, and for d = 7 and 16 at least 10 run all 25 rounds -- under plain and under corrected min-sum."""
    for setting in (None,) + fc.SETTINGS:
        it = fc.want(d, kind, setting)["iters"]
        run_r, run_q = fc.tap_frames(it)
        full = int((it == fc.MAXIT).sum())
        print("d=%d %s %s: %d frames compare R, %d compare Q, %d distinct rounds, %d reach %d"
              % (d, kind, setting, run_r.size, run_q.size, np.unique(it).size, full, fc.MAXIT))
        assert it.size == fc.FRAMES and run_q.size >= 60 and np.unique(it).size >= 5, (d, kind, setting)
        if setting is None and d in (7, 16):
            assert full >= 10, (d, kind)
        assert not np.isnan(fc.want(d, kind, setting)["q_tap"][run_q]).any()
        assert np.isnan(fc.want(d, kind, setting)["q_tap"][it <= fc.TAP]).all()


@pytest.mark.parametrize("d,kind", fc.CASES, ids=IDS)
def test_fp16_and_fp32_messages_differ_in_every_compared_frame(d, kind):
    """A kernel that kept fp32 messages where the definition stores binary16 cannot pass: the two oracles' Q taps differ,
    as bits, in every frame whose Q is compared."""
    w16, w32 = fc.want(d, kind), fc.want(d, kind, None, False)
    run_q = fc.tap_frames(w16["iters"])[1]
    differ = [f for f in run_q if w32["iters"][f] <= fc.TAP or not np.array_equal(_bits(w16["q_tap"][f]), _bits(w32["q_tap"][f]))]
    print("d=%d %s: Q of fp16 and fp32 messages differs in %d of %d frames" % (d, kind, len(differ), run_q.size))
    assert len(differ) == run_q.size


@pytest.mark.parametrize("d", fc.DEGREES)
def test_r_kept_unrounded_in_registers_shows_in_the_q_tap_only(d):
    """Why the GPU tests must compare Q.  The corrected fp16 kernels round the corrected magnitude to binary16 where R is
    produced, because the column-fused kernels keep the staircase columns' R in registers and never store it.  The model
    of a kernel that forgot this (flood_ms: raw_cols -- those columns see R before its rounding, every stored R is still
    rounded by its store) leaves every iteration count as it is, changes the hard bits of a handful of frames at most,
    and changes the Q tap in every frame that is compared."""
    c = fc.staircase(d, "ride")
    assert fc.fused_columns(c).sum() == fc.LINKED_ROWS - 1
    for setting in fc.SETTINGS:
        good, bad = fc.want(d, "ride", setting), fc.want_registers_unrounded(d, setting)
        run_q = fc.tap_frames(good["iters"])[1]
        q_frames = [f for f in run_q if not fc.same_floats(bad["q_tap"][f], good["q_tap"][f])]
        q_values = int((_bits(bad["q_tap"][run_q]) != _bits(good["q_tap"][run_q])).sum())
        hard_frames = int((good["hard"] != bad["hard"]).any(axis=1).sum())
        print("d=%d %s: iterations equal, hard bits differ in %d of %d frames, Q tap in %d of %d frames (%d values)"
              % (d, setting, hard_frames, fc.FRAMES, len(q_frames), run_q.size, q_values))
        assert np.array_equal(good["iters"], bad["iters"]), (d, setting)
        assert len(q_frames) == run_q.size >= 60, (d, setting)
        assert hard_frames <= 5, (d, setting)


@pytest.mark.parametrize("d,kind", fc.CASES, ids=IDS)
def test_linked_class_is_the_degree_d_rows(d, kind):
    """build_classes may fuse the degree-d class (at least 300 linkable rows) and no other; "ride" leaves at most 64
    unlinked rows (they run in the column-fused launch), "own" more."""
    c = fc.staircase(d, kind)
    link = km.linkable_rows(c["rows"], c["cols"], c["M"], c["N"])
    print("d=%d %s: N=%d K=%d, linkable rows %s" % (d, kind, c["N"], c["K"], {k: v for k, v in link.items() if v}))
    assert link[d] >= 300 and not any(v for k, v in link.items() if k != d)
    assert 2 <= d <= 16 and c["K"] % 8 == 0 and c["N"] <= 2313
    unlinked = c["M"] - fc.LINKED_ROWS
    assert (unlinked <= 64) == (kind == "ride") and unlinked > 0


@pytest.mark.parametrize("B", fc.HANDOVER_BATCHES)
def test_hand_over_batch_has_90_stragglers(B):
    """Exactly 90 frames run all 30 rounds and every other frame stops before round 12, for fp16 and fp32 messages and
    for the corrected run of the polled test: once the easy frames are done a hand-over moves two child tiles' worth."""
    for setting, f16 in ((None, True), (None, False)) + (((fc.SETTINGS[0], True),) if B == fc.HANDOVER_BATCHES[0] else ()):
        w = fc.handover_want(B, setting, f16)
        it = w["iters"]
        full, early = int((it == fc.HANDOVER_MAXIT).sum()), int((it < 12).sum())
        print("B=%d %s f16=%s: %d frames run %d rounds, %d stop before round 12, %d converge"
              % (B, setting, f16, full, fc.HANDOVER_MAXIT, early, w["n_conv"]))
        assert it.size == B and full == fc.HANDOVER_STRAGGLERS and early == B - fc.HANDOVER_STRAGGLERS
        assert w["n_conv"] >= early


def test_oracle_f16_round_is_numpy_float16():
    """What the kernels' (_Float16) stores must produce is well defined: the oracle's f16_round equals numpy's
    astype(float16), as bits, on the overlay's values and on 200 000 seeded values of magnitude 2^-30 ... 2^17 (binary16
    subnormals, the ties of both grids, overflow to infinity), and the overlay's values round as its docstring says."""
    rng = np.random.default_rng(16)
    x = (np.exp2(rng.uniform(-30, 17, 200000)) * rng.choice([-1.0, 1.0], 200000)).astype(np.float32)
    # exact ties of the subnormal grid (odd multiples of 2^-25) and of the normal grid (11th mantissa bit alone)
    ties = np.concatenate([(2 * np.arange(0, 600) + 1) * 2.0 ** -25, (1 + (2 * np.arange(0, 600) + 1) * 2.0 ** -11) * 2.0 ** -3])
    special = np.array(list(fc.OVERLAY_VALUES.values()) + [0.0, -0.0, np.inf, -np.inf, 65504.0, -65520.0, 2.0 ** -24, 2.0 ** -14],
                       np.float32)
    vals = np.concatenate([x, ties.astype(np.float32), -ties.astype(np.float32), special])
    with np.errstate(over="ignore"):
        ref = vals.astype(np.float16).astype(np.float32)
    got = fc.f16_round(vals)
    assert np.array_equal(_bits(got), _bits(ref))
    assert np.isnan(fc.f16_round(np.array([np.nan], np.float32))).all()
    sub = int(((np.abs(ref) < 2.0 ** -14) & (ref != 0)).sum())
    print("f16_round == astype(float16) on %d values: %d binary16 subnormals, %d zeros, %d infinities"
          % (vals.size, sub, int((ref == 0).sum()), int(np.isinf(ref).sum())))
    assert sub > 1000 and np.isinf(ref).sum() > 1000
    v = {k: fc.f16_round(np.array([val], np.float32))[0] for k, val in fc.OVERLAY_VALUES.items()}
    assert v["just_finite"] == 65504.0 and v["to_inf"] == np.inf and v["far_out"] == -np.inf
    assert 0 < v["erasure_llr"] < 2.0 ** -14 and v["erasure_llr"] == 17 * 2.0 ** -24
    assert v["tie_to_zero"] == 0.0 and not np.signbit(v["tie_to_zero"]) and v["tie_to_even"] == 2.0 ** -23
    assert v["to_minus_zero"] == 0.0 and np.signbit(v["to_minus_zero"])
    assert v["tie_11th_bit"] == 1.0 and v["near_max"] == 64512.0 and v["fp32_denormal"] == 0.0


@pytest.mark.parametrize("name", ["wimax", "ira"])
def test_degenerate_frames_reach_the_edges(name):
    """The overlay's frames as the oracle sees them: the stored channel values hold infinities of both signs, NaN, binary16
    subnormals and -0; the NaN frame and the frames with infinities are still running at the tap, so their messages are
    compared; and Q holds infinities that the channel values of its frame do not (Q = y + sum of R left binary16's range)."""
    y = fc.degenerate_inputs(name)
    ch = fc.f16_round(y)
    assert np.isnan(ch[7]).sum() == 5 and np.isposinf(ch[3]).sum() == 40 and np.isneginf(ch[4]).sum() == 40
    assert not np.isinf(ch[2]).any() and (ch[2] == 65504.0).sum() == 40
    assert ((ch[8] != 0) & (np.abs(ch[8]) < 2.0 ** -14)).sum() >= y.shape[1] // 4
    assert (np.signbit(ch[11]) & (ch[11] == 0)).sum() == y.shape[1] // 4
    for corrected in (False, True):
        w = fc.degenerate_want(name, corrected)
        run_q = fc.tap_frames(w["iters"])[1]
        q = w["q_tap"]
        overflow = [f for f in run_q if np.isinf(q[f]).any() and not np.isinf(ch[f]).any()]
        print("%s corrected=%s: iterations %s; Q compared on %d frames, NaN in frames %s, Q overflows in frames %s"
              % (name, corrected, w["iters"].tolist(), run_q.size, [f for f in run_q if np.isnan(q[f]).any()], overflow))
        assert {3, 4, 5, 6, 7, 18} <= set(run_q.tolist())
        assert np.isnan(q[7]).any() and np.isinf(q[3]).any()
        assert 18 in overflow, "no frame's Q leaves binary16's range"
