"""CPU side of the layered log-domain sum-product (algo = layered_bp): the numpy restatement (tests/layered_bp_ref.py)
against layered min-sum -- with the correction c == 0 the row is min with the sign parity --, the premise of the feature,
exact zeros at punctured columns, the premises of the GPU cases (tests/test_gpu_layered_bp.py), and the bindings.  Only the
bindings test touches the library under test.  Every test prints the counts it found (pytest -s shows them)."""
import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import codes

import bp_cases as bc
import bp_ref as RB
import fp16_cases as fc
import layered_bp_cases as lc
import layered_bp_ref as LB
import ratematch_util as U
import soft_ref as SR
from ms_correction_ref import Code, layered_ms

f32 = np.float32
LDPC_ERR_ARG, LDPC_ERR_HIP, LDPC_ERR_UNSUPPORTED = 1, 2, 4


# ---- the anchor: c == 0 is layered min-sum ---------------------------------------------------------------------------

def test_zero_correction_is_layered_min_sum():
    """c == 0, llr_scale = 1 against ms_correction_ref.layered_ms on WiMAX (960, 480), 96 frames, 25 rounds, and on WiMAX
    (1152, 960) of rate 5/6 (rows of degree 20), 64 frames: bytes, iteration counts and hard bits are equal, R after round
    TAP is equal in value.

    Excluded inputs, and why.  layered_ms takes a row's sign from the running fp32 PRODUCT of its q, the chain from the
    parity of (q < 0).  The two differ where a q is an exact zero (the product is 0 and the row's messages are 0; the chain
    gives the others their minimum with a sign) or a NaN, and where the product of non-zero q underflows to 0.  A row in
    that state shows in layered_ms's own R: every message of the row is an exact zero (a regular row has at most the
    argmin's message at 0, and only if the second minimum is 0 too).  Frames with such a row in the R tap of round 1, 2 or
    3 -- told from layered_ms alone -- are excluded; the share is capped at 5 %.  The inputs are chosen so that the cap
    holds: no zero and no NaN in y, |y| around 1 and row degrees up to 20, so a product stays far above 1e-38; and the
    WiMAX codes, not the BG1-profile test code -- there min-sum's messages, which are copies of other messages' magnitudes,
    meet an exact zero q in a third of such frames (23 of 70 by the criterion above; zeros are the erasure test's subject).
    Magnitudes stay far below the start values 1000 / 1001, where the two rules' clamps differ."""
    w = fc.wimax()
    K5, M5, z5 = codes.wimax_dims(codes.RATE_5_6, 1152)
    r5, c5 = codes.wimax_edges(codes.RATE_5_6, 1152)
    cases = (("wimax 1/2", w["code"], w["z"], fc.noisy_frames(w["N"], 96, 0.55, 0.95, seed=31), 25),
             ("wimax 5/6", Code(r5, c5, M5, 1152, K5), z5, fc.noisy_frames(1152, 64, 0.3, 0.55, seed=32), 15))
    for name, code, z, y, maxit in cases:
        assert not (y == 0).any() and not np.isnan(y).any()
        got = LB.layered_bp(code, y, z, maxit, c=RB.zero, llr_scale=1.0, tap_iter=lc.TAP)
        want = layered_ms(code, y, z, maxit, tap_iter=lc.TAP)
        dead = np.zeros(y.shape[0], bool)
        for t in (1, 2, 3):
            r = layered_ms(code, y, z, maxit, tap_iter=t)["r_tap"]
            ran = ~np.isnan(r).all(axis=1)
            rz = np.concatenate([r == 0, np.ones((r.shape[0], 1), bool)], axis=1)[:, code.row_edges]       # [F, M, dmax]
            dead |= ran & (rz.all(axis=2) & (np.diff(code.row_ptr) >= 2)[None, :]).any(axis=1)
        keep = ~dead
        it = want["iters"]
        print("%s: %d of %d frames excluded, %d distinct iteration counts, largest |R| %.1f"
              % (name, int(dead.sum()), dead.size, np.unique(it).size, float(np.nanmax(np.abs(want["r_tap"])))))
        assert dead.sum() <= dead.size // 20, name
        assert np.unique(it).size >= 4, name
        assert np.array_equal(got["iters"][keep], it[keep]), name
        assert np.array_equal(got["hard"][keep], want["hard"][keep]), name
        if not dead.any():
            assert np.array_equal(got["out"], want["out"]), name
        run = np.nonzero(keep & (it >= lc.TAP))[0]
        assert run.size >= 10
        assert np.array_equal(got["r_tap"][run], want["r_tap"][run]), name                 # equal in value: -0 == +0
        # and the correction is not a no-op on these inputs
        assert not np.array_equal(LB.layered_bp(code, y, z, maxit, llr_scale=1.0)["iters"], it), name


def test_layered_row_update_written_out():
    """One row of degree 4 in a code of one layer, by hand from the definition: q = P - R, the BP row of q, R = out,
    P = q + R -- twice, so that the second round reads the first one's R."""
    code = Code(np.zeros(4, np.int64), np.arange(4), 1, 4, 1)
    y = np.array([[0.5, -1.25, 2.0, 0.75], [1.0, 0.0, -0.0, 3.0]], f32)
    w = LB.layered_bp(code, y, 1, 2, llr_scale=1.7, tap_iter=2, early_term=False)
    P = (f32(1.7) * y).astype(f32)
    R = np.zeros_like(P)
    for _ in range(2):
        q = (P - R).astype(f32)
        R = RB.check(code, q)
        P = (q + R).astype(f32)
    assert fc.same_floats(w["r_tap"], R) and fc.same_floats(w["p_tap"], P) and fc.same_floats(w["post"], P)
    assert np.array_equal(w["hard"], (P < 0).astype(np.uint8)) and (w["iters"] == 2).all()


# ---- the premise of the feature --------------------------------------------------------------------------------------

def test_layered_bp_is_the_strongest_of_the_three():
    """WiMAX (2304, 1152), z = 96, all-zero codeword, 1.6 dB, 256 frames, llr_scale = 2 / sd^2, max_iter = 10: layered BP
    leaves no more frame errors than flooding BP and no more than layered min-sum at the same max_iter."""
    rate, N = codes.RATE_1_2, 2304
    K, M, z = codes.wimax_dims(rate, N)
    assert z == 96
    rows, cols = codes.wimax_edges(rate, N)
    code = Code(rows, cols, M, N, K)
    y, sd = bc.wimax_frames(N, 256, 1.6, seed=16)
    scale = 2.0 / (sd * sd)
    errors, rounds = {}, {}
    for name, r in (("layered bp", LB.layered_bp(code, y, z, 10, llr_scale=scale)),
                    ("flooding bp", RB.flood(code, y, 10, llr_scale=scale)),
                    ("layered min-sum", layered_ms(code, y, z, 10))):
        errors[name], rounds[name] = int(r["hard"].any(axis=1).sum()), float(r["iters"].mean())
        print("%-16s frame errors %3d of 256, mean rounds %.2f" % (name, errors[name], rounds[name]))
    assert errors["layered bp"] <= errors["flooding bp"]
    assert errors["layered bp"] <= errors["layered min-sum"]


# ---- erasures --------------------------------------------------------------------------------------------------------

def test_exact_zeros_at_punctured_columns():
    """Scenario S1 of ratematch_util (BG1-profile, the first 32 code bits punctured) with erasure_llr = 0: the oracle's
    layered min-sum gets no frame right -- the documented finding.  The layered BP reference, on the same input with its
    exact zeros, gets at least as many frames right as layered min-sum does with erasure_llr = 1e-6."""
    _, _, wrong0 = U.oracle_decode(lc.ERASURE_SCENARIO, 0.0, 1, "layered")
    assert wrong0 == U.FRAMES
    y = U.recovered(lc.ERASURE_SCENARIO, 0.0, 1)
    assert (y[:, :U.P] == 0).all()
    _, _, wrong_ms = U.oracle_decode(lc.ERASURE_SCENARIO, 1e-6, 1, "layered")
    w = lc.erasure_want()
    right_bp, right_ms = lc.frames_right(w["out"]), U.FRAMES - wrong_ms
    print("frames right of %d: layered bp with exact zeros %d (mean rounds %.2f), layered min-sum with 1e-6 %d, with 0: %d"
          % (U.FRAMES, right_bp, float(w["iters"].mean()), right_ms, U.FRAMES - wrong0))
    assert right_bp >= right_ms


# ---- premises of the GPU cases ---------------------------------------------------------------------------------------

def test_premises_of_the_bg1_cases():
    """Frames stop in several distinct rounds, some in round 1 and some never (under both scales); enough frames reach the tap; iteration
    counts differ from layered min-sum's with c == 0 (a kernel that ran min-sum would fail); the two scales give different
    channel values and bytes; without early termination every frame runs max_iter rounds."""
    c = lc.bg1_code()
    for frames in (70, lc.BG1_TWO_TILES):
        w = lc.bg1_want(frames)
        it = w["iters"]
        never = int((~c["code"].syndrome_ok(w["hard"])).sum())
        ms = LB.layered_bp(c["code"], lc.bg1_inputs(frames), c["z"], lc.BG1_MAXIT, c=RB.zero, llr_scale=lc.SCALES[0])
        differ = int((ms["iters"] != it).sum())
        print("%d frames: rounds %s, %d never stop, %d reach the tap, iterations differ from c == 0 in %d"
              % (frames, np.unique(it).tolist(), never, int((it >= lc.TAP).sum()), differ))
        assert np.unique(it).size >= 4 and never >= 1 and (it >= lc.TAP).sum() >= 10 and differ >= 3
        assert SR.sign_disagreements(w["post"], w["hard"]) == 0
    w, other = lc.bg1_want(70), lc.bg1_want(70, lc.SCALES[1])
    assert not np.array_equal(other["out"], w["out"]) and not fc.same_floats(other["chan"], w["chan"])
    full = lc.bg1_want(70, lc.SCALES[0], 0, False)
    assert (full["iters"] == lc.BG1_MAXIT).all()
    for x in (w, other):
        assert (x["iters"] == 1).any() and (~c["code"].syndrome_ok(x["hard"])).any()


def test_premises_of_matrix_degenerate_and_crc_cases():
    """The matrix code with every row a layer: frames reach the tap and differ in their stop round.  The degenerate frames
    keep NaN and infinities in the posterior tap.  At least one frame of the CRC case is stopped by the CRC alone."""
    w = lc.matrix_want()
    print("matrix: rounds %s" % np.unique(w["iters"]).tolist())
    assert (w["iters"] >= lc.TAP).sum() >= 10 and np.unique(w["iters"]).size >= 2
    assert not np.array_equal(lc.matrix_want(lc.SCALES[1])["out"], w["out"])
    for name in ("wimax", "ira"):
        d = lc.degenerate_want(name)
        run = d["iters"] >= lc.TAP
        print(name, "frames at the tap:", int(run.sum()), "NaN in P:", int(np.isnan(d["p_tap"][run]).sum()),
              "|R| at the clamp:", int((np.abs(d["r_tap"][run]) == 1000).sum()))
        assert run.sum() >= 5 and np.isnan(d["chan"]).sum() == 5 and np.isinf(d["chan"]).sum() >= 40
    kind, bits, y, wc = lc.crc_case()
    print("frames stopped by the CRC alone: %d of %d" % (wc["by_stop"].size, y.shape[0]))
    assert wc["by_stop"].size >= 1


# ---- bindings --------------------------------------------------------------------------------------------------------

def test_bindings_know_layered_bp_and_refuse_before_the_device(built):
    """algo="layered_bp" reaches the library as LDPC_ALGO_LAYERED_BP = 6: without a device its creation fails with
    LDPC_ERR_HIP (there is no CPU path), with one it succeeds.  The refusals -- no layer_rows, fp16 / fp8 messages, a min-sum
    correction, the one-launch / record kernels forced on, a bad llr_scale -- give their codes before the device is
    touched, so on any machine.  algo = 7 stays unknown."""
    assert L.capi.ALGOS["layered_bp"] == L.capi.ALGO_LAYERED_BP == 6
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 648)
    g = L.Graph(rows, cols, 324, 648)
    K = 324

    def refused(code, **kw):
        kw.setdefault("layer_rows", 27)
        with pytest.raises(L.LdpcError) as e:
            L.Decoder(g, K, 4, algo="layered_bp", **kw)
        assert e.value.code == code, (kw, str(e.value))

    refused(LDPC_ERR_ARG, layer_rows=0)
    refused(LDPC_ERR_ARG, layer_rows=25)                    # does not divide M
    for tune in ({"fused": True}, {"ldsp": True}):
        refused(LDPC_ERR_UNSUPPORTED, tune=tune)
    refused(LDPC_ERR_UNSUPPORTED, msg_dtype="f16")
    refused(LDPC_ERR_UNSUPPORTED, msg_dtype="f8")
    refused(LDPC_ERR_UNSUPPORTED, ms_scale=0.75)
    refused(LDPC_ERR_UNSUPPORTED, ms_offset=0.15)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(LDPC_ERR_ARG, llr_scale=bad)
    with pytest.raises(L.LdpcError) as e:
        L.Decoder(g, K, 4, algo=7, layer_rows=27)
    assert e.value.code == LDPC_ERR_ARG
    if L.device_count() > 0:
        L.Decoder(g, K, 4, algo="layered_bp", layer_rows=27).close()
    else:
        refused(LDPC_ERR_HIP)
