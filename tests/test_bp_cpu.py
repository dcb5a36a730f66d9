"""CPU side of the log-domain sum-product (algo = bp): the numpy restatement (tests/bp_ref.py) against the references that
exist for min-sum -- with the correction c == 0 the definition IS flooding min-sum --, box-plus itself, the premise of the
feature (it decodes what min-sum does not), the premises of the GPU cases (tests/test_gpu_bp.py), and the bindings.  Only
the bindings test touches the library under test.  Every test prints the counts it found (pytest -s shows them)."""
import numpy as np
import pytest

import oracle
import myldpccppapi_amd as L
from myldpccppapi_amd import codes

import bp_cases as bc
import bp_ref as RB
import fp16_cases as fc
import kernel_matrix as km
import soft_ref as SR
from ms_correction_ref import Code, _check_ms, flood_ms

f32 = np.float32
LDPC_ERR_ARG, LDPC_ERR_HIP, LDPC_ERR_UNSUPPORTED = 1, 2, 4


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the anchor: c == 0 is the oracle's min-sum ---------------------------------------------------------------------

def _anchor_codes():
    c = fc.wimax()
    yield "wimax", c["og"], c["code"], fc.noisy_frames(c["N"], 96, 0.55, 0.95, seed=31), 25
    m = bc.matrix()
    yield "matrix", oracle.Graph(m["rows"], m["cols"], m["M"], m["N"], m["K"]), m["code"], m["y"], bc.MATRIX_MAXIT


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_zero_correction_is_the_oracles_min_sum(storage):
    """c == 0, llr_scale = 1: bytes, iteration counts, hard bits, the R and Q taps and the stop-round posteriors of
    oracle.decode(..., "ms") -- fp32 with the identity rounding, the fp16 oracle with binary16 rounding -- as bits.  On
    WiMAX (960, 480) and on the matrix code, whose rows have every degree 0 ... 33 and 40: the short rows (0, 1, 2) and the
    association of the long ones are covered."""
    f16 = storage == "f16"
    for name, og, code, y, maxit in _anchor_codes():
        got = RB.flood(code, y, maxit, c=RB.zero, rnd=bc.RND[storage], llr_scale=1.0, tap_iter=fc.TAP)
        want = fc.as_ref(oracle.decode(og, y, "ms", max_iter=maxit, tap_iter=fc.TAP, msg_f16=f16))
        it = want["iters"]
        never = int((it == maxit).sum()) - int(code.syndrome_ok(want["hard"][it == maxit]).sum())
        print("%s %s: %d distinct iteration counts, %d frames never converge" % (name, storage, np.unique(it).size, never))
        assert np.unique(it).size >= 8 and never >= 3, name
        for key in ("out", "iters", "hard"):
            assert np.array_equal(got[key], want[key]), (name, key)
        run_r, run_q = fc.tap_frames(it)
        assert run_q.size >= 10
        # The one place where the chain is not min-sum: a row that reads an exact zero.  Min-sum's sign is the parity of all
        # other inputs; the chain's passes through (u < 0), which a -0 on the way fails, so the ZERO it returns can have the
        # other sign (test_a_zero_message_carries_no_sign pins that).  Nothing but the sign of zeros follows from it.  The R
        # tap of round 2 is a function of Q after round 1: frames with an exact zero there -- binary16 cancels to zero now
        # and then -- are told from the oracle alone and compare their R tap by value instead of by bits.
        q1 = oracle.decode(og, y, "ms", max_iter=maxit, tap_iter=fc.TAP - 1, msg_f16=f16)["taps"]["q"]
        zero_q = (q1 == 0).any(axis=1)
        print("    frames with an exact zero in Q after round %d: %d of %d compared" % (fc.TAP - 1, int(zero_q[run_r].sum()), run_r.size))
        assert zero_q[run_r].sum() <= run_r.size // 10
        assert np.array_equal(got["r_tap"][run_r[zero_q[run_r]]], want["r_tap"][run_r[zero_q[run_r]]])
        run_r = run_r[~zero_q[run_r]]
        assert fc.same_floats(got["r_tap"][run_r], want["r_tap"][run_r]), name
        assert fc.same_floats(got["q_tap"][run_q], want["q_tap"][run_q]), name
        SR.assert_same_bits(got["post"], SR.expected(og, y, "ms", maxit, f16=f16)["post"], None, name)
        # and the correction is not a no-op on these inputs
        assert not np.array_equal(RB.flood(code, y, maxit, rnd=bc.RND[storage], llr_scale=1.0)["iters"], it), name


# ---- box-plus itself ------------------------------------------------------------------------------------------------

def test_boxplus_properties():
    """2 * 10^5 random pairs, magnitudes log-uniform over 2^-20 ... 2^10 and both signs: bitwise commutative, never larger
    than the smaller input, never NaN; the clamps of a row's inputs; and within 0.2 of the exact
    2 atanh(tanh(u/2) tanh(v/2)) in float64 on pairs of magnitude <= 20."""
    rng = np.random.default_rng(5)
    n = 2 * 10 ** 5
    u = (np.exp2(rng.uniform(-20, 10, n)) * rng.choice([-1.0, 1.0], n)).astype(f32)
    v = (np.exp2(rng.uniform(-20, 10, n)) * rng.choice([-1.0, 1.0], n)).astype(f32)
    u[:1000] = v[:1000] * rng.choice([-1.0, 1.0], 1000).astype(f32)                 # equal magnitudes
    u, v = RB.clamp(u), RB.clamp(v)
    a, b = RB.boxplus(u, v), RB.boxplus(v, u)
    assert np.array_equal(_bits(a), _bits(b))
    assert not np.isnan(a).any() and (np.abs(a) <= np.minimum(np.abs(u), np.abs(v))).all()
    assert ((a < 0) == ((u < 0) != (v < 0)))[a != 0].all()
    x = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e30, -1e30, 999.5, -1000.0, 1e-41], f32)
    want = np.array([1000, 1000, -1000, 0.0, 0.0, 1000, -1000, 999.5, -1000, 1e-41], f32)
    assert np.array_equal(_bits(RB.clamp(x)), _bits(want))                          # -0 reads +0, NaN reads +1000
    assert RB.linear(f32(0)) == RB.LN2 and RB.linear(f32(4)) == 0 and RB.linear(f32(1)) == f32(f32(0.6931472) - f32(0.25))
    # against the exact rule
    u = rng.uniform(-20, 20, n).astype(f32)
    v = rng.uniform(-20, 20, n).astype(f32)
    exact = 2.0 * np.arctanh(np.tanh(u.astype(np.float64) / 2) * np.tanh(v.astype(np.float64) / 2))
    err = np.abs(RB.boxplus(u, v).astype(np.float64) - exact)
    print("largest distance from the exact box-plus on |.| <= 20: %.4f" % err.max())
    assert err.max() <= 0.2
    # c == 0: the minimum with the product of the signs
    z = RB.boxplus(u, v, RB.zero)
    assert np.array_equal(np.abs(z), np.minimum(np.abs(u), np.abs(v))) and np.array_equal(z < 0, (u < 0) != (v < 0))


def test_a_zero_message_carries_no_sign():
    """The row (+, +, 0, -): min-sum gives message 0 the sign of the parity of the others, -0; the chain of the definition
    gives +0, with any correction, because (-0 < 0) is false.  Every non-zero message has min-sum's sign.  This is the one
    difference between c == 0 and the oracle's min-sum, and it is confined to the sign of zeros: x + (-0) = x + 0 for every
    x but -0."""
    code = Code(np.zeros(4, np.int64), np.arange(4), 1, 4, 1)
    Q = np.array([[2.0, 1.0, 0.0, -0.5]], f32)
    r_ms = _check_ms(code, Q, 0.0, 0.0, False)
    assert np.array_equal(_bits(r_ms), _bits(np.array([[-0.0, -0.0, -0.5, 0.0]], f32)))
    for c in (RB.zero, RB.linear):
        r = RB.check(code, Q, c)
        assert np.array_equal(_bits(r), _bits(np.array([[0.0, 0.0, r[0, 2], 0.0]], f32))) and r[0, 2] < 0, (c, r)
    assert np.array_equal(RB.check(code, Q, RB.zero), r_ms)                 # equal as values


def test_boxplus_is_not_associative_and_the_row_follows_the_definition():
    """A row of degree 5, written out by hand from the definition, equals bp_ref.check; and re-associating it changes bits
    on most random rows -- so the association is something a kernel can get wrong."""
    rng = np.random.default_rng(6)
    code = Code(np.zeros(5, np.int64), np.arange(5), 1, 5, 1)
    Q = rng.uniform(-6, 6, (4000, 5)).astype(f32)
    t = [RB.clamp(Q[:, j]) for j in range(5)]
    bp = RB.boxplus
    f1, f2, f3 = bp(t[0], t[1]), bp(bp(t[0], t[1]), t[2]), bp(bp(bp(t[0], t[1]), t[2]), t[3])
    b3, b2, b1 = bp(t[3], t[4]), bp(t[2], bp(t[3], t[4])), bp(t[1], bp(t[2], bp(t[3], t[4])))
    want = np.stack([b1, bp(t[0], b2), bp(f1, b3), bp(f2, t[4]), f3], axis=1)
    assert np.array_equal(_bits(RB.check(code, Q)), _bits(want))
    other = bp(bp(t[1], t[2]), bp(t[3], t[4]))                                       # out_0, associated as a tree
    differ = int((_bits(other) != _bits(b1)).sum())
    print("out_0 of a degree-5 row: a tree association differs in %d of 4000 rows" % differ)
    assert differ >= 400


# ---- the premise of the feature -------------------------------------------------------------------------------------

def test_bp_decodes_what_min_sum_does_not():
    """WiMAX (2304, 1152), 1.6 dB, 512 frames, 20 rounds, llr_scale = 2 / sd^2: BP leaves fewer frame errors than offset
    min-sum with beta = 0.15, and fewer than a quarter of plain min-sum's."""
    rate, N = codes.RATE_1_2, 2304
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    code = Code(rows, cols, M, N, K)
    y, sd = bc.wimax_frames(N, 512, 1.6, seed=16)
    errors, rounds = {}, {}
    for name, r in (("min-sum", flood_ms(code, y, 20)), ("offset 0.15", flood_ms(code, y, 20, 0.0, 0.15)),
                    ("bp", RB.flood(code, y, 20, llr_scale=2.0 / (sd * sd)))):
        errors[name], rounds[name] = int(r["hard"].any(axis=1).sum()), float(r["iters"].mean())
        print("%-12s frame errors %3d of 512, mean rounds %.2f" % (name, errors[name], rounds[name]))
    assert errors["bp"] < errors["offset 0.15"]
    assert 4 * errors["bp"] < errors["min-sum"]


# ---- premises of the GPU cases --------------------------------------------------------------------------------------

def test_premises_of_the_matrix_case():
    """The 70 frames of the matrix code under BP: several distinct stop rounds, frames that never stop, frames that
    compare their Q tap; iteration counts that differ from min-sum's on the same input (a kernel that silently ran min-sum
    would fail) and between the two storages; two llr_scale values give different bytes and different channel taps."""
    m = bc.matrix()
    for storage in ("f32", "f16"):
        w = bc.matrix_want(storage)
        it = w["iters"]
        never = int((it == bc.MATRIX_MAXIT).sum()) - int(m["code"].syndrome_ok(w["hard"][it == bc.MATRIX_MAXIT]).sum())
        ms = RB.flood(m["code"], m["y"], bc.MATRIX_MAXIT, c=RB.zero, rnd=bc.RND[storage], llr_scale=bc.SCALE)
        differ = int((ms["iters"] != it).sum())
        run_r, run_q = fc.tap_frames(it)
        print("%s: %d distinct rounds, %d frames never stop, iterations differ from min-sum in %d of %d frames, %d compare Q"
              % (storage, np.unique(it).size, never, differ, it.size, run_q.size))
        assert np.unique(it).size >= 4 and never >= 1 and differ >= 5 and run_q.size >= 5, storage
        other = bc.matrix_want(storage, bc.SCALES[1])
        assert not np.array_equal(other["out"], w["out"]) and not np.array_equal(_bits(other["chan"]), _bits(w["chan"])), storage
    assert not np.array_equal(bc.matrix_want("f32")["iters"], bc.matrix_want("f16")["iters"]) or \
        not fc.same_floats(bc.matrix_want("f32")["r_tap"], bc.matrix_want("f16")["r_tap"])
    assert sorted(set(km.MATRIX_ROW_DEGS)) == list(range(34)) + [40]


@pytest.mark.parametrize("d", fc.DEGREES)
def test_premises_of_the_staircase_cases(d):
    """On staircase(d), 133 frames, 25 rounds: frames stop at several distinct rounds and some never do for d = 7 and 16;
    iteration counts differ from min-sum's; and the model of an fp16 kernel whose fused columns see unrounded R differs
    from the right answer in the Q tap of at least one compared frame -- R of a box-plus is in general no binary16 value."""
    c = fc.staircase(d, "ride")
    for storage in ("f32", "f16"):
        w = bc.want(d, "ride", storage)
        it = w["iters"]
        never = int((it == fc.MAXIT).sum()) - int(c["code"].syndrome_ok(w["hard"][it == fc.MAXIT]).sum())
        differ = int((it != fc.want(d, "ride", None, f16=storage == "f16")["iters"]).sum())
        run_r, run_q = fc.tap_frames(it)
        print("d=%d %s: %d distinct rounds, %d frames never stop, iterations differ from min-sum (on y) in %d frames, %d compare Q"
              % (d, storage, np.unique(it).size, never, differ, run_q.size))
        assert np.unique(it).size >= 3 and differ >= 1 and run_q.size >= 1, (d, storage)
        if d in (7, 16):
            assert never >= 1, (d, storage)
    w, bad = bc.want(d, "ride", "f16"), bc.want_registers_unrounded(d)
    run_r, run_q = fc.tap_frames(w["iters"])
    q_frames = [f for f in run_q if not fc.same_floats(bad["q_tap"][f], w["q_tap"][f])]
    print("    R unrounded in registers: Q tap differs in %d of %d compared frames" % (len(q_frames), run_q.size))
    assert len(q_frames) >= 1, d


def test_premises_of_degenerate_and_handover_cases():
    """The degenerate frames keep NaN, infinities and -0 in what is stored and compared; the hand-over batch has
    stragglers that run all rounds and many frames that stop early."""
    for name in ("wimax", "ira"):
        y = fc.degenerate_inputs(name)
        for storage in ("f32", "f16"):
            w = bc.degenerate_want(name, storage)
            ch = w["chan"]
            assert np.isnan(ch).sum() == 5 and np.isinf(ch).sum() >= 40 and (_bits(ch) == 0x80000000).sum() >= (1 if storage == "f16" else 0)
            run_r, run_q = fc.tap_frames(w["iters"])
            beyond = int((np.abs(w["q_tap"][run_q]) > 1000).sum())          # NaN compares false
            print(name, storage, "frames comparing Q:", run_q.size, "Q beyond the clamp:", beyond)
            assert run_q.size >= 5 and beyond >= 1
    for B in fc.HANDOVER_BATCHES:
        w = bc.handover_want(B)
        full = int((w["iters"] == fc.HANDOVER_MAXIT).sum())
        print("hand-over %d: %d frames run all rounds, %d distinct rounds" % (B, full, np.unique(w["iters"]).size))
        assert 20 <= full <= fc.HANDOVER_STRAGGLERS + 10
        assert SR.sign_disagreements(w["post"], w["hard"]) == 0


def test_premise_of_the_crc_case():
    """At least four of the 150 frames are stopped by the CRC in a round in which their syndrome is not clean."""
    kind, bits, y, w = bc.crc_case()
    print("frames stopped by the CRC alone: %d of %d, %d distinct rounds" % (w["by_stop"].size, y.shape[0], np.unique(w["iters"]).size))
    assert w["by_stop"].size >= 4


# ---- bindings -------------------------------------------------------------------------------------------------------

def test_bindings_know_bp_and_refuse_before_the_device(built):
    """algo="bp" reaches the library as LDPC_ALGO_BP = 5: without a device its creation fails with LDPC_ERR_HIP (there is no
    CPU path), with one it succeeds.  The three refusals (one-launch / record kernels forced on, fp8 messages, a min-sum
    correction) are LDPC_ERR_UNSUPPORTED and a bad llr_scale is LDPC_ERR_ARG, all before the device is touched -- so on any
    machine.  algo = 7 stays unknown."""
    assert L.capi.ALGOS["bp"] == L.capi.ALGO_BP == 5
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 648)
    g = L.Graph(rows, cols, 324, 648)
    K = 324

    def refused(code, **kw):
        with pytest.raises(L.LdpcError) as e:
            L.Decoder(g, K, 4, algo="bp", **kw)
        assert e.value.code == code, (kw, str(e.value))

    for tune in ({"fused": True}, {"ldsp": True}):
        refused(LDPC_ERR_UNSUPPORTED, layer_rows=27, tune=tune)
    refused(LDPC_ERR_UNSUPPORTED, msg_dtype="f8")
    refused(LDPC_ERR_UNSUPPORTED, ms_scale=0.75)
    refused(LDPC_ERR_UNSUPPORTED, ms_offset=0.15)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(LDPC_ERR_ARG, llr_scale=bad)
    with pytest.raises(L.LdpcError) as e:
        L.Decoder(g, K, 4, algo=7)
    assert e.value.code == LDPC_ERR_ARG
    for kw in ({}, {"msg_dtype": "f16"}, {"layer_rows": 27}):
        if L.device_count() > 0:
            L.Decoder(g, K, 4, algo="bp", **kw).close()
        else:
            refused(LDPC_ERR_HIP, **kw)
