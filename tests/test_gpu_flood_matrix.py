"""Every degree class of the streaming flooding kernels on every message type that has kernels of its own.

tests/test_gpu_kernel_matrix.py and tests/test_gpu_bp.py run the unrolled bodies, bucket launches and generic kernels of sp,
ms, ms16, bp and bp16 on the irregular matrix code (rows of every degree 0 ... 33 and 40, columns of every degree 0 ... 17
and 20).  Corrected min-sum (msc, msc16), fp8 (ms8, msc8) and fixed point (msi4/5/6/8, msci4/5/6/8) are separately compiled
instantiations with loads, stores and start values of their own; this module runs them on the same code, at 1, 2 and 4 frames
per lane, against their CPU references (tests/flood_matrix_cases.py).  A second code without rows above degree 32 takes
every arithmetic through the first round that reads the channel array.  Nothing has a tolerance: bytes, iteration counts,
all N hard bits, R on the frames that reached the tap round and Q on those that went on are compared bit for bit or integer
for integer, and by kernel name the launches are the ones the plan is made of."""
import numpy as np
import pytest

import myldpccppapi_amd as L

import flood_matrix_cases as fm
import fp16_cases as fc
import kernel_matrix as km

pytestmark = pytest.mark.gpu


def _decoder(c, arith, B, V, **kw):
    return L.Decoder(L.Graph(c["rows"], c["cols"], c["M"], c["N"]), c["K"], max_batch=B, max_iter=fm.MAXIT, frames_per_lane=V,
                     **fm.decoder_args(arith), **kw)


def _names(dec):
    """the kernels of the last timed call ("other": transposes, syndrome and bookkeeping launches)"""
    return {k["name"] for k in dec.kernel_times() if k["name"] != "other"}


def _check_result(dec, c, want, y, rows, what, hard=True):
    """One decode of y, whose frame i is frame rows[i] of the reference: bytes, iteration counts and all N hard bits (the
    hard bits: of the last launch group).  Returns what the call returned."""
    B = y.shape[0]
    try:
        out, iters = dec.decode(y)
    except L.LdpcError as e:
        pytest.fail("%s: %s" % (what, e))
    assert np.array_equal(iters, want["iters"][rows]), ("iterations",) + what
    assert np.array_equal(fm.frame_bytes(out, c["K"], B), fm.frame_bytes(want["out"], c["K"], fm.FRAMES)[rows]), ("bytes",) + what
    if hard:
        assert np.array_equal(dec.dump(3, B).astype(np.uint8), want["hard"][rows]), ("hard bits",) + what
    return out, iters


def _check_taps(dec, arith, want, y, rows, what):
    """One decode that stops after round TAP: R on the frames that reached it, Q on those that went on"""
    B = y.shape[0]
    run_r, run_q = fc.tap_frames(want["iters"][rows])
    assert run_q.size > 0, what
    dec.set_tap(fc.TAP)
    dec.decode(y)
    assert fm.same_messages(arith, dec.dump(0, B)[run_r], want["r_tap"][rows][run_r]), ("R tap",) + what
    assert fm.same_messages(arith, dec.dump(1, B)[run_q], want["q_tap"][rows][run_q]), ("Q tap",) + what
    dec.set_tap(0)


@pytest.mark.parametrize("V", [1, 2, 4])
@pytest.mark.parametrize("arith", list(fm.ARITHS))
def test_every_degree_class(built, arith, V):
    """The matrix code, 2 * 64 * V + 5 frames (two full tiles and a ragged one), 20 rounds, every launch plan of
    kernel_matrix.FLOOD_PLANS.  With merging off the timed decode is one launch per class: check_kernel<a,d,V> for all 34 row
    degrees above 0 (33 and 40: the generic kernel) and var_kernel<a,d,V> for all 19 column degrees (0: the empty-column
    kernel; 17 and 20: the generic one).  The default plan is the bucket launches the arithmetic's table has kernels for
    plus the classes left alone (flood_matrix_cases.default_launches, from plan_launches and the table, not from the run).
    Then single-frame calls, two launch groups, and host polling with tail compaction through child decoders.
    (The rows of degree 1 launched alone are what this test first found: with a correction their check body issued a
    scalar load through a null CheckArgs::edge_col in every round that read Q -- check_args in csrc/engine_flood.hip.)"""
    c, want = fm.full(), fm.want("full", arith)
    y, rows = fm.frames("full", V)
    B = y.shape[0]
    rd, cd = km.degree_maps(c["rows"], c["cols"], c["M"], c["N"])
    # no linked class: the plans below are the bucket / solo launches alone
    assert not any(km.linkable_rows(c["rows"], c["cols"], c["M"], c["N"]).values())
    for plan, tune in km.FLOOD_PLANS.items():
        what = (arith, V, plan)
        dec = _decoder(c, arith, B, V, tune=tune)
        dec.set_timing(True)
        _check_result(dec, c, want, y, rows, what)
        names = _names(dec)
        dec.set_timing(False)
        assert not any(n.startswith("check_link") for n in names), (what, sorted(names))
        if plan == "merge_off":
            solo = fm.solo_launches(arith, rd, cd, V)
            assert names == solo, (what, sorted(names ^ solo))
        elif plan == "default":
            expect, lacking = fm.default_launches(arith, rd, cd, V)
            assert not lacking, (what, "the table has no", lacking)
            assert names == expect, (what, sorted(names ^ expect))
        _check_taps(dec, arith, want, y, rows, what)
        if plan == "default":
            for j in (0, B - 1):                                       # one call of a single frame
                _check_result(dec, c, want, y[j:j + 1], rows[j:j + 1], what + ("single", j))
        dec.close()
    # two launch groups: max_batch smaller than the batch
    dec = _decoder(c, arith, 64 * V + 3, V)
    _check_result(dec, c, want, y, rows, (arith, V, "two groups"), hard=False)
    dec.close()
    # host polling with tail compaction over 5 tiles
    y4, rows4 = fm.frames("full", V, tiles=4)
    dec = _decoder(c, arith, y4.shape[0], V, poll_interval=1)
    _check_result(dec, c, want, y4, rows4, (arith, V, "poll"))
    assert dec.stats()["iterations_launched"] == fm.MAXIT
    dec.close()


@pytest.mark.parametrize("V", [1, 2, 4])
@pytest.mark.parametrize("arith", list(fm.FIRST_ROUND_ARITHS))
def test_first_round_from_the_channel_array(built, arith, V):
    """Round 1 of a min-sum or box-plus decode reads q = y from the channel array by column, and the input transpose writes no
    Q, when (run_flooding in csrc/engine_flood.hip: q_less / CheckArgs::first_chan) the call has no debug tap, max_iter > 1,
    no row class is linked, no rows ride as extras of a linked class, and no class launched alone lies above the unrolled
    check bodies.  The matrix code has rows of degree 33 and 40 and the staircase codes a linked class, so this path ran on
    WiMAX rows of degree 6 and 7 only.  The trimmed code meets the graph-side conditions -- tests/test_flood_matrix_cpu.py
    asserts them; the library has no introspection for the path -- so here the per-degree channel gather runs at every row
    degree 1 ... 32: in the bucket launches (default) and in every unrolled body launched alone (merge_off), for the
    arithmetics of this module and for ms, ms16, bp and bp16 (against oracle.decode and bp_ref.flood, as their own tests).
    The untapped decodes take the Q-less round 1 (bytes, iteration counts, all hard bits); the tapped one takes the
    Q-writing round 1 on the same handle (R and Q); an untapped decode after it must repeat the first exactly."""
    c, want = fm.trimmed(), fm.want("trimmed", arith)
    y, rows = fm.frames("trimmed", V)
    B = y.shape[0]
    rd, cd = km.degree_maps(c["rows"], c["cols"], c["M"], c["N"])
    for plan in ("default", "merge_off"):
        what = (arith, V, plan)
        dec = _decoder(c, arith, B, V, tune=km.FLOOD_PLANS[plan])
        dec.set_timing(True)
        out, iters = _check_result(dec, c, want, y, rows, what + ("from the channel array",))
        hard = dec.dump(3, B)
        names = _names(dec)
        dec.set_timing(False)
        expect, lacking = (fm.solo_launches(arith, rd, cd, V), []) if plan == "merge_off" else fm.default_launches(arith, rd, cd, V)
        assert not lacking, (what, "the table has no", lacking)
        assert names == expect, (what, sorted(names ^ expect))
        _check_taps(dec, arith, want, y, rows, what + ("from Q",))
        out2, iters2 = _check_result(dec, c, want, y, rows, what + ("from the channel array again",))
        assert np.array_equal(out2, out) and np.array_equal(iters2, iters) and np.array_equal(dec.dump(3, B), hard), what
        dec.close()
