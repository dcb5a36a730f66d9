"""CPU side of tests/test_gpu_flood_matrix.py: from the references alone, every case of tests/flood_matrix_cases.py reaches
what it is there for.  Frames stop at many rounds and on both sides of the tap, fixed-point messages saturate, the rows of
degree 1 store the start value as the storage type reads it, every correction and every width changes the result, the
launch model names what csrc/flood_tables.hpp declares, and the trimmed code meets the graph-side conditions under which
round 1 reads the channel array.  These are conditions, not measurements.  Every test prints the counts it found
(pytest -s shows them)."""
import os
import re

import numpy as np
import pytest

import fixed_ref as RI
import flood_matrix_cases as fm
import fp16_cases as fc
import kernel_matrix as km

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "myldpccppapi_amd", "csrc")


def test_the_arithmetics_under_test():
    """Eleven arithmetics with a degree matrix of their own here -- msc runs its few degrees elsewhere, the other ten
    none -- each correction of fp16_cases.SETTINGS on a floating-point type, and the truncating (3 m) >> 2 at 4 and 8 bits."""
    assert set(fm.ARITHS) == {"msc", "msc16", "ms8", "msc8"} | {"%s%d" % (p, q) for p in ("msi", "msci") for q in RI.WIDTHS}
    floats = [s["setting"] for a, s in fm.ARITHS.items() if s["setting"] and not s["q"]]
    assert sorted(floats) == sorted(fc.SETTINGS)
    kinds = {(s["setting"][0] != 0, s["setting"][1] != 0) for a, s in fm.ARITHS.items() if s["setting"] and s["q"]}
    assert kinds == {(True, False), (False, True), (True, True)}
    assert fm.ARITHS["msci4"]["setting"] == fm.ARITHS["msci8"]["setting"] == (0.75, 0.0)
    for a, s in fm.ARITHS.items():
        assert (a in fm.CORRECTED) == (s["setting"] is not None) == ("c" in a[2:4]), a
        assert fm.decoder_args(a)["algo"] == "ms"


def test_the_two_codes():
    """full(): the matrix code.  trimmed(): the same degree maps without the rows of degree 33 and 40, and the graph-side
    conditions of the Q-less first round (run_flooding in csrc/engine_flood.hip): no row class is linked, so no row rides as
    an extra of a linked class either, and no class lies above the unrolled check bodies."""
    c = fm.full()
    rd, cd = km.degree_maps(c["rows"], c["cols"], c["M"], c["N"])
    assert (c["M"], c["N"], len(c["rows"])) == (138, 583, 2353) and rd == km.MATRIX_ROW_DEGS
    assert c["y"].shape == (fm.FRAMES, c["N"]) and c["K"] % 8 == 0
    t = fm.trimmed()
    rd, cd = km.degree_maps(t["rows"], t["cols"], t["M"], t["N"])
    print("trimmed: M = %d, N = %d, E = %d" % (t["M"], t["N"], len(t["rows"])))
    assert (t["M"], t["N"], len(t["rows"])) == (132, 510, 2134)
    assert rd == {d: n for d, n in km.MATRIX_ROW_DEGS.items() if d <= 32}
    assert set(cd) == set(km.MATRIX_COL_FIXED) | {3} and all(cd[d] >= n for d, n in km.MATRIX_COL_FIXED.items())
    key = np.asarray(t["rows"], np.int64) * t["N"] + np.asarray(t["cols"], np.int64)
    assert np.all(np.diff(key) > 0)
    assert t["y"].shape == (fm.FRAMES, t["N"]) and t["K"] % 8 == 0 and not t["y"].flags.writeable
    linkable = km.linkable_rows(t["rows"], t["cols"], t["M"], t["N"])
    assert not any(linkable.values()), linkable
    assert max(rd) <= fm.TABLE_MS["max_check_unrolled"] == 32
    linked_classes = sum(1 for n in linkable.values() if n)
    assert linked_classes == 0 or sum(n for d, n in rd.items() if d) > 64
    # both codes have rows above the degrees at which one-byte messages take wide waves on their own: the default plan
    # merges classes into bucket launches for every arithmetic alike (ldpc_hip.hip: check_wide; plan_launches: merge)
    assert max(rd) > fm.MAX_VAR_UNROLLED
    assert fm.degree_one_edges(c).size == km.MATRIX_ROW_DEGS[1] == fm.degree_one_edges(t).size


def test_the_frame_helper():
    """2 * 64 * V + 5 frames: two full tiles and a ragged one at every V, each frame one of the 70"""
    for V in (1, 2, 4):
        for tiles in (2, 4):
            y, rows = fm.frames("trimmed", V, tiles)
            assert y.shape[0] == rows.size == tiles * 64 * V + 5 <= 1029
            assert np.array_equal(y, fm.trimmed()["y"][rows]) and set(rows) == set(range(fm.FRAMES))


# every arithmetic under test on both codes; the plain ones on the trimmed code, the only one they run on here
STOP_CASES = [(a, n) for n in fm.CODES for a in fm.ARITHS] + [(a, "trimmed") for a in fm.PLAIN]


@pytest.mark.parametrize("arith,code_name", STOP_CASES)
def test_frames_stop_on_both_sides_of_the_tap(arith, code_name):
    w = fm.want(code_name, arith)
    it = w["iters"]
    run_r, run_q = fc.tap_frames(it)
    print("%s %s: %d distinct rounds, %d frames at round 1, %d at round %d, %d compare Q"
          % (code_name, arith, np.unique(it).size, (it == 1).sum(), (it == fm.MAXIT).sum(), fm.MAXIT, run_q.size))
    assert np.unique(it).size >= 5
    assert (it == 1).sum() >= 10
    assert (it == fm.MAXIT).sum() >= 10
    assert run_q.size >= 20
    assert w["hard"].shape == (fm.FRAMES, fm.CODES[code_name]()["N"])


@pytest.mark.parametrize("code_name", list(fm.CODES))
@pytest.mark.parametrize("arith", fm.FIXED)
def test_fixed_point_messages_saturate(arith, code_name):
    """Among the frames that ran round TAP, stored R and stored Q sit at the limit, |R| = L and |Q| = L, and none beyond"""
    w = fm.want(code_name, arith)
    Lq = RI.limit(fm.ARITHS[arith]["q"])
    run_r, run_q = fc.tap_frames(w["iters"])
    r, q = w["r_tap"][run_r], w["q_tap"][run_q]
    print("%s %s: %d R and %d Q at +-%d" % (code_name, arith, (np.abs(r) == Lq).sum(), (np.abs(q) == Lq).sum(), Lq))
    assert np.abs(r).max() == Lq and np.abs(q).max() == Lq


@pytest.mark.parametrize("arith", [a for a in fm.ARITHS if fm.ARITHS[a]["storage"] in ("i8", "f8")])
def test_degree_one_rows_store_the_start_value_as_the_type_reads_it(arith):
    """A row of degree 1 has no other edge: the start value 1000 survives to the stored R, which reads L in fixed point and
    448 in E4M3 -- plain and corrected (every correction here leaves 1000 above the largest code)."""
    c, w = fm.full(), fm.want("full", arith)
    one = fm.degree_one_edges(c)
    run_r, _ = fc.tap_frames(w["iters"])
    r = w["r_tap"][run_r][:, one]
    assert one.size >= 3 and run_r.size >= 20
    if fm.is_fixed(arith):
        assert r.dtype == np.int32 and (r == RI.limit(fm.ARITHS[arith]["q"])).all(), arith
    else:
        assert np.array_equal(r.view(np.uint32), np.full(r.shape, 448.0, f32).view(np.uint32)), arith


@pytest.mark.parametrize("code_name", list(fm.CODES))
@pytest.mark.parametrize("arith", fm.CORRECTED)
def test_every_correction_changes_the_result(arith, code_name):
    """A kernel table that dispatched to the uncorrected instantiation of the same type would fail"""
    c, w = fm.CODES[code_name](), fm.want(code_name, arith)
    plain = fm.reference(arith, c, c["y"], corrected=False)
    run_r, _ = fc.tap_frames(w["iters"])
    differ = int((w["iters"] != plain["iters"]).sum())
    taps = int(sum(not np.array_equal(w["r_tap"][f], plain["r_tap"][f], equal_nan=True) for f in run_r))
    print("%s %s: iteration counts differ in %d frames, the R tap in %d of %d" % (code_name, arith, differ, taps, run_r.size))
    assert differ >= 1 or taps >= 1


@pytest.mark.parametrize("code_name", list(fm.CODES))
@pytest.mark.parametrize("arith", fm.FIXED)
def test_every_width_changes_the_result(arith, code_name):
    """The neighbouring width (the next one; for 8 bits the one below) at this width's llr_scale: a table that dispatched to
    the wrong L would fail"""
    c, w = fm.CODES[code_name](), fm.want(code_name, arith)
    q = fm.ARITHS[arith]["q"]
    other = RI.WIDTHS[(RI.WIDTHS.index(q) + 1) % len(RI.WIDTHS)] if q != max(RI.WIDTHS) else sorted(RI.WIDTHS)[-2]
    assert other != q
    o = fm.reference(arith, c, c["y"], q=other)
    run_r, _ = fc.tap_frames(w["iters"])
    differ = int((w["iters"] != o["iters"]).sum())
    taps = int(sum(not np.array_equal(w["r_tap"][f], o["r_tap"][f]) for f in run_r))
    print("%s %s against %d bits: iteration counts differ in %d frames, the R tap in %d of %d" % (code_name, arith, other, differ, taps, run_r.size))
    assert differ >= 1 or taps >= 1


def test_plain_arithmetics_differ_from_each_other_on_the_trimmed_code():
    """ms, ms16, bp, bp16: four different results (a decoder that silently ran another of them would fail)"""
    its = [fm.want("trimmed", a) for a in fm.PLAIN]
    for i in range(len(its)):
        for j in range(i):
            assert not (np.array_equal(its[i]["iters"], its[j]["iters"]) and
                        np.array_equal(its[i]["r_tap"], its[j]["r_tap"], equal_nan=True)), (i, j)


def _constant(text, name):
    m = re.search(r"\b%s(?:\[\w+\])? = (?:\{([\d, ]+)\}|(\d+))" % name, text)
    assert m, name
    return tuple(int(x) for x in (m.group(1) or m.group(2)).split(","))


def test_the_launch_model_restates_the_tables():
    """flood_matrix_cases.default_launches against what the sources declare: the degree buckets and the unrolled limits of
    csrc/flood_tables.hpp and csrc/flood_common.hpp, the bucket kernels fill_v of csrc/flood_tables_impl.hpp assigns; and on
    the two codes, what the model names."""
    with open(os.path.join(CSRC, "flood_tables.hpp")) as f:
        tables = f.read()
    with open(os.path.join(CSRC, "flood_common.hpp")) as f:
        common = f.read()
    with open(os.path.join(CSRC, "flood_tables_impl.hpp")) as f:
        impl = f.read()
    assert tuple(zip(_constant(tables, "kCheckBucketLo"), _constant(tables, "kCheckBucketHi"))) == fm.CHECK_BUCKETS
    assert tuple(zip(_constant(tables, "kVarBucketLo"), _constant(tables, "kVarBucketHi"))) == fm.VAR_BUCKETS
    assert _constant(common, "kMaxUnrolledDegree") == (fm.MAX_VAR_UNROLLED,)
    assert _constant(common, "kMaxUnrolledCheckDegreeMS") == (fm.TABLE_MS["max_check_unrolled"],)
    for k, (lo, hi) in enumerate(fm.CHECK_BUCKETS):
        assert re.search(r"check_group\[%d\] = (?:f->check_group\[\d\] = )?check_group_kernel<ALGO, V, T, %d, %d, GW>" % (k, lo, hi), impl), k
    for k, (lo, hi) in enumerate(fm.VAR_BUCKETS):
        assert re.search(r"var_group\[%d\] = var_group_kernel<ALGO, V, T, %d, %d>" % (k, lo, hi), impl), k
    assert all(all(t["check_group"]) and all(t["var_group"]) for t in fm.TABLES.values())
    c = fm.full()
    rd, cd = km.degree_maps(c["rows"], c["cols"], c["M"], c["N"])
    names, lacking = fm.default_launches("msi6", rd, cd, 2)
    assert not lacking
    assert names == ({"check_group_kernel<msi6,%d-%d,2>" % b for b in fm.CHECK_BUCKETS} | {"check_kernel<msi6,33,2>", "check_kernel<msi6,40,2>"} |
                     {"var_group_kernel<msi6,%d-%d,2>" % b for b in fm.VAR_BUCKETS} |
                     {"var_kernel<msi6,0,2>", "var_kernel<msi6,17,2>", "var_kernel<msi6,20,2>"})
    solo = fm.solo_launches("msi6", rd, cd, 2)
    assert sum(n.startswith("check_kernel<") for n in solo) == 34 and sum(n.startswith("var_kernel<") for n in solo) == 19
    t = fm.trimmed()
    rd, cd = km.degree_maps(t["rows"], t["cols"], t["M"], t["N"])
    names, lacking = fm.default_launches("bp16", rd, cd, 4)
    assert not lacking and not any(n.startswith("check_kernel<") for n in names) and len(names) == 4 + 3 + 3
    # a table without a bucket kernel: its classes are launched alone and the kernel is named
    fm.TABLES["gap"] = dict(max_check_unrolled=32, check_group=(True, True, False, True), var_group=(True, True, True))
    try:
        names, lacking = fm.default_launches("gap", {17: 3, 18: 3, 4: 3, 5: 3, 30: 3}, {2: 5}, 1)
    finally:
        del fm.TABLES["gap"]
    assert names == {"check_kernel<gap,17,1>", "check_kernel<gap,18,1>", "check_group_kernel<gap,1-8,1>", "check_kernel<gap,30,1>",
                     "var_kernel<gap,2,1>"}
    assert lacking == ["check_group_kernel<gap,17-24,1>"]
