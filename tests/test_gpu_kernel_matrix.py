"""Every degree class and tuning form of the decoders against the oracle.

The streaming flooding kernels on an irregular code with rows of every degree 0 ... 33 and 40 and columns of every
degree 0 ... 17 and 20 (tests/kernel_matrix.py); the column-fused check kernel and the rows that ride along with it on
IRA codes; the one-launch kernels (LDS-resident, record, fused sum-product) and the streaming layered kernels on QC
shapes that reach their wave counts, row loops and packed forms.  Bytes, iteration counts, hard bits and the messages
at the iteration-2 tap are compared exactly, and every case asserts by kernel name or launch shape which kernels ran."""
import numpy as np
import pytest

import oracle
import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes
import kernel_matrix as km
from util import kernel_choice

pytestmark = pytest.mark.gpu
f32 = np.float32
MAXIT = 20


def _frame_bytes(out, K, frames):
    return np.asarray(out).reshape(frames, K // 8)


# --------------------------------------------------------------------------- streaming flooding, every degree class

@pytest.fixture(scope="module")
def mcode():
    rows, cols, M, N = km.matrix_code()
    K = (N - M) // 8 * 8
    g = L.Graph(rows, cols, M, N)
    og = oracle.Graph(rows, cols, M, N, K)
    y = km.channel_frames(N, 4 * 64 * 4 + 5, 0.15, 0.8, seed=20261016)
    want = {}
    for algo in ("sp", "ms", "ms16"):
        want[algo] = oracle.decode(og, y, "ms" if algo == "ms16" else algo, max_iter=MAXIT, tap_iter=2,
                                   msg_f16=algo == "ms16")
    rd, cd = km.degree_maps(rows, cols, M, N)
    return dict(g=g, K=K, M=M, N=N, y=y, want=want, row_degs=rd, col_degs=cd)


def _check_result(dec, mc, algo, y, lo, hi, what, hard=True):
    """bytes, iteration counts and all N hard bits of frames [lo, hi) against the oracle (the hard bits: of the last
    launch group)"""
    want, K = mc["want"][algo], mc["K"]
    out, iters = dec.decode(y[lo:hi])
    wb = _frame_bytes(want["out"], K, y.shape[0])[lo:hi]
    assert np.array_equal(_frame_bytes(out, K, hi - lo), wb), what
    assert np.array_equal(iters, want["iters"][lo:hi]), what
    if hard:
        assert np.array_equal(dec.dump(3, hi - lo).astype(np.uint8), want["hard"][lo:hi]), what


def _check_taps(dec, mc, algo, B, what):
    """R and Q after two rounds, bitwise, on the frames still running (as test_sum_product_fused_and_streaming_paths_agree)"""
    want = mc["want"][algo]
    dec.set_tap(2)
    dec.decode(mc["y"][:B])
    run_r = np.nonzero(want["iters"][:B] >= 2)[0]
    run_q = np.nonzero(want["iters"][:B] > 2)[0]
    assert run_q.size > 0
    R, Q = dec.dump(0, B), dec.dump(1, B)
    taps = {k: v[:B] for k, v in want["taps"].items()}
    if algo == "sp":
        assert np.array_equal(((f32(1) + R) * f32(0.5))[run_r], taps["r0"][run_r], equal_nan=True), what
        assert np.array_equal(((f32(1) - R) * f32(0.5))[run_r], taps["r1"][run_r], equal_nan=True), what
        dq = taps["q0"] - taps["q1"]
        assert np.array_equal(Q[run_q], dq[run_q], equal_nan=True), what
    else:
        assert np.array_equal(R[run_r], taps["r"][run_r], equal_nan=True), what
        assert np.array_equal(Q[run_q], taps["q"][run_q], equal_nan=True), what
    dec.set_tap(0)


def _names(dec):
    """the kernels of the last timed call ("other": transposes, syndrome and bookkeeping launches)"""
    return {k["name"] for k in dec.kernel_times() if k["name"] != "other"}


def _expected_solo(mc, a, V):
    rows = {"check_kernel<%s,%d,%d>" % (a, d, V) for d in mc["row_degs"] if d > 0}
    cols = {"var_kernel<%s,%d,%d>" % (a, d, V) for d in mc["col_degs"]}
    return rows | cols


@pytest.mark.parametrize("V", [1, 2, 4])
@pytest.mark.parametrize("algo", ["sp", "ms", "ms16"])
def test_streaming_flooding_every_degree_class(built, mcode, algo, V):
    """Streaming flooding kernels (layer_rows = 0) on the irregular matrix code, every launch plan of
    kernel_matrix.FLOOD_PLANS, a ragged last tile (2 * 64 * V + 5 frames), against the oracle."""
    mc, a = mcode, algo                # also the library's name of the arithmetic in kernel names
    y = mc["y"]
    B = 2 * 64 * V + 5
    kw = dict(algo="ms" if algo == "ms16" else algo, max_iter=MAXIT, frames_per_lane=V,
              msg_dtype="f16" if algo == "ms16" else "f32")
    # the code has no linked class: the plans below are the bucket / solo launches alone
    assert not any(km.linkable_rows(mc["g"].rows, mc["g"].cols, mc["M"], mc["N"]).values())
    for plan, tune in km.FLOOD_PLANS.items():
        what = (algo, V, plan)
        dec = L.Decoder(mc["g"], mc["K"], max_batch=B, tune=tune, **kw)
        dec.set_timing(True)
        _check_result(dec, mc, algo, y, 0, B, what)
        names = _names(dec)
        dec.set_timing(False)
        assert not any(n.startswith("check_link") for n in names), (what, names)
        if plan in ("merge_off", "check_wide"):
            # one launch per class: every unrolled check body 1 ... 32 (sum-product: 1 ... 16), the generic kernels above
            assert names == _expected_solo(mc, a, V), (what, sorted(names ^ _expected_solo(mc, a, V)))
        elif plan == "default":
            want = {"var_kernel<%s,0,%d>" % (a, V), "var_kernel<%s,17,%d>" % (a, V), "var_kernel<%s,20,%d>" % (a, V),
                    "var_group_kernel<%s,1-4,%d>" % (a, V), "var_group_kernel<%s,5-8,%d>" % (a, V),
                    "var_group_kernel<%s,9-16,%d>" % (a, V),
                    "check_group_kernel<%s,1-8,%d>" % (a, V), "check_group_kernel<%s,9-16,%d>" % (a, V)}
            if algo == "sp":       # sum-product rows above 16: check_kernel_generic, one launch per class
                want |= {"check_kernel<sp,%d,%d>" % (d, V) for d in mc["row_degs"] if d > 16}
            else:
                want |= {"check_group_kernel<%s,17-24,%d>" % (a, V), "check_group_kernel<%s,25-32,%d>" % (a, V),
                         "check_kernel<%s,33,%d>" % (a, V), "check_kernel<%s,40,%d>" % (a, V)}
            assert names == want, (what, sorted(names ^ want))
        _check_taps(dec, mc, algo, B, what)
        if plan == "default":
            for j in (0, B - 1):                                       # one call of a single frame
                _check_result(dec, mc, algo, y, j, j + 1, what + ("single", j))
        dec.close()
    # two launch groups: max_batch smaller than the batch
    dec = L.Decoder(mc["g"], mc["K"], max_batch=64 * V + 3, **kw)
    _check_result(dec, mc, algo, y, 0, B, (algo, V, "two groups"), hard=False)
    dec.close()
    # host polling with tail compaction over 5 tiles
    B4 = 4 * 64 * V + 5
    dec = L.Decoder(mc["g"], mc["K"], max_batch=B4, poll_interval=1, **kw)
    _check_result(dec, mc, algo, y, 0, B4, (algo, V, "poll"))
    assert dec.stats()["iterations_launched"] == MAXIT
    dec.close()
    # early termination off: every round runs; frames the oracle ran to the end are unaffected
    dec = L.Decoder(mc["g"], mc["K"], max_batch=B4, early_term=False, **kw)
    out, _ = dec.decode(y[:B4])
    full = np.nonzero(mc["want"][algo]["iters"][:B4] == MAXIT)[0]
    assert full.size > 20
    K = mc["K"]
    assert np.array_equal(_frame_bytes(out, K, B4)[full], _frame_bytes(mc["want"][algo]["out"], K, y.shape[0])[full])
    assert np.array_equal(dec.dump(3, B4).astype(np.uint8)[full], mc["want"][algo]["hard"][full])
    assert dec.stats()["iterations_launched"] == MAXIT
    dec.close()


# --------------------------------------------------------------------------- column-fused check kernel

IRA_EXTRA = {"ride": {5: 20, 7: 11, 20: 2}, "own": {5: 50, 7: 20, 20: 2}}     # 33 (<= 64) / 72 unlinked rows


@pytest.fixture(scope="module")
def ira_codes():
    out = {}
    for d in (3, 9, 16):
        for kind, extra in IRA_EXTRA.items():
            rows, cols, M, N, K = km.ira_code(d, 400, extra, seed=d)
            K8 = K // 8 * 8
            og = oracle.Graph(rows, cols, M, N, K8)
            y = km.channel_frames(N, 133, 0.5, 0.9, seed=100 + d)
            out[d, kind] = dict(g=L.Graph(rows, cols, M, N), K=K8, y=y,
                                want=oracle.decode(og, y, "ms", max_iter=25, tap_iter=2),
                                want_sp=oracle.decode(og, y, "sp", max_iter=25) if kind == "ride" else None)
    return out


LINK_FORMS = {"default": {}, "narrow_off": {"link_narrow": False}, "narrow": {"link_narrow": True},
              "half": {"link_half": True}, "deep": {"link_deep": True}, "rows_5": {"link_rows": 5}}


def _link_kernel_name(form, V):
    """The name the timing report gives the form asked for; None where the decoder chooses (V = 1 takes narrow, above
    that the creation-time calibration picks).  The deep form reports as narrow; half exists at V = 4 only."""
    if form == "narrow_off":
        return "check_link_kernel<"
    if form == "half" and V == 4:
        return "check_link_half_kernel<"
    if form in ("narrow", "deep", "half"):
        return "check_link_narrow_kernel<"
    return "check_link_narrow_kernel<" if V == 1 else None


@pytest.mark.parametrize("d", [3, 9, 16])
def test_column_fused_forms(built, ira_codes, d):
    """IRA codes with the linked class at degree d: with <= 64 unlinked rows they ride along in the column-fused
    launch (only check_link_* in phase 0); with more they get launches of their own.  Every form against the
    oracle, V = 1, 2 and 4 (V = 2: the 32-bit mask fields of the narrow forms): bytes, iteration counts, all N hard
    bits (the staircase columns are parity columns: their bits never reach the bytes), R and Q after two rounds.
    Then sum-product through every form: its variable node keeps the previous bit on a tie or NaN, in every form's
    own mask handling, and the fixture holds frames that run all 25 iterations."""
    for kind in ("ride", "own"):
        c = ira_codes[d, kind]
        B, want = c["y"].shape[0], c["want"]
        for form, tune in (LINK_FORMS.items() if kind == "ride" else [("default", {})]):
            for V in (1, 2, 4):
                what = (d, kind, form, V)
                dec = L.Decoder(c["g"], c["K"], max_batch=B, algo="ms", max_iter=25, frames_per_lane=V, tune=tune)
                dec.set_timing(True)
                out, iters = dec.decode(c["y"])
                assert np.array_equal(out, want["out"]) and np.array_equal(iters, want["iters"]), what
                assert np.array_equal(dec.dump(3, B).astype(np.uint8), want["hard"]), what
                kt = dec.kernel_times()
                dec.set_timing(False)
                phase0 = {k["name"] for k in kt if k["phase"] == 0}
                assert any(n.startswith("check_link") and n.endswith(",%d,%d>" % (d, V)) for n in phase0), (what, phase0)
                if kind == "ride":
                    assert all(n.startswith(_link_kernel_name(form, V) or "check_link") for n in phase0), (what, phase0)
                else:
                    assert any(n.startswith("check_group_kernel<ms,") or n.startswith("check_kernel<ms,20,")
                               for n in phase0), (what, phase0)
                dec.set_tap(2)
                dec.decode(c["y"])
                run_r = np.nonzero(want["iters"] >= 2)[0]
                run_q = np.nonzero(want["iters"] > 2)[0]
                assert np.array_equal(dec.dump(0, B)[run_r], want["taps"]["r"][run_r]), what
                assert np.array_equal(dec.dump(1, B)[run_q], want["taps"]["q"][run_q], equal_nan=True), what
                dec.close()
        if kind == "ride":               # sum-product through the same launch, every form
            want_sp = c["want_sp"]
            assert (want_sp["iters"] == 25).any(), (d, "no sum-product frame runs all 25 iterations")
            for form, tune in LINK_FORMS.items():
                for V in (1, 2, 4):
                    what = (d, "sp", form, V)
                    dec = L.Decoder(c["g"], c["K"], max_batch=B, algo="sp", max_iter=25, frames_per_lane=V, tune=tune)
                    dec.set_timing(True)
                    out, iters = dec.decode(c["y"])
                    phase0 = {k["name"] for k in dec.kernel_times() if k["phase"] == 0}
                    dec.set_timing(False)
                    assert np.array_equal(out, want_sp["out"]) and np.array_equal(iters, want_sp["iters"]), what
                    assert np.array_equal(dec.dump(3, B).astype(np.uint8), want_sp["hard"]), what
                    assert phase0 and all(n.startswith(_link_kernel_name(form, V) or "check_link")
                                          and n.endswith(",%d,%d>" % (d, V)) for n in phase0), (what, phase0)
                    dec.close()


# --------------------------------------------------------------------------- one-launch kernels on QC shapes

@pytest.fixture(scope="module")
def qc_cases():
    out = {}
    for name, (z, base, elig) in km.QC_SHAPES.items():
        mb, nb = base.shape
        rows, cols = codes.qc_edges(base, z)
        M, N = mb * z, nb * z
        K = (nb - mb) * z // 8 * 8
        og = oracle.Graph(rows, cols, M, N, K)
        B = 12
        y = km.channel_frames(N, B, 0.55, 0.85, seed=z)
        y[3, ::3] = 0.0                          # zeros: rows that take the slow path of the record kernel
        want = {a: oracle.decode(og, y, a, layer_rows=z if a == "layered" else 0, max_iter=12, tap_iter=2)
                for a in ("layered", "ms", "ms_fused", "sp")}
        out[name] = dict(z=z, base=base, elig=elig, g=L.Graph(rows, cols, M, N), K=K, B=B, y=y, want=want,
                         max_row=int(((base >= 0).sum(axis=1)).max()))
    return out


def _expected_kernel(algo, choice, elig, max_row):
    """The name prefix the selector's choice reports in kernel_times(), or an LdpcError code."""
    fused, sp, ldsp = elig["fused"], elig["sp"], elig["ldsp"]
    if algo == "layered":
        if choice == "ldsp" and ldsp:
            return "layered_ldsp_kernel["
        if choice in ("1", "ldsp") and fused:
            return "fused_layered_kernel"
        return "layer_kernel<layered,%d," % max_row
    if algo == "ms":
        if choice == "ldsp" and ldsp:
            return "flood_ldsp_kernel["
        if choice in ("1", "ldsp") and fused:
            return "fused_flood_kernel"
        return "check_"
    if algo == "ms_fused":
        if choice == "ldsp" and ldsp:
            return "flood_ldsp_kernel["
        return "fused_flood_kernel" if fused else 4            # LDPC_ERR_UNSUPPORTED: nothing one-launch fits
    if algo == "sp":
        return "fused_sp_kernel" if choice == "1" and sp else "check_"
    raise ValueError(algo)


QC_RUNS = [(algo, choice, extra) for algo in ("layered", "ms", "ms_fused", "sp")
           for choice in {"layered": ("1", "ldsp", "0"), "ms": ("1", "ldsp", "0"), "ms_fused": ("1", "ldsp"),
                          "sp": ("1", "0")}[algo]
           for extra in ({}, {"fused_loop": True} if choice == "1" else None,
                         {"ldsp_waves": 12} if choice == "ldsp" else None,
                         {"ldsp_ext": False} if choice == "ldsp" and algo != "layered" else None,
                         {"ldsp_pack": False} if choice == "ldsp" else None,
                         {"fused_pack": False} if choice == "1" and algo == "layered" else None)
           if extra is not None]


@pytest.mark.parametrize("shape", list(km.QC_SHAPES))
def test_one_launch_kernels_on_qc_shapes(built, qc_cases, shape):
    """layered, ms, ms_fused and sp through the LDS-resident, record and streaming choices (plus run-time row
    loops, 12 record waves, record kernels without external columns or without frame packing, the unpacked
    LDS-resident layered kernel) on a QC shape: bytes and iteration counts (frames the oracle marks undefined
    masked), R and posteriors at the iteration-2 tap for layered, and the kernel that ran."""
    c = qc_cases[shape]
    z, B, K = c["z"], c["B"], c["K"]
    kb = K // 8
    for algo, choice, extra in QC_RUNS:
        tune = dict(kernel_choice(choice), **extra)
        what = (shape, algo, choice, extra)
        want = c["want"][algo]
        expect = _expected_kernel(algo, choice, c["elig"], c["max_row"]) if c["elig"] else None
        if isinstance(expect, int):
            with pytest.raises(L.LdpcError) as e:
                L.Decoder(c["g"], K, max_batch=B, algo=algo, max_iter=12, layer_rows=z, tune=tune)
            assert e.value.code == expect, what
            continue
        try:
            dec = L.Decoder(c["g"], K, max_batch=B, algo=algo, max_iter=12, layer_rows=z, tune=tune)
        except L.LdpcError as e:
            # a structure the one-launch planners turn down: only MS_FUSED has no streaming fall-back
            if expect is None and algo == "ms_fused" and e.code == 4:
                continue
            raise
        dec.set_timing(True)
        try:
            out, iters = dec.decode(c["y"])
        except L.LdpcError as e:
            pytest.fail("%s: %s" % (what, e))
        names = _names(dec)
        dec.set_timing(False)
        ok = want["undefined"] == 0 if "undefined" in want else np.ones(B, bool)
        assert np.array_equal(out.reshape(B, kb)[ok], want["out"].reshape(B, kb)[ok]), what
        assert np.array_equal(iters[ok], want["iters"][ok]), what
        if expect is not None:
            assert any(n.startswith(expect) for n in names), (what, expect, names)
            ld = [km.ldsp_shape(n) for n in names if "ldsp_kernel[" in n]
            if ld:
                grid, block, frames = ld[0]
                waves = max((z + 63) // 64, extra.get("ldsp_waves", 0))
                assert block == 64 * waves, (what, names)               # > 512: the MAXW = 16 kernels
                packed = z <= 32 and waves == 1 and extra.get("ldsp_pack", True)
                assert frames == (64 // z if packed else 1), (what, names)
        if algo == "layered":
            dec.set_tap(2)
            dec.decode(c["y"])
            run = ok & (want["iters"] >= 2)
            assert np.array_equal(dec.dump(0, B)[run], want["taps"]["r"][run]), what
            assert np.array_equal(dec.dump(2, B)[run], want["taps"]["post"][run]), what
        dec.close()


@pytest.mark.parametrize("per_cu", [1, 3])
def test_record_kernel_grid_and_waves(built, per_cu):
    """ldsp_per_cu: the record kernels' persistent grid holds per_cu workgroups per CU, so a batch larger than
    the grid walks several frames per workgroup; with ldsp_waves 12 the workgroup has 12 waves (the MAXW = 16
    kernel).  Layered and flooding min-sum against the oracle."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    z = 48
    base = km.qc_base(z, 4, [4, 6, 5, 3], 8, seed=6)
    rows, cols = codes.qc_edges(base, z)
    M, N = base.shape[0] * z, base.shape[1] * z
    K = (N - M) // 8 * 8
    g, og = L.Graph(rows, cols, M, N), oracle.Graph(rows, cols, M, N, K)
    B = cus + 37
    y = km.channel_frames(N, B, 0.5, 0.85, seed=48)
    for algo in ("layered", "ms"):
        want = oracle.decode(og, y, algo, layer_rows=z if algo == "layered" else 0, max_iter=12)
        ok = want["undefined"] == 0 if "undefined" in want else np.ones(B, bool)
        for waves in (0, 12):
            tune = dict(kernel_choice("ldsp"), ldsp_per_cu=per_cu, ldsp_waves=waves)
            dec = L.Decoder(g, K, max_batch=B, algo=algo, max_iter=12, layer_rows=z, tune=tune)
            dec.set_timing(True)
            out, iters = dec.decode(y)
            names = [n for n in _names(dec) if "ldsp_kernel[" in n]
            dec.set_timing(False)
            assert np.array_equal(out.reshape(B, K // 8)[ok], want["out"].reshape(B, K // 8)[ok]), (algo, per_cu, waves)
            assert np.array_equal(iters[ok], want["iters"][ok]), (algo, per_cu, waves)
            assert len(names) == 1, names
            grid, block, frames = km.ldsp_shape(names[0])
            assert (grid, block, frames) == (min(B, per_cu * cus), 64 * max(1, waves), 1), (algo, per_cu, waves, names)
            dec.close()
