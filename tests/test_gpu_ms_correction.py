"""Normalized / offset min-sum on the MI355X: every kernel form that carries the correction -- the record kernels
(flood_ldsp_corr_kernel, layered_ldsp_corr_kernel), the streaming flooding kernels of every form, the streaming
layered kernels -- against the numpy restatement (ms_correction_ref.py, itself checked against the CPU oracle in
test_ms_correction_cpu.py): bytes, iteration counts, all N hard bits and the check->variable tap, bit for bit.  Each
case asserts which kernels ran; the LDS-resident one-launch kernels carry no correction and are refused."""
import functools
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
import oracle
from myldpccppapi_amd import channel, codes
from ms_correction_ref import Code, flood_ms, layered_ms
from coder_harness import coder_ms_correction_exe
from util import kernel_choice
import bp_cases as bc
import kernel_matrix as km

pytestmark = pytest.mark.gpu

SETTINGS = [(0.75, 0.0), (0.0, 0.15), (0.8, 0.05)]      # pure scale, pure offset, both


def _wimax(rate, N):
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    return rows, cols, M, N, K, z


def _kernels_run(dec, y):
    """decode once with timing on: (bytes, iterations, names of the kernels launched)"""
    dec.set_timing(True)
    out, iters = dec.decode(y)
    names = [k["name"] for k in dec.kernel_times()]
    dec.set_timing(False)
    return out, iters, names


def _flood_case(rows, cols, M, N, K, y, scale, offset, f16=False, z=0, it=12, expect="<msc", **kw):
    code = Code(rows, cols, M, N, K)
    ref = flood_ms(code, y, it, scale=scale, offset=offset, f16=f16, tap_iter=2)
    g = L.Graph(rows, cols, M, N)
    dec = L.Decoder(g, K, max_batch=y.shape[0], algo="ms", max_iter=it, layer_rows=z,
                    msg_dtype="f16" if f16 else "f32", ms_scale=scale, ms_offset=offset, **kw)
    out, iters, names = _kernels_run(dec, y)
    assert names and all(expect in n or n == "other" for n in names), (expect, names)
    assert np.array_equal(out, ref["out"]), ("bytes", scale, offset, f16, kw)
    assert np.array_equal(iters, ref["iters"]), ("iterations", scale, offset, f16, kw)
    _taps_and_hard(dec, y, ref, expect, ("flood", scale, offset, f16, kw))
    dec.close()


def _taps_and_hard(dec, y, ref, expect, what, ok=None):
    """R and the hard bits at iteration 2 (the tap stops the decode there; the record kernels' hard bits are
    those of the tapped posteriors), and for the streaming kernels all N final hard bits as well."""
    B = y.shape[0]
    ok = np.ones(B, bool) if ok is None else ok
    dec.set_tap(2)
    dec.decode(y)
    run = ok & (ref["iters"] >= 2)
    assert np.array_equal(dec.dump(0, B)[run], ref["r_tap"][run]), ("R tap",) + what
    if "ldsp" in expect:
        assert np.array_equal(dec.dump(3, B).astype(np.uint8)[run], ref["hard_tap"][run]), ("hard bits at the tap",) + what
    dec.set_tap(0)
    if "ldsp" not in expect:
        dec.decode(y)
        assert np.array_equal(dec.dump(3, B).astype(np.uint8)[ok], ref["hard"][ok]), ("hard bits",) + what


@pytest.mark.parametrize("scale,offset", SETTINGS)
@pytest.mark.parametrize("mode,expect", [("ldsp", "flood_ldsp_corr_kernel"), ("0", "<msc")])
@pytest.mark.parametrize("N", [576, 1152])
def test_flooding_corrected_record_and_streaming_kernels(built, scale, offset, mode, expect, N):
    """The record kernel (z = 24: several frames per wave, the packed form; z = 48: one frame per workgroup) and
    the streaming kernels on a quasi-cyclic code."""
    rows, cols, M, N, K, z = _wimax(codes.RATE_1_2, N)
    y = channel.awgn_frames(N, 0, 150, 0.8, seed=31)
    _flood_case(rows, cols, M, N, K, y, scale, offset, z=z, tune=kernel_choice(mode), expect=expect)


@pytest.mark.parametrize("algo", ["ms", "layered"])
def test_forced_lds_resident_kernels_refuse_a_correction(built, algo):
    """LDPC_TUNE_FUSED on with LDPC_TUNE_LDSP off asks for the LDS-resident one-launch kernel, which carries no
    correction: LDPC_ERR_UNSUPPORTED instead of a silent change of kernel."""
    rows, cols, M, N, K, z = _wimax(codes.RATE_1_2, 576)
    g = L.Graph(rows, cols, M, N)
    with pytest.raises(L.LdpcError) as e:
        L.Decoder(g, K, max_batch=64, algo=algo, layer_rows=z, tune=kernel_choice("1"), ms_scale=0.75)
    assert e.value.code == 4


@pytest.mark.parametrize("fpl", [1, 2, 4])
@pytest.mark.parametrize("link_rows", [0, -1])
def test_flooding_corrected_frames_per_lane_and_link_fusion(built, fpl, link_rows):
    """A staircase (IRA) code, whose degree-2 parity columns are fused into the check kernel unless
    link_rows = -1; the fused forms (wide / narrow / deep / half) are all exercised through V."""
    N, K = 12960, 6480
    rows, cols = codes.dvbs2_profile_edges(N, K)
    M = N - K
    y = channel.awgn_frames(N, 0, 128, 0.8, seed=fpl)
    tune = {"link_rows": link_rows} if link_rows else None
    for scale, offset in SETTINGS:
        _flood_case(rows, cols, M, N, K, y, scale, offset, it=8, frames_per_lane=fpl, tune=tune)
    if fpl >= 2 and link_rows == 0:
        for extra in ({"link_narrow": True}, {"link_narrow": False}, {"link_deep": True}, {"link_half": True}):
            _flood_case(rows, cols, M, N, K, y, 0.8, 0.05, it=8, frames_per_lane=fpl, tune=extra)


def test_flooding_corrected_generic_degree_rows(built):
    """A row wider than the unrolled min-sum kernels (degree 40 > 32) runs the generic check kernel."""
    z = 16
    base = -np.ones((4, 44), np.int64)
    rng = np.random.default_rng(7)
    base[0, :40] = rng.integers(0, z, 40)
    for i in range(1, 4):
        base[i, rng.choice(44, 6, replace=False)] = rng.integers(0, z, 6)
    base[1:, 40:] = np.array([[0, -1, -1, -1], [-1, 0, 3, -1], [-1, -1, 0, 5]])
    rows, cols = codes.qc_edges(base, z)
    M, N = 4 * z, 44 * z
    K = N - M
    y = channel.awgn_frames(N, 0, 64, 0.7, seed=3)
    for scale, offset in SETTINGS:
        for fpl in (1, 4):
            _flood_case(rows, cols, M, N, K, y, scale, offset, frames_per_lane=fpl)


@pytest.mark.parametrize("poll", [0, 1])
def test_flooding_corrected_fp16_with_tail(built, poll):
    """fp16 messages; poll_interval = 1: host-polled tail compaction (child decoders); 0 with 2048 frames:
    the device-side tail (overflow tiles)."""
    rows, cols, M, N, K, z = _wimax(codes.RATE_1_2, 576)
    y = channel.awgn_frames(N, 0, 2048, 0.72, seed=11 + poll)
    for scale, offset in SETTINGS:
        _flood_case(rows, cols, M, N, K, y, scale, offset, f16=True, it=16, poll_interval=poll,
                    frames_per_lane=1 if poll == 0 else 4)


LAYERED_MODES = (("ldsp", "layered_ldsp_corr_kernel"), ("0", "layer_corr_kernel"))


def _layered_case(rows, cols, M, N, K, z, y, scale, offset, it=12, modes=LAYERED_MODES):
    code = Code(rows, cols, M, N, K)
    ref = layered_ms(code, y, z, it, scale=scale, offset=offset, tap_iter=2)
    ok = ref["undefined"] == 0
    g = L.Graph(rows, cols, M, N)
    kb = K // 8
    for mode, expect in modes:
        dec = L.Decoder(g, K, max_batch=y.shape[0], algo="layered", layer_rows=z, max_iter=it,
                        tune=kernel_choice(mode), ms_scale=scale, ms_offset=offset)
        out, iters, names = _kernels_run(dec, y)
        assert names and all(expect in n or n == "other" for n in names), (expect, names)
        B = y.shape[0]
        assert np.array_equal(out.reshape(B, kb)[ok], ref["out"].reshape(B, kb)[ok]), (z, mode, scale, offset)
        assert np.array_equal(iters[ok], ref["iters"][ok]), (z, mode, scale, offset)
        _taps_and_hard(dec, y, ref, expect, ("layered", z, mode, scale, offset), ok)
        dec.close()


@pytest.mark.parametrize("rate,N", [(codes.RATE_1_2, 2304), (codes.RATE_2_3_A, 576), (codes.RATE_3_4_B, 1152),
                                    (codes.RATE_5_6, 960)])
def test_layered_corrected_wimax(built, rate, N):
    rows, cols, M, N, K, z = _wimax(rate, N)
    y = channel.awgn_frames(N, 0, 70, 0.75, seed=N)
    for scale, offset in SETTINGS:
        _layered_case(rows, cols, M, N, K, z, y, scale, offset)


def test_layered_corrected_random_quasi_cyclic_codes(built):
    """The case list of test_gpu_parity.py::test_layered_on_random_quasi_cyclic_codes."""
    rng = np.random.default_rng(20261004)
    cases = []
    for z, mb, nb, dmax in ((5, 3, 9, 5), (17, 6, 14, 6), (64, 4, 12, 8), (65, 5, 30, 24), (100, 1, 10, 10),
                            (40, 8, 12, 3), (96, 12, 36, 7), (130, 3, 26, 24), (24, 10, 16, 2), (33, 7, 40, 20)):
        base = -np.ones((mb, nb), np.int64)
        for i in range(mb):
            d = int(rng.integers(1, min(dmax, nb) + 1))
            base[i, rng.choice(nb, d, replace=False)] = rng.integers(0, z, d)
        for j in range(nb):
            if (base[:, j] < 0).all():
                i = int(rng.integers(0, mb))
                if (base[i] >= 0).sum() < 24:
                    base[i, j] = rng.integers(0, z)
        keep = [j for j in range(nb) if (base[:, j] >= 0).any()]
        base = base[:, keep]
        nb = len(keep)
        K = max(8, ((nb - min(mb, nb - 1)) * z - int(rng.integers(0, z))) // 8 * 8)
        cases.append((z, base, min(K, nb * z // 8 * 8)))
    for n, (z, base, K) in enumerate(cases):
        mb, nb = base.shape
        rows, cols = codes.qc_edges(base, z)
        M, N = mb * z, nb * z
        sigma = 0.9 if M * 2 > N else 0.6
        y = channel.awgn_frames(N, 0, 11, sigma, seed=z)
        y[3, ::3] = 0.0
        scale, offset = SETTINGS[n % 3]
        _layered_case(rows, cols, M, N, K, z, y, scale, offset, it=9)


UNROLLED = 24                       # kMaxUnrolledLayerDegree: wider rows take the run-time kernel
MATRIX_MAXIT = 5                    # about 135 launches per round with layer_rows = 1
MATRIX_TAP = 2
MATRIX_SETTINGS = [(0.0, 0.0), (0.75, 0.0), (0.0, 0.25)]       # the plain rule, then the corrected one: scale, offset


@functools.lru_cache(maxsize=None)
def _matrix_want(scale, offset):
    """The expectation of one setting on bp_cases.matrix(), every row a layer, computed once per process and read-only:
    the plain rule's is the CPU oracle's (with its P tap), the corrected rule's layered_ms's (which taps no P).  The
    oracle taps no bits, so the plain rule takes those of round MATRIX_TAP from layered_ms, which must agree with the
    oracle on everything both give."""
    m = bc.matrix()
    w = layered_ms(m["code"], m["y"], 1, MATRIX_MAXIT, scale=scale, offset=offset, tap_iter=MATRIX_TAP)
    w["p_tap"] = None
    if scale == 0.0 and offset == 0.0:
        og = oracle.Graph(m["rows"], m["cols"], m["M"], m["N"], m["K"])
        o = oracle.decode(og, m["y"], "layered", layer_rows=1, max_iter=MATRIX_MAXIT, tap_iter=MATRIX_TAP)
        run = o["iters"] >= MATRIX_TAP
        for a, b in ((o["out"], w["out"]), (o["iters"], w["iters"]), (o["hard"], w["hard"]), (o["undefined"], w["undefined"]),
                     (o["taps"]["r"][run], w["r_tap"][run])):
            assert np.array_equal(a, b)
        w = dict(out=o["out"], iters=o["iters"], hard=o["hard"], undefined=o["undefined"], r_tap=o["taps"]["r"],
                 p_tap=o["taps"]["post"], hard_tap=w["hard_tap"])
    for v in w.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return w


@pytest.mark.parametrize("scale,offset", MATRIX_SETTINGS)
@pytest.mark.parametrize("V", [1, 2, 4])
def test_layered_min_sum_every_degree_class(built, V, scale, offset):
    """The float min-sum rules of the streaming layered engine, plain and corrected, on the irregular matrix code with
    layer_rows = 1 -- every row a layer of its own: rows of degree 0, 1, 2, every unrolled degree up to 24, and 25 ... 33
    and 40 for the run-time kernel -- 70 frames, 5 rounds.  No frame is undefined in either reference, so none is masked:
    bytes, iteration counts, all N hard bits, and R, the bits and (plain rule) P after round 2 of the frames that ran it,
    exactly.  The timing spans name a launch of every degree, so both the unrolled and the run-time kernel ran."""
    m = bc.matrix()
    want = _matrix_want(scale, offset)
    assert want["undefined"].sum() == 0
    what = (V, scale, offset)
    B = bc.MATRIX_FRAMES
    dec = L.Decoder(L.Graph(m["rows"], m["cols"], m["M"], m["N"]), m["K"], max_batch=B, algo="layered", layer_rows=1,
                    max_iter=MATRIX_MAXIT, frames_per_lane=V, tune=kernel_choice("0"), ms_scale=scale, ms_offset=offset)
    dec.set_timing(True)
    out, iters = dec.decode(m["y"])
    names = {k["name"]: k["degree"] for k in dec.kernel_times() if k["phase"] == 2}
    dec.set_timing(False)
    assert np.array_equal(iters, want["iters"]), ("iterations",) + what
    assert np.array_equal(out, want["out"]), ("bytes",) + what
    assert np.array_equal(dec.dump(3, B).astype(np.uint8), want["hard"]), ("hard bits",) + what
    run = np.nonzero(want["iters"] >= MATRIX_TAP)[0]
    early = np.nonzero(want["iters"] < MATRIX_TAP)[0]
    assert run.size > 0 and early.size > 0, what
    dec.set_tap(MATRIX_TAP)
    dec.decode(m["y"])
    assert np.array_equal(dec.dump(0, B)[run], want["r_tap"][run]), ("R tap",) + what
    if want["p_tap"] is not None:
        assert np.array_equal(dec.dump(2, B)[run], want["p_tap"][run]), ("P tap",) + what
    bits = dec.dump(3, B).astype(np.uint8)
    assert np.array_equal(bits[run], want["hard_tap"][run]), ("bit tap",) + what
    assert np.array_equal(bits[early], want["hard"][early]), ("bits of the frames that had stopped",) + what
    dec.close()
    rd, _ = km.degree_maps(m["rows"], m["cols"], m["M"], m["N"])
    kernel = "layer_corr_kernel" if (scale, offset) != (0.0, 0.0) else "layer_kernel"
    assert set(names) == {"%s<layered,%d,%d>" % (kernel, d, V) for d in rd if d > 0}, (what, sorted(names))
    degrees = set(names.values())
    assert {1, 2, 3, UNROLLED} <= degrees and {UNROLLED + 1, 33, 40} <= degrees, (what, sorted(degrees))


def test_layered_corrected_bg1_profile(built):
    Z = 384
    rows, cols = codes.nr_bg1_profile_edges(Z)
    M, N = 46 * Z, 68 * Z
    K = 22 * Z
    y = channel.awgn_frames(N, 0, 6, 0.7, seed=5)
    _layered_case(rows, cols, M, N, K, Z, y, 0.75, 0.0, it=8)


# name: (km.QC_SHAPES entry, extra tuning, frames per workgroup); the workgroup is
# ceil(z / 64) waves: z = 600 has 10, which only the 16-wave instantiations hold
RECORD_FORMS = {
    "z24_packed": ("z24", {}, 2),
    "z24_unpacked": ("z24", {"ldsp_pack": False}, 1),
    "z200_4waves": ("z200_4waves", {}, 1),
    "z600_maxw16": ("z600_maxw16", {}, 1),
}
_record_refs = {}


def _record_ref(shape, algo, scale, offset):
    """code, channel values and the numpy reference of one (shape, algorithm, setting): 12 frames, 12 iterations"""
    key = (shape, algo, scale, offset)
    if key not in _record_refs:
        z, base, _ = km.QC_SHAPES[shape]
        mb, nb = base.shape
        rows, cols = codes.qc_edges(base, z)
        M, N = mb * z, nb * z
        K = (nb - mb) * z // 8 * 8
        # a noise level per frame: in every case some frames stop after 1 to 5 iterations and some run all 12
        y = km.channel_frames(N, 12, 0.3, 0.7, seed=z)
        y[3, ::3] = 0.0                          # zeros: rows that take the slow path of the record kernels
        code = Code(rows, cols, M, N, K)
        ref = (layered_ms(code, y, z, 12, scale=scale, offset=offset) if algo == "layered"
               else flood_ms(code, y, 12, scale=scale, offset=offset))
        _record_refs[key] = (rows, cols, M, N, K, z, y, ref)
    return _record_refs[key]


@pytest.mark.parametrize("scale,offset", [(0.75, 0.0), (0.0, 0.25)])
@pytest.mark.parametrize("form", list(RECORD_FORMS))
def test_corrected_record_kernels_in_every_launch_form(built, form, scale, offset):
    """The corrected record kernels in each form the selector can pick -- several frames per wave, one frame per
    one-wave workgroup, 4 waves, 10 waves (MAXW = 16) -- layered and flooding: bytes, iteration counts, the reported
    kernel name and launch shape [grid x block, frames per workgroup].  The name comes from the decoder's settings, not
    from the selector's pointer: which instantiation ran shows in the bytes (the correction) and in the launch itself
    (640 threads need the 16-wave kernel's launch bound)."""
    shape, extra, wg_frames = RECORD_FORMS[form]
    for algo, expect in (("layered", "layered_ldsp_corr_kernel["), ("ms", "flood_ldsp_corr_kernel[")):
        rows, cols, M, N, K, z, y, ref = _record_ref(shape, algo, scale, offset)
        B, kb = y.shape[0], K // 8
        what = (form, algo, scale, offset)
        ok = ref["undefined"] == 0 if algo == "layered" else np.ones(B, bool)
        dec = L.Decoder(L.Graph(rows, cols, M, N), K, max_batch=B, algo=algo, layer_rows=z, max_iter=12,
                        tune=dict(kernel_choice("ldsp"), **extra), ms_scale=scale, ms_offset=offset)
        out, iters, names = _kernels_run(dec, y)
        dec.close()
        assert np.array_equal(out.reshape(B, kb)[ok], ref["out"].reshape(B, kb)[ok]), what
        assert np.array_equal(iters[ok], ref["iters"][ok]), what
        assert names and all(n.startswith(expect) or n == "other" for n in names), (what, names)
        shapes = {km.ldsp_shape(n) for n in names if n != "other"}
        assert shapes == {((B + wg_frames - 1) // wg_frames, 64 * ((z + 63) // 64), wg_frames)}, (what, names)


def test_coder_min_sum_correction_equals_the_c_abi(built, tmp_path):
    exe = coder_ms_correction_exe(tmp_path)
    rate, N = codes.RATE_1_2, 576
    rows, cols, M, N, K, z = _wimax(rate, N)
    g = L.Graph(rows, cols, M, N)
    frames = 40
    y = channel.awgn_frames(N, 0, frames, 0.8, seed=9)
    y.astype(np.float32).tofile(str(tmp_path / "in"))
    for mode, algo, pack in (("MS", "ms", L.PACK_BYTES), ("CPU", "ms", L.PACK_BITS), ("TDMPCL", "layered", L.PACK_BYTES)):
        for scale, offset in SETTINGS:
            p = subprocess.run([exe, str(int(rate)), str(N), str(frames), mode, repr(scale), repr(offset),
                                str(tmp_path / "in"), str(tmp_path / "out")], capture_output=True, text=True)
            assert p.returncode == 0, p.stdout + p.stderr
            got = np.fromfile(str(tmp_path / "out"), np.uint8)
            dec = L.Decoder(g, K, max_batch=frames, algo=algo, max_iter=20, layer_rows=z, pack_mode=pack,
                            ms_scale=scale, ms_offset=offset)
            out, _ = dec.decode(y)
            dec.close()
            assert np.array_equal(got, out[:got.size]), (mode, scale, offset)


def test_error_rate_gain_wimax_layered(built):
    """WiMAX (2304, 1152) rate 1/2, layered, 20 iterations, 2048 frames of the seeded device channel
    (all-zero codeword, sd = 0.832, i.e. 20 log10(1/sd) = 1.6 dB): measured on an MI355X, plain min-sum
    leaves 515 frames in error, normalized min-sum with alpha = 0.75 48 (alpha = 0.8: 27; offset 0.15: 29).
    Both decoders are bit-exact and the channel is seeded, so the counts are deterministic; the test asks
    for a margin of 400 frames."""
    rows, cols, M, N, K, z = _wimax(codes.RATE_1_2, 2304)
    g = L.Graph(rows, cols, M, N)
    frames = 2048
    y = channel.awgn_device(N, 0, frames, 0.832, seed=20261016).cpu().numpy()
    fe = {}
    for scale in (0.0, 0.75):
        dec = L.Decoder(g, K, max_batch=frames, algo="layered", layer_rows=z, max_iter=20, ms_scale=scale)
        out, _ = dec.decode(y)
        dec.close()
        fe[scale] = int(np.any(out.reshape(frames, K // 8) != 0, axis=1).sum())
    assert fe[0.75] + MARGIN <= fe[0.0], fe


MARGIN = 400
