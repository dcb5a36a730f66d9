"""Layered log-domain sum-product (algo = layered_bp) on the GPU against tests/layered_bp_ref.py: the BG1-profile test code
at every tile width, every degree class of the unrolled and the run-time kernel, degenerate channel values, early
termination off, the CRC stop, soft output, the host path and a device list, exact zeros from the rate matcher, the
refusals that need a device and Coder's DecodeLayeredBP.

layered_bp is this repository's own definition (include/ldpc_hip.h: LDPC_ALGO_LAYERED_BP), so the expectation is the numpy
restatement, which tests/test_layered_bp_cpu.py holds to layered min-sum (correction c == 0).  The definition has no libm
call in it, so everything is compared bit for bit: bytes, iteration counts, all N hard bits, R, P and the bits after round
TAP, soft values at 0 ulp."""
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, channel, codes

import bp_cases as bc
import bp_ref as RB
import crc_term_cases as CC
import fp16_cases as fc
import kernel_matrix as km
import layered_bp_cases as lc
import layered_bp_ref as LB
import ratematch_util as U
import soft_ref as SR
from ms_correction_ref import Code

pytestmark = pytest.mark.gpu

f32 = np.float32
LDPC_ERR_ARG, LDPC_ERR_UNSUPPORTED = 1, 4
UNROLLED = 24                       # kMaxUnrolledLayerDegree: wider rows take the run-time kernel


def _decoder(c, B, max_iter, V, layer_rows, scale=lc.SCALES[0], **kw):
    return L.Decoder(L.Graph(c["rows"], c["cols"], c["M"], c["N"]), c["K"], max_batch=B, algo="layered_bp", max_iter=max_iter,
                     frames_per_lane=V, layer_rows=layer_rows, llr_scale=scale, **kw)


def _compare(dec, y, want, what):
    """One timed decode and one that stops at the tap: bytes, iteration counts and all N hard bits; R, P and the bits of
    the frames that ran round TAP (the others' P and R evolve unread on the device, their bits are their final ones).
    Returns {kernel name: degree} of the layer launches of the timed decode."""
    B = y.shape[0]
    dec.set_timing(True)
    out, iters = dec.decode(y)
    names = {k["name"]: k["degree"] for k in dec.kernel_times() if k["phase"] == 2}
    dec.set_timing(False)
    assert np.array_equal(iters, want["iters"]), ("iterations",) + what
    assert np.array_equal(out, want["out"]), ("bytes",) + what
    assert np.array_equal(dec.dump(3, B).astype(np.uint8), want["hard"]), ("hard bits",) + what
    run = np.nonzero(want["iters"] >= lc.TAP)[0]
    early = np.nonzero(want["iters"] < lc.TAP)[0]
    assert run.size > 0, what
    dec.set_tap(lc.TAP)
    dec.decode(y)
    assert fc.same_floats(dec.dump(0, B)[run], want["r_tap"][run]), ("R tap",) + what
    assert fc.same_floats(dec.dump(2, B)[run], want["p_tap"][run]), ("P tap",) + what
    bits = dec.dump(3, B).astype(np.uint8)
    assert np.array_equal(bits[run], want["hard_tap"][run]), ("bit tap",) + what
    assert np.array_equal(bits[early], want["hard"][early]), ("bits of the frames that had stopped",) + what
    dec.set_tap(0)
    return names


@pytest.mark.parametrize("V", [1, 2, 4])
def test_layered_bp_on_the_bg1_profile_code(built, V):
    """N = 1088, z = 16, row degrees 3 ... 19; 70 frames of mixed noise (a ragged second tile at V = 1, a partial tile at
    V = 2 and 4) under both llr_scale values, and at V = 4 also 262 frames: a full tile and a ragged one.  By kernel name,
    the layered BP instantiations ran."""
    c = lc.bg1_code()
    cases = [(70, s) for s in lc.SCALES] + ([(lc.BG1_TWO_TILES, lc.SCALES[0])] if V == 4 else [])
    for frames, scale in cases:
        what = (V, frames, scale)
        dec = _decoder(c, frames, lc.BG1_MAXIT, V, c["z"], scale=scale)
        names = _compare(dec, lc.bg1_inputs(frames), lc.bg1_want(frames, scale), what)
        rd, _ = km.degree_maps(c["rows"], c["cols"], c["M"], c["N"])
        assert set(names) == {"layer_kernel<layered_bp,%d,%d>" % (d, V) for d in rd if d > 0}, (what, sorted(names))
        dec.close()


@pytest.mark.parametrize("V", [1, 2, 4])
def test_layered_bp_every_degree_class(built, V):
    """The irregular matrix code with layer_rows = 1 -- every row a layer of its own: rows of degree 0, 1, 2, every unrolled
    degree up to 24, and 25 ... 33 and 40 for the run-time kernel -- 70 frames, both llr_scale values.  The timing spans
    name a launch of every degree, so both the unrolled and the run-time kernel ran."""
    m = bc.matrix()
    rd, _ = km.degree_maps(m["rows"], m["cols"], m["M"], m["N"])
    for scale in lc.SCALES:
        dec = _decoder(m, bc.MATRIX_FRAMES, lc.MATRIX_MAXIT, V, 1, scale=scale)
        names = _compare(dec, m["y"], lc.matrix_want(scale), (V, scale))
        assert set(names) == {"layer_kernel<layered_bp,%d,%d>" % (d, V) for d in rd if d > 0}, sorted(names)
        degrees = set(names.values())
        assert {1, 2, 3, UNROLLED} <= degrees and {UNROLLED + 1, 33, 40} <= degrees, sorted(degrees)
        dec.close()


@pytest.mark.parametrize("name", ["wimax", "ira"])
def test_layered_bp_degenerate_channel_values(built, name):
    """Zeros, infinities, NaN, subnormals, -0, values at +-64500 in y: WiMAX (960, 480) layered by its circulant size, the
    staircase code (consecutive rows share a column) with every row a layer.  NaN reads +1000 in a row and stays NaN in P,
    infinities read +-1000."""
    c, y = fc.degenerate_code(name), fc.degenerate_inputs(name)
    want = lc.degenerate_want(name)
    for V in (1, 2, 4):
        dec = _decoder(c, y.shape[0], lc.DEGENERATE_MAXIT[name], V, lc.degenerate_layer_rows(name), scale=bc.DEGENERATE_SCALE)
        _compare(dec, y, want, (name, V))
        dec.close()


def test_layered_bp_without_early_termination(built):
    """early_term = 0: every frame runs max_iter rounds and reports them, the bytes are the last round's."""
    c = lc.bg1_code()
    want = lc.bg1_want(70, lc.SCALES[0], 0, False)
    assert (want["iters"] == lc.BG1_MAXIT).all() and not (lc.bg1_want(70)["iters"] == lc.BG1_MAXIT).all()
    for V in (1, 4):
        dec = _decoder(c, 70, lc.BG1_MAXIT, V, c["z"], early_term=False)
        out, iters = dec.decode(lc.bg1_inputs(70))
        assert np.array_equal(iters, want["iters"]) and np.array_equal(out, want["out"]), V
        assert np.array_equal(dec.dump(3, 70).astype(np.uint8), want["hard"]), V
        dec.close()


def test_layered_bp_crc_stop(built):
    """bp_cases.crc_case's 150 frames: iteration counts, bytes and the number of frames the CRC stopped before their
    syndrome was clean, against the reference with the stop predicate."""
    kind, bits, y, w = lc.crc_case()
    assert w["by_stop"].size >= 1
    c = lc.bg1_code()
    for V in (1, 4):
        dec = _decoder(c, 150, CC.MAXIT, V, c["z"], scale=bc.SCALE, crc_kind=kind, crc_bits=bits)
        out, iters = dec.decode(y)
        assert np.array_equal(iters, w["iters"]), V
        assert np.array_equal(out, w["out"]), V
        assert dec.crc_stops() == w["by_stop"].size, (V, dec.crc_stops(), w["by_stop"].size)
        dec.close()


@pytest.mark.parametrize("kind", ["posterior", "extrinsic"])
def test_layered_bp_soft_output(built, kind):
    """P after the last layer of the stop round (and that minus chan = llr_scale * y, the product rounded first) at 0 ulp,
    V = 1, 2, 4, under the scale whose product rounds; a frame that stops in round 1 and one that never stops are
    present; a plain call before and after the soft call gives the same bytes."""
    c = lc.bg1_code()
    y, w = lc.bg1_inputs(70), lc.bg1_want(70, lc.SCALES[1])
    assert (w["iters"] == 1).any() and (~c["code"].syndrome_ok(w["hard"])).any()
    assert SR.sign_disagreements(w["post"], w["hard"]) == 0
    for V in (1, 2, 4):
        dec = _decoder(c, 70, lc.BG1_MAXIT, V, c["z"], scale=lc.SCALES[1])
        before, _ = dec.decode(y)
        out, iters, soft = dec.decode(y, soft=kind)
        after, _ = dec.decode(y)
        assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), V
        assert np.array_equal(before, out) and np.array_equal(after, out), V
        SR.assert_same_bits(soft, RB.soft_of(w, kind), None, str((V, kind)))
        if kind == "posterior":
            assert SR.sign_disagreements(soft, dec.dump(3, 70)) == 0, V
        dec.close()


def test_layered_bp_host_path_and_device_list(built):
    """262 frames through ldpc_decode_soft with max_batch = 64 (four full launch groups and a ragged one), and through a
    handle over the same ordinal twice: bytes, iteration counts and soft values of the single-call result and of the
    reference; the guard bytes behind out / iters / soft untouched."""
    c = lc.bg1_code()
    frames, guard = lc.BG1_TWO_TILES, 64
    y, w = lc.bg1_inputs(frames), lc.bg1_want(frames)
    lib = _lib.load()
    nb = L.out_bytes(c["K"], frames)
    single = _decoder(c, frames, lc.BG1_MAXIT, 2, c["z"])
    out1, iters1 = single.decode(y)
    single.close()
    assert np.array_equal(out1, w["out"]) and np.array_equal(iters1, w["iters"])
    for V in (1, 4):
        dec = _decoder(c, 64, lc.BG1_MAXIT, V, c["z"])
        out = np.full(nb + guard, 0xEE, np.uint8)
        iters = np.full(frames + guard, -7, np.int32)
        soft = np.full(frames * c["N"] + guard, -12345.0, np.float32)
        _lib.check(lib.ldpc_decode_soft(dec._h, y.ctypes.data, frames, out.ctypes.data, nb, iters.ctypes.data, soft.ctypes.data,
                                        frames * c["N"], L.capi.SOFT_KINDS["extrinsic"]))
        assert np.array_equal(iters[:frames], iters1) and np.array_equal(out[:nb], out1), V
        SR.assert_same_bits(soft[:frames * c["N"]].reshape(frames, -1), RB.soft_of(w, "extrinsic"), None, str(("host path", V)))
        assert (out[nb:] == 0xEE).all() and (iters[frames:] == -7).all() and (soft[frames * c["N"]:] == np.float32(-12345.0)).all(), V
        assert dec.stats()["frames"] == frames
        dec.close()
    multi = _decoder(c, 64, lc.BG1_MAXIT, 1, c["z"], devices=[0, 0])
    out2, iters2 = multi.decode(y)
    assert np.array_equal(out2, out1) and np.array_equal(iters2, iters1)
    multi.close()


def test_layered_bp_takes_exact_zeros_from_the_rate_matcher(built):
    """Scenario S1 end to end on the device: match, channel, ldpc_rate_recover_device with erasure_llr = 0 -- exact zeros at
    the punctured columns --, then layered_bp on the device buffer: the bytes and iteration counts of the reference, which
    decodes the frames (tests/test_layered_bp_cpu.py) where layered min-sum gets none."""
    import torch
    from test_gpu_ratematch import _same, _stream
    rows, cols, _ = U.bg1()
    g = L.Graph(rows, cols, U.M, U.N)
    code = torch.from_numpy(np.array(U.payload()[2])).cuda()
    rm = L.RateMatcher(**U.scenario_spec(0.0).kwargs())
    soft = torch.full((U.FRAMES, U.N), float("nan"), dtype=torch.float32, device="cuda")
    y = torch.full((U.FRAMES, U.N), float("nan"), dtype=torch.float32, device="cuda")
    txs, sd = U.received(lc.ERASURE_SCENARIO)
    for t, (k0, E, tx_want, rx_want) in enumerate(txs[:1]):
        tx = torch.empty((U.FRAMES, E), dtype=torch.uint8, device="cuda")
        rm.match_device(code.data_ptr(), U.FRAMES, k0, E, tx.data_ptr(), tx.numel(), "bits", "bits", _stream())
        rx = channel.awgn_device(E, 0, U.FRAMES, sd, seed=100 + t, codewords=tx)
        rm.recover_device(rx.data_ptr(), U.FRAMES, k0, E, soft.data_ptr(), t > 0, y.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _same(y.cpu().numpy(), U.recovered(lc.ERASURE_SCENARIO, 0.0, 1))
    assert bool((y[:, :U.P] == 0).all())
    w = lc.erasure_want()
    dec = L.Decoder(g, U.K, max_batch=U.FRAMES, algo="layered_bp", max_iter=U.MAX_ITER, llr_scale=lc.erasure_scale(), layer_rows=U.Z)
    out = torch.zeros(L.out_bytes(U.K, U.FRAMES), dtype=torch.uint8, device="cuda")
    iters = torch.zeros(U.FRAMES, dtype=torch.int32, device="cuda")
    dec.decode_device(y.data_ptr(), U.FRAMES, out.data_ptr(), out.numel(), iters.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), w["out"]) and np.array_equal(iters.cpu().numpy(), w["iters"])
    assert lc.frames_right(out.cpu().numpy()) == lc.frames_right(w["out"])
    dec.close()


def test_layered_bp_refusals(built):
    """With the one-launch or the record kernels forced on, layered_bp is LDPC_ERR_UNSUPPORTED.  A refused creation leaves
    nothing behind: a decoder made right after it runs the streaming layered BP kernels and decodes as the reference says."""
    import torch
    c = lc.bg1_code()
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    for tune in ({"fused": True}, {"ldsp": True}, {"fused": True, "ldsp": True}):
        with pytest.raises(L.LdpcError) as e:
            L.Decoder(g, c["K"], max_batch=64, max_iter=lc.BG1_MAXIT, algo="layered_bp", layer_rows=c["z"], tune=tune)
        assert e.value.code == LDPC_ERR_UNSUPPORTED, (tune, str(e.value))
        torch.cuda.synchronize()
    with pytest.raises(L.LdpcError) as e:                   # rows of a layer share a column
        L.Decoder(g, c["K"], max_batch=64, algo="layered_bp", layer_rows=2 * c["z"])
    assert e.value.code == LDPC_ERR_ARG
    want = lc.bg1_want(70)
    dec = L.Decoder(g, c["K"], max_batch=70, algo="layered_bp", max_iter=lc.BG1_MAXIT, layer_rows=c["z"], llr_scale=lc.SCALES[0])
    dec.set_timing(True)
    out, iters = dec.decode(lc.bg1_inputs(70))
    assert np.array_equal(iters, want["iters"]) and np.array_equal(out, want["out"])
    names = [k["name"] for k in dec.kernel_times() if k["phase"] == 2]
    assert names and all(n.startswith("layer_kernel<layered_bp,") for n in names), names
    dec.close()


def test_coder_decode_layered_bp_equals_the_c_abi(built, tmp_path):
    """Coder's DecodeLayeredBP with setLlrScale gives the bytes and the soft values (both kinds) of the C ABI decoder with
    algo = layered_bp and the Coder's circulant size -- and of the reference --, also over a device list; with
    setMinSumCorrection or a message type other than F32 addDecodeType fails as ldpc_decoder_create does."""
    from coder_layered_bp_harness import coder_layered_bp_exe
    exe = coder_layered_bp_exe(tmp_path)
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    g = L.Graph(rows, cols, M, N)
    frames = 40
    y = channel.awgn_frames(N, 0, frames, 0.8, seed=9)
    y.astype(np.float32).tofile(str(tmp_path / "in"))
    scale = 3.125                                    # 2 / 0.8^2

    def run(dtype=L.capi.MSG_F32, kind=0, ms_scale=0.0, ms_offset=0.0, ndev=1):
        return subprocess.run([exe, str(int(rate)), str(N), str(frames), str(dtype), repr(scale), repr(ms_scale), repr(ms_offset),
                               str(kind), str(ndev), str(tmp_path / "in"), str(tmp_path / "out"), str(tmp_path / "soft")],
                              capture_output=True, text=True)

    w = LB.layered_bp(Code(rows, cols, M, N, K), y, z, 20, llr_scale=scale)
    assert np.unique(w["iters"]).size >= 2
    for kind_name, kind, ndev in ((None, 0, 1), ("posterior", 1, 1), ("extrinsic", 2, 1), (None, 0, 2)):
        p = run(kind=kind, ndev=ndev)
        assert p.returncode == 0, p.stdout + p.stderr
        got = np.fromfile(str(tmp_path / "out"), np.uint8)
        dec = L.Decoder(g, K, max_batch=frames, algo="layered_bp", max_iter=20, layer_rows=z, llr_scale=scale, poll_interval=4)
        res = dec.decode(y, soft=kind_name)
        dec.close()
        assert np.array_equal(got, res[0][:got.size]) and np.array_equal(got, w["out"][:got.size]), (kind, ndev)
        if kind:
            soft = np.fromfile(str(tmp_path / "soft"), np.float32).reshape(frames, N)
            SR.assert_same_bits(soft, res[2], None, str(("coder against the C ABI", kind_name)))
            SR.assert_same_bits(soft, RB.soft_of(w, kind_name), None, str(("coder against the reference", kind_name)))
    for kw in (dict(ms_scale=0.75), dict(ms_offset=0.15)):
        p = run(**kw)
        assert p.returncode == 3 and "ms_scale" in p.stdout, p.stdout + p.stderr
    p = run(dtype=L.capi.MSG_F16)
    assert p.returncode == 3 and "fp16" in p.stdout, p.stdout + p.stderr
    p = run(dtype=L.capi.MSG_F8)
    assert p.returncode == 3 and "fp8" in p.stdout, p.stdout + p.stderr
