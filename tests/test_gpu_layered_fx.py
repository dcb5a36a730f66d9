"""Fixed-point layered min-sum (algo = layered_fx) on the GPU against tests/layered_fx_ref.py: the BG1-profile test code at
every tile width, every degree class of the unrolled and the run-time kernel, the saturation overlay and degenerate
channel values, a posterior that outgrows 16 bits, early termination off, the CRC stop, soft output, int8 and fp16 input,
the host path and a device list, both pack modes, the refusals that need a device and Coder's DecodeLayeredFixed.

layered_fx is this repository's own definition (include/ldpc_hip.h: LDPC_ALGO_LAYERED_FX), so the expectation is the numpy
restatement in integers, which tests/test_layered_fx_cpu.py holds to the float layered min-sum where nothing saturates.
Every comparison is exact: bytes, iteration counts, all N hard bits, R, P and the bits after round TAP, soft values."""
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, channel, codes

import crc_term_cases as CC
import kernel_matrix as km
import layered_fx_cases as xc
import layered_fx_ref as FX
from ms_correction_ref import Code

pytestmark = pytest.mark.gpu

f32 = np.float32
LDPC_ERR_ARG, LDPC_ERR_UNSUPPORTED = 1, 4
UNROLLED = 24                       # kMaxUnrolledLayerDegree: wider rows take the run-time kernel


def _decoder(c, B, max_iter, V, q, p, corrected=False, **kw):
    scale, offset = xc.setting(corrected)
    kw.setdefault("llr_scale", xc.LLR_SCALE[q])
    return L.Decoder(L.Graph(c["rows"], c["cols"], c["M"], c["N"]), c["K"], max_batch=B, algo="layered_fx", msg_dtype="i8",
                     msg_bits=q, post_bits=p, max_iter=max_iter, frames_per_lane=V, layer_rows=c["z"], ms_scale=scale,
                     ms_offset=offset, **kw)


def _compare(dec, y, want, what, tap=xc.TAP):
    """One timed decode and one that stops at the tap: bytes, iteration counts and all N hard bits; R, P and the bits of
    the frames that ran round `tap` (the others' P and R evolve unread on the device, their bits are their final ones).
    Returns {kernel name: degree} of the layer launches of the timed decode."""
    B = y.shape[0]
    dec.set_timing(True)
    out, iters = dec.decode(y)
    names = {k["name"]: k["degree"] for k in dec.kernel_times() if k["phase"] == 2}
    dec.set_timing(False)
    assert np.array_equal(iters, want["iters"]), ("iterations",) + what
    assert np.array_equal(out, want["out"]), ("bytes",) + what
    assert np.array_equal(dec.dump(3, B).astype(np.uint8), want["hard"]), ("hard bits",) + what
    run = np.nonzero(want["iters"] >= tap)[0]
    early = np.nonzero(want["iters"] < tap)[0]
    assert run.size > 0, what
    dec.set_tap(tap)
    dec.decode(y)
    assert np.array_equal(dec.dump(0, B)[run], xc.as_float(want["r_tap"][run])), ("R tap",) + what
    assert np.array_equal(dec.dump(2, B)[run], xc.as_float(want["p_tap"][run])), ("P tap",) + what
    bits = dec.dump(3, B).astype(np.uint8)
    assert np.array_equal(bits[run], want["hard_tap"][run]), ("bit tap",) + what
    assert np.array_equal(bits[early], want["hard"][early]), ("bits of the frames that had stopped",) + what
    dec.set_tap(0)
    return names


@pytest.mark.parametrize("V", [1, 2, 4])
def test_layered_fx_on_the_bg1_profile_code(built, V):
    """N = 1088, z = 16, row degrees 3 ... 19; 70 frames of mixed noise (a ragged second tile at V = 1, a partial tile at
    V = 2 and 4), q = 6 / p = 8 (the posterior memory saturates) and q = 8 / p = 16, 12 rounds, plain and corrected; at
    V = 4 also 262 frames: a full tile and a ragged one.  By kernel name, the fixed-point instantiations ran."""
    c = xc.bg1_code()
    rd, _ = km.degree_maps(c["rows"], c["cols"], c["M"], c["N"])
    for frames in (70,) + ((xc.BG1_TWO_TILES,) if V == 4 else ()):
        for q, p in xc.WIDTHS:
            for corrected in (False, True):
                what = (V, frames, q, p, corrected)
                dec = _decoder(c, frames, xc.BG1_MAXIT, V, q, p, corrected)
                names = _compare(dec, xc.bg1_inputs(frames), xc.bg1_want(frames, q, p, corrected), what)
                assert set(names) == {"layer_kernel<lfx,%d,%d>" % (d, V) for d in rd if d > 0}, (what, sorted(names))
                dec.close()


def test_layered_fx_automatic_tile_width(built):
    """frames_per_lane = 0: four frames per lane from 256 frames on (a dword of R and a dwordx2 of P per lane), one below;
    the result does not depend on it."""
    c = xc.bg1_code()
    for frames, V in ((xc.BG1_TWO_TILES, 4), (70, 1)):
        dec = _decoder(c, frames, xc.BG1_MAXIT, 0, 6, 8)
        dec.set_timing(True)
        out, iters = dec.decode(xc.bg1_inputs(frames))
        w = xc.bg1_want(frames, 6, 8, False)
        assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"])
        names = [k["name"] for k in dec.kernel_times() if k["phase"] == 2]
        assert names and all(n.endswith(",%d>" % V) for n in names), (frames, names)
        dec.close()


@pytest.mark.parametrize("V", [1, 2, 4])
def test_layered_fx_every_degree_class(built, V):
    """The irregular matrix code with layer_rows = 1 -- every row a layer of its own: rows of degree 0, 1, 2, every unrolled
    degree up to 24, and 25 ... 33 and 40 for the run-time kernel -- 70 frames, 5 rounds.  The timing spans name a launch of
    every degree, so both the unrolled and the run-time kernel ran."""
    m = dict(xc.matrix(), z=1)
    rd, _ = km.degree_maps(m["rows"], m["cols"], m["M"], m["N"])
    for (q, p), corrected in zip(xc.WIDTHS, (True, False)):
        dec = _decoder(m, m["y"].shape[0], xc.MATRIX_MAXIT, V, q, p, corrected)
        names = _compare(dec, m["y"], xc.matrix_want(q, p, corrected), (V, q, p, corrected))
        assert set(names) == {"layer_kernel<lfx,%d,%d>" % (d, V) for d in rd if d > 0}, sorted(names)
        degrees = set(names.values())
        assert {1, 2, 3, UNROLLED} <= degrees and {UNROLLED + 1, 33, 40} <= degrees, sorted(degrees)
        dec.close()


@pytest.mark.parametrize("name", ["wimax", "ira"])
def test_layered_fx_saturation_and_degenerate_channel_values(built, name):
    """The overlay of fixed_cases.py -- zeros, +-L, L + 1, 1000, +-inf, NaN, the ties of sq, -0, a denormal and the frame of
    +-(L - 1) -- over AWGN frames at q = 4 / p = 4, q = 6 / p = 8 and q = 8 / p = 16: WiMAX (576, 288) layered by its
    circulant size, the staircase code with every row a layer.  |t| leaves [-L, L] and P sits at +-LP
    (tests/test_layered_fx_cpu.py asserts both on the reference)."""
    c = xc.saturation_code(name)
    for q, p in xc.SATURATION_WIDTHS:
        y = xc.saturation_inputs(name, q)
        for V in (1, 2, 4):
            corrected = V == 2
            dec = _decoder(c, y.shape[0], xc.SATURATION_MAXIT[name], V, q, p, corrected)
            _compare(dec, y, xc.saturation_want(name, q, p, corrected), (name, q, p, V))
            dec.close()


def test_layered_fx_posterior_beyond_16_bits(built):
    """The star code: one column in all 300 rows, every row a layer.  With every channel value at +127 (-127) the centre
    column's t + R passes 32767 in round 1 and the memory holds +-32767: a wrapping 16-bit store would flip its sign."""
    c, y, w = xc.star_code(), xc.star_inputs(), xc.star_want()
    for V in (1, 2, 4):
        dec = _decoder(c, y.shape[0], 2, V, 8, 16)
        _compare(dec, y, w, ("star", V), tap=xc.STAR_TAP)
        dec.set_tap(xc.STAR_TAP)
        dec.decode(y)
        assert dec.dump(2, y.shape[0])[:2, 0].tolist() == [32767.0, -32767.0], V
        dec.close()


def test_layered_fx_without_early_termination(built):
    """early_term = 0: every frame runs max_iter rounds and reports them, the bytes are the last round's."""
    c = xc.bg1_code()
    want = xc.bg1_want(70, 6, 8, False, 0, False)
    assert (want["iters"] == xc.BG1_MAXIT).all()
    for V in (1, 4):
        dec = _decoder(c, 70, xc.BG1_MAXIT, V, 6, 8, early_term=False)
        out, iters = dec.decode(xc.bg1_inputs(70))
        assert np.array_equal(iters, want["iters"]) and np.array_equal(out, want["out"]), V
        assert np.array_equal(dec.dump(3, 70).astype(np.uint8), want["hard"]), V
        dec.close()


def test_layered_fx_crc_stop(built):
    """bp_cases.crc_case's 150 frames: iteration counts, bytes and the number of frames the CRC stopped before their
    syndrome was clean, against the reference with the stop predicate."""
    kind, bits, y, w = xc.crc_case()
    assert w["by_stop"].size >= 1
    c = xc.bg1_code()
    q, p = xc.CRC_WIDTH
    for V in (1, 4):
        dec = _decoder(c, 150, CC.MAXIT, V, q, p, crc_kind=kind, crc_bits=bits)
        out, iters = dec.decode(y)
        assert np.array_equal(iters, w["iters"]), V
        assert np.array_equal(out, w["out"]), V
        assert dec.crc_stops() == w["by_stop"].size, (V, dec.crc_stops(), w["by_stop"].size)
        dec.close()


@pytest.mark.parametrize("kind", ["posterior", "extrinsic"])
def test_layered_fx_soft_output(built, kind):
    """P after the last layer of the stop round, in LSBs as floats, and that minus c = sq(llr_scale * y); V = 1, 2, 4; a
    frame that stops in round 1 and one that never stops are present; a plain call before and after the soft call gives
    the same bytes."""
    c = xc.bg1_code()
    y, w = xc.bg1_inputs(70), xc.bg1_want(70, 6, 8, True)
    assert (w["iters"] == 1).any() and (~c["code"].syndrome_ok(w["hard"])).any()
    for V in (1, 2, 4):
        dec = _decoder(c, 70, xc.BG1_MAXIT, V, 6, 8, True)
        before, _ = dec.decode(y)
        out, iters, soft = dec.decode(y, soft=kind)
        after, _ = dec.decode(y)
        assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), V
        assert np.array_equal(before, out) and np.array_equal(after, out), V
        assert np.array_equal(soft, FX.soft_of(w, kind)), (V, kind)
        dec.close()


@pytest.mark.parametrize("kind", ["i8", "f16"])
def test_layered_fx_typed_input(built, kind):
    """int8 (unit 1/8) and binary16 channel values through ldpc_decode_typed and ldpc_decode_soft_typed: y = x * unit, then
    the rule; the extrinsic value subtracts c formed from that y."""
    c = xc.bg1_code()
    x, w = xc.typed_inputs(kind), xc.typed_want(kind, 6, 8)
    for V in (1, 4):
        dec = _decoder(c, 70, xc.BG1_MAXIT, V, 6, 8)
        out, iters = dec.decode(x, llr_unit=xc.TYPED_UNIT[kind])
        assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), (kind, V)
        out, iters, soft = dec.decode(x, soft="extrinsic", llr_unit=xc.TYPED_UNIT[kind])
        assert np.array_equal(out, w["out"]) and np.array_equal(soft, FX.soft_of(w, "extrinsic")), (kind, V)
        dec.close()


def test_layered_fx_host_path_device_list_and_pack_modes(built):
    """262 frames through ldpc_decode_soft with max_batch = 64 (four full launch groups and a ragged one), and through a
    handle over the same ordinal twice: bytes, iteration counts and soft values of the reference; the guard bytes behind
    out / iters / soft untouched.  Then the same frames packed at bit offsets."""
    c = xc.bg1_code()
    frames, guard = xc.BG1_TWO_TILES, 64
    y, w = xc.bg1_inputs(frames), xc.bg1_want(frames, 6, 8, False)
    lib = _lib.load()
    nb = L.out_bytes(c["K"], frames)
    for V in (1, 4):
        dec = _decoder(c, 64, xc.BG1_MAXIT, V, 6, 8)
        out = np.full(nb + guard, 0xEE, np.uint8)
        iters = np.full(frames + guard, -7, np.int32)
        soft = np.full(frames * c["N"] + guard, -12345.0, np.float32)
        _lib.check(lib.ldpc_decode_soft(dec._h, y.ctypes.data, frames, out.ctypes.data, nb, iters.ctypes.data, soft.ctypes.data,
                                        frames * c["N"], L.capi.SOFT_KINDS["extrinsic"]))
        assert np.array_equal(iters[:frames], w["iters"]) and np.array_equal(out[:nb], w["out"]), V
        assert np.array_equal(soft[:frames * c["N"]].reshape(frames, -1), FX.soft_of(w, "extrinsic")), V
        assert (out[nb:] == 0xEE).all() and (iters[frames:] == -7).all() and (soft[frames * c["N"]:] == np.float32(-12345.0)).all(), V
        assert dec.stats()["frames"] == frames
        dec.close()
    multi = _decoder(c, 64, xc.BG1_MAXIT, 1, 6, 8, devices=[0, 0])
    out2, iters2 = multi.decode(y)
    assert np.array_equal(out2, w["out"]) and np.array_equal(iters2, w["iters"])
    multi.close()
    # bit offsets, with a K that is no multiple of 8
    k = dict(c, K=c["K"] - 3)
    code = Code(c["rows"], c["cols"], c["M"], c["N"], k["K"])
    for mode in (L.capi.PACK_BYTES, L.capi.PACK_BITS):
        dec = _decoder(k, 70, xc.BG1_MAXIT, 4, 6, 8, pack_mode=mode)
        out, iters = dec.decode(xc.bg1_inputs(70))
        w70 = xc.bg1_want(70, 6, 8, False)
        assert np.array_equal(iters, w70["iters"]) and np.array_equal(out, code.pack(w70["hard"], mode)), mode
        dec.close()


def test_layered_fx_refusals(built):
    """With the one-launch or the record kernels forced on, layered_fx is LDPC_ERR_UNSUPPORTED; a layering whose rows share
    a column is LDPC_ERR_ARG.  A refused creation leaves nothing behind: a decoder made right after it runs the fixed-point
    layer kernels and decodes as the reference says."""
    import torch
    c = xc.bg1_code()
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    base = dict(algo="layered_fx", msg_dtype="i8", msg_bits=6, post_bits=8, llr_scale=xc.LLR_SCALE[6])
    for tune in ({"fused": True}, {"ldsp": True}, {"fused": True, "ldsp": True}):
        with pytest.raises(L.LdpcError) as e:
            L.Decoder(g, c["K"], max_batch=64, max_iter=xc.BG1_MAXIT, layer_rows=c["z"], tune=tune, **base)
        assert e.value.code == LDPC_ERR_UNSUPPORTED, (tune, str(e.value))
        torch.cuda.synchronize()
    with pytest.raises(L.LdpcError) as e:                   # rows of a layer share a column
        L.Decoder(g, c["K"], max_batch=64, layer_rows=2 * c["z"], **base)
    assert e.value.code == LDPC_ERR_ARG
    with pytest.raises(L.LdpcError) as e:
        L.Decoder(g, c["K"], max_batch=64, layer_rows=c["z"], **dict(base, post_bits=5))
    assert e.value.code == LDPC_ERR_ARG
    want = xc.bg1_want(70, 6, 8, False)
    dec = L.Decoder(g, c["K"], max_batch=70, max_iter=xc.BG1_MAXIT, layer_rows=c["z"], **base)
    dec.set_timing(True)
    out, iters = dec.decode(xc.bg1_inputs(70))
    assert np.array_equal(iters, want["iters"]) and np.array_equal(out, want["out"])
    names = [k["name"] for k in dec.kernel_times() if k["phase"] == 2]
    assert names and all(n.startswith("layer_kernel<lfx,") for n in names), names
    dec.close()


def test_coder_decode_layered_fixed_equals_the_c_abi(built, tmp_path):
    """Coder's DecodeLayeredFixed with setMessageType(LDPC_MSG_I8, bits), setPosteriorBits, setLlrScale and
    setMinSumCorrection gives the bytes and the soft values (both kinds) of the C ABI decoder with algo = layered_fx and the
    Coder's circulant size -- and of the reference --, also over a device list and on int8 input; with another message type
    or a posterior narrower than a message addDecodeType fails as ldpc_decoder_create does."""
    from coder_layered_fx_harness import coder_layered_fx_exe
    exe = coder_layered_fx_exe(tmp_path)
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    g = L.Graph(rows, cols, M, N)
    frames, q, p, scale = 40, 6, 8, 8.0
    y = channel.awgn_frames(N, 0, frames, 0.8, seed=9)
    y.astype(np.float32).tofile(str(tmp_path / "in"))
    x8 = np.clip(np.rint(y * f32(8)), -127, 127).astype(np.int8)
    x8.tofile(str(tmp_path / "in8"))

    def run(dtype=L.capi.MSG_I8, bits=q, post=p, kind=0, ms_scale=0.75, ms_offset=1.0, ndev=1, unit=0.0):
        return subprocess.run([exe, str(int(rate)), str(N), str(frames), str(dtype), str(bits), str(post), repr(scale), repr(ms_scale),
                               repr(ms_offset), str(kind), str(ndev), repr(unit), str(tmp_path / ("in8" if unit else "in")),
                               str(tmp_path / "out"), str(tmp_path / "soft")], capture_output=True, text=True)

    code = Code(rows, cols, M, N, K)
    w = FX.layered_fx(code, y, z, 20, 0.75, 1.0, q=q, p=p, llr_scale=scale)
    w8 = FX.layered_fx(code, (x8.astype(f32) * f32(0.125)).astype(f32), z, 20, 0.75, 1.0, q=q, p=p, llr_scale=scale)
    assert np.unique(w["iters"]).size >= 2
    for kind_name, kind, ndev, unit in ((None, 0, 1, 0.0), ("posterior", 1, 1, 0.0), ("extrinsic", 2, 1, 0.0), (None, 0, 2, 0.0),
                                        ("extrinsic", 2, 1, 0.125)):
        pr = run(kind=kind, ndev=ndev, unit=unit)
        assert pr.returncode == 0, pr.stdout + pr.stderr
        got = np.fromfile(str(tmp_path / "out"), np.uint8)
        dec = L.Decoder(g, K, max_batch=frames, algo="layered_fx", msg_dtype="i8", msg_bits=q, post_bits=p, max_iter=20,
                        layer_rows=z, llr_scale=scale, ms_scale=0.75, ms_offset=1.0, poll_interval=4)
        res = dec.decode(x8, soft=kind_name, llr_unit=0.125) if unit else dec.decode(y, soft=kind_name)
        dec.close()
        ref = w8 if unit else w
        assert np.array_equal(got, res[0][:got.size]) and np.array_equal(got, ref["out"][:got.size]), (kind, ndev, unit)
        if kind:
            soft = np.fromfile(str(tmp_path / "soft"), np.float32).reshape(frames, N)
            assert np.array_equal(soft, res[2]) and np.array_equal(soft, FX.soft_of(ref, kind_name)), (kind_name, unit)
    pr = run(dtype=L.capi.MSG_F32, bits=0)
    assert pr.returncode == 3 and "LDPC_MSG_I8" in pr.stdout, pr.stdout + pr.stderr
    pr = run(post=5)
    assert pr.returncode == 3 and "post_bits" in pr.stdout, pr.stdout + pr.stderr
