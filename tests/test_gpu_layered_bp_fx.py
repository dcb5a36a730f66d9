"""Fixed-point layered box-plus (algo = layered_bp_fx) on the GPU against tests/layered_bp_fx_ref.py: the BG1-profile test
code at every tile width, every degree class of the unrolled and the run-time kernel, the saturation overlay, early
termination off, the CRC stop, soft output, int8 and fp16 input, the host path and a device list, both pack modes, the
refusals that need a device and Coder's DecodeLayeredBPFixed.

layered_bp_fx is this repository's own definition (include/ldpc_hip.h: LDPC_ALGO_LAYERED_BP_FX), so the expectation is the
numpy restatement in integers with the table the library hands out; tests/test_layered_bp_fx_cpu.py holds that restatement to
layered_fx's min-sum row where the table is zero and to examples by hand.  Every comparison is exact: bytes, iteration
counts, all N hard bits, R, P and the bits after round TAP, soft values."""
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, channel, codes

import crc_term_cases as CC
import kernel_matrix as km
import layered_bp_fx_cases as bx
import layered_bp_fx_ref as BX
from ms_correction_ref import Code

pytestmark = pytest.mark.gpu

f32 = np.float32
LDPC_ERR_ARG, LDPC_ERR_UNSUPPORTED = 1, 4
UNROLLED = 24                       # kMaxUnrolledLayerDegree: wider rows take the run-time kernel


def _decoder(c, B, max_iter, V, q, p, f, **kw):
    kw.setdefault("llr_scale", bx.LLR_SCALE[q])
    return L.Decoder(L.Graph(c["rows"], c["cols"], c["M"], c["N"]), c["K"], max_batch=B, algo="layered_bp_fx", msg_dtype="i8",
                     msg_bits=q, post_bits=p, bp_frac_bits=f, max_iter=max_iter, frames_per_lane=V, layer_rows=c["z"], **kw)


def _compare(dec, y, want, what, tap=bx.TAP):
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
    assert np.array_equal(dec.dump(0, B)[run], bx.as_float(want["r_tap"][run])), ("R tap",) + what
    assert np.array_equal(dec.dump(2, B)[run], bx.as_float(want["p_tap"][run])), ("P tap",) + what
    bits = dec.dump(3, B).astype(np.uint8)
    assert np.array_equal(bits[run], want["hard_tap"][run]), ("bit tap",) + what
    assert np.array_equal(bits[early], want["hard"][early]), ("bits of the frames that had stopped",) + what
    dec.set_tap(0)
    return names


@pytest.mark.parametrize("V", [1, 2, 4])
def test_layered_bp_fx_on_the_bg1_profile_code(built, V):
    """N = 1088, z = 16, row degrees 3 ... 19; 70 frames of mixed noise (a ragged second tile at V = 1, a partial tile at
    V = 2 and 4), q / p / f = 6 / 8 / 2 (the posterior memory saturates) and 8 / 16 / 4, 12 rounds; at V = 4 also 262 frames:
    a full tile and a ragged one.  By kernel name, the box-plus instantiations ran, one per row degree."""
    c = bx.bg1_code()
    rd, _ = km.degree_maps(c["rows"], c["cols"], c["M"], c["N"])
    for frames in (70,) + ((bx.BG1_TWO_TILES,) if V == 4 else ()):
        for q, p, f in bx.WIDTHS:
            what = (V, frames, q, p, f)
            dec = _decoder(c, frames, bx.BG1_MAXIT, V, q, p, f)
            names = _compare(dec, bx.bg1_inputs(frames), bx.bg1_want(frames, q, p, f), what)
            assert set(names) == {"layer_kernel<lbfx,%d,%d>" % (d, V) for d in rd if d > 0}, (what, sorted(names))
            assert all(int(n.split(",")[1]) == d for n, d in names.items()), names
            dec.close()


def test_layered_bp_fx_automatic_tile_width_and_bytes(built):
    """frames_per_lane = 0 is layered_fx's choice: four frames per lane from 256 frames on, one below; the result does not
    depend on it.  The timing hook counts 6 bytes per edge and frame-round."""
    c = bx.bg1_code()
    for frames, V in ((bx.BG1_TWO_TILES, 4), (70, 1)):
        dec = _decoder(c, frames, bx.BG1_MAXIT, 0, 6, 8, 2, early_term=False)
        dec.set_timing(True)
        out, iters = dec.decode(bx.bg1_inputs(frames))
        w = bx.bg1_want(frames, 6, 8, 2, 0, False)
        assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"])
        times = [k for k in dec.kernel_times() if k["phase"] == 2]
        assert times and all(k["name"].endswith(",%d>" % V) for k in times), (frames, times)
        assert sum(k["bytes_total"] for k in times) == 6 * c["code"].E * frames * bx.BG1_MAXIT, frames
        dec.close()


@pytest.mark.parametrize("V", [1, 2, 4])
def test_layered_bp_fx_every_degree_class(built, V):
    """The irregular matrix code with layer_rows = 1 -- every row a layer of its own: rows of degree 0, 1, 2, every unrolled
    degree up to 24, and 25 ... 33 and 40 for the run-time kernel -- 70 frames, 5 rounds.  The timing spans name a launch of
    every degree, so both the unrolled and the run-time kernel ran."""
    m = dict(bx.matrix(), z=1)
    rd, _ = km.degree_maps(m["rows"], m["cols"], m["M"], m["N"])
    for q, p, f in bx.WIDTHS:
        dec = _decoder(m, m["y"].shape[0], bx.MATRIX_MAXIT, V, q, p, f)
        names = _compare(dec, m["y"], bx.matrix_want(q, p, f), (V, q, p, f))
        assert set(names) == {"layer_kernel<lbfx,%d,%d>" % (d, V) for d in rd if d > 0}, sorted(names)
        degrees = set(names.values())
        assert set(range(1, UNROLLED + 1)) <= degrees and {UNROLLED + 1, 33, 40} <= degrees, sorted(degrees)
        dec.close()


def test_layered_bp_fx_saturation_and_degenerate_channel_values(built):
    """The overlay of fixed_cases.py -- zeros, +-L, L + 1, 1000, +-inf, NaN, the ties of sq, -0, a denormal and the frame of
    +-(L - 1) -- over AWGN frames on WiMAX (576, 288) at q / p / f = 4 / 4 / 0, 6 / 8 / 2 and 8 / 16 / 3.  |t| leaves
    [-L, L], P sits at +-LP and box-plus results are 0 from non-zero inputs (tests/test_layered_bp_fx_cpu.py asserts all
    three on the reference)."""
    c = bx.saturation_code()
    for q, p, f in bx.SATURATION_WIDTHS:
        y = bx.saturation_inputs(q)
        for V in (1, 2, 4):
            dec = _decoder(c, y.shape[0], bx.SATURATION_MAXIT, V, q, p, f)
            _compare(dec, y, bx.saturation_want(q, p, f), (q, p, f, V))
            dec.close()


def test_layered_bp_fx_without_early_termination(built):
    """early_term = 0: every frame runs max_iter rounds and reports them, the bytes are the last round's."""
    c = bx.bg1_code()
    want = bx.bg1_want(70, 6, 8, 2, 0, False)
    assert (want["iters"] == bx.BG1_MAXIT).all()
    for V in (1, 4):
        dec = _decoder(c, 70, bx.BG1_MAXIT, V, 6, 8, 2, early_term=False)
        out, iters = dec.decode(bx.bg1_inputs(70))
        assert np.array_equal(iters, want["iters"]) and np.array_equal(out, want["out"]), V
        assert np.array_equal(dec.dump(3, 70).astype(np.uint8), want["hard"]), V
        dec.close()


def test_layered_bp_fx_crc_stop(built):
    """bp_cases.crc_case's 150 frames: iteration counts, bytes and the number of frames the CRC stopped before their
    syndrome was clean, against the reference with the stop predicate."""
    kind, bits, y, w = bx.crc_case()
    assert w["by_stop"].size >= 1
    c = bx.bg1_code()
    q, p, f = bx.CRC_WIDTH
    for V in (1, 4):
        dec = _decoder(c, 150, CC.MAXIT, V, q, p, f, crc_kind=kind, crc_bits=bits)
        out, iters = dec.decode(y)
        assert np.array_equal(iters, w["iters"]), V
        assert np.array_equal(out, w["out"]), V
        assert dec.crc_stops() == w["by_stop"].size, (V, dec.crc_stops(), w["by_stop"].size)
        dec.close()


@pytest.mark.parametrize("kind", ["posterior", "extrinsic"])
def test_layered_bp_fx_soft_output(built, kind):
    """P after the last layer of the stop round, in LSBs as floats, and that minus c = sq(llr_scale * y); V = 1, 2, 4; a
    frame that stops in round 1 and one that never stops are present; a plain call before and after the soft call gives
    the same bytes."""
    c = bx.bg1_code()
    y, w = bx.bg1_inputs(70), bx.bg1_want(70, 6, 8, 2)
    assert (w["iters"] == 1).any() and (~c["code"].syndrome_ok(w["hard"])).any()
    for V in (1, 2, 4):
        dec = _decoder(c, 70, bx.BG1_MAXIT, V, 6, 8, 2)
        before, _ = dec.decode(y)
        out, iters, soft = dec.decode(y, soft=kind)
        after, _ = dec.decode(y)
        assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), V
        assert np.array_equal(before, out) and np.array_equal(after, out), V
        assert np.array_equal(soft, BX.soft_of(w, kind)), (V, kind)
        dec.close()


@pytest.mark.parametrize("kind", ["i8", "f16"])
def test_layered_bp_fx_typed_input(built, kind):
    """int8 (unit 1/8) and binary16 channel values through ldpc_decode_typed and ldpc_decode_soft_typed: y = x * unit, then
    the rule; the extrinsic value subtracts c formed from that y."""
    c = bx.bg1_code()
    x, w = bx.typed_inputs(kind), bx.typed_want(kind, 6, 8, 2)
    for V in (1, 4):
        dec = _decoder(c, 70, bx.BG1_MAXIT, V, 6, 8, 2)
        out, iters = dec.decode(x, llr_unit=bx.TYPED_UNIT[kind])
        assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), (kind, V)
        out, iters, soft = dec.decode(x, soft="extrinsic", llr_unit=bx.TYPED_UNIT[kind])
        assert np.array_equal(out, w["out"]) and np.array_equal(soft, BX.soft_of(w, "extrinsic")), (kind, V)
        dec.close()


def test_layered_bp_fx_host_path_device_list_and_pack_modes(built):
    """262 frames through ldpc_decode_soft with max_batch = 64 (four full launch groups and a ragged one), and through a
    handle over the same ordinal twice: bytes, iteration counts and soft values of the reference; the guard bytes behind
    out / iters / soft untouched.  Then the same frames packed at bit offsets."""
    c = bx.bg1_code()
    frames, guard = bx.BG1_TWO_TILES, 64
    y, w = bx.bg1_inputs(frames), bx.bg1_want(frames, 6, 8, 2)
    lib = _lib.load()
    nb = L.out_bytes(c["K"], frames)
    for V in (1, 4):
        dec = _decoder(c, 64, bx.BG1_MAXIT, V, 6, 8, 2)
        out = np.full(nb + guard, 0xEE, np.uint8)
        iters = np.full(frames + guard, -7, np.int32)
        soft = np.full(frames * c["N"] + guard, -12345.0, np.float32)
        _lib.check(lib.ldpc_decode_soft(dec._h, y.ctypes.data, frames, out.ctypes.data, nb, iters.ctypes.data, soft.ctypes.data,
                                        frames * c["N"], L.capi.SOFT_KINDS["extrinsic"]))
        assert np.array_equal(iters[:frames], w["iters"]) and np.array_equal(out[:nb], w["out"]), V
        assert np.array_equal(soft[:frames * c["N"]].reshape(frames, -1), BX.soft_of(w, "extrinsic")), V
        assert (out[nb:] == 0xEE).all() and (iters[frames:] == -7).all() and (soft[frames * c["N"]:] == np.float32(-12345.0)).all(), V
        assert dec.stats()["frames"] == frames
        dec.close()
    multi = _decoder(c, 64, bx.BG1_MAXIT, 1, 6, 8, 2, devices=[0, 0])
    out2, iters2 = multi.decode(y)
    assert np.array_equal(out2, w["out"]) and np.array_equal(iters2, w["iters"])
    multi.close()
    # bit offsets, with a K that is no multiple of 8
    k = dict(c, K=c["K"] - 3)
    code = Code(c["rows"], c["cols"], c["M"], c["N"], k["K"])
    for mode in (L.capi.PACK_BYTES, L.capi.PACK_BITS):
        dec = _decoder(k, 70, bx.BG1_MAXIT, 4, 6, 8, 2, pack_mode=mode)
        out, iters = dec.decode(bx.bg1_inputs(70))
        w70 = bx.bg1_want(70, 6, 8, 2)
        assert np.array_equal(iters, w70["iters"]) and np.array_equal(out, code.pack(w70["hard"], mode)), mode
        dec.close()


def test_layered_bp_fx_refusals(built):
    """With the one-launch or the record kernels forced on, or a min-sum correction, layered_bp_fx is LDPC_ERR_UNSUPPORTED; a
    layering whose rows share a column and a bp_frac_bits of 5 are LDPC_ERR_ARG.  A refused creation leaves nothing behind:
    a decoder made right after it runs the box-plus layer kernels and decodes as the reference says."""
    import torch
    c = bx.bg1_code()
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    base = dict(algo="layered_bp_fx", msg_dtype="i8", msg_bits=6, post_bits=8, bp_frac_bits=2, llr_scale=bx.LLR_SCALE[6])
    for extra in (dict(tune={"fused": True}), dict(tune={"ldsp": True}), dict(tune={"fused": True, "ldsp": True}),
                  dict(ms_scale=0.75), dict(ms_offset=1.0)):
        with pytest.raises(L.LdpcError) as e:
            L.Decoder(g, c["K"], max_batch=64, max_iter=bx.BG1_MAXIT, layer_rows=c["z"], **base, **extra)
        assert e.value.code == LDPC_ERR_UNSUPPORTED, (extra, str(e.value))
        torch.cuda.synchronize()
    with pytest.raises(L.LdpcError) as e:                   # rows of a layer share a column
        L.Decoder(g, c["K"], max_batch=64, layer_rows=2 * c["z"], **base)
    assert e.value.code == LDPC_ERR_ARG
    with pytest.raises(L.LdpcError) as e:
        L.Decoder(g, c["K"], max_batch=64, layer_rows=c["z"], **dict(base, bp_frac_bits=5))
    assert e.value.code == LDPC_ERR_ARG
    want = bx.bg1_want(70, 6, 8, 2)
    dec = L.Decoder(g, c["K"], max_batch=70, max_iter=bx.BG1_MAXIT, layer_rows=c["z"], **base)
    dec.set_timing(True)
    out, iters = dec.decode(bx.bg1_inputs(70))
    assert np.array_equal(iters, want["iters"]) and np.array_equal(out, want["out"])
    names = [k["name"] for k in dec.kernel_times() if k["phase"] == 2]
    assert names and all(n.startswith("layer_kernel<lbfx,") for n in names), names
    dec.close()


def test_coder_decode_layered_bp_fixed_equals_the_c_abi(built, tmp_path):
    """Coder's DecodeLayeredBPFixed with setMessageType(LDPC_MSG_I8, bits), setPosteriorBits, setLlrFractionBits and
    setLlrScale gives the bytes and the soft values (both kinds) of the C ABI decoder with algo = layered_bp_fx and the Coder's
    circulant size -- and of the reference --, also over a device list and on int8 input; with another message type, a
    fraction width out of range or a min-sum correction addDecodeType fails as ldpc_decoder_create does."""
    from coder_layered_bp_fx_harness import coder_layered_bp_fx_exe
    exe = coder_layered_bp_fx_exe(tmp_path)
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    g = L.Graph(rows, cols, M, N)
    frames, q, p, f, scale = 40, 5, 7, 1, 4.0
    y = channel.awgn_frames(N, 0, frames, 0.8, seed=9)
    y.astype(np.float32).tofile(str(tmp_path / "in"))
    x8 = np.clip(np.rint(y * f32(8)), -127, 127).astype(np.int8)
    x8.tofile(str(tmp_path / "in8"))

    def run(dtype=L.capi.MSG_I8, bits=q, post=p, frac=f, kind=0, ms_scale=0.0, ms_offset=0.0, ndev=1, unit=0.0):
        return subprocess.run([exe, str(int(rate)), str(N), str(frames), str(dtype), str(bits), str(post), repr(scale), repr(ms_scale),
                               repr(ms_offset), str(kind), str(ndev), repr(unit), str(tmp_path / ("in8" if unit else "in")),
                               str(tmp_path / "out"), str(tmp_path / "soft"), str(frac)], capture_output=True, text=True)

    code = Code(rows, cols, M, N, K)
    w = BX.layered_bp_fx(code, y, z, 20, bx.table(f), q=q, p=p, llr_scale=scale)
    w8 = BX.layered_bp_fx(code, (x8.astype(f32) * f32(0.125)).astype(f32), z, 20, bx.table(f), q=q, p=p, llr_scale=scale)
    assert np.unique(w["iters"]).size >= 2
    for kind_name, kind, ndev, unit in ((None, 0, 1, 0.0), ("posterior", 1, 1, 0.0), ("extrinsic", 2, 1, 0.0), (None, 0, 2, 0.0),
                                        ("extrinsic", 2, 1, 0.125)):
        pr = run(kind=kind, ndev=ndev, unit=unit)
        assert pr.returncode == 0, pr.stdout + pr.stderr
        got = np.fromfile(str(tmp_path / "out"), np.uint8)
        dec = L.Decoder(g, K, max_batch=frames, algo="layered_bp_fx", msg_dtype="i8", msg_bits=q, post_bits=p, bp_frac_bits=f,
                        max_iter=20, layer_rows=z, llr_scale=scale, poll_interval=4)
        res = dec.decode(x8, soft=kind_name, llr_unit=0.125) if unit else dec.decode(y, soft=kind_name)
        dec.close()
        ref = w8 if unit else w
        assert np.array_equal(got, res[0][:got.size]) and np.array_equal(got, ref["out"][:got.size]), (kind, ndev, unit)
        if kind:
            soft = np.fromfile(str(tmp_path / "soft"), np.float32).reshape(frames, N)
            assert np.array_equal(soft, res[2]) and np.array_equal(soft, BX.soft_of(ref, kind_name)), (kind_name, unit)
    pr = run(dtype=L.capi.MSG_F32, bits=0)
    assert pr.returncode == 3 and "LDPC_MSG_I8" in pr.stdout, pr.stdout + pr.stderr
    pr = run(frac=5)
    assert pr.returncode == 3 and "bp_frac_bits" in pr.stdout, pr.stdout + pr.stderr
    pr = run(ms_scale=0.75)
    assert pr.returncode == 3 and "ms_scale" in pr.stdout, pr.stdout + pr.stderr
