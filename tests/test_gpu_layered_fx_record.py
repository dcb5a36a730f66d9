"""Fixed-point layered min-sum on the record kernel (algo = layered_fx with tune fx_record, LDPC_TUNE_FX_RECORD) on the GPU
against tests/layered_fx_ref.py: a partial wave, exactly one wave, two waves with a ragged second one, no external column,
every column external, saturation and degenerate channel values, a posterior that outgrows 16 bits, a code the kernel
cannot serve, soft output, typed input, the host path, a device list, both pack modes, the refusals and Coder.

Every comparison is exact: bytes, iteration counts, all N hard bits, the posterior of the round each frame stopped in, R, P
and the bits after round TAP, soft values.  By kernel name, layered_ldsp_fx_kernel ran wherever it is expected."""
import functools
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, channel, codes

import fp16_cases as fc
import kernel_matrix as km
import layered_fx_cases as xc
import layered_fx_ref as FX
from ms_correction_ref import Code

pytestmark = pytest.mark.gpu

f32 = np.float32
LDPC_ERR_ARG, LDPC_ERR_UNSUPPORTED, LDPC_ERR_STATE = 1, 4, 5
RECORD = "layered_ldsp_fx_kernel["


def _decoder(c, B, max_iter, q, p, corrected=False, tune=None, **kw):
    scale, offset = xc.setting(corrected)
    kw.setdefault("llr_scale", xc.LLR_SCALE[q])
    return L.Decoder(L.Graph(c["rows"], c["cols"], c["M"], c["N"]), c["K"], max_batch=B, algo="layered_fx", msg_dtype="i8",
                     msg_bits=q, post_bits=p, max_iter=max_iter, layer_rows=c["z"], ms_scale=scale, ms_offset=offset,
                     tune=dict({"fx_record": True}, **(tune or {})), **kw)


def _names(dec):
    return [k["name"] for k in dec.kernel_times() if k["phase"] == 2]


def _compare(dec, y, want, what, max_iter, tap=xc.TAP, record=True):
    """A timed decode: bytes and iteration counts, and the name of its launch.  A decode tapped at the last round, which
    stops every frame where the plain one does: all N hard bits and the posterior of each frame's stop round.  A decode
    tapped at `tap`: R, P and bits of the frames that ran that round, the final bits of those that had stopped."""
    B = y.shape[0]
    dec.set_timing(True)
    out, iters = dec.decode(y)
    names = _names(dec)
    dec.set_timing(False)
    print(what, "rounds", np.bincount(want["iters"]).tolist(), names[:2])
    assert np.array_equal(iters, want["iters"]), ("iterations",) + what
    assert np.array_equal(out, want["out"]), ("bytes",) + what
    if record:
        assert len(names) == 1 and names[0].startswith(RECORD), (names,) + what
    dec.set_tap(max_iter)
    out2, iters2 = dec.decode(y)
    assert np.array_equal(out2, out) and np.array_equal(iters2, iters), ("second decode on the same rings",) + what
    assert np.array_equal(dec.dump(3, B).astype(np.uint8), want["hard"]), ("hard bits",) + what
    if record:                          # the streaming engine's P goes on after a frame has stopped
        assert np.array_equal(dec.dump(2, B), xc.as_float(want["post"])), ("posterior at the stop round",) + what
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


# ---- (a) the BG1-profile test code, z = 16: a partial wave, external columns, three persistent workgroups ---------------

@pytest.mark.parametrize("q,p", xc.WIDTHS)
def test_record_kernel_on_the_bg1_profile_test_code(built, q, p):
    """70 frames on a grid of 3 workgroups (each walks ~23 frames: P and the rings are refilled), row degrees 3 ... 19, plain
    and corrected."""
    c = xc.bg1_code()
    for corrected in (False, True):
        dec = _decoder(c, 70, xc.BG1_MAXIT, q, p, corrected, tune={"ldsp_grid": 3})
        names = _compare(dec, xc.bg1_inputs(70), xc.bg1_want(70, q, p, corrected), ("bg1", q, p, corrected), xc.BG1_MAXIT)
        assert names[0] == RECORD + "3x64,1]", names
        dec.close()


def test_record_kernel_without_early_termination_and_in_both_pack_modes(built):
    c = xc.bg1_code()
    want = xc.bg1_want(70, 6, 8, False, 0, False)
    assert (want["iters"] == xc.BG1_MAXIT).all()
    dec = _decoder(c, 70, xc.BG1_MAXIT, 6, 8, early_term=False, tune={"ldsp_grid": 3})
    dec.set_timing(True)
    out, iters = dec.decode(xc.bg1_inputs(70))
    assert _names(dec)[0].startswith(RECORD)
    assert np.array_equal(iters, want["iters"]) and np.array_equal(out, want["out"])
    dec.set_tap(xc.BG1_MAXIT)
    dec.decode(xc.bg1_inputs(70))
    assert np.array_equal(dec.dump(3, 70).astype(np.uint8), want["hard"])
    dec.close()
    w = xc.bg1_want(70, 6, 8, False)
    for mode in (L.capi.PACK_BYTES, L.capi.PACK_BITS):
        dec = _decoder(c, 70, xc.BG1_MAXIT, 6, 8, pack_mode=mode, tune={"ldsp_grid": 3})
        dec.set_timing(True)
        out, iters = dec.decode(xc.bg1_inputs(70))
        assert _names(dec)[0].startswith(RECORD), mode
        assert np.array_equal(iters, w["iters"]) and np.array_equal(out, c["code"].pack(w["hard"], mode)), mode
        dec.close()


# ---- (b), (c) BG1-profile codes at Z = 64 and Z = 80: one full wave; two waves, the second ragged -----------------------

PROFILE_FRAMES, PROFILE_MAXIT = 40, 8


@functools.lru_cache(maxsize=None)
def _profile(Z):
    rows, cols = codes.nr_bg1_profile_edges(Z=Z)
    M, N, K = 46 * Z, 68 * Z, 22 * Z
    y = fc.noisy_frames(N, PROFILE_FRAMES, 0.4, 1.3, seed=20261021 + Z)
    y.setflags(write=False)
    return dict(rows=rows, cols=cols, M=M, N=N, K=K, z=Z, code=Code(rows, cols, M, N, K), y=y)


@functools.lru_cache(maxsize=None)
def _profile_want(Z, q, p, corrected):
    c = _profile(Z)
    w = FX.layered_fx(c["code"], c["y"], Z, PROFILE_MAXIT, *xc.setting(corrected), q=q, p=p, llr_scale=xc.LLR_SCALE[q],
                      tap_iter=xc.TAP)
    assert np.unique(w["iters"]).size >= 3 and (w["iters"] >= xc.TAP).sum() >= 5
    return w


@pytest.mark.parametrize("q,p,corrected", [(6, 8, True), (8, 16, False)])
def test_record_kernel_on_exactly_one_wave(built, q, p, corrected):
    c = _profile(64)
    dec = _decoder(c, PROFILE_FRAMES, PROFILE_MAXIT, q, p, corrected)
    names = _compare(dec, c["y"], _profile_want(64, q, p, corrected), (64, q, p, corrected), PROFILE_MAXIT)
    assert names[0] == RECORD + "%dx64,1]" % PROFILE_FRAMES, names
    dec.close()


@pytest.mark.parametrize("q,p,corrected", [(6, 8, True), (8, 16, False)])
def test_record_kernel_on_two_waves_the_second_ragged(built, q, p, corrected):
    """Z = 80: the barrier between the waves, 16 rows in the second, 48 lanes that request spare records, the external
    posterior in the record, rows of 19 + 1 entries.  Once more with every column in LDS (ldsp_ext off), and with an idle
    third wave on two persistent workgroups."""
    c = _profile(80)
    want = _profile_want(80, q, p, corrected)
    for tune, shape in (({}, "%dx128,1]" % PROFILE_FRAMES), ({"ldsp_ext": False}, "%dx128,1]" % PROFILE_FRAMES),
                        ({"ldsp_waves": 3, "ldsp_per_cu": 1, "ldsp_grid": 2}, "2x192,1]")):
        dec = _decoder(c, PROFILE_FRAMES, PROFILE_MAXIT, q, p, corrected, tune=tune)
        names = _compare(dec, c["y"], want, (80, q, p, corrected, sorted(tune)), PROFILE_MAXIT)
        assert names[0] == RECORD + shape, names
        dec.close()


# ---- (d) WiMAX (2304, 1152): z = 96, no external column ---------------------------------------------------------------

def test_record_kernel_without_external_columns(built):
    rate, N = codes.RATE_1_2, 2304
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    c = dict(rows=rows, cols=cols, M=M, N=N, K=K, z=z)
    y = fc.noisy_frames(N, 40, 0.4, 1.3, seed=20261022)
    want = FX.layered_fx(Code(rows, cols, M, N, K), y, z, 10, q=6, p=8, llr_scale=xc.LLR_SCALE[6], tap_iter=xc.TAP)
    assert np.unique(want["iters"]).size >= 3
    dec = _decoder(c, 40, 10, 6, 8)
    names = _compare(dec, y, want, ("wimax2304",), 10)
    assert names[0] == RECORD + "40x128,1]", names
    dec.close()


# ---- (e) saturation and degenerate channel values ---------------------------------------------------------------------

@pytest.mark.parametrize("q,p", xc.SATURATION_WIDTHS)
def test_record_kernel_saturation_and_degenerate_channel_values(built, q, p):
    """zeros, +-L, L + 1, 1000, +-inf, NaN, the ties of sq, -0; with p = q = 4 the posterior sits at +-LP"""
    c = xc.saturation_code("wimax")
    y = xc.saturation_inputs("wimax", q)
    for corrected in (False, True):
        dec = _decoder(c, y.shape[0], xc.SATURATION_MAXIT["wimax"], q, p, corrected)
        _compare(dec, y, xc.saturation_want("wimax", q, p, corrected), ("saturation", q, p, corrected), xc.SATURATION_MAXIT["wimax"])
        dec.close()


# ---- (f) a posterior that outgrows 16 bits ---------------------------------------------------------------------------

def test_record_kernel_posterior_beyond_16_bits(built):
    """The star code: z = 1, 300 layers, 293 external columns.  The centre column's t + R passes 32767 in round 1: a wrapping
    int16 store in LDS would flip its sign."""
    c, y, w = xc.star_code(), xc.star_inputs(), xc.star_want()
    dec = _decoder(c, y.shape[0], 2, 8, 16)
    _compare(dec, y, w, ("star",), 2, tap=xc.STAR_TAP)
    dec.set_tap(xc.STAR_TAP)
    dec.decode(y)
    assert dec.dump(2, y.shape[0])[:2, 0].tolist() == [32767.0, -32767.0]
    dec.close()


# ---- (g) a code the record kernel cannot serve -----------------------------------------------------------------------

def test_a_code_that_does_not_fit_decodes_on_the_streaming_engine(built):
    """The irregular matrix code at layer_rows = 1: rows of up to 40 entries.  With fx_record on it runs the streaming
    layer kernels and gives xc.matrix_want; so does LDPC_PACK_BITS with a K that is no multiple of 8."""
    m = dict(xc.matrix(), z=1)
    rd, _ = km.degree_maps(m["rows"], m["cols"], m["M"], m["N"])
    for (q, p), corrected in zip(xc.WIDTHS, (True, False)):
        dec = _decoder(m, m["y"].shape[0], xc.MATRIX_MAXIT, q, p, corrected)
        names = _compare(dec, m["y"], xc.matrix_want(q, p, corrected), ("matrix", q, p, corrected), xc.MATRIX_MAXIT, record=False)
        assert set(names) == {"layer_kernel<lfx,%d,1>" % d for d in rd if d > 0}, sorted(names)
        dec.close()
    c = xc.bg1_code()
    k = dict(c, K=c["K"] - 3)
    code = Code(c["rows"], c["cols"], c["M"], c["N"], k["K"])
    w = xc.bg1_want(70, 6, 8, False)
    for mode, record in ((L.capi.PACK_BITS, False), (L.capi.PACK_BYTES, True)):
        dec = _decoder(k, 70, xc.BG1_MAXIT, 6, 8, pack_mode=mode)
        dec.set_timing(True)
        out, iters = dec.decode(xc.bg1_inputs(70))
        names = _names(dec)
        assert all(n.startswith(RECORD if record else "layer_kernel<lfx,") for n in names) and names, (mode, names)
        assert np.array_equal(iters, w["iters"]) and np.array_equal(out, code.pack(w["hard"], mode)), mode
        dec.close()


# ---- (h) soft output -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["posterior", "extrinsic"])
def test_record_kernel_soft_output(built, kind):
    """P of the stop round in LSBs, and that minus c = sq(llr_scale * y) -- not minus y; a plain call before and after"""
    c = xc.bg1_code()
    y, w = xc.bg1_inputs(70), xc.bg1_want(70, 6, 8, True)
    dec = _decoder(c, 70, xc.BG1_MAXIT, 6, 8, True, tune={"ldsp_grid": 3})
    before, _ = dec.decode(y)
    dec.set_timing(True)
    out, iters, soft = dec.decode(y, soft=kind)
    assert any(n.startswith(RECORD) for n in _names(dec))
    after, _ = dec.decode(y)
    assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"])
    assert np.array_equal(before, out) and np.array_equal(after, out)
    assert np.array_equal(soft, FX.soft_of(w, kind)), kind
    dec.close()


# ---- (i) typed input -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["i8", "f16"])
def test_record_kernel_typed_input(built, kind):
    c = xc.bg1_code()
    x, w = xc.typed_inputs(kind), xc.typed_want(kind, 6, 8)
    dec = _decoder(c, 70, xc.BG1_MAXIT, 6, 8, tune={"ldsp_grid": 3})
    dec.set_timing(True)
    out, iters = dec.decode(x, llr_unit=xc.TYPED_UNIT[kind])
    names = [k["name"] for k in dec.kernel_times()]
    assert "llr_widen_kernel" in names and any(n.startswith(RECORD) for n in names), names
    assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), kind
    out, iters, soft = dec.decode(x, soft="extrinsic", llr_unit=xc.TYPED_UNIT[kind])
    assert np.array_equal(out, w["out"]) and np.array_equal(soft, FX.soft_of(w, "extrinsic")), kind
    dec.close()


# ---- (j) the host path, device buffers, a device list ----------------------------------------------------------------

def test_record_kernel_host_path_device_buffers_and_device_list(built):
    """262 frames through ldpc_decode_soft with max_batch = 64 (four full launch groups and a ragged one) with guard bytes;
    ldpc_decode_device on torch buffers, two different batches in a row on the same handle; a device list of one device."""
    import torch
    c = xc.bg1_code()
    frames, guard = xc.BG1_TWO_TILES, 64
    y, w = xc.bg1_inputs(frames), xc.bg1_want(frames, 6, 8, False)
    lib = _lib.load()
    nb = L.out_bytes(c["K"], frames)
    dec = _decoder(c, 64, xc.BG1_MAXIT, 6, 8)
    out = np.full(nb + guard, 0xEE, np.uint8)
    iters = np.full(frames + guard, -7, np.int32)
    soft = np.full(frames * c["N"] + guard, -12345.0, np.float32)
    dec.set_timing(True)
    _lib.check(lib.ldpc_decode_soft(dec._h, y.ctypes.data, frames, out.ctypes.data, nb, iters.ctypes.data, soft.ctypes.data,
                                    frames * c["N"], L.capi.SOFT_KINDS["extrinsic"]))
    assert any(n.startswith(RECORD) for n in _names(dec))
    assert np.array_equal(iters[:frames], w["iters"]) and np.array_equal(out[:nb], w["out"])
    assert np.array_equal(soft[:frames * c["N"]].reshape(frames, -1), FX.soft_of(w, "extrinsic"))
    assert (out[nb:] == 0xEE).all() and (iters[frames:] == -7).all() and (soft[frames * c["N"]:] == np.float32(-12345.0)).all()
    assert dec.stats()["frames"] == frames
    dec.close()
    # device buffers: the 70-frame batch, then the first 70 of the 262-frame batch, then the first again
    dec = _decoder(c, 70, xc.BG1_MAXIT, 6, 8, tune={"ldsp_grid": 3})
    n70 = L.out_bytes(c["K"], 70)
    for ya, wa in ((xc.bg1_inputs(70), xc.bg1_want(70, 6, 8, False)), (y[:70], None), (xc.bg1_inputs(70), xc.bg1_want(70, 6, 8, False))):
        t_y = torch.from_numpy(np.array(ya, np.float32)).cuda()
        t_out = torch.full((n70 + guard,), 0xEE, dtype=torch.uint8, device="cuda")
        t_it = torch.full((70 + guard,), -7, dtype=torch.int32, device="cuda")
        dec.decode_device(t_y.data_ptr(), 70, t_out.data_ptr(), n70, t_it.data_ptr())
        torch.cuda.synchronize()
        o, i = t_out.cpu().numpy(), t_it.cpu().numpy()
        assert (o[n70:] == 0xEE).all() and (i[70:] == -7).all()
        if wa is None:
            assert np.array_equal(i[:70], w["iters"][:70]) and np.array_equal(o[:n70], w["out"][:n70])
        else:
            assert np.array_equal(i[:70], wa["iters"]) and np.array_equal(o[:n70], wa["out"])
    dec.close()
    multi = _decoder(c, 64, xc.BG1_MAXIT, 6, 8, devices=[0])
    out2, iters2 = multi.decode(y)
    assert np.array_equal(out2, w["out"]) and np.array_equal(iters2, w["iters"])
    multi.close()


# ---- refusals that need a device --------------------------------------------------------------------------------------

def test_record_kernel_refusals_with_a_device(built):
    """Soft output while a tap is set is LDPC_ERR_STATE, a dump without a tap LDPC_ERR_ARG, more frames than max_batch
    LDPC_ERR_ARG; refused creations (box-plus rows, a CRC) leave nothing behind: the decoder made right after them runs the
    record kernel and decodes as the reference says."""
    c = xc.bg1_code()
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    base = dict(msg_dtype="i8", msg_bits=6, post_bits=8, llr_scale=xc.LLR_SCALE[6], max_batch=70, max_iter=xc.BG1_MAXIT,
                layer_rows=c["z"], tune={"fx_record": True})
    for kw in (dict(algo="layered_bp_fx"), dict(algo="layered_fx", crc_kind=24, crc_bits=64),
               dict(algo="layered_fx", tune={"fx_record": True, "ldsp": True})):
        with pytest.raises(L.LdpcError) as e:
            L.Decoder(g, c["K"], **dict(base, **kw))
        assert e.value.code == LDPC_ERR_UNSUPPORTED, (kw, str(e.value))
    want = xc.bg1_want(70, 6, 8, False)
    dec = L.Decoder(g, c["K"], algo="layered_fx", **base)
    dec.set_timing(True)
    out, iters = dec.decode(xc.bg1_inputs(70))
    assert np.array_equal(iters, want["iters"]) and np.array_equal(out, want["out"])
    assert _names(dec)[0].startswith(RECORD)
    with pytest.raises(L.LdpcError) as e:
        dec.dump(2, 70)
    assert e.value.code == LDPC_ERR_ARG
    with pytest.raises(L.LdpcError) as e:
        dec.decode_device(1, 71, None, 0)                          # more frames than max_batch: refused before llr is read
    assert e.value.code == LDPC_ERR_ARG
    dec.set_tap(2)
    with pytest.raises(L.LdpcError) as e:
        dec.decode(xc.bg1_inputs(70), soft="posterior")
    assert e.value.code == LDPC_ERR_STATE
    dec.set_tap(0)
    out, iters = dec.decode(xc.bg1_inputs(70))
    assert np.array_equal(iters, want["iters"]) and np.array_equal(out, want["out"])
    dec.close()


# ---- (k) Coder --------------------------------------------------------------------------------------------------------

def test_coder_decode_layered_fixed_on_the_record_kernel(built, tmp_path):
    """Coder's DecodeLayeredFixed with setFixedRecordKernel(true): the bytes and soft values of the C ABI decoder with
    fx_record, of Coder without it, and of the reference."""
    from coder_layered_fx_record_harness import coder_layered_fx_record_exe
    exe = coder_layered_fx_record_exe(tmp_path)
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    g = L.Graph(rows, cols, M, N)
    frames, q, p, scale = 40, 6, 8, 8.0
    y = channel.awgn_frames(N, 0, frames, 0.8, seed=9)
    y.astype(np.float32).tofile(str(tmp_path / "in"))

    def run(kind, record):
        pr = subprocess.run([exe, str(int(rate)), str(N), str(frames), str(L.capi.MSG_I8), str(q), str(p), repr(scale), "0.75", "1.0",
                             str(kind), "1", "0.0", str(tmp_path / "in"), str(tmp_path / "out"), str(tmp_path / "soft"),
                             str(int(record))], capture_output=True, text=True)
        assert pr.returncode == 0, pr.stdout + pr.stderr
        got = np.fromfile(str(tmp_path / "out"), np.uint8)
        soft = np.fromfile(str(tmp_path / "soft"), np.float32).reshape(frames, N) if kind else None
        return got, soft

    w = FX.layered_fx(Code(rows, cols, M, N, K), y, z, 20, 0.75, 1.0, q=q, p=p, llr_scale=scale)
    assert np.unique(w["iters"]).size >= 2
    for kind_name, kind in ((None, 0), ("extrinsic", 2)):
        got, soft = run(kind, True)
        plain, plain_soft = run(kind, False)
        dec = L.Decoder(g, K, max_batch=frames, algo="layered_fx", msg_dtype="i8", msg_bits=q, post_bits=p, max_iter=20,
                        layer_rows=z, llr_scale=scale, ms_scale=0.75, ms_offset=1.0, poll_interval=4, tune={"fx_record": True})
        dec.set_timing(True)
        res = dec.decode(y, soft=kind_name)
        assert any(n.startswith(RECORD) for n in _names(dec))
        dec.close()
        assert np.array_equal(got, res[0][:got.size]) and np.array_equal(got, w["out"][:got.size]) and np.array_equal(got, plain), kind
        if kind:
            assert np.array_equal(soft, res[2]) and np.array_equal(soft, FX.soft_of(w, kind_name)) and np.array_equal(soft, plain_soft)
