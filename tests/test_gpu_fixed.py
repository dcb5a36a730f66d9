"""Fixed-point messages (msg_dtype = i8, msg_bits = 4, 5, 6, 8) on the GPU against tests/fixed_ref.py: the conversion,
every form of the column-fused check kernels, degenerate channel values, typed input, both hand-overs, soft output, the CRC
stop, the host path, a device list, early termination off, the refusals and Coder::setMessageType.

LDPC_MSG_I8 is this repository's own definition (include/ldpc_hip.h), so the expectation is the integer restatement, which
tests/test_fixed_cpu.py holds to the oracle where nothing saturates.  Everything is compared exactly: bytes, iteration
counts, all N hard bits, the check->variable and the variable->check messages after two rounds, soft values.  The Q tap is
what sees a column-fused kernel that forgets MsgRound in a register (test_fixed_cpu.py)."""
import ctypes
import functools
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, channel, codes

import crc_term_cases as CC
import crc_term_ref as CR
import fp16_cases as fc
import fixed_cases as fxc
import fixed_ref as RI
import ratematch_util as U
from ms_correction_ref import Code
from test_gpu_kernel_matrix import LINK_FORMS

pytestmark = pytest.mark.gpu

FORMS = dict(LINK_FORMS, guided={"link_guided": True})
LINK_KERNELS = {"wide": "check_link_kernel", "narrow": "check_link_narrow_kernel", "half": "check_link_half_kernel"}
LDPC_ERR_ARG, LDPC_ERR_UNSUPPORTED = 1, 4


def _arith(q, setting):
    return "%s%d" % ("msci" if setting is not None else "msi", q)


def _decoder(c, q, setting, B, max_iter, V, llr_scale=None, **kw):
    scale, offset = setting or (0.0, 0.0)
    return L.Decoder(L.Graph(c["rows"], c["cols"], c["M"], c["N"]), c["K"], max_batch=B, algo="ms", msg_dtype="i8", msg_bits=q,
                     llr_scale=fxc.LLR_SCALE[q] if llr_scale is None else llr_scale, max_iter=max_iter, frames_per_lane=V,
                     ms_scale=scale, ms_offset=offset, **kw)


def _same(got, ref):
    """the library's float32 report of messages against the reference's int32"""
    return bool(np.array_equal(np.ascontiguousarray(got, np.float32).view(np.uint32), fxc.as_float(ref).view(np.uint32)))


def _compare(dec, y, want, what, rows=None):
    """One timed decode and one that stops at the tap: bytes, iteration counts, all N hard bits, R on the frames that
    reached round TAP, Q on those that went on.  rows: the reference's frame of every frame of y (a batch that repeats the
    case's frames).  Returns the names of the check-phase kernels of the timed decode."""
    B = y.shape[0]
    rows = np.arange(B) if rows is None else rows
    dec.set_timing(True)
    out, iters = dec.decode(y)
    phase0 = {k["name"] for k in dec.kernel_times() if k["phase"] == 0 and k["name"] != "other"}
    dec.set_timing(False)
    assert np.array_equal(iters, want["iters"][rows]), ("iterations",) + what
    if rows.size == want["iters"].size:
        assert np.array_equal(out, want["out"]), ("bytes",) + what
    assert np.array_equal(dec.dump(3, B).astype(np.uint8), want["hard"][rows]), ("hard bits",) + what
    run_r, run_q = fc.tap_frames(want["iters"][rows])
    assert run_q.size > 0, what
    dec.set_tap(fc.TAP)
    dec.decode(y)
    assert _same(dec.dump(0, B)[run_r], want["r_tap"][rows][run_r]), ("R tap",) + what
    assert _same(dec.dump(1, B)[run_q], want["q_tap"][rows][run_q]), ("Q tap",) + what
    dec.set_tap(0)
    return phase0


def _expected_link_kernel(dec, tune, V):
    """The form the tuning fixes (deep is a narrow form; half has kernels for V = 4 only and falls back to narrow below).
    Where it fixes none, one-byte messages take the wide form at V = 1 and the one timed fastest at creation above, where
    the narrow form -- one byte per lane -- is no candidate."""
    if tune.get("link_half"):
        return LINK_KERNELS["half" if V == 4 else "narrow"]
    if "link_narrow" in tune:
        return LINK_KERNELS["narrow" if tune["link_narrow"] else "wide"]
    if tune.get("link_deep"):
        return LINK_KERNELS["narrow"]
    if V == 1:
        return LINK_KERNELS["wide"]
    lf = dec.link_form()
    assert lf["chosen_by_measurement"] and lf["form"] in (("wide", "half") if V == 4 else ("wide",)), lf
    return LINK_KERNELS[lf["form"]]


@pytest.mark.parametrize("q", [4, 8])
def test_fixed_conversion_is_sq(built, q):
    """Frames filled with every integer around [-L, L], every half-integer tie and its fp32 neighbours, L + 0.49, L + 0.5,
    1000, infinities, NaN, -0, a denormal, 128, 255, 256: after a decode of one round the stored channel values and the Q
    array (round 1 reads c as Q; one round stores no other) are sq(y) exactly, at 1, 2 and 4 frames per lane; with
    llr_scale 0.5 they are sq(0.5 * y)."""
    c = fc.wimax()
    y = fxc.conversion_inputs(c["N"], fc.DEGENERATE_FRAMES, q)
    assert y.size >= RI.edge_inputs(q).size
    for llr_scale in (1.0, 0.5):
        stored = RI.channel_values(y, llr_scale, q)
        for V in (1, 2, 4):
            dec = _decoder(c, q, None, y.shape[0], 1, V, llr_scale=llr_scale)
            dec.set_tap(1)
            dec.decode(y)
            assert _same(dec.dump(2, y.shape[0]), stored), (q, llr_scale, V)
            assert _same(dec.dump(1, y.shape[0]), stored[:, c["cols"]]), (q, llr_scale, V)
            dec.close()


@pytest.mark.parametrize("corrected", [False, True], ids=["msi", "msci"])
@pytest.mark.parametrize("d,q", fxc.FUSED_CASES)
def test_fixed_column_fused_forms(built, d, q, corrected):
    """Staircase codes with the linked class at degree d, q-bit messages, plain and corrected min-sum: every form of the
    column-fused check kernel at V = 1, 2, 4 (133 frames: a ragged last tile) with the unlinked rows riding along in its
    launch, the fusion off, and 300 frames at V = 4 (two tiles).  By kernel name, the instantiation of this width and of the
    expected form ran."""
    c = fc.staircase(d, "ride")
    n = 0
    for form, tune in list(FORMS.items()) + [("unfused", {"link_rows": -1})]:
        for V in (1, 2, 4):
            n += 1
            setting = fc.SETTINGS[n % 3] if corrected else None
            arith = _arith(q, setting)
            what = (d, arith, setting, form, V)
            dec = _decoder(c, q, setting, fc.FRAMES, fc.MAXIT, V, tune=tune)
            phase0 = _compare(dec, c["y"], fxc.want(d, q, "ride", setting), what)
            link = {k for k in phase0 if k.startswith("check_link")}
            if form == "unfused":
                assert not link and phase0 and all("<%s," % arith in k for k in phase0), (what, phase0)
            else:
                assert link == {"%s<%s,%d,%d>" % (_expected_link_kernel(dec, tune, V), arith, d, V)}, (what, phase0)
                assert phase0 == link, (what, phase0)
            dec.close()
    setting = fc.SETTINGS[0] if corrected else None
    rows = np.arange(fxc.TWO_TILES) % fc.FRAMES
    y = np.ascontiguousarray(c["y"][rows])
    dec = _decoder(c, q, setting, fxc.TWO_TILES, fc.MAXIT, 4)
    _compare(dec, y, fxc.want(d, q, "ride", setting), (d, q, setting, "two tiles"), rows)
    dec.close()


@pytest.mark.parametrize("corrected", [False, True], ids=["msi", "msci"])
@pytest.mark.parametrize("q", [6, 8])
@pytest.mark.parametrize("name", ["wimax", "ira"])
def test_fixed_degenerate_channel_values(built, name, q, corrected):
    """Zeros, a zero frame, +-L, L + 1, 1000, infinities, NaN, the ties, L + 0.49 / L + 0.5, -0, an fp32 denormal, and a
    frame of +-(L - 1) whose P - R leaves the range after round 1 (at q = 8 beyond 255): the stored channel values are sq of
    the input and everything derived from them is what the definition makes of them.  WiMAX 960 runs the check kernels in
    wide waves (the automatic choice for one-byte messages) and in narrow ones, the staircase code the column-fused kernel."""
    c, y = fc.degenerate_code(name), fxc.degenerate_inputs(name, q)
    B = y.shape[0]
    setting = fc.DEGENERATE_SETTING if corrected else None
    arith = _arith(q, setting)
    want = fxc.degenerate_want(name, q, corrected)
    for V in (1, 2, 4):
        for tune in ({}, {"check_wide": False}):
            what = (name, arith, V, str(tune))
            dec = _decoder(c, q, setting, B, fc.DEGENERATE_MAXIT, V, tune=tune)
            phase0 = _compare(dec, y, want, what)
            assert phase0 and all("<%s," % arith in k for k in phase0), (what, phase0)
            if name == "ira":
                assert any(k.startswith("check_link") for k in phase0), (what, phase0)
            assert _same(dec.dump(2, B), want["c"]), ("channel values",) + what
            dec.close()


def test_fixed_typed_input(built):
    """int8 channel values with llr_unit 1 and llr_scale 1 go straight through; fp16 values with llr_scale 4: both equal the
    reference -- and the float path of the library -- on the widened values, at q = 6, through the init kernels of every
    input type (rows of 960 values: the 16-byte loads; 133 frames at V = 1, 2, 4)."""
    c = fc.staircase(7, "ride")
    q = 6
    rng = np.random.default_rng(3)
    x8 = np.clip(np.rint(c["y"] * np.float32(8)), -128, 127).astype(np.int8)
    x8[0, rng.choice(c["N"], 30, replace=False)] = -128
    x16 = c["y"].astype(np.float16)
    for x, unit, llr_scale in ((x8, 1.0, 1.0), (x16, 1.0, 4.0), (x8, 0.125, 8.0)):
        wide = (x.astype(np.float32) * np.float32(unit)).astype(np.float32)
        want = RI.flood(c["code"], wide, fc.MAXIT, q=q, llr_scale=llr_scale)
        assert np.unique(want["iters"]).size >= 3
        for V in (1, 2, 4):
            dec = _decoder(c, q, None, fc.FRAMES, fc.MAXIT, V, llr_scale=llr_scale)
            out, iters = dec.decode(x, llr_unit=unit)
            assert np.array_equal(iters, want["iters"]) and np.array_equal(out, want["out"]), (x.dtype, unit, V)
            assert _same(dec.dump(2, fc.FRAMES), want["c"]), (x.dtype, unit, V)
            out2, iters2 = dec.decode(wide)
            assert np.array_equal(iters2, iters) and np.array_equal(out2, out), (x.dtype, unit, V)
            dec.close()


def _stats_ok(dec, want, what):
    st = dec.stats()
    assert st["frames_converged"] == want["n_conv"], (what, st)
    assert st["iterations_launched"] == fc.HANDOVER_MAXIT, (what, st)
    return st


def test_fixed_hand_over_on_a_staircase_code(built):
    """6-bit messages on the d = 7 staircase code with 90 scattered stragglers: the host-polled hand-over to child decoders
    (the row-wise gather at 512, the per-element gather at 7, off) and the device-side tail, two calls per decoder."""
    import torch
    c = fc.staircase(7, "ride")
    q = fxc.HANDOVER_Q
    B = fc.HANDOVER_BATCHES[0]
    y = fc.handover_inputs(B)
    runs = [(None, compact, V) for compact in (512, 7, -1) for V in (1, 4)] + [(fc.SETTINGS[0], 0, 4)]
    for setting, compact, V in runs:
        want = fxc.handover_want(B, setting)
        dec = _decoder(c, q, setting, B, fc.HANDOVER_MAXIT, V, poll_interval=1, tune={"compact": compact} if compact else {})
        for call in range(2):
            what = ("polled", setting, compact, V, call)
            out, iters = dec.decode(y)
            assert np.array_equal(iters, want["iters"]), what
            assert np.array_equal(out, want["out"]), what
            _stats_ok(dec, want, what)
        dec.close()
    B = fc.HANDOVER_BATCHES[1]
    y, want = fc.handover_inputs(B), fxc.handover_want(B)
    yd = torch.from_numpy(y.copy()).cuda()
    nb = L.out_bytes(c["K"], B)
    for tune in ({}, {"compact": 100}, {"device_tail": False}):
        for V in (1, 4):
            dec = _decoder(c, q, None, B, fc.HANDOVER_MAXIT, V, poll_interval=0, tune=tune)
            for call in range(2):
                what = ("device", tune, V, call)
                out = torch.full((nb,), 0xEE, dtype=torch.uint8, device="cuda")
                it = torch.zeros(B, dtype=torch.int32, device="cuda")
                dec.decode_device(yd.data_ptr(), B, out.data_ptr(), nb, it.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert np.array_equal(it.cpu().numpy(), want["iters"]), what
                assert np.array_equal(out.cpu().numpy(), want["out"]), what
                assert _stats_ok(dec, want, what)["batch_time"] == fc.HANDOVER_MAXIT, what
            dec.close()


@pytest.mark.parametrize("kind", ["posterior", "extrinsic"])
def test_fixed_soft_output(built, kind):
    """The stop-round posterior c + sum of R (and that minus c), in LSBs, exactly: on the streaming engine (staircase
    d = 7, plain and corrected, the fused columns' R stored because the call asks), through the polled hand-over, and
    through the device-side tail."""
    import torch
    c = fc.staircase(7, "ride")
    q = 6
    for setting in (None, fc.SETTINGS[2]):
        w = fxc.want(7, q, "ride", setting)
        for V in (1, 4):
            dec = _decoder(c, q, setting, fc.FRAMES, fc.MAXIT, V)
            out, iters, soft = dec.decode(c["y"], soft=kind)
            assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), (setting, V)
            assert np.array_equal(soft, fxc.soft_of(w, kind)), ("streaming", setting, V, kind)
            dec.close()
    B = fc.HANDOVER_BATCHES[0]
    y, w = fc.handover_inputs(B), fxc.handover_want(B)
    for V in (1, 4):
        dec = _decoder(c, q, None, B, fc.HANDOVER_MAXIT, V, poll_interval=1)
        out, iters, soft = dec.decode(y, soft=kind)
        assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), V
        assert np.array_equal(soft, fxc.soft_of(w, kind)), ("polled hand-over", V, kind)
        dec.close()
    B = fc.HANDOVER_BATCHES[1]
    y, w = fc.handover_inputs(B), fxc.handover_want(B)
    yd = torch.from_numpy(y.copy()).cuda()
    nb = L.out_bytes(c["K"], B)
    dec = _decoder(c, q, None, B, fc.HANDOVER_MAXIT, 4, poll_interval=0)
    out = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    soft = torch.full((B, c["N"]), float("nan"), dtype=torch.float32, device="cuda")
    dec.decode_device(yd.data_ptr(), B, out.data_ptr(), nb, it.data_ptr(), torch.cuda.current_stream().cuda_stream,
                      soft_ptr=soft.data_ptr(), soft_floats=soft.numel(), soft=kind)
    torch.cuda.synchronize()
    assert np.array_equal(it.cpu().numpy(), w["iters"]) and np.array_equal(out.cpu().numpy(), w["out"])
    assert np.array_equal(soft.cpu().numpy(), fxc.soft_of(w, kind)), ("device tail", kind)
    dec.close()


@functools.lru_cache(maxsize=None)
def _crc_case():
    kind, bits, _ = CC.frame_crc("chain")
    rows, cols, _ = U.bg1()
    y = CC.received("chain", 150, 0.75, 0.98, 3)
    w = RI.flood(Code(rows, cols, U.M, U.N, U.K), y, CC.MAXIT, q=6, llr_scale=8.0, stop=lambda h: CR.crc_passes(kind, h[:, :bits]))
    return kind, bits, y, w


def test_fixed_crc_stop(built):
    """150 frames of the BG1-profile code that carry a CRC16, every third at the hard noise: iteration counts, bytes and
    the number of frames the CRC stopped before their syndrome was clean, against the reference with the stop predicate."""
    kind, bits, y, w = _crc_case()
    assert w["by_stop"].size >= 4
    rows, cols, _ = U.bg1()
    g = L.Graph(rows, cols, U.M, U.N)
    for V in (1, 4):
        dec = L.Decoder(g, U.K, max_batch=150, algo="ms", msg_dtype="i8", msg_bits=6, llr_scale=8.0, max_iter=CC.MAXIT, frames_per_lane=V,
                        crc_kind=kind, crc_bits=bits)
        out, iters = dec.decode(y)
        assert np.array_equal(iters, w["iters"]), V
        assert np.array_equal(out, w["out"]), V
        assert dec.crc_stops() == w["by_stop"].size, (V, dec.crc_stops(), w["by_stop"].size)
        dec.close()


def test_fixed_host_path_in_groups_and_device_list(built):
    """150 frames through ldpc_decode_soft in launch groups of 64 (two full, one ragged): bytes, iteration counts and soft
    values of the reference, and the guard bytes behind out / iters / soft untouched; the same frames through a handle made
    over a device list."""
    c = fc.staircase(7, "ride")
    q = 5
    frames, guard = 150, 64
    y = np.ascontiguousarray(np.resize(c["y"], (frames, c["N"])), np.float32)
    w = RI.flood(c["code"], y, fc.MAXIT, q=q, llr_scale=fxc.LLR_SCALE[q])
    nb = L.out_bytes(c["K"], frames)
    lib = _lib.load()
    for V in (1, 2):
        dec = _decoder(c, q, None, 64, fc.MAXIT, V)
        out = np.full(nb + guard, 0xEE, np.uint8)
        iters = np.full(frames + guard, -7, np.int32)
        soft = np.full(frames * c["N"] + guard, -12345.0, np.float32)
        _lib.check(lib.ldpc_decode_soft(dec._h, y.ctypes.data, frames, out.ctypes.data, nb, iters.ctypes.data, soft.ctypes.data,
                                        frames * c["N"], L.capi.SOFT_KINDS["posterior"]))
        assert np.array_equal(iters[:frames], w["iters"]) and np.array_equal(out[:nb], w["out"]), V
        assert np.array_equal(soft[:frames * c["N"]].reshape(frames, -1), fxc.as_float(w["post"])), V
        assert (out[nb:] == 0xEE).all() and (iters[frames:] == -7).all() and (soft[frames * c["N"]:] == np.float32(-12345.0)).all(), V
        assert dec.stats()["frames"] == frames
        out2, iters2 = dec.decode(y)
        assert np.array_equal(iters2, w["iters"]) and np.array_equal(out2, w["out"]), V
        dec.close()
    dec = _decoder(c, q, None, 64, fc.MAXIT, 1, devices=[0])
    out, iters = dec.decode(y)
    assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"])
    dec.close()


def test_fixed_without_early_termination(built):
    """early_term = 0: every frame runs all rounds; bytes and hard bits are those of the last round -- the reference's with
    no frame ever frozen (a stop predicate that never holds cannot express that: the syndrome stops too, so the reference is
    run on a code object whose syndrome never passes)."""
    c = fc.staircase(3, "ride")
    q, maxit = 6, 6

    class NeverClean(Code):
        def syndrome_ok(self, hard):
            return np.zeros(len(hard), bool)

    w = RI.flood(NeverClean(c["rows"], c["cols"], c["M"], c["N"], c["K"]), c["y"], maxit, q=q, llr_scale=fxc.LLR_SCALE[q])
    assert fxc.want(3, q)["iters"].min() < maxit                 # with early termination frames would have frozen before
    for V in (1, 4):
        dec = _decoder(c, q, None, fc.FRAMES, maxit, V, early_term=False)
        out, iters = dec.decode(c["y"])
        assert (iters == maxit).all(), V
        assert np.array_equal(out, w["out"]), V
        assert np.array_equal(dec.dump(3, fc.FRAMES).astype(np.uint8), w["hard"]), V
        dec.close()


def test_fixed_refusals(built):
    """i8 with the one-launch or record kernels forced on is LDPC_ERR_UNSUPPORTED, as with every algorithm but flooding
    min-sum; an unknown width and a width with another type are LDPC_ERR_ARG.  A refused creation leaves nothing behind, and
    with the circulant size given and nothing forced, i8 takes the streaming kernels."""
    import torch
    c = fc.wimax()
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    q = 6
    y = fxc.degenerate_inputs("wimax", q)
    want = fxc.degenerate_want("wimax", q, False)

    def refused(code, **kw):
        with pytest.raises(L.LdpcError) as e:
            L.Decoder(g, c["K"], max_batch=64, max_iter=fc.DEGENERATE_MAXIT, **kw)
        assert e.value.code == code, (kw, str(e.value))
        torch.cuda.synchronize()

    for algo in ("sp", "layered", "ms_fused", "layered_host", "bp", "layered_bp"):
        refused(LDPC_ERR_UNSUPPORTED, algo=algo, msg_dtype="i8", msg_bits=q, layer_rows=c["z"])
    for tune in ({"fused": True}, {"ldsp": True}, {"fused": True, "ldsp": True}):
        refused(LDPC_ERR_UNSUPPORTED, algo="ms", msg_dtype="i8", msg_bits=q, layer_rows=c["z"], tune=tune)
    refused(LDPC_ERR_ARG, algo="ms", msg_dtype="i8", msg_bits=7)
    refused(LDPC_ERR_ARG, algo="ms", msg_dtype="f8", msg_bits=6)
    refused(LDPC_ERR_ARG, algo="ms", msg_dtype="i8", msg_bits=6, llr_scale=0.0)
    refused(LDPC_ERR_ARG, algo="ms", msg_dtype=5)
    refused(LDPC_ERR_ARG, algo="ms", msg_dtype=3, msg_bits=6)
    for bits, name in ((q, "msi6"), (0, "msi8")):
        dec = L.Decoder(g, c["K"], max_batch=y.shape[0], algo="ms", msg_dtype="i8", msg_bits=bits, llr_scale=fxc.LLR_SCALE[q],
                        max_iter=fc.DEGENERATE_MAXIT, layer_rows=c["z"])
        dec.set_timing(True)
        out, iters = dec.decode(y)
        if bits == q:
            assert np.array_equal(iters, want["iters"]) and np.array_equal(out, want["out"])
        names = [k["name"] for k in dec.kernel_times() if k["phase"] == 0 and k["name"] != "other"]
        assert names and all("<%s," % name in n for n in names), names
        dec.close()


def test_coder_fixed_equals_the_c_abi(built, tmp_path):
    """Coder::setMessageType(LDPC_MSG_I8, bits) with setLlrScale: DecodeMS and DecodeCPU, plain and corrected, give the
    bytes of the C ABI decoder with that width and of the reference; DecodeSP, DecodeTDMPCL and DecodeMSCL refuse it in
    addDecodeType, and so does DecodeMS with a width of 7 or a width next to another type."""
    exe = fxc.coder_fixed_exe(tmp_path)
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    g = L.Graph(rows, cols, M, N)
    frames = 40
    y = channel.awgn_frames(N, 0, frames, 0.8, seed=9)
    y.astype(np.float32).tofile(str(tmp_path / "in"))
    I8 = L.capi.MSG_I8

    def run(mode, dtype, bits, llr_scale, scale=0.0, offset=0.0):
        return subprocess.run([exe, str(int(rate)), str(N), str(frames), mode, str(dtype), str(bits), repr(llr_scale), repr(scale),
                               repr(offset), str(tmp_path / "in"), str(tmp_path / "out")], capture_output=True, text=True)

    code = Code(rows, cols, M, N, K)
    for mode, pack in (("MS", L.PACK_BYTES), ("CPU", L.PACK_BITS)):
        for bits, scale in ((6, 0.0), (6, 0.75), (4, 0.0), (0, 0.0)):
            llr_scale = fxc.LLR_SCALE[bits or 8]
            p = run(mode, I8, bits, llr_scale, scale)
            assert p.returncode == 0, p.stdout + p.stderr
            got = np.fromfile(str(tmp_path / "out"), np.uint8)
            dec = L.Decoder(g, K, max_batch=frames, algo="ms", max_iter=20, layer_rows=z, pack_mode=pack, msg_dtype="i8", msg_bits=bits,
                            llr_scale=llr_scale, ms_scale=scale)
            out, _ = dec.decode(y)
            dec.close()
            assert np.array_equal(got, out[:got.size]), (mode, bits, scale)
            ref = RI.flood(code, y, 20, scale, q=bits or 8, llr_scale=llr_scale, pack_mode=pack)
            assert np.array_equal(got, ref["out"][:got.size]), (mode, bits, scale)
    for mode in ("SP", "TDMPCL", "MSCL"):
        p = run(mode, I8, 6, 8.0)
        assert p.returncode == 3 and "fixed-point" in p.stdout, (mode, p.stdout + p.stderr)
    p = run("MS", I8, 7, 8.0)
    assert p.returncode == 3 and "msg_bits" in p.stdout, p.stdout + p.stderr
    p = run("MS", L.capi.MSG_F16, 6, 8.0)
    assert p.returncode == 3 and "msg_bits" in p.stdout, p.stdout + p.stderr
