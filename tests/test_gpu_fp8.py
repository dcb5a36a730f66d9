"""fp8 (E4M3) messages (msg_dtype = f8) on the GPU against tests/fp8_ref.py: the conversion, every form of the
column-fused check kernels, degenerate channel values, both hand-overs, soft output, the CRC stop, the host path, the
refusals and Coder::setMessageType.

fp8 is this repository's own definition (include/ldpc_hip.h: LDPC_MSG_F8), so the expectation is the numpy restatement,
which tests/test_fp8_cpu.py holds to the oracle (identity rounding) and to the fp16 reference (binary16 rounding) and
whose rounding it checks against the table of the 256 codes.  Everything is compared bit for bit: bytes, iteration counts,
all N hard bits, the check->variable and the variable->check messages after two rounds, soft values at 0 ulp.  The Q tap
is what sees a column-fused kernel that keeps an unrounded R in a register (test_fp8_cpu.py)."""
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
import fp8_cases as f8c
import fp8_ref as R8
import ratematch_util as U
import soft_ref as SR
from ms_correction_ref import Code
from test_gpu_kernel_matrix import LINK_FORMS

pytestmark = pytest.mark.gpu

FORMS = dict(LINK_FORMS, guided={"link_guided": True})
LINK_KERNELS = {"wide": "check_link_kernel", "narrow": "check_link_narrow_kernel", "half": "check_link_half_kernel"}
LDPC_ERR_ARG, LDPC_ERR_UNSUPPORTED = 1, 4


def _decoder(c, arith, setting, B, max_iter, V, **kw):
    assert (arith == "msc8") == (setting is not None)
    scale, offset = setting or (0.0, 0.0)
    return L.Decoder(L.Graph(c["rows"], c["cols"], c["M"], c["N"]), c["K"], max_batch=B, algo="ms", msg_dtype="f8",
                     max_iter=max_iter, frames_per_lane=V, ms_scale=scale, ms_offset=offset, **kw)


def _compare(dec, y, want, what):
    """One timed decode and one that stops at the tap: bytes, iteration counts, all N hard bits, R on the frames that
    reached round TAP, Q on those that went on.  Returns the names of the check-phase kernels of the timed decode."""
    B = y.shape[0]
    dec.set_timing(True)
    out, iters = dec.decode(y)
    phase0 = {k["name"] for k in dec.kernel_times() if k["phase"] == 0 and k["name"] != "other"}
    dec.set_timing(False)
    assert np.array_equal(iters, want["iters"]), ("iterations",) + what
    assert np.array_equal(out, want["out"]), ("bytes",) + what
    assert np.array_equal(dec.dump(3, B).astype(np.uint8), want["hard"]), ("hard bits",) + what
    run_r, run_q = fc.tap_frames(want["iters"])
    assert run_q.size > 0, what
    dec.set_tap(fc.TAP)
    dec.decode(y)
    assert fc.same_floats(dec.dump(0, B)[run_r], want["r_tap"][run_r]), ("R tap",) + what
    assert fc.same_floats(dec.dump(1, B)[run_q], want["q_tap"][run_q]), ("Q tap",) + what
    dec.set_tap(0)
    return phase0


def _expected_link_kernel(dec, tune, V):
    """The form the tuning fixes (deep is a narrow form; half has kernels for V = 4 only and falls back to narrow below).
    Where it fixes none, fp8 takes the wide form at V = 1 and the one timed fastest at creation above, where the narrow
    form -- one byte per lane -- is no candidate."""
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


def test_fp8_conversion_is_s8(built):
    """Frames filled with every code value, the midpoint of every neighbouring pair, its fp32 neighbours and the edge list
    of the definition (464, 1000, infinities, NaN, subnormal ties, -1e-8, 1e-41, ...): the stored channel values are
    s8(y) as bits, NaN where NaN is expected, at 1, 2 and 4 frames per lane."""
    c = fc.wimax()
    y = f8c.conversion_inputs(c["N"], fc.DEGENERATE_FRAMES)
    assert y.size >= R8.edge_inputs().size
    stored = R8.s8(y)
    for V in (1, 2, 4):
        dec = _decoder(c, "ms8", None, y.shape[0], 2, V)
        dec.decode(y)
        assert fc.same_floats(dec.dump(2, y.shape[0]), stored), V
        dec.close()


@pytest.mark.parametrize("arith", ["ms8", "msc8"])
@pytest.mark.parametrize("d", fc.DEGREES)
def test_fp8_column_fused_forms(built, d, arith):
    """Staircase codes with the linked class at degree d, fp8 messages, plain and corrected min-sum: every form of the
    column-fused check kernel at V = 1, 2, 4 with the unlinked rows riding along in its launch; for d = 7 also with
    launches of their own; and with the fusion off.  By kernel name, the fp8 instantiation of the expected form ran."""
    runs = [("ride", form, tune) for form, tune in FORMS.items()] + [("ride", "unfused", {"link_rows": -1})]
    if d == 7:
        runs.append(("own", "default", {}))
    n = 0
    for kind, form, tune in runs:
        c = fc.staircase(d, kind)
        for V in (1, 2, 4):
            n += 1
            if arith == "ms8":
                settings = (None,)
            else:                # all three on the default form, one of them in turn on the others
                settings = fc.SETTINGS if form == "default" else (fc.SETTINGS[n % 3],)
            for setting in settings:
                what = (d, arith, setting, kind, form, V)
                dec = _decoder(c, arith, setting, fc.FRAMES, fc.MAXIT, V, tune=tune)
                phase0 = _compare(dec, c["y"], f8c.want(d, kind, setting), what)
                link = {k for k in phase0 if k.startswith("check_link")}
                if form == "unfused":
                    assert not link and phase0 and all("<%s," % arith in k for k in phase0), (what, phase0)
                else:
                    assert link == {"%s<%s,%d,%d>" % (_expected_link_kernel(dec, tune, V), arith, d, V)}, (what, phase0)
                    if kind == "ride":
                        assert phase0 == link, (what, phase0)
                    else:
                        assert phase0 - link == {"check_group_kernel<%s,1-8,%d>" % (arith, V), "check_kernel<%s,20,%d>" % (arith, V)}, (what, phase0)
                dec.close()


@pytest.mark.parametrize("arith", ["ms8", "msc8"])
@pytest.mark.parametrize("name", ["wimax", "ira"])
def test_fp8_degenerate_channel_values(built, name, arith):
    """Zeros, +-448, 464, 1000, infinities, NaN, E4M3 subnormals, ties of both kinds, -0, an fp32 denormal, and a frame of
    +-400 whose Q saturates after round 1: the stored channel values are s8 of the input, as bits, and everything derived
    from them is what the definition makes of them.  WiMAX 960 runs the check kernels in wide waves (the automatic choice
    for fp8), the staircase code the column-fused kernel."""
    c, y = fc.degenerate_code(name), f8c.degenerate_inputs(name)
    B = y.shape[0]
    setting = fc.DEGENERATE_SETTING if arith == "msc8" else None
    want = f8c.degenerate_want(name, setting is not None)
    stored = R8.s8(y)
    for V in (1, 2, 4):
        for tune in ({}, {"check_wide": False}):
            what = (name, arith, V, str(tune))
            dec = _decoder(c, arith, setting, B, fc.DEGENERATE_MAXIT, V, tune=tune)
            phase0 = _compare(dec, y, want, what)
            assert phase0 and all("<%s," % arith in k for k in phase0), (what, phase0)
            if name == "ira":
                assert any(k.startswith("check_link") for k in phase0), (what, phase0)
            assert fc.same_floats(dec.dump(2, B), stored), ("channel values",) + what
            dec.close()


def _stats_ok(dec, want, what):
    st = dec.stats()
    assert st["frames_converged"] == want["n_conv"], (what, st)
    assert st["iterations_launched"] == fc.HANDOVER_MAXIT, (what, st)
    return st


def test_fp8_hand_over_on_a_staircase_code(built):
    """fp8 messages on the d = 7 staircase code with 90 scattered stragglers: the host-polled hand-over to child decoders
    (row segments of 64 bytes at V = 1; the row-wise gather at 512, the per-element gather at 7) and the device-side tail,
    two calls per decoder."""
    import torch
    c = fc.staircase(7, "ride")
    B = fc.HANDOVER_BATCHES[0]
    y = fc.handover_inputs(B)
    runs = [("ms8", None, compact, V) for compact in (512, 7, -1) for V in (1, 4)] + [("msc8", fc.SETTINGS[0], 0, 4)]
    for arith, setting, compact, V in runs:
        want = f8c.handover_want(B, setting)
        dec = _decoder(c, arith, setting, B, fc.HANDOVER_MAXIT, V, poll_interval=1, tune={"compact": compact} if compact else {})
        for call in range(2):
            what = ("polled", arith, compact, V, call)
            out, iters = dec.decode(y)
            assert np.array_equal(iters, want["iters"]), what
            assert np.array_equal(out, want["out"]), what
            _stats_ok(dec, want, what)
        dec.close()
    B = fc.HANDOVER_BATCHES[1]
    y, want = fc.handover_inputs(B), f8c.handover_want(B)
    yd = torch.from_numpy(y.copy()).cuda()
    nb = L.out_bytes(c["K"], B)
    for tune in ({}, {"compact": 100}, {"device_tail": False}):
        for V in (1, 4):
            dec = _decoder(c, "ms8", None, B, fc.HANDOVER_MAXIT, V, poll_interval=0, tune=tune)
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
def test_fp8_soft_output(built, kind):
    """The stop-round posterior y8 + sum of R (and that minus y8) at 0 ulp: on the streaming engine (staircase d = 7, plain
    and corrected, the fused columns' R stored because the call asks), through the polled hand-over, and through the
    device-side tail."""
    import torch
    c = fc.staircase(7, "ride")
    for arith, setting in (("ms8", None), ("msc8", fc.SETTINGS[2])):
        w = f8c.want(7, "ride", setting)
        for V in (1, 4):
            dec = _decoder(c, arith, setting, fc.FRAMES, fc.MAXIT, V)
            out, iters, soft = dec.decode(c["y"], soft=kind)
            assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), (arith, V)
            SR.assert_same_bits(soft, f8c.soft_of(w, kind), None, str(("streaming", arith, V, kind)))
            dec.close()
    B = fc.HANDOVER_BATCHES[0]
    y, w = fc.handover_inputs(B), f8c.handover_want(B)
    for V in (1, 4):
        dec = _decoder(c, "ms8", None, B, fc.HANDOVER_MAXIT, V, poll_interval=1)
        out, iters, soft = dec.decode(y, soft=kind)
        assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), V
        SR.assert_same_bits(soft, f8c.soft_of(w, kind), None, str(("polled hand-over", V, kind)))
        dec.close()
    B = fc.HANDOVER_BATCHES[1]
    y, w = fc.handover_inputs(B), f8c.handover_want(B)
    yd = torch.from_numpy(y.copy()).cuda()
    nb = L.out_bytes(c["K"], B)
    dec = _decoder(c, "ms8", None, B, fc.HANDOVER_MAXIT, 4, poll_interval=0)
    out = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    soft = torch.full((B, c["N"]), float("nan"), dtype=torch.float32, device="cuda")
    dec.decode_device(yd.data_ptr(), B, out.data_ptr(), nb, it.data_ptr(), torch.cuda.current_stream().cuda_stream,
                      soft_ptr=soft.data_ptr(), soft_floats=soft.numel(), soft=kind)
    torch.cuda.synchronize()
    assert np.array_equal(it.cpu().numpy(), w["iters"]) and np.array_equal(out.cpu().numpy(), w["out"])
    SR.assert_same_bits(soft.cpu().numpy(), f8c.soft_of(w, kind), None, str(("device tail", kind)))
    dec.close()


@functools.lru_cache(maxsize=None)
def _crc_case():
    kind, bits, _ = CC.frame_crc("chain")
    rows, cols, _ = U.bg1()
    y = CC.received("chain", 150, 0.75, 0.98, 3)
    w = R8.flood(Code(rows, cols, U.M, U.N, U.K), y, CC.MAXIT, stop=lambda h: CR.crc_passes(kind, h[:, :bits]))
    return kind, bits, y, w


def test_fp8_crc_stop(built):
    """150 frames of the BG1-profile code that carry a CRC16, every third at the hard noise: iteration counts, bytes and
    the number of frames the CRC stopped before their syndrome was clean, against the reference with the stop predicate."""
    kind, bits, y, w = _crc_case()
    assert w["by_stop"].size >= 4
    rows, cols, _ = U.bg1()
    g = L.Graph(rows, cols, U.M, U.N)
    for V in (1, 4):
        dec = L.Decoder(g, U.K, max_batch=150, algo="ms", msg_dtype="f8", max_iter=CC.MAXIT, frames_per_lane=V, crc_kind=kind, crc_bits=bits)
        out, iters = dec.decode(y)
        assert np.array_equal(iters, w["iters"]), V
        assert np.array_equal(out, w["out"]), V
        assert dec.crc_stops() == w["by_stop"].size, (V, dec.crc_stops(), w["by_stop"].size)
        dec.close()


def test_fp8_host_path_in_groups(built):
    """150 frames through ldpc_decode_soft in launch groups of 64 (two full, one ragged): bytes, iteration counts and soft
    values of the reference, and the guard bytes behind out / iters / soft untouched."""
    c = fc.staircase(7, "ride")
    frames, guard = 150, 64
    y = np.ascontiguousarray(np.resize(c["y"], (frames, c["N"])), np.float32)
    w = R8.flood(c["code"], y, fc.MAXIT)
    nb = L.out_bytes(c["K"], frames)
    lib = _lib.load()
    for V in (1, 2):
        dec = _decoder(c, "ms8", None, 64, fc.MAXIT, V)
        out = np.full(nb + guard, 0xEE, np.uint8)
        iters = np.full(frames + guard, -7, np.int32)
        soft = np.full(frames * c["N"] + guard, -12345.0, np.float32)
        _lib.check(lib.ldpc_decode_soft(dec._h, y.ctypes.data, frames, out.ctypes.data, nb, iters.ctypes.data, soft.ctypes.data,
                                        frames * c["N"], L.capi.SOFT_KINDS["posterior"]))
        assert np.array_equal(iters[:frames], w["iters"]) and np.array_equal(out[:nb], w["out"]), V
        SR.assert_same_bits(soft[:frames * c["N"]].reshape(frames, -1), w["post"], None, str(("host path", V)))
        assert (out[nb:] == 0xEE).all() and (iters[frames:] == -7).all() and (soft[frames * c["N"]:] == np.float32(-12345.0)).all(), V
        assert dec.stats()["frames"] == frames
        out2, iters2 = dec.decode(y)
        assert np.array_equal(iters2, w["iters"]) and np.array_equal(out2, w["out"]), V
        dec.close()


def test_fp8_refusals(built):
    """f8 with every algorithm but flooding min-sum, and with the one-launch or record kernels forced on, is
    LDPC_ERR_UNSUPPORTED; msg_dtype 3 is LDPC_ERR_ARG.  A refused creation leaves nothing behind: the device is idle and
    a decoder made right after it decodes as the reference says."""
    import torch
    c = fc.wimax()
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    y = f8c.degenerate_inputs("wimax")
    want = f8c.degenerate_want("wimax", False)

    def refused(code, **kw):
        with pytest.raises(L.LdpcError) as e:
            L.Decoder(g, c["K"], max_batch=64, max_iter=fc.DEGENERATE_MAXIT, **kw)
        assert e.value.code == code, (kw, str(e.value))
        torch.cuda.synchronize()

    for algo in ("sp", "layered", "ms_fused", "layered_host"):
        refused(LDPC_ERR_UNSUPPORTED, algo=algo, msg_dtype="f8", layer_rows=c["z"])
    for tune in ({"fused": True}, {"ldsp": True}, {"fused": True, "ldsp": True}):
        refused(LDPC_ERR_UNSUPPORTED, algo="ms", msg_dtype="f8", layer_rows=c["z"], tune=tune)
    refused(LDPC_ERR_ARG, algo="ms", msg_dtype=3)
    refused(LDPC_ERR_ARG, algo="ms", msg_dtype=-1)
    # with the circulant size given and nothing forced, f8 takes the streaming kernels (the one-launch kernels are fp32)
    dec = L.Decoder(g, c["K"], max_batch=y.shape[0], algo="ms", msg_dtype="f8", max_iter=fc.DEGENERATE_MAXIT, layer_rows=c["z"])
    dec.set_timing(True)
    out, iters = dec.decode(y)
    assert np.array_equal(iters, want["iters"]) and np.array_equal(out, want["out"])
    names = [k["name"] for k in dec.kernel_times() if k["phase"] == 0 and k["name"] != "other"]
    assert names and all("<ms8," in n for n in names), names
    dec.close()


def test_coder_message_type_equals_the_c_abi(built, tmp_path):
    """Coder::setMessageType: DecodeMS and DecodeCPU with F8 (plain and corrected) and F16 give the bytes of the C ABI decoder
    with that msg_dtype -- and of the reference for F8; DecodeSP, DecodeTDMPCL and DecodeMSCL refuse a type other than F32
    in addDecodeType, an unknown type is refused for DecodeMS too."""
    from coder_message_type_harness import coder_message_type_exe
    exe = coder_message_type_exe(tmp_path)
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    g = L.Graph(rows, cols, M, N)
    frames = 40
    y = channel.awgn_frames(N, 0, frames, 0.8, seed=9)
    y.astype(np.float32).tofile(str(tmp_path / "in"))

    def run(mode, dtype, scale=0.0, offset=0.0):
        return subprocess.run([exe, str(int(rate)), str(N), str(frames), mode, str(dtype), repr(scale), repr(offset),
                               str(tmp_path / "in"), str(tmp_path / "out")], capture_output=True, text=True)

    code = Code(rows, cols, M, N, K)
    for mode, pack in (("MS", L.PACK_BYTES), ("CPU", L.PACK_BITS)):
        for name, dtype, scale in (("f8", L.capi.MSG_F8, 0.0), ("f8", L.capi.MSG_F8, 0.75), ("f16", L.capi.MSG_F16, 0.0), ("f32", L.capi.MSG_F32, 0.0)):
            p = run(mode, dtype, scale)
            assert p.returncode == 0, p.stdout + p.stderr
            got = np.fromfile(str(tmp_path / "out"), np.uint8)
            dec = L.Decoder(g, K, max_batch=frames, algo="ms", max_iter=20, layer_rows=z, pack_mode=pack, msg_dtype=name, ms_scale=scale)
            out, _ = dec.decode(y)
            dec.close()
            assert np.array_equal(got, out[:got.size]), (mode, name, scale)
            if name == "f8":
                assert np.array_equal(got, R8.flood(code, y, 20, scale, pack_mode=pack)["out"][:got.size]), (mode, scale)
    for mode in ("SP", "TDMPCL", "MSCL"):
        p = run(mode, L.capi.MSG_F8)
        assert p.returncode == 3 and "fp8" in p.stdout, (mode, p.stdout + p.stderr)
    p = run("MS", 3)
    assert p.returncode == 3 and "msg_dtype" in p.stdout, p.stdout + p.stderr
