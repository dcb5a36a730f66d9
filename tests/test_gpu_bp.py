"""Log-domain sum-product (algo = bp) on the GPU against tests/bp_ref.py: every degree class of the check kernels, every
form of the column-fused check kernels, degenerate channel values, both hand-overs, soft output, the CRC stop, the host
path, the refusals and Coder's DecodeBP.

BP is this repository's own definition (include/ldpc_hip.h: LDPC_ALGO_BP), so the expectation is the numpy restatement,
which tests/test_bp_cpu.py holds to the oracle's min-sum (correction c == 0) in fp32 and fp16.  The definition has no libm
call in it, so everything is compared bit for bit: bytes, iteration counts, all N hard bits, the check->variable and the
variable->check messages after two rounds, the stored channel values, soft values at 0 ulp.  The Q tap is what sees a
column-fused fp16 kernel that keeps an unrounded R in a register (test_bp_cpu.py)."""
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, channel, codes

import bp_cases as bc
import bp_ref as RB
import crc_term_cases as CC
import crc_term_ref as CR
import fp16_cases as fc
import kernel_matrix as km
import ratematch_util as U
import soft_ref as SR
from ms_correction_ref import Code
from test_gpu_kernel_matrix import LINK_FORMS, _link_kernel_name

pytestmark = pytest.mark.gpu

f32 = np.float32
FORMS = dict(LINK_FORMS, guided={"link_guided": True})
ARITH = {"f32": "bp", "f16": "bp16"}            # the library's name of the arithmetic in kernel names
LDPC_ERR_ARG, LDPC_ERR_UNSUPPORTED = 1, 4


def _decoder(c, storage, B, max_iter, V, scale=bc.SCALE, **kw):
    return L.Decoder(L.Graph(c["rows"], c["cols"], c["M"], c["N"]), c["K"], max_batch=B, algo="bp", msg_dtype=storage,
                     max_iter=max_iter, frames_per_lane=V, llr_scale=scale, **kw)


def _compare(dec, y, want, what):
    """One timed decode and one that stops at the tap: bytes, iteration counts, all N hard bits, the stored channel values,
    R on the frames that reached round TAP, Q on those that went on.  Returns the names of the check-phase kernels of
    the timed decode."""
    B = y.shape[0]
    dec.set_timing(True)
    out, iters = dec.decode(y)
    phase0 = {k["name"] for k in dec.kernel_times() if k["phase"] == 0 and k["name"] != "other"}
    dec.set_timing(False)
    assert np.array_equal(iters, want["iters"]), ("iterations",) + what
    assert np.array_equal(out, want["out"]), ("bytes",) + what
    assert np.array_equal(dec.dump(3, B).astype(np.uint8), want["hard"]), ("hard bits",) + what
    assert fc.same_floats(dec.dump(2, B), want["chan"]), ("channel values",) + what
    run_r, run_q = fc.tap_frames(want["iters"])
    assert run_q.size > 0, what
    dec.set_tap(fc.TAP)
    dec.decode(y)
    assert fc.same_floats(dec.dump(0, B)[run_r], want["r_tap"][run_r]), ("R tap",) + what
    assert fc.same_floats(dec.dump(1, B)[run_q], want["q_tap"][run_q]), ("Q tap",) + what
    dec.set_tap(0)
    return phase0


MATRIX_PLANS = {"default": {}, "q_order_edge": {"q_order": -1}, "q_order_on": {"q_order": 1}, "merge_off": {"merge": False},
                "merge_on": {"merge": True}, "check_wide": {"check_wide": True}, "check_wide_off": {"check_wide": False},
                "per_wave_3": {"rows_per_wave": 3, "cols_per_wave": 3}}


@pytest.mark.parametrize("V", [1, 2, 4])
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_bp_every_degree_class(built, storage, V):
    """The irregular matrix code -- rows of every degree 0 ... 33 and 40: the short rows, every unrolled body up to 32, the
    run-time rows above -- 70 frames (a ragged tile at every V), the launch plans that change which check kernel runs or
    where it finds its inputs, and a second llr_scale on the default plan.  By kernel name, the BP instantiations ran:
    one launch per degree with the buckets off, the four bucket launches and the run-time kernel for 33 and 40 otherwise."""
    m, a = bc.matrix(), ARITH[storage]
    rd, _ = km.degree_maps(m["rows"], m["cols"], m["M"], m["N"])
    for plan, tune in MATRIX_PLANS.items():
        what = (storage, V, plan)
        dec = _decoder(m, storage, bc.MATRIX_FRAMES, bc.MATRIX_MAXIT, V, tune=tune)
        phase0 = _compare(dec, m["y"], bc.matrix_want(storage), what)
        assert phase0 and all("<%s," % a in k for k in phase0), (what, phase0)
        if plan in ("merge_off", "check_wide"):
            assert phase0 == {"check_kernel<%s,%d,%d>" % (a, d, V) for d in rd if d > 0}, (what, sorted(phase0))
        elif plan in ("default", "merge_on"):
            assert phase0 == {"check_group_kernel<%s,1-8,%d>" % (a, V), "check_group_kernel<%s,9-16,%d>" % (a, V),
                              "check_group_kernel<%s,17-24,%d>" % (a, V), "check_group_kernel<%s,25-32,%d>" % (a, V),
                              "check_kernel<%s,33,%d>" % (a, V), "check_kernel<%s,40,%d>" % (a, V)}, (what, sorted(phase0))
        dec.close()
    dec = _decoder(m, storage, bc.MATRIX_FRAMES, bc.MATRIX_MAXIT, V, scale=bc.SCALES[1])
    _compare(dec, m["y"], bc.matrix_want(storage, bc.SCALES[1]), (storage, V, "second scale"))
    dec.close()


@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("d", fc.DEGREES)
def test_bp_column_fused_forms(built, d, storage):
    """Staircase codes with the linked class at degree d: every form of the column-fused check kernel at V = 1, 2, 4 with
    the unlinked rows riding along in its launch; for d = 7 also with launches of their own; and with the fusion off.  By
    kernel name, the BP instantiation of a column-fused kernel ran (or none, with the fusion off)."""
    a = ARITH[storage]
    runs = [("ride", form, tune) for form, tune in FORMS.items()] + [("ride", "unfused", {"link_rows": -1})]
    if d == 7:
        runs.append(("own", "default", {}))
    for kind, form, tune in runs:
        c = fc.staircase(d, kind)
        for V in (1, 2, 4):
            what = (d, storage, kind, form, V)
            dec = _decoder(c, storage, fc.FRAMES, fc.MAXIT, V, tune=tune)
            phase0 = _compare(dec, c["y"], bc.want(d, kind, storage), what)
            link = {k for k in phase0 if k.startswith("check_link")}
            if form == "unfused":
                assert not link and phase0 and all("<%s," % a in k for k in phase0), (what, phase0)
            else:
                assert len(link) == 1 and all(k.endswith("<%s,%d,%d>" % (a, d, V)) for k in link), (what, phase0)
                expect = _link_kernel_name(form, V)          # None: the decoder times the forms and keeps the fastest
                assert expect is None or all(k.startswith(expect) for k in link), (what, phase0)
                if kind == "ride":
                    assert phase0 == link, (what, phase0)
                else:
                    assert phase0 - link == {"check_group_kernel<%s,1-8,%d>" % (a, V), "check_kernel<%s,20,%d>" % (a, V)}, (what, phase0)
            dec.close()


@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("name", ["wimax", "ira"])
def test_bp_degenerate_channel_values(built, name, storage):
    """Zeros, values at and beyond binary16's range, infinities, NaN, subnormals, ties, -0, a frame of +-64500 whose
    messages all sit at the clamp: the stored channel values are llr_scale * y (rounded to binary16 for f16) as bits, and
    everything derived from them is what the definition makes of them -- NaN reads +1000, infinities +-1000."""
    c, y = fc.degenerate_code(name), fc.degenerate_inputs(name)
    want = bc.degenerate_want(name, storage)
    for V in (1, 2, 4):
        for tune in ({}, {"check_wide": True}):
            what = (name, storage, V, str(tune))
            dec = _decoder(c, storage, y.shape[0], fc.DEGENERATE_MAXIT, V, scale=bc.DEGENERATE_SCALE, tune=tune)
            phase0 = _compare(dec, y, want, what)
            assert phase0 and all("<%s," % ARITH[storage] in k for k in phase0), (what, phase0)
            if name == "ira":
                assert any(k.startswith("check_link") for k in phase0), (what, phase0)
            dec.close()


def _stats_ok(dec, want, what):
    st = dec.stats()
    assert st["frames_converged"] == want["n_conv"], (what, st)
    assert st["iterations_launched"] == fc.HANDOVER_MAXIT, (what, st)
    return st


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_bp_hand_over_on_a_staircase_code(built, storage):
    """The d = 7 staircase code with 90 scattered stragglers.  700 frames with host polling: the hand-over to child decoders
    (at 512, at 7) against the reference and against a decode with the hand-over off.  700 and 2100 frames without
    polling: at 2100 (33 tiles of 64) the device-side tail takes the stragglers over; against the reference and against
    decodes with the tail off.  Two calls per decoder."""
    import torch
    c = fc.staircase(7, "ride")
    B = fc.HANDOVER_BATCHES[0]
    y, want = fc.handover_inputs(B), bc.handover_want(B, storage)
    for compact, V in [(compact, V) for compact in (512, 7, -1) for V in (1, 4)]:
        dec = _decoder(c, storage, B, fc.HANDOVER_MAXIT, V, poll_interval=1, tune={"compact": compact})
        for call in range(2):
            what = ("polled", storage, compact, V, call)
            out, iters = dec.decode(y)
            assert np.array_equal(iters, want["iters"]), what
            assert np.array_equal(out, want["out"]), what
            _stats_ok(dec, want, what)
        dec.close()
    for B, tunes in zip(fc.HANDOVER_BATCHES, (({}, {"compact": -1}), ({}, {"compact": 100}, {"device_tail": False}))):
        y, want = fc.handover_inputs(B), bc.handover_want(B, storage)
        yd = torch.from_numpy(y.copy()).cuda()
        nb = L.out_bytes(c["K"], B)
        for tune in tunes:
            for V in (1, 4):
                dec = _decoder(c, storage, B, fc.HANDOVER_MAXIT, V, poll_interval=0, tune=tune)
                for call in range(2):
                    what = ("device", storage, B, tune, V, call)
                    out = torch.full((nb,), 0xEE, dtype=torch.uint8, device="cuda")
                    it = torch.zeros(B, dtype=torch.int32, device="cuda")
                    dec.decode_device(yd.data_ptr(), B, out.data_ptr(), nb, it.data_ptr(), torch.cuda.current_stream().cuda_stream)
                    torch.cuda.synchronize()
                    assert np.array_equal(it.cpu().numpy(), want["iters"]), what
                    assert np.array_equal(out.cpu().numpy(), want["out"]), what
                    assert _stats_ok(dec, want, what)["batch_time"] == fc.HANDOVER_MAXIT, what
                dec.close()


@pytest.mark.parametrize("kind", ["posterior", "extrinsic"])
def test_bp_soft_output(built, kind):
    """The stop-round posterior chan + sum of R (and that minus chan) at 0 ulp: on the streaming engine (staircase d = 7,
    both storages, the fused columns' R stored because the call asks), through the polled hand-over, and through the
    device-side tail.  Wherever the posterior is finite and not zero, its sign is the output bit."""
    import torch
    c = fc.staircase(7, "ride")
    for storage in ("f32", "f16"):
        w = bc.want(7, "ride", storage)
        assert SR.sign_disagreements(w["post"], w["hard"]) == 0
        for V in (1, 4):
            dec = _decoder(c, storage, fc.FRAMES, fc.MAXIT, V)
            out, iters, soft = dec.decode(c["y"], soft=kind)
            assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), (storage, V)
            SR.assert_same_bits(soft, RB.soft_of(w, kind), None, str(("streaming", storage, V, kind)))
            if kind == "posterior":
                assert SR.sign_disagreements(soft, dec.dump(3, fc.FRAMES)) == 0, (storage, V)
            dec.close()
    B = fc.HANDOVER_BATCHES[0]
    y, w = fc.handover_inputs(B), bc.handover_want(B)
    for V in (1, 4):
        dec = _decoder(c, "f32", B, fc.HANDOVER_MAXIT, V, poll_interval=1)
        out, iters, soft = dec.decode(y, soft=kind)
        assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), V
        SR.assert_same_bits(soft, RB.soft_of(w, kind), None, str(("polled hand-over", V, kind)))
        dec.close()
    B = fc.HANDOVER_BATCHES[1]
    y, w = fc.handover_inputs(B), bc.handover_want(B)
    yd = torch.from_numpy(y.copy()).cuda()
    nb = L.out_bytes(c["K"], B)
    dec = _decoder(c, "f32", B, fc.HANDOVER_MAXIT, 4, poll_interval=0)
    out = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    soft = torch.full((B, c["N"]), float("nan"), dtype=torch.float32, device="cuda")
    dec.decode_device(yd.data_ptr(), B, out.data_ptr(), nb, it.data_ptr(), torch.cuda.current_stream().cuda_stream,
                      soft_ptr=soft.data_ptr(), soft_floats=soft.numel(), soft=kind)
    torch.cuda.synchronize()
    assert np.array_equal(it.cpu().numpy(), w["iters"]) and np.array_equal(out.cpu().numpy(), w["out"])
    SR.assert_same_bits(soft.cpu().numpy(), RB.soft_of(w, kind), None, str(("device tail", kind)))
    dec.close()


def test_bp_crc_stop(built):
    """150 frames of the BG1-profile code that carry a CRC16, every third at the hard noise: iteration counts, bytes and
    the number of frames the CRC stopped before their syndrome was clean, against the reference with the stop predicate."""
    kind, bits, y, w = bc.crc_case()
    assert w["by_stop"].size >= 1
    rows, cols, _ = U.bg1()
    g = L.Graph(rows, cols, U.M, U.N)
    for storage in ("f32", "f16"):
        if storage == "f16":
            w = RB.flood(Code(rows, cols, U.M, U.N, U.K), y, CC.MAXIT, rnd=RB.f16, llr_scale=bc.SCALE,
                         stop=lambda h: CR.crc_passes(kind, h[:, :bits]))
        for V in (1, 4):
            dec = L.Decoder(g, U.K, max_batch=150, algo="bp", msg_dtype=storage, max_iter=CC.MAXIT, frames_per_lane=V,
                            llr_scale=bc.SCALE, crc_kind=kind, crc_bits=bits)
            out, iters = dec.decode(y)
            assert np.array_equal(iters, w["iters"]), (storage, V)
            assert np.array_equal(out, w["out"]), (storage, V)
            assert dec.crc_stops() == w["by_stop"].size, (storage, V, dec.crc_stops(), w["by_stop"].size)
            dec.close()


def test_bp_host_path_in_groups(built):
    """150 frames through ldpc_decode_soft in launch groups of 64 (two full, one ragged): bytes, iteration counts and soft
    values of the reference, and the guard bytes behind out / iters / soft untouched."""
    c = fc.staircase(7, "ride")
    frames, guard = 150, 64
    y = np.ascontiguousarray(np.resize(c["y"], (frames, c["N"])), np.float32)
    lib = _lib.load()
    for storage, V in (("f32", 1), ("f32", 2), ("f16", 1)):
        w = RB.flood(c["code"], y, fc.MAXIT, rnd=bc.RND[storage], llr_scale=bc.SCALE)
        nb = L.out_bytes(c["K"], frames)
        dec = _decoder(c, storage, 64, fc.MAXIT, V)
        out = np.full(nb + guard, 0xEE, np.uint8)
        iters = np.full(frames + guard, -7, np.int32)
        soft = np.full(frames * c["N"] + guard, -12345.0, np.float32)
        _lib.check(lib.ldpc_decode_soft(dec._h, y.ctypes.data, frames, out.ctypes.data, nb, iters.ctypes.data, soft.ctypes.data,
                                        frames * c["N"], L.capi.SOFT_KINDS["posterior"]))
        assert np.array_equal(iters[:frames], w["iters"]) and np.array_equal(out[:nb], w["out"]), (storage, V)
        SR.assert_same_bits(soft[:frames * c["N"]].reshape(frames, -1), w["post"], None, str(("host path", storage, V)))
        assert (out[nb:] == 0xEE).all() and (iters[frames:] == -7).all() and (soft[frames * c["N"]:] == np.float32(-12345.0)).all(), V
        assert dec.stats()["frames"] == frames
        out2, iters2 = dec.decode(y)
        assert np.array_equal(iters2, w["iters"]) and np.array_equal(out2, w["out"]), (storage, V)
        dec.close()


def test_bp_refusals(built):
    """BP with the one-launch or record kernels forced on, with fp8 messages or with a min-sum correction is
    LDPC_ERR_UNSUPPORTED; a llr_scale that is not positive and finite is LDPC_ERR_ARG.  A refused creation leaves nothing
    behind: the device is idle and a decoder made right after it -- with the circulant size given, which selects no
    engine -- runs the streaming BP kernels and decodes as the reference says."""
    import torch
    c = fc.wimax()
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    y = fc.degenerate_inputs("wimax")
    want = bc.degenerate_want("wimax", "f32")

    def refused(code, **kw):
        with pytest.raises(L.LdpcError) as e:
            L.Decoder(g, c["K"], max_batch=64, max_iter=fc.DEGENERATE_MAXIT, algo="bp", **kw)
        assert e.value.code == code, (kw, str(e.value))
        torch.cuda.synchronize()

    for tune in ({"fused": True}, {"ldsp": True}, {"fused": True, "ldsp": True}):
        refused(LDPC_ERR_UNSUPPORTED, layer_rows=c["z"], tune=tune)
    refused(LDPC_ERR_UNSUPPORTED, msg_dtype="f8")
    refused(LDPC_ERR_UNSUPPORTED, ms_scale=0.75)
    refused(LDPC_ERR_UNSUPPORTED, ms_offset=0.15)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        refused(LDPC_ERR_ARG, llr_scale=bad)
    dec = L.Decoder(g, c["K"], max_batch=y.shape[0], algo="bp", max_iter=fc.DEGENERATE_MAXIT, layer_rows=c["z"],
                    llr_scale=bc.DEGENERATE_SCALE)
    dec.set_timing(True)
    out, iters = dec.decode(y)
    assert np.array_equal(iters, want["iters"]) and np.array_equal(out, want["out"])
    names = [k["name"] for k in dec.kernel_times() if k["phase"] == 0 and k["name"] != "other"]
    assert names and all("<bp," in n for n in names), names
    dec.close()
    sp = L.Decoder(g, c["K"], max_batch=4, algo="sp")                                       # SP still has no soft output
    with pytest.raises(L.LdpcError) as e:
        sp.decode(y[:4], soft="posterior")
    assert e.value.code == LDPC_ERR_UNSUPPORTED
    sp.close()


def test_coder_decode_bp_equals_the_c_abi(built, tmp_path):
    """Coder's DecodeBP with setLlrScale and setMessageType (F32, F16) gives the bytes and the soft values (both kinds) of
    the C ABI decoder with algo = bp -- and of the reference; with setMinSumCorrection or LDPC_MSG_F8 addDecodeType fails
    as ldpc_decoder_create does."""
    from coder_bp_harness import coder_bp_exe
    exe = coder_bp_exe(tmp_path)
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    g = L.Graph(rows, cols, M, N)
    frames = 40
    y = channel.awgn_frames(N, 0, frames, 0.8, seed=9)
    y.astype(np.float32).tofile(str(tmp_path / "in"))
    scale = 3.125                                    # 2 / 0.8^2

    def run(dtype, kind=0, ms_scale=0.0, ms_offset=0.0):
        return subprocess.run([exe, str(int(rate)), str(N), str(frames), str(dtype), repr(scale), repr(ms_scale), repr(ms_offset),
                               str(kind), str(tmp_path / "in"), str(tmp_path / "out"), str(tmp_path / "soft")],
                              capture_output=True, text=True)

    code = Code(rows, cols, M, N, K)
    for name, dtype in (("f32", L.capi.MSG_F32), ("f16", L.capi.MSG_F16)):
        w = RB.flood(code, y, 20, rnd=bc.RND[name], llr_scale=scale)
        for kind_name, kind in ((None, 0), ("posterior", 1), ("extrinsic", 2)):
            p = run(dtype, kind)
            assert p.returncode == 0, p.stdout + p.stderr
            got = np.fromfile(str(tmp_path / "out"), np.uint8)
            dec = L.Decoder(g, K, max_batch=frames, algo="bp", max_iter=20, layer_rows=z, msg_dtype=name, llr_scale=scale,
                            poll_interval=4)
            res = dec.decode(y, soft=kind_name)
            dec.close()
            assert np.array_equal(got, res[0][:got.size]) and np.array_equal(got, w["out"][:got.size]), (name, kind)
            if kind:
                soft = np.fromfile(str(tmp_path / "soft"), np.float32).reshape(frames, N)
                SR.assert_same_bits(soft, res[2], None, str(("coder against the C ABI", name, kind_name)))
                SR.assert_same_bits(soft, RB.soft_of(w, kind_name), None, str(("coder against the reference", name, kind_name)))
    for kw in (dict(ms_scale=0.75), dict(ms_offset=0.15)):
        p = run(L.capi.MSG_F32, **kw)
        assert p.returncode == 3 and "ms_scale" in p.stdout, p.stdout + p.stderr
    p = run(L.capi.MSG_F8)
    assert p.returncode == 3 and "fp8" in p.stdout, p.stdout + p.stderr
