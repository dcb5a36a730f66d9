"""Soft output on the GPU (ldpc_decode_soft / ldpc_decode_soft_device) against tests/soft_ref.py: per frame the CPU
oracle's posterior of the round the frame stopped in, or that minus the channel value -- 0 ulp on the uint32 bit patterns,
together with the bytes and the iteration counts, on every engine, through both hand-overs and the host path."""
import functools
import os
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes

import oracle

import arena_cases as ac
import crc_term_cases as CC
import ms_correction_ref as MC
import ratematch_util as U
import soft_ref as SR
import tb_util as TU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("posterior", "extrinsic")
KEY = {"posterior": "post", "extrinsic": "ext"}
STREAM, RECORD, RESIDENT = {"fused": False, "ldsp": False}, {"fused": True, "ldsp": True}, {"fused": True, "ldsp": False}


@pytest.fixture(scope="module")
def graph(built):
    rows, cols, _ = U.bg1()
    return L.Graph(rows, cols, U.M, U.N)


@functools.lru_cache(maxsize=None)
def bg1_code():
    rows, cols, _ = U.bg1()
    return MC.Code(rows, cols, U.M, U.N, U.K)


@functools.lru_cache(maxsize=None)
def chain_want(algo, variant, snr):
    kw = {"": {}, "f16": dict(f16=True), "scale": dict(scale=0.75, code=bg1_code())}[variant]
    return SR.expected(U.bg1()[2], TU.chain_received(snr)[2], algo, U.MAX_ITER, layer_rows=U.Z, **kw)


def _check(w, out, iters, soft, kind, what):
    assert np.array_equal(iters, w["iters"]), what
    assert np.array_equal(out, w["out"]), what
    keep = ~w["undefined"]
    assert keep.sum() * 8 >= keep.size * 7, what          # at most one frame in eight is undefined in the oracle
    SR.assert_same_bits(soft, w[KEY[kind]], keep, str(what))
    if kind == "posterior":
        assert SR.sign_disagreements(np.asarray(soft).reshape(w["post"].shape)[keep], w["hard"][keep]) == 0, what


VARIANT_KW = {"": {}, "f16": dict(msg_dtype="f16"), "scale": dict(ms_scale=0.75)}
# (id, algo, variant, Decoder keywords): the engine is forced with the tuning fields, as the parity tests do
CHAIN = [("ms-%s-stream%d" % (v or "f32", fpl), "ms", v, dict(layer_rows=0, frames_per_lane=fpl))
         for v in ("", "f16", "scale") for fpl in (1, 2, 4)]
CHAIN += [("ms-f32-record", "ms", "", dict(layer_rows=U.Z, tune=RECORD)), ("ms-scale-record", "ms", "scale", dict(layer_rows=U.Z, tune=RECORD)),
          ("ms-f32-resident", "ms", "", dict(layer_rows=U.Z, tune=RESIDENT))]
CHAIN += [("layered-stream%d" % fpl, "layered", "", dict(layer_rows=U.Z, frames_per_lane=fpl, tune=STREAM)) for fpl in (1, 2, 4)]
CHAIN += [("layered-record", "layered", "", dict(layer_rows=U.Z, tune=RECORD)), ("layered-resident", "layered", "", dict(layer_rows=U.Z, tune=RESIDENT))]


@pytest.mark.parametrize("point", [0, 1], ids=["clean", "hard"])
@pytest.mark.parametrize("name,algo,variant,kw", CHAIN, ids=[c[0] for c in CHAIN])
def test_chain_scenario(graph, name, algo, variant, kw, point):
    """64 frames at 3.0 and 0.0 dB, two calls per decoder and kind."""
    snr = TU.chain_points(algo)[point]
    w = chain_want(algo, variant, snr)
    y = TU.chain_received(snr)[2]
    dec = L.Decoder(graph, U.K, max_batch=64, algo=algo, max_iter=U.MAX_ITER, llr_scale=U.LLR_SCALE, **dict(kw, **VARIANT_KW[variant]))
    dec.set_timing(True)
    for call in range(2):
        for kind in KINDS:
            out, iters, soft = dec.decode(y, soft=kind)
            _check(w, out, iters, soft, kind, (name, snr, kind, call))
    names = [k["name"] for k in dec.kernel_times()]
    want_kernel = {"stream": "soft_settle_kernel" if "stream" in name else None, "record": "ldsp_", "resident": "fused_"}
    for key, frag in want_kernel.items():
        if key in name and frag:
            assert any(frag in n for n in names), (name, names)        # the engine the case is named after really ran
    dec.close()


@pytest.mark.parametrize("algo,rate,sd", [("ms_fused", codes.RATE_1_2, 0.8), ("ms_fused", codes.RATE_5_6, 0.52),
                                          ("layered_host", codes.RATE_5_6, 0.52)], ids=["ms_fused-r12", "ms_fused-r56", "layered_host-r56"])
def test_reference_kernel_algorithms(built, algo, rate, sd):
    """LDPC_ALGO_MS_FUSED (record and LDS-resident kernels) and LDPC_ALGO_LAYERED_HOST (streaming layered kernels; it
    exists where every row of H has one weight: rate 5/6) on the 802.16e codes of N = 576, 64 frames, against the
    oracle's ms_fused / layered_host posterior taps."""
    N = 576
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    g, og = L.Graph(rows, cols, M, N), oracle.Graph(rows, cols, M, N, K)
    y = channel.awgn_frames(N, 0, 64, sd, seed=31)
    w = SR.expected(og, y, algo, 20, layer_rows=z)
    assert np.unique(w["iters"]).size >= 3
    for kw in ((dict(tune={"ldsp": True}), dict(tune={"ldsp": False})) if algo == "ms_fused" else
               (dict(frames_per_lane=1), dict(frames_per_lane=4))):
        dec = L.Decoder(g, K, max_batch=64, algo=algo, max_iter=20, layer_rows=z, **kw)
        for kind in KINDS:
            out, iters, soft = dec.decode(y, soft=kind)
            _check(w, out, iters, soft, kind, (algo, rate, kw, kind))
        dec.close()


@functools.lru_cache(maxsize=None)
def staircase():
    N2, K2 = 12960, 6480
    rows, cols = codes.dvbs2_profile_edges(N2, K2)
    return rows, cols, N2, K2, oracle.Graph(rows, cols, N2 - K2, N2, K2)


@functools.lru_cache(maxsize=None)
def staircase_want(frames, f16):
    rows, cols, N2, K2, og = staircase()
    y = channel.awgn_frames(N2, 0, frames, 0.72, seed=14)
    y.setflags(write=False)
    return y, SR.expected(og, y, "ms", 25, f16=f16)


@pytest.mark.parametrize("frames", [64, 256])
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_column_fused_rows(built, f16, frames):
    """DVB-S2-profile staircase code (N = 12960): the fused degree-2 columns' R reach memory only because a soft call asks
    the column-fused check kernels to store them.  Wide form at 1 frame per lane; wide, narrow and half at 4."""
    rows, cols, N2, K2, og = staircase()
    g = L.Graph(rows, cols, N2 - K2, N2)
    y, w = staircase_want(frames, f16)
    assert np.unique(w["iters"]).size >= 3
    for fpl, form in ((1, {"link_narrow": False}), (4, {"link_narrow": False}), (4, {"link_narrow": True}), (4, {"link_half": True})):
        dec = L.Decoder(g, K2, max_batch=frames, algo="ms", max_iter=25, frames_per_lane=fpl, msg_dtype="f16" if f16 else "f32", tune=form)
        dec.set_timing(True)
        for kind in KINDS:
            out, iters, soft = dec.decode(y, soft=kind)
            _check(w, out, iters, soft, kind, (f16, frames, fpl, form, kind))
        names = [k["name"] for k in dec.kernel_times()]
        assert any(n.startswith("check_link") for n in names), names        # a decoder with linked rows
        dec.close()


@pytest.mark.parametrize("name,algo,kw", [("ms-stream", "ms", dict(layer_rows=0, frames_per_lane=2)),
                                          ("layered-stream", "layered", dict(layer_rows=U.Z, frames_per_lane=2, tune=STREAM)),
                                          ("layered-record", "layered", dict(layer_rows=U.Z, tune=RECORD))],
                         ids=["ms-stream", "layered-stream", "layered-record"])
def test_full_work(graph, name, algo, kw):
    """early_term = 0 with max_iter below the batch's smallest iteration count: every frame's expectation is the
    oracle's posterior of round max_iter."""
    snr = TU.chain_points(algo)[1]
    y = TU.chain_received(snr)[2]
    smallest = int(TU.chain_oracle(algo, snr)[1].min())
    max_iter = smallest - 1
    assert max_iter >= 2
    w = SR.expected(U.bg1()[2], y, algo, max_iter, layer_rows=U.Z)
    assert (w["iters"] == max_iter).all()
    dec = L.Decoder(graph, U.K, max_batch=64, algo=algo, max_iter=max_iter, early_term=False, **kw)
    for kind in KINDS:
        out, iters, soft = dec.decode(y, soft=kind)
        _check(w, out, iters, soft, kind, (name, kind))
    dec.close()


def _handover_want(case):
    block, algo, frames, sd_easy, sd_hard, every = case
    y = CC.received(block, frames, sd_easy, sd_hard, every)
    return y, SR.expected(U.bg1()[2], y, algo, CC.MAXIT)


def _device_soft(dec, yd, B, kind):
    import torch
    nb = L.out_bytes(U.K, B)
    out = torch.full((nb,), 0xEE, dtype=torch.uint8, device="cuda")
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    soft = torch.full((B * U.N,), float("nan"), dtype=torch.float32, device="cuda")
    dec.decode_device(yd.data_ptr(), B, out.data_ptr(), nb, it.data_ptr(), torch.cuda.current_stream().cuda_stream,
                      soft_ptr=soft.data_ptr(), soft_floats=B * U.N, soft=kind)
    torch.cuda.synchronize()
    return out.cpu().numpy(), it.cpu().numpy(), soft.cpu().numpy()


def test_polled_hand_over(graph):
    """256 frames, polled every round, CRC off: after round 3 the 46 frames still running go to the child decoder, which
    catches the 42 that freeze later and the 4 that reach max_iter in its own rounds, addressed through the slot map."""
    import torch
    case = CC.POLLED
    B = case[2]
    y, w = _handover_want(case)
    assert np.array_equal(w["iters"], CC.want_syndrome(*case)[1])
    rnd = CC.handover_round(w["iters"], B, 64)
    running = w["iters"] > rnd
    print("polled: hand-over after round", rnd, "running", int(running.sum()), "reach max_iter", int((w["iters"] == CC.MAXIT).sum()))
    assert rnd == 3 and running.sum() == 46 and (w["iters"][running] == CC.MAXIT).sum() == 4
    yd = torch.tensor(y).cuda()
    results = []
    for tune in ({}, {"compact": -1}):
        dec = L.Decoder(graph, U.K, max_batch=B, algo="ms", max_iter=CC.MAXIT, frames_per_lane=1, poll_interval=1, tune=tune)
        for kind in KINDS:
            out, it, soft = _device_soft(dec, yd, B, kind)
            _check(w, out, it, soft, kind, ("polled", tune, kind))
            results.append(soft)
            full = ac.frame_rounds_without_handover(w["iters"], 64, CC.MAXIT)
            assert (dec.stats()["frame_rounds"] < full) == (not tune), (tune, dec.stats()["frame_rounds"], full)
        dec.close()
    assert np.array_equal(SR.bits(results[0]), SR.bits(results[2])) and np.array_equal(SR.bits(results[1]), SR.bits(results[3]))


def test_device_side_tail(graph):
    """2048 frames without host polling, CRC off: after round 3 the 127 frames still running move to the overflow tiles,
    where 122 freeze later and 5 reach max_iter; the kernel follows tile_select and addresses them through tail_map."""
    import torch
    case = CC.TAIL
    B = case[2]
    y, w = _handover_want(case)
    assert np.array_equal(w["iters"], CC.want_syndrome(*case)[1])
    rnd = CC.handover_round(w["iters"], B, 512)
    running = w["iters"] > rnd
    print("tail: hand-over after round", rnd, "running", int(running.sum()), "reach max_iter", int((w["iters"] == CC.MAXIT).sum()))
    assert rnd == 3 and running.sum() == 127 and (w["iters"][running] == CC.MAXIT).sum() == 5
    yd = torch.tensor(y).cuda()
    results = []
    for tune in ({}, {"device_tail": False}):
        dec = L.Decoder(graph, U.K, max_batch=B, algo="ms", max_iter=CC.MAXIT, frames_per_lane=1, poll_interval=0, tune=tune)
        for kind in KINDS:
            out, it, soft = _device_soft(dec, yd, B, kind)
            _check(w, out, it, soft, kind, ("tail", tune, kind))
            results.append(soft)
            full = ac.frame_rounds_without_handover(w["iters"], 64, CC.MAXIT)
            assert (dec.stats()["frame_rounds"] < full) == (not tune), (tune, dec.stats()["frame_rounds"], full)
        dec.close()
    assert np.array_equal(SR.bits(results[0]), SR.bits(results[2])) and np.array_equal(SR.bits(results[1]), SR.bits(results[3]))


@pytest.mark.parametrize("algo,kw", [("ms", dict(layer_rows=0, frames_per_lane=2)), ("layered", dict(layer_rows=U.Z, frames_per_lane=2, tune=STREAM)),
                                     ("layered", dict(layer_rows=U.Z, tune=RECORD))], ids=["ms-stream", "layered-stream", "layered-record"])
def test_entry_point_buffers(graph, algo, kw):
    """soft_dev at 4 modulo 16 bytes between guard floats, 70 frames on max_batch = 128 (a ragged tile and 58 padding
    frames): guards and the rows behind frame 70 are untouched; out_dev = NULL and iters_dev = NULL leave soft correct."""
    import torch
    B = 70
    y = CC.received("chain", 150, 0.75, 0.98, 3)[:B]
    w = SR.expected(U.bg1()[2], y, algo, CC.MAXIT, layer_rows=U.Z)
    dec = L.Decoder(graph, U.K, max_batch=128, algo=algo, max_iter=CC.MAXIT, **kw)
    yd = torch.tensor(y).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    nb = L.out_bytes(U.K, B)
    guard, room = 33, 128 * U.N                 # 33 floats: the buffer starts 4 bytes past a 16-byte boundary
    for kind in KINDS:
        for with_out in (True, False):
            buf = torch.full((guard + room + guard,), -777.0, dtype=torch.float32, device="cuda")
            assert (buf.data_ptr() + 4 * guard) % 16 == 4
            out = torch.zeros(nb, dtype=torch.uint8, device="cuda")
            it = torch.zeros(B, dtype=torch.int32, device="cuda")
            dec.decode_device(yd.data_ptr(), B, out.data_ptr() if with_out else None, nb if with_out else 0,
                              it.data_ptr() if with_out else None, stream, soft_ptr=buf.data_ptr() + 4 * guard, soft_floats=B * U.N, soft=kind)
            torch.cuda.synchronize()
            h = buf.cpu().numpy()
            assert (h[:guard] == -777.0).all() and (h[guard + B * U.N:] == -777.0).all(), (kind, with_out)
            SR.assert_same_bits(h[guard:guard + B * U.N], w[KEY[kind]], ~w["undefined"], str((algo, kind, with_out)))
            if with_out:
                assert np.array_equal(out.cpu().numpy(), w["out"]) and np.array_equal(it.cpu().numpy(), w["iters"])
    dec.close()


def test_refusals_enqueue_nothing_and_leave_no_state(graph):
    """soft_floats one short, an unknown kind, a NULL buffer, an overlap with llr_dev, a set tap and LDPC_ALGO_SP: the
    0xEE-filled buffers stay as they are and the next plain call is correct.  A plain call after a soft call launches what
    a decoder that never made a soft call launches."""
    import torch
    B = 64
    snr = TU.chain_points("ms")[1]
    y = TU.chain_received(snr)[2]
    want = TU.chain_oracle("ms", snr)
    yd = torch.tensor(y).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    nb = L.out_bytes(U.K, B)

    def plain(dec):
        out = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        it = torch.zeros(B, dtype=torch.int32, device="cuda")
        dec.decode_device(yd.data_ptr(), B, out.data_ptr(), nb, it.data_ptr(), stream)
        torch.cuda.synchronize()
        return out.cpu().numpy(), it.cpu().numpy()

    def refused(dec, code, **kw):
        out = torch.full((nb,), 0xEE, dtype=torch.uint8, device="cuda")
        it = torch.full((B,), -286331154, dtype=torch.int32, device="cuda")          # 0xEEEEEEEE
        soft = torch.full((B * U.N,), -286331154, dtype=torch.int32, device="cuda")
        args = dict(soft_ptr=soft.data_ptr(), soft_floats=B * U.N, soft="posterior")
        args.update(kw)
        if args["soft_ptr"] == "llr":
            args["soft_ptr"] = yd.data_ptr() + 4 * U.N
        with pytest.raises(L.LdpcError) as e:
            dec.decode_device(yd.data_ptr(), B, out.data_ptr(), nb, it.data_ptr(), stream, **args)
        assert e.value.code == code, (kw, str(e.value))
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0xEE).all() and (it.cpu().numpy() == -286331154).all() and (soft.cpu().numpy() == -286331154).all(), kw
        assert np.array_equal(yd.cpu().numpy(), y), kw

    ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = 1, 4, 5
    dec = L.Decoder(graph, U.K, max_batch=B, algo="ms", max_iter=U.MAX_ITER, layer_rows=0, frames_per_lane=2)
    for kw in (dict(soft_floats=B * U.N - 1), dict(soft=3), dict(soft_ptr=None), dict(soft_ptr="llr")):
        refused(dec, ERR_ARG, **kw)
        out, it = plain(dec)
        assert np.array_equal(out, want[0]) and np.array_equal(it, want[1]), kw
    dec.set_tap(2)
    refused(dec, ERR_STATE)
    dec.set_tap(0)
    out, it = plain(dec)
    assert np.array_equal(out, want[0]) and np.array_equal(it, want[1])
    # a plain call after a soft call: the launches of a decoder that never made one
    fresh = L.Decoder(graph, U.K, max_batch=B, algo="ms", max_iter=U.MAX_ITER, layer_rows=0, frames_per_lane=2)
    _device_soft(dec, yd, B, "posterior")
    seen = []
    for d in (dec, fresh):
        d.set_timing(True)
        out, it = plain(d)
        assert np.array_equal(out, want[0]) and np.array_equal(it, want[1])
        st = d.stats()
        seen.append((st["launches_check"], st["launches_var"], sorted((k["name"], k["launches"]) for k in d.kernel_times())))
    assert seen[0] == seen[1], seen
    assert seen[0][2] and not any("soft_settle_kernel" in n for n, _ in seen[0][2])
    dec.set_timing(True)
    _device_soft(dec, yd, B, "posterior")
    assert any("soft_settle_kernel" in k["name"] for k in dec.kernel_times())
    dec.close()
    fresh.close()
    sp = L.Decoder(graph, U.K, max_batch=B, algo="sp", max_iter=U.MAX_ITER, layer_rows=0, frames_per_lane=2)
    refused(sp, ERR_UNSUPPORTED)
    out, it = plain(sp)
    w_sp = oracle.decode(U.bg1()[2], y, "sp", max_iter=U.MAX_ITER, llr_scale=8.0)
    assert np.array_equal(out, w_sp["out"]) and np.array_equal(it, w_sp["iters"])
    sp.close()


@pytest.mark.parametrize("max_batch", [64, 70])
def test_host_path_in_groups(graph, max_batch):
    """150 frames through ldpc_decode_soft in launch groups of 64 and of 70 (ragged tiles), and the same over the device
    list [0, 0]."""
    y = CC.received("chain", 150, 0.75, 0.98, 3)
    w = SR.expected(U.bg1()[2], y, "ms", CC.MAXIT)
    for kw in (dict(), dict(frames_per_lane=2, poll_interval=1), dict(devices=[0, 0])):
        dec = L.Decoder(graph, U.K, max_batch=max_batch, algo="ms", max_iter=CC.MAXIT, **kw)
        for kind in KINDS:
            out, iters, soft = dec.decode(y, soft=kind)
            _check(w, out, iters, soft, kind, (max_batch, kw, kind))
        out, iters = dec.decode(y)              # and the plain call on the same handle afterwards
        assert np.array_equal(out, w["out"]) and np.array_equal(iters, w["iters"])
        dec.close()


def test_coder_decode_soft(built, tmp_path):
    """Coder::decodeSoft under setRateMatch and setTransportBlock (tests/cpp/coder_soft.cpp)."""
    exe = str(tmp_path / "coder_soft")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "coder_soft.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "myldpccppapi_amd"), "-lmyldpc", "-lldpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myldpccppapi_amd")])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    f = dict(kv.split("=") for kv in p.stdout.split())
    assert f["refused"] == "ok" and f["same"] == "ok" and f["ext"] == "ok", p.stdout
    assert int(f["signs"]) == 0 and int(f["checked"]) > 30 * 1128, p.stdout
