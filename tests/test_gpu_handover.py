"""The straggler hand-over on batches of more than 4096 frames, against the CPU oracle on every frame: all output bytes,
all iteration counts and the converged count of the whole batch, bit for bit.

Above 4096 frames the row gather walks the parent's tiles in chunks, sum-product's hard bits travel through the per-wave
gather (whole words, or 16-bit fields of four words for a child with tiles of 256), the device-side tail lists more than one
mask word per thread, and the polled chain runs 1024 -> 512 -> 64 frames.  That each case reaches the path it is there for
follows from the oracle's iteration counts alone: tests/test_handover_cpu.py (inputs and model: handover_cases.py)."""
import numpy as np
import pytest

import myldpccppapi_amd as L
import arena_cases as ac
import handover_cases as hc

pytestmark = pytest.mark.gpu
ALGO_IDS = ["sp", "ms", "ms16"]


def _graph(name):
    cd = hc.case_code(name)
    return L.Graph(cd["rows"], cd["cols"], cd["M"], cd["N"]), cd


def _assert_oracle(dec, out, iters, w, what):
    assert np.array_equal(out, w["out"]), what
    assert np.array_equal(iters, w["iters"]), what
    st = dec.stats()
    assert st["frames_converged"] == w["n_conv"], (what, st)     # syndrome-clean frames, flags scattered back by the chain
    return st


def _polled(name, algo, f16, tune, lanes):
    """Two calls per decoder (the chain is reused by the second) against the oracle; frame_rounds between the model's
    lower bound and the value of a decoder that never hands over."""
    g, cd = _graph(name)
    y, w = hc.inputs(name), hc.want(name, algo, f16)
    B = y.shape[0]
    for fpl in lanes:
        ev = hc.model(w["iters"], B, fpl, tune.get("compact", 0))
        assert bool(ev) == (tune.get("compact", 0) != -1)
        dec = L.Decoder(g, cd["K"], max_batch=B, algo=algo, max_iter=hc.MAXIT, poll_interval=1, frames_per_lane=fpl,
                        msg_dtype="f16" if f16 else "f32", tune=tune)
        for call in range(2):
            out, iters = dec.decode(y)
            st = _assert_oracle(dec, out, iters, w, (tune, fpl, call))
            assert st["iterations_launched"] == hc.MAXIT and st["frames"] == B, (tune, fpl, st)
            if ev:
                full = ac.frame_rounds_without_handover(w["iters"], 64 * fpl, hc.MAXIT)
                low = hc.frame_rounds_lower_bound(w["iters"], fpl, ev)
                print("frame_rounds", name, algo, f16, tune, fpl, low, st["frame_rounds"], full)
                assert low <= st["frame_rounds"] < full, (tune, fpl, ev, low, st["frame_rounds"], full)
        dec.close()


@pytest.mark.parametrize("tune_name", list(hc.POLLED_TUNES))
@pytest.mark.parametrize("algo,f16", hc.ALGOS, ids=ALGO_IDS)
def test_polled_chain_above_4096_frames(built, algo, f16, tune_name):
    """4500 frames with host polling.  Default threshold: 513..1024 frames go to the 1024-frame decoder through the chunked
    row gather (sum-product's hard bits as whole words at V = 1, 2 and as 16-bit fields at V = 4), 65..127 of them on to
    the 512-frame decoder and, for min-sum, the rest to the last tile of 64.  Thresholds 400 / 100 / 60 enter the chain at
    the 512-frame decoder row by row, there value by value, and at the last decoder; -1: no hand-over; q_order -1: Q rows
    in edge order in every decoder of the chain."""
    _polled("A", algo, f16, hc.POLLED_TUNES[tune_name], hc.polled_lanes(algo, tune_name))


@pytest.mark.parametrize("algo", ["sp", "ms"])
def test_staircase_code_above_4096_frames(built, algo):
    """The same on the staircase code: its column-fused check launch keeps the linked rows of Q at other places in a
    decoder with tiles of 64 than in one with tiles of 256, and the chunked gather translates between the two."""
    _polled("S", algo, False, {}, (1, 4))


@pytest.mark.parametrize("algo", ["sp", "ms"])
def test_one_large_handle_changing_calls(built, algo):
    """max_batch = 8192: calls of 4500, 3000 and 4500 frames, then an easy batch and a single tile of it.  The gather's
    branch follows the call's tiles, not the handle's, and no call sees the slot maps, the moved-bit masks or the chain of
    the call before."""
    g, cd = _graph("A")
    dec = L.Decoder(g, cd["K"], max_batch=hc.SEQUENCE_BATCH, algo=algo, max_iter=hc.MAXIT, poll_interval=1, frames_per_lane=4)
    for name, n in hc.SEQUENCE:
        w = hc.want(name, algo, False, n)
        out, iters = dec.decode(hc.inputs(name)[:n])
        st = _assert_oracle(dec, out, iters, w, (name, n))
        assert st["frames"] == n and st["iterations_launched"] == int(w["iters"].max()), (name, n, st)
        assert st["batch_time"] == int(w["iters"].max()), (name, n, st)
        full = ac.frame_rounds_without_handover(w["iters"], 256, hc.MAXIT)
        if hc.model(w["iters"], hc.SEQUENCE_BATCH, 4):
            assert 0 < st["frame_rounds"] < full, (name, n, st, full)
        else:
            assert st["frame_rounds"] == full, (name, n, st, full)
    dec.close()


@pytest.mark.parametrize("tune_name", list(hc.DEVICE_TUNES))
@pytest.mark.parametrize("algo,f16", hc.ALGOS, ids=ALGO_IDS)
def test_device_side_tail_above_256_mask_words(built, algo, f16, tune_name):
    """16500 frames without host polling: 258 mask words at V = 1 and 260 at V = 4, so every thread of a block lists two
    words before the scan.  With the tail off and with a threshold that is reached later the same results."""
    import torch
    tune = hc.DEVICE_TUNES[tune_name]
    g, cd = _graph("B")
    y, w = hc.inputs("B"), hc.want("B", algo, f16)
    B, K = y.shape[0], cd["K"]
    yd = torch.tensor(y).cuda()                                   # a copy: the shared inputs are read-only
    nb = L.out_bytes(K, B)
    for fpl in (1, 4):
        dec = L.Decoder(g, K, max_batch=B, algo=algo, max_iter=hc.MAXIT, poll_interval=0, frames_per_lane=fpl,
                        msg_dtype="f16" if f16 else "f32", tune=tune)
        for call in range(2):
            out = torch.full((nb,), 0xEE, dtype=torch.uint8, device="cuda")
            it = torch.zeros(B, dtype=torch.int32, device="cuda")
            dec.decode_device(yd.data_ptr(), B, out.data_ptr(), nb, it.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            st = _assert_oracle(dec, out.cpu().numpy(), it.cpu().numpy(), w, (tune, fpl, call))
            assert st["batch_time"] == hc.MAXIT and st["iterations_launched"] == hc.MAXIT, (tune, fpl, st)
            full = ac.frame_rounds_without_handover(w["iters"], 64 * fpl, hc.MAXIT)
            print("frame_rounds B", algo, f16, tune, fpl, st["frame_rounds"], full)
            if tune.get("device_tail", True):
                assert 0 < st["frame_rounds"] < full, (tune, fpl, st, full)
        dec.close()
