"""CPU side of tests/test_gpu_handover.py: the model of the hand-over rule on hand-made iteration counts, and the
oracle-side premises of the GPU cases for the committed seeds (handover_cases.py) -- from the oracle's iteration counts alone
every case must reach the hand-over path it is there for; a seed which does not fails here."""
import numpy as np
import pytest

import arena_cases as ac
import handover_cases as hc

ALGO_IDS = ["sp", "ms", "ms16"]


def _iters(*groups):
    """iteration counts from (frames, rounds) pairs"""
    return np.concatenate([np.full(n, r, np.int32) for n, r in groups])


def _stuck_frames_run_to_the_end(name, algo, it):
    """Sum-product: the frames with NaN priors never stop, so every hand-over of the call carries frames whose hard bits
    are kept, not decided anew (the only state a wrong hard-bit gather could spoil)."""
    stuck = hc.stuck_frames(name)
    y = hc.inputs(name)
    assert stuck.size >= 5 and ((y[stuck] == hc.STUCK_VALUE).sum(axis=1) == hc.STUCK_COLUMNS).all()
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(np.float32(8) * np.float32(hc.STUCK_VALUE)))
    if algo == "sp":
        assert (it[stuck] == hc.MAXIT).all(), it[stuck]


def test_model_on_hand_made_iteration_counts():
    # 5000 frames, 1000 / 400 / 100 / 40 of them still running after rounds 2 / 4 / 6 / 8
    it = _iters((4000, 2), (600, 4), (300, 6), (60, 8), (40, 30))
    assert [hc.running_after(it, r) for r in (1, 2, 4, 6, 8, 29, 30)] == [5000, 1000, 400, 100, 40, 40, 0]
    # 1000 <= 1024 and a fifth of the batch; 400 is more than a quarter of 1000, 100 is not; 40 is more than a quarter of 100
    assert hc.model(it, 5000, 1) == [(2, 1000, 1024), (6, 100, 512)]
    assert hc.model(it, 5000, 4) == [(2, 1000, 1024), (6, 100, 512)]
    assert hc.chain(5000, 4)[0] == (1024, 256) and hc.chain(5000, 2)[0] == (1024, 64) and hc.chain(4095, 4)[0] == (512, 64)
    assert hc.model(it, 5000, 1, compact=400) == [(4, 400, 512), (8, 40, 64)]
    assert hc.model(it, 5000, 1, compact=99) == [(8, 40, 64)]       # straight to the last decoder, which keeps them
    assert hc.model(it, 5000, 1, compact=-1) == []
    assert hc.model(it, 5000, 1, compact=39) == []
    # below 4096 frames of max_batch the chain begins with the 512-frame decoder
    it = _iters((1500, 2), (440, 3), (60, 30))
    assert hc.model(it, 2000, 2) == [(2, 500, 512), (3, 60, 64)]
    # one tile: nothing moves; 1024 frames in four tiles of 256 (V = 4) do, in one tile they would not
    assert hc.model(_iters((200, 2), (40, 30)), 8192, 4) == []
    assert hc.model(_iters((200, 2), (40, 30)), 8192, 1) == [(2, 40, 64)]
    # everything stops: no hand-over after the round that finishes the batch
    assert hc.model(_iters((3000, 2), (1000, 3)), 8192, 4) == [(2, 1000, 1024)]
    # lower bound of frame_rounds: 79 tiles of 64 for two rounds, then one tile per round up to the last
    it = _iters((4000, 2), (600, 4), (300, 6), (60, 8), (40, 30))
    assert hc.frame_rounds_lower_bound(it, 1, hc.model(it, 5000, 1)) == 64 * 79 * 2 + 64 * 28


@pytest.mark.parametrize("algo,f16", hc.ALGOS, ids=ALGO_IDS)
def test_case_a_walks_the_chain_above_4096_frames(algo, f16):
    """More than 4096 frames, so that at every V the row gather takes its chunked branch (more than 4096 / F parent tiles)
    and sum-product's hard bits take the per-wave gather (more than 64 parent mask words per column); the default
    threshold hands 513..1024 frames to the 1024-frame decoder (tiles of 256 at V = 4: 16-bit fields), that one 65..127 to
    the 512-frame decoder, and for min-sum that one the rest to the last; the smaller thresholds enter the chain lower."""
    c = hc.CASES["A"]
    it = hc.want("A", algo, f16)["iters"]
    B = c["frames"]
    assert it.size == B > 4096 and (it == hc.MAXIT).sum() >= 10
    _stuck_frames_run_to_the_end("A", algo, it)
    for V in (1, 2, 4):
        F = 64 * V
        tiles = -(-B // F)
        assert tiles > 4096 // F and tiles * V > 64
        ev = hc.model(it, B, V)
        assert 513 <= ev[0][1] <= 1024 and ev[0][2] == 1024, ev
        assert 65 <= ev[1][1] <= 127 and ev[1][2] == 512, ev
        if algo == "ms":
            assert len(ev) == 3 and ev[2][2] == 64 and ev[2][1] >= (it == hc.MAXIT).sum(), ev
        ev = hc.model(it, B, V, compact=400)
        assert 128 <= ev[0][1] <= 512 and ev[0][2] == 512, ev          # row-wise gather into tiles of 64
        ev = hc.model(it, B, V, compact=100)
        assert 65 <= ev[0][1] <= 100 and ev[0][2] == 512, ev           # one value per thread, two child tiles
        ev = hc.model(it, B, V, compact=60)
        assert ev[0][1] <= 60 and ev[0][2] == 64 and len(ev) == 1, ev
        assert hc.model(it, B, V, compact=-1) == []
        for name, tune in hc.POLLED_TUNES.items():
            ev = hc.model(it, B, V, tune.get("compact", 0))
            if ev:       # the two bounds on frame_rounds leave room for a decoder that hands over, and none for one that does not
                assert ev[0][0] <= hc.MAXIT - 3 and ev[0][1] >= (it == hc.MAXIT).sum()
                assert hc.frame_rounds_lower_bound(it, V, ev) < ac.frame_rounds_without_handover(it, F, hc.MAXIT), (name, V)
    if f16:      # the issue's table: fp16 messages stay within a frame of fp32 in every round
        it32 = hc.want("A", algo, False)["iters"]
        assert all(abs(hc.running_after(it, r) - hc.running_after(it32, r)) <= 1 for r in range(1, 11))


@pytest.mark.parametrize("algo,f16", hc.ALGOS, ids=ALGO_IDS)
def test_case_b_lists_more_than_256_mask_words(algo, f16):
    """The device-side tail hands over after the first round with at most 512 frames and a quarter of the batch still
    running: 128..512 frames then, listed from more than 256 mask words (each thread of the block lists several)."""
    c = hc.CASES["B"]
    it = hc.want("B", algo, f16)["iters"]
    B = c["frames"]
    assert it.size == B and (it == hc.MAXIT).sum() >= 10
    _stuck_frames_run_to_the_end("B", algo, it)
    assert -(-B // 64) > 256
    for V in (1, 4):
        F = 64 * V
        tiles = -(-B // F)
        assert tiles * V > 256 and tiles >= 4 * (512 // F)             # words to list; tiles >= 4 x overflow tiles
    for threshold, lo in ((512, 128), (100, 10)):
        rnd = next(r for r in range(1, hc.MAXIT) if hc.running_after(it, r) <= threshold and 4 * hc.running_after(it, r) <= B)
        run = hc.running_after(it, rnd)
        assert lo <= run <= threshold and rnd <= hc.MAXIT - 3, (threshold, rnd, run)
        assert run >= (it == hc.MAXIT).sum()
    # every tile of 64 does not keep a frame to the end here; the value without a hand-over still lies far above what the
    # overflow tiles need from the hand-over round on
    assert ac.frame_rounds_without_handover(it, 64, hc.MAXIT) > 64 * 8 * hc.MAXIT


@pytest.mark.parametrize("algo", ["sp", "ms"])
def test_call_sequence_of_one_large_handle(algo):
    """max_batch = 8192 at V = 4 (32 tiles of 256): the 4500-frame calls enter the chain at the top, the 3000-frame call
    has 12 parent tiles -- a gather sized by the handle's 32 would take the other branch -- and hands over too; every
    frame of the easy batch converges, and its 200-frame call is one tile: no hand-over."""
    assert -(-hc.SEQUENCE_BATCH // 256) > 16
    seen = []
    for name, n in hc.SEQUENCE:
        it = hc.want(name, algo, False, n)["iters"]
        assert it.size == n
        ev = hc.model(it, hc.SEQUENCE_BATCH, 4)
        seen.append((name, n, ev))
        if name == "A":
            assert (it == hc.MAXIT).sum() >= 10
            assert ev and ev[0][1] >= 128, ev
            assert (ev[0][2] == 1024 and -(-n // 256) > 16) if n > 4096 else (ev[0][2] == 512 and -(-n // 256) <= 16), ev
        else:
            assert it.max() < hc.MAXIT and hc.want(name, algo, False, n)["n_conv"] == n
    assert seen[-1][2] == [] and seen[-1][1] <= 256
    assert [s[0] for s in seen] == ["A", "A", "A", "easy", "easy"] and seen[0][1] > seen[1][1] < seen[2][1]
    # frames are independent: the oracle of the first 3000 frames is the first 3000 frames of the oracle
    assert np.array_equal(hc.want("A", algo, False, 3000)["iters"], hc.want("A", algo, False)["iters"][:3000])


@pytest.mark.parametrize("algo", ["sp", "ms"])
def test_staircase_case_hands_over_hundreds_of_frames(algo):
    """The staircase code (column-fused check launch: linked rows sit elsewhere in parent and child) at 4500 frames: the
    first hand-over moves 128..1024 frames, row by row through the chunked gather, and at least 10 frames run to the end."""
    c = hc.CASES["S"]
    it = hc.want("S", algo, False)["iters"]
    B = c["frames"]
    assert it.size == B > 4096 and (it == hc.MAXIT).sum() >= 10
    _stuck_frames_run_to_the_end("S", algo, it)
    for V in (1, 4):
        ev = hc.model(it, B, V)
        assert 128 <= ev[0][1] <= 1024 and ev[0][0] <= hc.MAXIT - 3, ev
        assert hc.frame_rounds_lower_bound(it, V, ev) < ac.frame_rounds_without_handover(it, 64 * V, hc.MAXIT)
