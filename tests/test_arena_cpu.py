"""CPU side of tests/test_gpu_arena.py: the carve arithmetic of arena_util.Arena on a CPU tensor, and the oracle-side
preconditions of the GPU cases for the committed seeds (arena_cases.py) -- a seed that tests nothing fails here."""
import numpy as np
import pytest

import arena_cases as ac
from arena_util import Arena, FILL, NAN_WORD


def test_carve_phases_guards_and_disjoint_intervals():
    a = Arena(1 << 16, device="cpu")
    asked = []
    for i, (n, align, phase, guard) in enumerate([(100, 16, 4, 64), (1, 2, 1, 64), (0, 16, 0, 64), (333, 16, 12, 64),
                                                  (64, 256, 0, 64), (7, 2, 1, 0), (41, 16, 8, 200), (5, 1, 0, 1),
                                                  (1000, 4, 0, 64), (9, 16, 15, 64)]):
        p = a.carve(n, align, phase, guard, name="b%d" % i)
        assert p % align == phase
        asked.append((p - a.base, n, guard))
    assert [(lo, n) for lo, n, _ in a.carved] == [(lo, n) for lo, n, _ in asked]
    end = 0
    for lo, n, guard in asked:                     # ascending, disjoint, `guard` free bytes before each ...
        assert lo >= end + guard
        end = lo + n
    assert a.size - end >= asked[-1][2]            # ... and behind the last
    m = a.outside_mask()
    assert m.sum() == a.size - sum(n for _, n, _ in asked)
    for lo, n, guard in asked:
        assert not m[lo:lo + n].any() and m[lo - guard:lo].all()
    with pytest.raises(MemoryError):
        a.carve(1 << 16)
    with pytest.raises(ValueError):
        a.carve(8, align=4, phase=4)
    # the guard behind a buffer is what the NEXT carve leaves: at least its own guard
    b = Arena(4096, device="cpu")
    p0 = b.carve(10, 2, 1, guard=64)
    p1 = b.carve(10, 2, 1, guard=64)
    assert p1 - (p0 + 10) >= 64 and p0 - b.base >= 64
    with pytest.raises(MemoryError):               # no room for the guard behind it
        b.carve(4096 - (p1 + 10 - b.base) - 64 - 63, 1, 0, guard=64)


def test_data_round_trip_poison_and_the_untouched_checks():
    a = Arena(4096, device="cpu")
    pf = a.carve(40, 16, 4, name="floats")
    pb = a.carve(33, 2, 1, name="bytes")
    a.assert_untouched()
    a.assert_all_untouched()
    x = np.arange(10, dtype=np.float32) - 3.5
    a.put_floats(pf, x)
    assert np.array_equal(a.get(pf, 10, np.float32), x)
    a.poison(pf + 8, 3)
    assert np.array_equal(a.get(pf, 10, np.uint32)[2:5], np.full(3, NAN_WORD, np.uint32))
    assert np.isnan(a.get(pf, 10, np.float32)[2:5]).all()
    a.put(pb, np.arange(20, dtype=np.uint8))
    a.assert_tail_untouched(pb, 20, 33)
    with pytest.raises(AssertionError):
        a.assert_tail_untouched(pb, 19, 33)
    a.assert_untouched()                           # writes inside carved buffers are not its business
    with pytest.raises(AssertionError):
        a.assert_all_untouched()
    a.fill(pb, 33)
    a.fill(pf, 40)
    a.assert_all_untouched()
    with pytest.raises(ValueError):                # not inside a carved buffer
        a.put(pb + 30, np.zeros(4, np.uint8))
    # a byte behind the end of "bytes" and one before the start of "floats": named, with the offset
    a.buf[pb + 33 - a.base] = 0
    with pytest.raises(AssertionError, match=r"1 bytes past its end of 'bytes' \(offset \+33"):
        a.assert_untouched()
    a.buf[pb + 33 - a.base] = FILL
    a.buf[pf - 2 - a.base] = 1
    with pytest.raises(AssertionError, match=r"2 bytes before its start of 'floats' \(offset -2"):
        a.assert_untouched()


@pytest.mark.parametrize("group", list(ac.GROUPS))
def test_every_engine_row_stops_frames_at_several_iterations(group):
    """Each case's frames stop at three or more distinct iteration counts, at least one runs to max_iter, at least one
    converges, and the oracle defines all of them (the layered and fused arithmetic can leave a frame undefined)."""
    for name in ac.GROUPS[group]:
        c = ac.CASES[name]
        w = ac.case_want(c)
        it = w["iters"]
        assert it.size == c["frames"] and w["ok"].all(), name
        assert np.unique(it).size >= 3, (name, np.unique(it))
        assert (it == ac.MAXIT).any() and (it < ac.MAXIT).any(), name
        assert w["converged"].any() and not w["converged"].all(), name
        assert c["max_batch"] == c["frames"] + 64 * max(c["V"], 1)
        if c["pack"] == ac.PACK_BYTES and ac.code(c["code"])["K"] % 8:
            # the gap bits between frames exist: some byte of the output belongs to no frame
            K = ac.code(c["code"])["K"]
            assert np.setdiff1d(np.arange(w["out"].size), ac.frame_byte_index(K, c["frames"]).reshape(-1)).size > 0


@pytest.mark.parametrize("name", ac.GROUPS["polled_tail"] + ac.GROUPS["device_tail"])
def test_tail_cases_reach_their_hand_over(name):
    """From the oracle's iteration counts alone: after some round at most 512 frames and at most a quarter of the batch
    still run, at least 10 of them to max_iter; every tile keeps a running frame to the last round, so without a
    hand-over frame_rounds would be iterations x tiles x tile size."""
    c = ac.CASES[name]
    F = 64 * c["V"]
    tiles = -(-c["frames"] // F)
    variants = (0, 1, 2, 3) if c["poll"] else (0,)              # the call sequence draws other hard frames per call
    seen = set()
    for v in variants:
        if c["poll"]:            # the call sequence decodes max_batch frames of the same kind
            full = ac.case_want(c, frames=c["max_batch"], variant=v)["iters"]
            assert ac.handover_round(full) is not None and (full == ac.MAXIT).sum() >= 10
            assert ac.frame_rounds_without_handover(full, F) == ac.MAXIT * -(-c["max_batch"] // F) * F
        it = ac.case_want(c, variant=v)["iters"]
        rnd = ac.handover_round(it)
        assert rnd is not None and rnd <= ac.MAXIT - 3, (name, v, rnd)
        assert (it == ac.MAXIT).sum() >= 10, (name, v)
        assert ac.running_after(it, rnd) >= (it == ac.MAXIT).sum()
        assert ac.frame_rounds_without_handover(it, F) == ac.MAXIT * tiles * F, (name, v)
        seen.add(tuple(np.nonzero(it == ac.MAXIT)[0]))
    assert len(seen) == len(variants)
    if not c["poll"]:
        assert tiles >= 4 * (512 // F) and c["frames"] == 2100     # tiles >= 4 * overflow tiles
        # the smaller call of the sequence has too few tiles for the device-side tail
        assert -(-300 // F) < 4 * (512 // F)
        easy = ac.case_want(c, kind="easy")["iters"]
        assert easy.max() < ac.MAXIT and easy.min() >= 1
