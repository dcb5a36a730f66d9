"""Inputs, oracle results and a model of the hand-over rule for tests/test_gpu_handover.py (a helper, not a test module).

The straggler hand-over above 4096 frames: the chunked row gather, the per-wave hard-bit gather of sum-product, the
device-side tail that lists more than 256 mask words, and the chain 1024 -> 512 -> 64 frames.  Everything here runs on
the CPU; tests/test_handover_cpu.py checks from the oracle's iteration counts alone that every case reaches the path it is
there for, so that a seed which tests nothing fails there instead of passing silently on the GPU."""
import functools

import numpy as np

import oracle
from myldpccppapi_amd import channel
import arena_cases as ac
from util import converged_frames

MAXIT = 30
ALGOS = (("sp", False), ("ms", False), ("ms", True))        # (algo, fp16 messages)

# frames: batch; base / med / hard: noise sd of the three populations; n_med, n_hard: how many frames of a random subset
# (default_rng(perm).permutation) are replaced by the medium and by the hard population; n_stuck: frames of the
# medium population with STUCK_COLUMNS values of 12 (exp(8 * 12) = inf: sum-product's priors are NaN there, the NaNs spread
# over the frame within a few rounds, and its rule then keeps every bit as it was last decided -- the hard bits of these
# frames are state that a hand-over in any round has to carry; min-sum just sees three very reliable values)
CASES = {
    # polled chain: hundreds of frames still run when a quarter of the batch is reached, a few dozen some rounds later
    "A": dict(code="w576", frames=4500, base=0.55, n_med=720, med=0.70, n_hard=14, hard=1.3, n_stuck=5, perm=7),
    # device-side tail: more than 256 tiles of 64 frames, i.e. more than 256 mask words at V = 1 and at V = 4
    "B": dict(code="w576", frames=16500, base=0.55, n_med=400, med=0.70, n_hard=14, hard=1.3, n_stuck=5, perm=7),
    # the staircase code: column-fused check launch, rows that sit at different places in parent and child
    "S": dict(code="ira", frames=4500, base=0.62, n_med=800, med=0.80, n_hard=14, hard=1.6, n_stuck=5, perm=7),
}
STUCK_COLUMNS, STUCK_VALUE = 3, 12.0


def stuck_frames(name):
    """indices of the case's frames with NaN priors under sum-product"""
    c = CASES[name]
    order = np.random.default_rng(c["perm"]).permutation(c["frames"])
    return np.sort(order[:c["n_stuck"]])


# the decoders of the polled tests on case A (poll_interval = 1, max_batch = frames), by name: Decoder(tune=...)
POLLED_TUNES = {"default": {}, "compact400": {"compact": 400}, "compact100": {"compact": 100}, "compact60": {"compact": 60},
                "off": {"compact": -1}, "edge_order": {"q_order": -1}}
# ... and of the asynchronous tests on case B (poll_interval = 0)
DEVICE_TUNES = {"default": {}, "compact100": {"compact": 100}, "off": {"device_tail": False}}


def polled_lanes(algo, tune_name):
    """frames_per_lane of the polled decoders: tiles of 64 and of 256 frames; of 128 once"""
    return (1, 2, 4) if algo == "sp" and tune_name == "default" else (1, 4)


# the calls of one max_batch = 8192 handle, in order: the first `frames` frames of a case or of the easy batch (every frame
# of which converges within a few rounds; its 200-frame call is a single tile at V = 4: no hand-over at all)
SEQUENCE_BATCH = 8192
SEQUENCE = (("A", 4500), ("A", 3000), ("A", 4500), ("easy", 4500), ("easy", 200))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """float32 [frames, N], read-only: the all-zero word over AWGN, three populations and the stuck frames"""
    if name == "easy":
        y = channel.awgn_frames(ac.code("w576")["N"], 60000, 4500, 0.5, seed=4)
    else:
        c = CASES[name]
        N, B = ac.code(c["code"])["N"], c["frames"]
        y = channel.awgn_frames(N, 0, B, c["base"], seed=1)
        order = np.random.default_rng(c["perm"]).permutation(B)
        med, hard = order[:c["n_med"]], order[c["n_med"]:c["n_med"] + c["n_hard"]]
        y[med] = channel.awgn_frames(N, 20000, med.size, c["med"], seed=2)
        y[hard] = channel.awgn_frames(N, 40000, hard.size, c["hard"], seed=3)
        rng = np.random.default_rng(c["perm"] + 1)
        for f in stuck_frames(name):
            y[f, rng.choice(N, STUCK_COLUMNS, replace=False)] = STUCK_VALUE
    y.setflags(write=False)
    return y


def case_code(name):
    return ac.code("w576" if name == "easy" else CASES[name]["code"])


@functools.lru_cache(maxsize=None)
def want(name, algo, f16, frames=None):
    """oracle.decode of the first `frames` frames of inputs(name) (default: all), once per process; "n_conv": the
    syndrome-clean frames of its hard bits"""
    cd = case_code(name)
    y = inputs(name)
    if frames == y.shape[0]:
        return want(name, algo, f16)
    r = oracle.decode(cd["og"], y if frames is None else y[:frames], algo, max_iter=MAXIT, msg_f16=f16)
    r["n_conv"] = int(converged_frames(cd["rows"], cd["cols"], cd["M"], r["hard"]).sum())
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def running_after(iters, rnd):
    """frames still running after round rnd"""
    return int((np.asarray(iters) > rnd).sum())


# ---- the hand-over rule as include/ldpc_hip.h and DESIGN.md state it; it knows nothing of the library ----

def chain(max_batch, V):
    """[(capacity, tile size)] of the decoders behind a batch decoder, largest first"""
    levels = [(1024, 256 if V == 4 else 64)] if max_batch >= 4096 else []
    return levels + [(512, 64), (64, 64)]


def model(iters, max_batch, V, compact=0, max_iter=MAXIT):
    """[(round, count, target capacity)]: the hand-overs of one polled call (poll_interval = 1) whose frames stop after
    `iters` rounds.  After a round the frames of a level move on when running <= threshold, 4 * running <= the frames of
    that level and the level has more than one tile; they go to the smallest decoder of the chain that holds them.  The
    batch decoder's threshold is tune_compact (default and maximum: the capacity of the first decoder of the chain, -1: no
    hand-over); a decoder of the chain hands over what the next one holds."""
    iters = np.asarray(iters)
    levels = chain(max_batch, V)
    out = []
    if compact < 0:
        return out
    frames, tile, at = iters.size, 64 * V, -1                # at: index into levels, -1 = the batch decoder
    threshold = min(levels[0][0], compact) if compact else levels[0][0]
    for rnd in range(1, max_iter):
        if at + 1 >= len(levels):
            break                                           # the last decoder keeps what it has
        run = running_after(iters, rnd)
        if run == 0:
            break
        if run <= threshold and 4 * run <= frames and -(-frames // tile) > 1:
            at = max(i for i in range(at + 1, len(levels)) if levels[i][0] >= run)
            out.append((rnd, run, levels[at][0]))
            frames, tile = run, levels[at][1]
            threshold = levels[at + 1][0] if at + 1 < len(levels) else 0
    return out


def frame_rounds_lower_bound(iters, V, events, max_iter=MAXIT):
    """What stats()["frame_rounds"] cannot be below: the batch decoder's occupied tiles in every round up to the first
    modelled hand-over, plus one tile of 64 frames per later round that still has a running frame (wherever the frames
    sit by then, some tile holds them, and no tile is smaller)."""
    iters = np.asarray(iters)
    F = 64 * V
    tiles = -(-iters.size // F)
    pad = np.zeros(tiles * F, iters.dtype)
    pad[:iters.size] = iters
    last = pad.reshape(tiles, F).max(axis=1)                # the tile works in rounds 1 .. last
    first = events[0][0]
    end = int(min(iters.max(), max_iter))
    return int(F * np.minimum(last, first).sum()) + 64 * max(0, end - first)
