"""Shared set-up of the rate-matching tests: the index grid and the BG1-profile scenarios S1 .. S4 (DESIGN.md, table of
the rate-matching section).  Everything here is derived from ratematch_ref, codes.py and the oracle, never from the
library under test; the expensive parts are computed once per process and handed out read-only."""
import functools

import numpy as np

import oracle
from myldpccppapi_amd import codes

import ratematch_ref as ref

N_GRID = 1088


def grid_specs():
    """(P, filler) of the index grid: P in {0, 32} x fillers in {none, [328, 352), [P, P + 8)}."""
    return [(P, f) for P in (0, 32) for f in ((0, 0), (328, 352), (P, P + 8))]


def grid_cases(N=N_GRID):
    """(spec, k0, E) over the grid: k0 in {0, a filler position, the position just behind the fillers, Ncb - 1} and
    E in {1, L - 1, L, L + 1, 2L + 5}."""
    out = []
    for P, filler in grid_specs():
        spec = ref.Spec(N, P, filler)
        Ncb, L = spec.Ncb, spec.L
        k0s = {0, Ncb - 1}
        if spec.hi > spec.lo:
            k0s.add(spec.lo - P + 3)                     # on a filler
            k0s.add((spec.hi - P) % Ncb)                 # just behind them
        for k0 in sorted(k0s):
            for E in (1, L - 1, L, L + 1, 2 * L + 5):
                out.append((spec, k0, E))
    return out


# ---- scenarios: codes.nr_bg1_profile_base(Z = 16), N = 1088, K = 352; 64 frames; punctured prefix 32, fillers = code
#      bits [328, 352); fill_llr 10; max_iter 20, llr_scale 8, layer_rows 16
Z, FRAMES = 16, 64
N, K, M = 68 * Z, 22 * Z, 46 * Z
P, FILLER = 2 * Z, (328, 352)
MAX_ITER, LLR_SCALE = 20, 8.0
#: name -> (snr dB, [(k0, E) per transmission])
SCENARIOS = {"S1": (3.0, [(0, 1032)]), "S2": (4.0, [(0, 616)]), "S4": (2.0, [(0, 464), (488, 464)])}


def scenario_spec(erasure_llr):
    return ref.Spec(N, P, FILLER, 10.0, erasure_llr)


@functools.lru_cache(maxsize=None)
def bg1():
    rows, cols = codes.nr_bg1_profile_edges(Z)
    return rows, cols, oracle.Graph(rows, cols, M, N, K)


@functools.lru_cache(maxsize=None)
def payload():
    """(info bits uint8 [64, K] with the fillers zeroed, their bytes uint8 [64 * K/8], codewords uint8 [64, N])."""
    info = np.random.default_rng(1).integers(0, 2, (FRAMES, K), dtype=np.uint8)
    info[:, FILLER[0]:FILLER[1]] = 0
    base = codes.nr_bg1_profile_base(Z=Z)
    code = np.stack([codes.nr_bg1_profile_encode(base, Z, info[f]) for f in range(FRAMES)]).astype(np.uint8)
    for a in (info, code):
        a.setflags(write=False)
    return info, np.packbits(info, axis=1, bitorder="little").reshape(-1), code


@functools.lru_cache(maxsize=None)
def received(name):
    """[(k0, E, tx uint8 [64, E], rx float32 [64, E]) per transmission t]: noise of oracle.awgn, seed 100 + t."""
    snr, txs = SCENARIOS[name]
    sd = 10.0 ** (-snr / 20.0)
    out = []
    for t, (k0, E) in enumerate(txs):
        tx = ref.match(scenario_spec(0.0), payload()[2], k0, E)
        rx = oracle.awgn(E, 0, FRAMES, sd, seed=100 + t, codewords=tx)
        rx.setflags(write=False)
        out.append((k0, E, tx, rx))
    return out, sd


@functools.lru_cache(maxsize=None)
def recovered(name, erasure_llr, transmissions):
    """Decoder input y float32 [64, N] after the first `transmissions` transmissions, by ratematch_ref alone."""
    spec = scenario_spec(erasure_llr)
    soft = y = None
    for k0, E, _, rx in received(name)[0][:transmissions]:
        soft, y = ref.recover(spec, rx, k0, E, soft)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def oracle_decode(name, erasure_llr, transmissions, algo):
    """(out bytes, iters, frames with a wrong information bit) of oracle.decode on recovered(...)."""
    r = oracle.decode(bg1()[2], recovered(name, erasure_llr, transmissions), algo, max_iter=MAX_ITER, llr_scale=LLR_SCALE,
                      layer_rows=Z)
    wrong = (np.asarray(r["out"]).reshape(FRAMES, K // 8) != payload()[1].reshape(FRAMES, K // 8)).any(axis=1)
    return r["out"], r["iters"], int(wrong.sum())
