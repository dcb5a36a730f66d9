"""Inputs of tests/test_osd_cpu.py and tests/test_gpu_osd.py (a helper, not a test module): the codes, the synthetic rows
of soft values and the decoder case.  Everything here runs on the CPU, is computed once per process and handed out
read-only; expectations come from osd_ref alone."""
import functools

import numpy as np

from myldpccppapi_amd import channel, codes

import osd_ref

f32 = np.float32
SCALE = 256.0

# ---- codes ------------------------------------------------------------------------------------------------------------

HAMMING = np.array([[1, 0, 1, 0, 1, 0, 1],
                    [0, 1, 1, 0, 0, 1, 1],
                    [0, 0, 0, 1, 1, 1, 1]], np.uint8)


def edges_of(H):
    """(rows, cols, M, N) in row-major order, as Graph takes them"""
    r, c = np.nonzero(H)
    return r.astype(np.int32), c.astype(np.int32), H.shape[0], H.shape[1]


def random_h(M, N, seed, weight=3):
    """every column has `weight` ones (fewer for M < weight), every row at least one"""
    rng = np.random.default_rng(seed)
    H = np.zeros((M, N), np.uint8)
    for n in range(N):
        H[rng.choice(M, min(weight, M), replace=False), n] = 1
    for m in range(M):
        if not H[m].any():
            H[m, rng.integers(N)] = 1
    return H


@functools.lru_cache(maxsize=None)
def code(name):
    """dict(H, rows, cols, M, N, K) of a named code; K is what the packed output carries (N - M for the standard codes,
    a multiple of 8 for the random ones, 4 for the Hamming code: no packed output)"""
    if name.startswith("wimax"):                      # "wimax_576_1/2"
        _, n, rate = name.split("_")
        N, rate = int(n), codes.RATE_NAMES.index(rate)
        rows, cols = codes.wimax_edges(rate, N)
        K, M, _ = codes.wimax_dims(rate, N)
        H = osd_ref.dense(rows, cols, M, N)
    elif name == "bg1":
        Z = 16
        rows, cols = codes.nr_bg1_profile_edges(Z)
        M, N, K = 46 * Z, 68 * Z, 22 * Z
        H = osd_ref.dense(rows, cols, M, N)
    elif name == "n100":                              # N no multiple of 32
        H = random_h(44, 100, seed=100)
        K = 56
    elif name == "deficient":                         # a duplicated row and an all-zero row: rank <= M - 2
        H = random_h(30, 72, seed=72)
        H[7] = H[3]
        H[11] = 0
        K = 40
    elif name == "hamming":
        H, K = HAMMING.copy(), 4
    else:
        raise KeyError(name)
    rows, cols, M, N = edges_of(H)
    H.setflags(write=False)
    return dict(H=H, rows=rows, cols=cols, M=M, N=N, K=K)


WIMAX_HALF, WIMAX_LONG, WIMAX_HIGH = "wimax_576_1/2", "wimax_1152_1/2", "wimax_1152_5/6"


# ---- soft rows with no decoder ------------------------------------------------------------------------------------------

def noisy(name, frames, sd, seed, llr=4.0):
    """float32 [frames, N]: the all-zero codeword over AWGN of standard deviation sd (a number, or (lo, hi): ascending
    over the batch), scaled to LLR-like units"""
    c = code(name)
    sd = np.linspace(sd[0], sd[1], frames).astype(f32)[:, None] if isinstance(sd, tuple) else f32(sd)
    y = channel.awgn_frames(c["N"], 0, frames, 1.0, seed=seed)
    return ((f32(1) + (y - f32(1)) * sd) * f32(llr)).astype(f32)


@functools.lru_cache(maxsize=None)
def synthetic(kind, name=WIMAX_HALF):
    """(soft float32 [frames, N], scale) for one of the edge cases"""
    c = code(name)
    N = c["N"]
    rng = np.random.default_rng(sum(map(ord, kind)))
    scale = SCALE
    if kind == "ties":                                # posteriors quantised to multiples of 1/4 with scale 4: weights 0 .. 12
        soft = np.clip(np.round(noisy(name, 24, 0.8, seed=11, llr=1.0) * 4), -12, 12).astype(f32) / f32(4)
        scale = 4.0
    elif kind == "specials":                          # zeros of both signs, NaN, +-inf, values above the cap, denormals
        soft = noisy(name, 24, 0.75, seed=12)
        vals = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 300.0, -300.0, 255.99, -256.0, 1e-40, -1e-40, 65535.0 / 256, -3.4e38], f32)
        for f in range(soft.shape[0]):
            at = rng.choice(N, 40, replace=False)
            soft[f, at] = vals[rng.integers(0, vals.size, 40)]
        soft[5] = np.nan                              # a whole row without information: all weights 0, h = 0, clean
        soft[6] = -np.inf                             # h = all ones
        soft[7] = 0.0
        soft[7, 3] = -1.0                             # one wrong bit among zeros
    elif kind == "all_clean":
        soft = np.abs(noisy(name, 16, 0.7, seed=13))
    elif kind == "all_dirty":
        soft = noisy(name, 16, 0.95, seed=14)
        soft[:, 0] = -np.abs(soft[:, 0]) - f32(20.0)  # a confident wrong bit: every frame is dirty
    else:
        raise KeyError(kind)
    soft = np.ascontiguousarray(soft, f32)
    soft.setflags(write=False)
    return soft, scale


@functools.lru_cache(maxsize=None)
def shape_rows(name, frames, seed):
    """float32 [frames, N]: noisy rows for the codes of the shape tests, every frame dirty or not as it falls"""
    soft = noisy(name, frames, 0.9, seed=seed)
    soft.setflags(write=False)
    return soft


@functools.lru_cache(maxsize=None)
def want(name, kind, order):
    """osd_ref.run on the synthetic case `kind` of code `name`"""
    c = code(name)
    soft, scale = synthetic(kind, name)
    r = osd_ref.run(c["H"], soft, order, scale, c["K"])
    for v in r.values():
        v.setflags(write=False)
    return r


# ---- crafted syndromes: hard decisions whose unsatisfied checks are exactly a chosen set of rows ---------------------------

FLAG_LANES = 256                   # rows m and m + 256 k are summed by one lane of the flag pass

CRAFTED = {
    WIMAX_HALF: ((0, 256), (5, 261), (31, 287), (256,), (287,), (17,)),
    WIMAX_LONG: ((0, 256), (3, 515), (260, 516), (10, 266, 20, 532), (300,), (570,)),
    "bg1": ((0, 256), (7, 519), (300, 556), (1, 257, 2, 514), (200, 456, 712, 5), (735,)),
}


def solve(H, s):
    """uint8 [N]: some x with H x = s over GF(2) (the free variables zero); None when there is none"""
    A = np.concatenate([H.astype(np.uint8), np.asarray(s, np.uint8)[:, None]], axis=1)
    M, N = H.shape
    piv, r = [], 0
    for c in range(N):
        rows = np.flatnonzero(A[r:, c])
        if rows.size == 0:
            continue
        p = r + rows[0]
        if p != r:
            A[[r, p]] = A[[p, r]]
        others = np.flatnonzero(A[:, c])
        others = others[others != r]
        A[others] ^= A[r]
        piv.append(c)
        r += 1
        if r == M:
            break
    if A[r:, N].any():
        return None
    x = np.zeros(N, np.uint8)
    x[piv] = A[:len(piv), N]
    return x


@functools.lru_cache(maxsize=None)
def crafted(name):
    """(soft float32 [frames, N], sets): frame f's hard decision has exactly the unsatisfied checks CRAFTED[name][f]; the
    magnitudes are those of noisy rows, none zero"""
    c = code(name)
    sets = CRAFTED[name]
    mag = np.abs(noisy(name, len(sets), 0.5, seed=300 + c["N"])) + f32(0.0625)
    soft = np.empty_like(mag)
    for f, rows in enumerate(sets):
        s = np.zeros(c["M"], np.uint8)
        s[list(rows)] = 1
        h = solve(c["H"], s)
        assert h is not None, (name, rows)
        soft[f] = np.where(h == 1, -mag[f], mag[f])
    soft.setflags(write=False)
    return soft, sets


@functools.lru_cache(maxsize=None)
def crafted_want(name, order):
    c = code(name)
    r = osd_ref.run(c["H"], crafted(name)[0], order, SCALE, c["K"])
    for v in r.values():
        v.setflags(write=False)
    return r


# ---- the decoder case: 96 frames of (576, 288) that a short decode leaves partly wrong -------------------------------

DECODER_FRAMES = 96
DECODER_MAXIT = 5                  # rounds of min-sum / BP: small, so that frames stay dirty
DECODER_SD = (0.62, 0.90)          # the frames' noise levels, ascending over the batch
DECODER_SEED = 20261020
BP_LLR_SCALE = 4.0                 # 2 / sd^2 around sd = 0.7


@functools.lru_cache(maxsize=None)
def decoder_y():
    c = code(WIMAX_HALF)
    sd = np.linspace(DECODER_SD[0], DECODER_SD[1], DECODER_FRAMES).astype(f32)
    y = channel.awgn_frames(c["N"], 0, DECODER_FRAMES, 1.0, seed=DECODER_SEED)
    y = (f32(1) + (y - f32(1)) * sd[:, None]).astype(f32)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def decoder_post(algo):
    """float32 [96, N]: the reference's posterior of the round each frame stopped in; algo "ms" or "bp" """
    c = code(WIMAX_HALF)
    if algo == "bp":
        import bp_ref
        from ms_correction_ref import Code
        post = bp_ref.flood(Code(c["rows"], c["cols"], c["M"], c["N"], c["K"]), decoder_y(), DECODER_MAXIT, llr_scale=BP_LLR_SCALE)["post"]
    else:
        import oracle
        import soft_ref
        post = soft_ref.expected(oracle.Graph(c["rows"], c["cols"], c["M"], c["N"], c["K"]), decoder_y(), "ms", DECODER_MAXIT)["post"]
    post = np.array(post, f32)
    post.setflags(write=False)
    return post
