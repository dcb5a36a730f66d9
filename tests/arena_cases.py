"""Codes, inputs and oracle results of tests/test_gpu_arena.py (a helper, not a test module).

Everything here runs on the CPU: tests/test_arena_cpu.py checks that every case's inputs make the oracle stop frames at
several different iterations and run some to the end, and that the tail cases reach their hand-over condition, so that a
seed which tests nothing fails there instead of passing silently on the GPU."""
import functools

import numpy as np

import oracle
from myldpccppapi_amd import channel, codes
import kernel_matrix as km
from util import golden_files, kernel_choice, load_golden

f32 = np.float32
MAXIT = 12
PACK_BYTES, PACK_BITS = 0, 1


def mix_channel(N, frames, lo, hi, seed):
    """All-zero codeword over AWGN, the noise level of each frame drawn from [lo, hi]: frames stop at many iterations."""
    y = channel.awgn_frames(N, 0, frames, 1.0, seed=seed)
    sd = np.random.default_rng(seed).uniform(lo, hi, frames).astype(f32)[:, None]
    return (f32(1) + (y - f32(1)) * sd).astype(f32)


def tail_channel(N, frames, seed, per_tile=3, easy_sd=0.6, hard_sd=1.3):
    """Most frames easy, `per_tile` scattered frames of every 64 that never converge: no tile of 64 (or of 256) finishes
    before the last round, so without a hand-over every round would run on every tile."""
    rng = np.random.default_rng(seed)
    y = channel.awgn_frames(N, 0, frames, easy_sd, seed=seed)
    hard = np.concatenate([t + rng.choice(min(64, frames - t), min(per_tile, frames - t), replace=False)
                           for t in range(0, frames, 64)])
    y[hard] = channel.awgn_frames(N, 50000, hard.size, hard_sd, seed=seed + 1)
    return y, np.sort(hard)


def easy_channel(N, frames, seed, sd=0.55):
    return channel.awgn_frames(N, 9000, frames, sd, seed=seed)


@functools.lru_cache(maxsize=None)
def code(name):
    """dict(rows, cols, M, N, K, z, og): "w576" / "w648" = 802.16e rate 1/2 (z = 24 / 27; K = 324 has K % 8 = 4),
    "ira" = the staircase code of the column-fused check launch, "host" = the code of the first tdmphost fixture."""
    if name in ("w576", "w648"):
        rate, N = codes.RATE_1_2, int(name[1:])
    elif name == "host":
        gd = load_golden(golden_files("tdmphost")[0])
        rate, N = int(gd["rate"]), int(gd["N"])
    if name == "ira":
        rows, cols, M, N, K = km.ira_code(3, 400, {5: 20, 7: 11, 20: 2}, seed=3)
        K, z = K // 8 * 8, 0
    else:
        K, M, z = codes.wimax_dims(rate, N)
        rows, cols = codes.wimax_edges(rate, N)
    return dict(rows=rows, cols=cols, M=M, N=N, K=K, z=z, og=oracle.Graph(rows, cols, M, N, K))


def _case(name, code_name, algo, frames, V=0, tune=None, f16=False, layer_rows=False, poll=0, pack=PACK_BYTES,
          kind="mix", noise=(0.55, 0.95), kernel=None):
    return dict(name=name, code=code_name, algo=algo, frames=frames, V=V, tune=tune or {}, f16=f16, layer_rows=layer_rows,
                poll=poll, pack=pack, kind=kind, noise=noise, kernel=kernel,
                max_batch=frames + 64 * max(V, 1))


def _qc_rows(code_name, pack):
    """The rows of the table that also run on the (648, 324) code."""
    out = []
    tag = code_name + ("b" if pack == PACK_BITS else "")
    for algo, f16 in (("sp", False), ("ms", False), ("ms", True)):
        for V in (1, 2, 4):
            out.append(_case("flood_%s%s_v%d_%s" % (algo, "16" if f16 else "", V, tag), code_name, algo, 64 * V + 5, V=V,
                             tune=kernel_choice("0"), f16=f16, pack=pack, kernel="check_"))
    for V in (1, 4):
        out.append(_case("layered_stream_v%d_%s" % (V, tag), code_name, "layered", 64 * V + 5, V=V, tune=kernel_choice("0"),
                         layer_rows=True, pack=pack, kernel="layer_kernel<"))
    return out


def _one_launch_rows(code_name):
    out = []
    for algo, kern in (("layered", "fused_layered_kernel"), ("ms", "fused_flood_kernel"), ("sp", "fused_sp_kernel"),
                       ("ms_fused", "fused_flood_kernel")):
        out.append(_case("lds_%s_%s" % (algo, code_name), code_name, algo, 13, tune=kernel_choice("1"), layer_rows=True,
                         kernel=kern))
    for algo, kern in (("layered", "layered_ldsp_kernel["), ("ms", "flood_ldsp_kernel["), ("ms_fused", "flood_ldsp_kernel[")):
        for packed in (True, False):
            tune = dict(kernel_choice("ldsp", 4), **({} if packed else {"ldsp_pack": False}))
            out.append(_case("record_%s_%s_%s" % (algo, "packed" if packed else "unpacked", code_name), code_name, algo, 13,
                             tune=tune, layer_rows=True, kernel=kern))
    return out


def engine_cases():
    """Every row of the table: one decoder each."""
    out = _qc_rows("w576", PACK_BYTES) + _one_launch_rows("w576")
    for V in (1, 4):
        out.append(_case("link_ms_v%d" % V, "ira", "ms", 69, V=V, noise=(0.7, 1.1), kernel="check_link"))
    out.append(_case("layered_host", "host", "layered_host", 69, V=1, layer_rows=True, noise=(0.35, 0.6), kernel="layer_kernel<"))
    for algo in ("ms", "sp"):
        out.append(_case("polled_tail_%s" % algo, "w576", algo, 300, V=1, tune=dict(kernel_choice("0"), compact=512), poll=1,
                         kind="tail", kernel="check_"))
        for V in (1, 4):
            out.append(_case("device_tail_%s_v%d" % (algo, V), "w576", algo, 2100, V=V, tune=kernel_choice("0"),
                             kind="tail", kernel="check_"))
    # K % 8 = 4: whole bytes per frame with gap bits in between, and bit packing where the engine has it (the one-launch
    # kernels pack whole bytes only: with LDPC_PACK_BITS and K % 8 != 0 layered / ms / sp decode with the streaming
    # kernels and ms_fused is refused)
    out += _qc_rows("w648", PACK_BYTES) + _one_launch_rows("w648") + _qc_rows("w648", PACK_BITS)
    return out


CASES = {c["name"]: c for c in engine_cases()}
GROUPS = {
    "flooding": [n for n in CASES if n.startswith("flood_")],
    "column_fused": [n for n in CASES if n.startswith("link_")],
    "lds_resident": [n for n in CASES if n.startswith("lds_")],
    "record": [n for n in CASES if n.startswith("record_")],
    "layered_streaming": [n for n in CASES if n.startswith("layered_stream")],
    "layered_host": ["layered_host"],
    "polled_tail": [n for n in CASES if n.startswith("polled_tail")],
    "device_tail": [n for n in CASES if n.startswith("device_tail")],
}
assert sorted(sum(GROUPS.values(), [])) == sorted(CASES)

_SEEDS = {"w576": 576, "w648": 648, "ira": 103, "host": 56}


@functools.lru_cache(maxsize=None)
def inputs(code_name, kind, frames, noise=(0.55, 0.95), variant=0):
    """float32 [frames, N], read-only; shared by every case of the same code, kind and size.  variant: another draw (the
    call sequences give the polled decoder different hard frames on every call)."""
    N = code(code_name)["N"]
    seed = _SEEDS[code_name] + 1000 * variant
    if kind == "mix":
        y = mix_channel(N, frames, noise[0], noise[1], seed)
    elif kind == "tail":
        y = tail_channel(N, frames, seed + frames)[0]
    elif kind == "easy":
        y = easy_channel(N, frames, seed)
    else:
        raise ValueError(kind)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def want(code_name, algo, f16, kind, frames, noise=(0.55, 0.95), pack=PACK_BYTES, variant=0):
    """oracle.decode of inputs(...), plus converged = syndrome-clean frames of its hard bits."""
    from util import converged_frames
    c = code(code_name)
    y = inputs(code_name, kind, frames, noise, variant)
    r = oracle.decode(c["og"], y, algo, max_iter=MAXIT, pack_mode=pack, msg_f16=f16,
                      layer_rows=c["z"] if algo in ("layered", "layered_host") else 0)
    r["converged"] = converged_frames(c["rows"], c["cols"], c["M"], r["hard"])
    r["ok"] = r["undefined"] == 0 if "undefined" in r else np.ones(frames, bool)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def case_inputs(c, kind=None, frames=None, variant=0):
    return inputs(c["code"], kind or c["kind"], frames or c["frames"], c["noise"], variant)


def case_want(c, kind=None, frames=None, variant=0):
    return want(c["code"], c["algo"], c["f16"], kind or c["kind"], frames or c["frames"], c["noise"], c["pack"], variant)


def frame_byte_index(K, frames):
    """int64 [frames, K/8]: the bytes of each frame in LDPC_PACK_BYTES, frame f from byte (f*K)/8 on."""
    return (np.arange(frames, dtype=np.int64)[:, None] * K // 8) + np.arange(K // 8, dtype=np.int64)[None, :]


def running_after(iters, rnd, max_iter=MAXIT):
    """frames still running after round rnd: not yet clean (a frame with iters == max_iter may never be)"""
    return int((np.asarray(iters) > rnd).sum())


def handover_round(iters, max_iter=MAXIT):
    """The first round after which at most 512 frames and at most a quarter of the batch still run, or None."""
    iters = np.asarray(iters)
    for rnd in range(1, max_iter):
        run = running_after(iters, rnd)
        if run <= 512 and 4 * run <= iters.size:
            return rnd
    return None


def frame_rounds_without_handover(iters, tile, max_iter=MAXIT):
    """sum over the rounds of tile size x tiles that still have a running frame when the round begins: what
    stats()["frame_rounds"] would report if no frame ever moved to another tile"""
    iters = np.asarray(iters)
    tiles = -(-iters.size // tile)
    pad = np.zeros(tiles * tile, iters.dtype)
    pad[:iters.size] = iters
    last = pad.reshape(tiles, tile).max(axis=1)             # the tile works in rounds 1 .. last
    return int(tile * np.minimum(last, max_iter).sum())
