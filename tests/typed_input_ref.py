"""The typed-input rule in numpy, and the inputs and expectations of tests/test_gpu_typed_input.py (a helper, not a test
module).

A typed decode call reads y = (float)x * llr_unit, one fp32 multiply, and then does what the handle does with that y
(include/ldpc_hip.h: enum ldpc_llr_type).  So every expectation here is the CPU reference the algorithm already has --
oracle.decode, ms_correction_ref, fp8_ref, bp_ref, layered_bp_ref, soft_ref -- run on dequantize(x, unit); never the GPU's
own float path.  quantize() is the sender's side (ldpc_llr_quantize_device).  Everything here runs on the CPU, is computed
once per process and handed out read-only; tests/test_typed_input_cpu.py checks that the cases reach what they are there
for."""
import ctypes
import ctypes.util
import functools

import numpy as np

import oracle
from myldpccppapi_amd import codes

import bp_cases as bc
import bp_ref as RB
import fp16_cases as fc
import fp8_ref as R8
import layered_bp_cases as lc
import layered_bp_ref as LB
from ms_correction_ref import Code

F32 = np.float32
LLR_F32, LLR_F16, LLR_I8 = 0, 1, 2
DTYPES = {"i8": np.int8, "f16": np.float16}
TYPE_IDS = {"i8": LLR_I8, "f16": LLR_F16, "f32": LLR_F32}
# no power of two either: the product x * unit rounds, and so does llr_scale * (x * unit) after it
UNITS = {"i8": 0.0371, "f16": 0.73}
SP_SCALE = 8.0                      # the reference's exp(8 y)
SP_SCALE_2 = 6.3                    # 8 is a power of two and commutes with the rounding of x * unit; this one does not
BP_SCALES = bc.SCALES               # 4.0 and 1.7
TAP = fc.TAP
MAXIT = 12


# ---- the rule -------------------------------------------------------------------------------------------------------

def dequantize(x, unit):
    """y = (float)x * llr_unit: the widening is exact, the product one fp32 multiply"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(x).astype(F32) * F32(unit)).astype(F32)


def quantize(y, unit, kind):
    """ldpc_llr_quantize_device: t = y / unit in fp32; i8: NaN -> 0, else rint (ties to even) clamped to [-127, 127];
    f16: NaN stays, else clamped to +-65504 and rounded to binary16 (nearest even)"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = (np.asarray(y, F32) / F32(unit)).astype(F32)
        if kind == "i8":
            r = np.clip(np.rint(t), F32(-127), F32(127))
            return np.where(np.isnan(t), F32(0), r).astype(np.int8)
        return np.clip(t, F32(-65504), F32(65504)).astype(np.float16)     # np.clip keeps NaN


def folded(x, unit, scale):
    """What a kernel that folds the two multiplies into one would read: x * fl(unit * scale)"""
    return (np.asarray(x).astype(F32) * F32(F32(unit) * F32(scale))).astype(F32)


def two_step(x, unit, scale):
    """The definition: fl(fl(x * unit) * scale)"""
    return (dequantize(x, unit) * F32(scale)).astype(F32)


def expf(a):
    """the host libm's expf, the oracle's exp (ldpc_expf equals it on every float: tests/test_host_cpu.py)"""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.expf.restype, libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    a = np.ascontiguousarray(a, F32)
    return np.array([libm.expf(float(v)) for v in a.ravel()], F32).reshape(a.shape)


# hand cases of the quantiser: (y / unit as the case is meant, expected code)
I8_HAND = ((0.5, 0), (-0.5, 0), (1.5, 2), (-1.5, -2), (2.5, 2), (126.5, 126), (-126.5, -126), (127.4, 127), (-127.4, -127),
           (200.0, 127), (-200.0, -127), (np.inf, 127), (-np.inf, -127), (np.nan, 0), (-0.0, 0), (127.5, 127), (-128.0, -127))
F16_HAND = ((65519.0, 65504.0), (65520.0, 65504.0), (-65520.0, -65504.0), (1e-8, 0.0), (np.nan, np.nan), (np.inf, 65504.0),
            (1.0 + 2.0 ** -11, 1.0), (1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -9))


def hand_values():
    """float32 [n]: the t of every hand case, for a quantiser run with unit 1"""
    return np.array([t for t, _ in I8_HAND] + [t for t, _ in F16_HAND], F32)


# ---- codes ----------------------------------------------------------------------------------------------------------

def _freeze(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def code(name):
    """dict(rows, cols, M, N, K, z, og, code): "w576" -- rows of 576 elements are 16-byte multiples in both narrow types;
    "w648" -- 648 int8 values are not (fp16 rows are); "matrix" -- the irregular code of bp_cases, N odd sizes and all"""
    if name == "matrix":
        m = bc.matrix()
        rows, cols, M, N, K, z = m["rows"], m["cols"], m["M"], m["N"], m["K"], 0
    elif name == "bg1":
        c = lc.bg1_code()
        rows, cols, M, N, K, z = c["rows"], c["cols"], c["M"], c["N"], c["K"], c["z"]
    else:
        # "h576": rate 5/6, every row of one weight -- what layered_host is defined for
        rate = codes.RATE_5_6 if name[0] == "h" else codes.RATE_1_2
        N = int(name[1:])
        K, M, z = codes.wimax_dims(rate, N)
        rows, cols = codes.wimax_edges(rate, N)
    return dict(rows=rows, cols=cols, M=M, N=N, K=K, z=z, og=oracle.Graph(rows, cols, M, N, K), code=Code(rows, cols, M, N, K))


FLOOD_CODES = ("w576", "w648", "matrix")
FLOOD_FRAMES = 64 * 4 + 5           # the V = 4 count; V = 1 and 2 decode the first 64 V + 5 of them
NOISE = {"w576": (0.45, 1.0), "w648": (0.45, 1.0), "matrix": (0.15, 0.8), "bg1": (0.4, 1.3), "h576": (0.25, 0.6)}


@functools.lru_cache(maxsize=None)
def inputs(cname, kind, frames=FLOOD_FRAMES):
    """The caller's buffer, [frames, N] of int8 or float16: noisy frames of the all-zero word whose noise level is drawn
    from a range -- they stop in round 1, 2, 3, ..., some never -- put through the quantiser rule; the int8 buffer also
    holds the codes -128 (which no quantiser produces) and +127"""
    c = code(cname)
    y = fc.noisy_frames(c["N"], frames, *NOISE[cname], seed=20261101 + c["N"] + (0 if kind == "i8" else 1))
    x = quantize(y, UNITS[kind], kind)
    if kind == "i8":
        x[3, 5], x[3, c["N"] - 1], x[frames - 1, 0] = -128, 127, -128
        x[frames - 2, 7] = 127
    x.setflags(write=False)
    return x


def values(cname, kind, frames=FLOOD_FRAMES):
    return dequantize(inputs(cname, kind, frames), UNITS[kind])


# ---- expectations ---------------------------------------------------------------------------------------------------

FLOOD_ARITH = (("sp", "f32"), ("ms", "f32"), ("ms", "f16"), ("ms", "f8"), ("bp", "f32"), ("bp", "f16"))
RND = {"f32": R8.identity, "f16": R8.f16, "f8": R8.s8}


def llr_scale(algo, cname):
    """SP: the reference's 8, and 6.3 on (648, 324); BP: 1.7 on the WiMAX codes, 4.0 on the matrix and BG1 codes (both of
    bp_cases.SCALES are run)"""
    if algo == "sp":
        return SP_SCALE_2 if cname == "w648" else SP_SCALE
    return BP_SCALES[1] if cname[0] == "w" else BP_SCALES[0]


def flood_reference(algo, storage, c, y, scale, maxit=MAXIT):
    """dict(out, iters, hard, hard_tap, chan): the CPU reference of a flooding decoder on float values y; hard_tap = all N
    bits after round TAP (a decode of TAP rounds), chan = the channel term as the decoder stores it (tap 2)"""
    if algo == "bp":
        r = RB.flood(c["code"], y, maxit, rnd={"f32": RB.identity, "f16": RB.f16}[storage], llr_scale=scale)
        t = RB.flood(c["code"], y, TAP, rnd={"f32": RB.identity, "f16": RB.f16}[storage], llr_scale=scale)
        return dict(out=r["out"], iters=r["iters"], hard=r["hard"], hard_tap=t["hard"], chan=r["chan"], post=r["post"])
    if algo == "ms" and storage == "f8":
        r, t = R8.flood(c["code"], y, maxit), R8.flood(c["code"], y, TAP)
        return dict(out=r["out"], iters=r["iters"], hard=r["hard"], hard_tap=t["hard"], chan=r["y8"], post=r["post"])
    f16 = storage == "f16"
    r = oracle.decode(c["og"], y, algo, max_iter=maxit, llr_scale=scale, msg_f16=f16)
    t = oracle.decode(c["og"], y, algo, max_iter=TAP, llr_scale=scale, msg_f16=f16)
    chan = expf((F32(scale) * y).astype(F32)) if algo == "sp" else RND[storage](y).astype(F32)
    return dict(out=r["out"], iters=r["iters"], hard=r["hard"], hard_tap=t["hard"], chan=chan)


@functools.lru_cache(maxsize=None)
def flood_want(cname, kind, algo, storage):
    return _freeze(flood_reference(algo, storage, code(cname), values(cname, kind), llr_scale(algo, cname)))


def head(w, frames, K):
    """the expectation of the first `frames` frames: frames are decoded independently, and with whole bytes per frame (frame
    f at byte f * K // 8, also for K % 8 != 0) the bytes of the first frames are a prefix"""
    r = {k: v[:frames] for k, v in w.items() if k != "out"}
    r["out"] = w["out"][:oracle.out_len(frames, K)]
    return r


LAYERED_FRAMES = lc.BG1_TWO_TILES   # 64 * 4 + 6


@functools.lru_cache(maxsize=None)
def layered_want(algo, kind):
    """layered / layered_bp on the BG1-profile test code, layered_host on WiMAX N = 576 at rate 5/6 (uniform row weight is
    what it is defined for): dict(out, iters, hard, p_tap, hard_tap, undefined)"""
    c = layered_code(algo)
    y = values(c["name"], kind, LAYERED_FRAMES)
    if algo == "layered_bp":
        r = LB.layered_bp(c["code"], y, c["z"], MAXIT, llr_scale=llr_scale("bp", c["name"]), tap_iter=TAP)
        r["undefined"] = np.zeros(y.shape[0], bool)
        return _freeze(r)
    r = oracle.decode(c["og"], y, algo, max_iter=MAXIT, layer_rows=c["z"])
    t = oracle.decode(c["og"], y, algo, max_iter=MAXIT, layer_rows=c["z"], tap_iter=TAP)
    tt = oracle.decode(c["og"], y, algo, max_iter=TAP, layer_rows=c["z"])
    return _freeze(dict(out=r["out"], iters=r["iters"], hard=r["hard"], p_tap=t["taps"]["post"], hard_tap=tt["hard"],
                        undefined=np.asarray(r.get("undefined", np.zeros(y.shape[0], np.uint8))).astype(bool)))


def layered_code(algo):
    n = "h576" if algo == "layered_host" else "bg1"
    return dict(code(n), name=n)
