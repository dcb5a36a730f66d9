"""Inputs and expectations of tests/test_gpu_flood_matrix.py (a helper, not a test module): the irregular matrix code of
kernel_matrix.py -- rows of every degree 0 ... 33 and 40, columns of every degree 0 ... 17 and 20 -- under every
arithmetic of the streaming flooding kernels that has a translation unit of its own and no degree matrix elsewhere:
corrected min-sum in fp32 and fp16 (msc, msc16), fp8 (ms8, msc8) and fixed point at 4, 5, 6 and 8 bits (msi*, msci*).  A
second code, the same degrees without the rows above 32, is the one on which round 1 reads the channel array.  Everything
here runs on the CPU, is computed once per process and handed out read-only; tests/test_flood_matrix_cpu.py checks that
every case reaches what it is there for."""
import functools

import numpy as np

import oracle

import bp_cases as bc
import bp_ref as RB
import fixed_cases as fxc
import fixed_ref as RI
import fp16_cases as fc
import fp8_ref as R8
import kernel_matrix as km
from ms_correction_ref import Code, flood_ms

f32 = np.float32
MAXIT = bc.MATRIX_MAXIT
FRAMES = bc.MATRIX_FRAMES
TRIMMED_SEED = 20261021
NO_CORRECTION = (0.0, 0.0)

# name (the library's own, as in its kernel names): the storage type, the fixed-point width, the correction (scale, offset).
# The float corrections: pure scale, pure offset and both once each (fp16_cases.SETTINGS); fixed point: the truncating
# (3 m) >> 2 at the narrowest and the widest width, the other two in between.
ARITHS = {
    "msc": dict(storage="f32", q=0, setting=fc.SETTINGS[0]),
    "msc16": dict(storage="f16", q=0, setting=fc.SETTINGS[1]),
    "ms8": dict(storage="f8", q=0, setting=None),
    "msc8": dict(storage="f8", q=0, setting=fc.SETTINGS[2]),
    "msi4": dict(storage="i8", q=4, setting=None),
    "msi5": dict(storage="i8", q=5, setting=None),
    "msi6": dict(storage="i8", q=6, setting=None),
    "msi8": dict(storage="i8", q=8, setting=None),
    "msci4": dict(storage="i8", q=4, setting=(0.75, 0.0)),
    "msci5": dict(storage="i8", q=5, setting=fc.SETTINGS[1]),
    "msci6": dict(storage="i8", q=6, setting=fc.SETTINGS[2]),
    "msci8": dict(storage="i8", q=8, setting=(0.75, 0.0)),
}
# the arithmetics that have their degree matrix elsewhere (test_gpu_kernel_matrix.py, test_gpu_bp.py) and join the ones above
# where round 1 reads the channel array
PLAIN = {
    "ms": dict(storage="f32", q=0, setting=None),
    "ms16": dict(storage="f16", q=0, setting=None),
    "bp": dict(storage="f32", q=0, setting=None, algo="bp"),
    "bp16": dict(storage="f16", q=0, setting=None, algo="bp"),
}
FIRST_ROUND_ARITHS = {**ARITHS, **PLAIN}
FIXED = tuple(a for a, s in ARITHS.items() if s["storage"] == "i8")
CORRECTED = tuple(a for a, s in ARITHS.items() if s["setting"] is not None)


def _freeze(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def is_fixed(arith):
    return FIRST_ROUND_ARITHS[arith]["storage"] == "i8"


def llr_scale(arith):
    """the llr_scale the decoder is made with: fixed point, the LSBs per unit of fixed_cases.py; BP, bp_cases.SCALE"""
    s = FIRST_ROUND_ARITHS[arith]
    return fxc.LLR_SCALE[s["q"]] if s["q"] else bc.SCALE if s.get("algo") == "bp" else 1.0


def decoder_args(arith):
    """the keyword arguments of myldpccppapi_amd.Decoder that select the arithmetic"""
    s = FIRST_ROUND_ARITHS[arith]
    scale, offset = s["setting"] or NO_CORRECTION
    kw = dict(algo=s.get("algo", "ms"), msg_dtype=s["storage"], ms_scale=scale, ms_offset=offset)
    if s["q"]:
        kw.update(msg_bits=s["q"], llr_scale=llr_scale(arith))
    elif s.get("algo") == "bp":
        kw.update(llr_scale=llr_scale(arith))
    return kw


# ---- the two codes --------------------------------------------------------------------------------------------------

def full():
    """bp_cases.matrix(): dict(rows, cols, M, N, K, code, y), 70 frames"""
    return bc.matrix()


@functools.lru_cache(maxsize=None)
def trimmed():
    """The degree maps of the matrix code without the rows of degree 33 and 40: no row above the unrolled check bodies, and --
    as on the matrix code -- no row the column-fused kernel could link.  70 frames at the noise levels of full()."""
    row = {d: n for d, n in km.MATRIX_ROW_DEGS.items() if d <= 32}
    E = sum(d * n for d, n in row.items())
    col = dict(km.MATRIX_COL_FIXED)                     # filled as kernel_matrix.matrix_code does
    rest = E - sum(d * n for d, n in col.items())
    col[3], r = divmod(rest, 3)
    if r == 1:
        col[4] += 1
        col[3] -= 1
    elif r == 2:
        col[2] += 1
    rows, cols, M, N = km.irregular_code(row, col, TRIMMED_SEED)
    K = (N - M) // 8 * 8
    y = fc.noisy_frames(N, FRAMES, 0.15, 0.8, seed=TRIMMED_SEED)
    y.setflags(write=False)
    return dict(rows=rows, cols=cols, M=M, N=N, K=K, code=Code(rows, cols, M, N, K), y=y)


CODES = {"full": full, "trimmed": trimmed}


def degree_one_edges(c):
    """the edge ids of the rows of degree 1"""
    rd = np.bincount(c["rows"], minlength=c["M"])
    return np.nonzero(rd[c["rows"]] == 1)[0]


# ---- expectations ---------------------------------------------------------------------------------------------------

def reference(arith, c, y, max_iter=MAXIT, tap_iter=fc.TAP, corrected=True, q=None):
    """The arithmetic's own CPU reference on the code c and the frames y, under the keys out, iters, hard, r_tap, q_tap.
    corrected=False: the same storage type without the correction; q: another fixed-point width at this arithmetic's
    llr_scale (what a kernel table that dispatched to the wrong instantiation would compute)."""
    s = FIRST_ROUND_ARITHS[arith]
    setting = (s["setting"] if corrected else None) or NO_CORRECTION
    if s.get("algo") == "bp":
        return RB.flood(c["code"], y, max_iter, rnd=bc.RND[s["storage"]], llr_scale=llr_scale(arith), tap_iter=tap_iter)
    if s["storage"] == "i8":
        return RI.flood(c["code"], y, max_iter, *setting, q=q or s["q"], llr_scale=llr_scale(arith), tap_iter=tap_iter)
    if s["storage"] == "f8":
        return R8.flood(c["code"], y, max_iter, *setting, tap_iter=tap_iter)
    if setting == NO_CORRECTION and corrected:          # plain min-sum: the C oracle, as the arithmetic's own tests
        og = oracle.Graph(c["rows"], c["cols"], c["M"], c["N"], c["K"])
        return fc.as_ref(oracle.decode(og, y, "ms", max_iter=max_iter, tap_iter=tap_iter, msg_f16=s["storage"] == "f16"))
    return flood_ms(c["code"], y, max_iter, *setting, f16=s["storage"] == "f16", tap_iter=tap_iter)


@functools.lru_cache(maxsize=None)
def want(code_name, arith):
    """reference() on the 70 frames of full() or trimmed(), 20 rounds, taps after round fc.TAP"""
    c = CODES[code_name]()
    return _freeze(reference(arith, c, c["y"]))


def frame_rows(B):
    """the frame of the 70 that frame i of a batch of B is (frames decode independently)"""
    return np.arange(B) % FRAMES


def frames(code_name, V, tiles=2):
    """(y, rows): the 70 frames continued periodically to tiles * 64 * V + 5 -- full tiles and a ragged one at every V"""
    B = tiles * 64 * V + 5
    rows = frame_rows(B)
    return np.ascontiguousarray(fxc.repeat_frames(CODES[code_name]()["y"], B)), rows


def frame_bytes(out, K, n):
    """packed bytes as [frames, K / 8] (K is a multiple of 8 on both codes)"""
    return np.asarray(out).reshape(n, K // 8)


def same_messages(arith, got, ref):
    """the library's float32 report of messages against the reference: fixed point, its int32 values as floats; the
    floating-point types, bit patterns where the expectation is a number, NaN where it is NaN"""
    if is_fixed(arith):
        return bool(np.array_equal(np.ascontiguousarray(got, f32).view(np.uint32), fxc.as_float(ref).view(np.uint32)))
    return fc.same_floats(got, ref)


# ---- which launches a plan is made of -------------------------------------------------------------------------------

# csrc/flood_tables.hpp: the degree buckets; csrc/flood_tables_impl.hpp (fill_v): what an arithmetic's table holds.  Every
# arithmetic but sum-product has unrolled check bodies up to 32 and all four check bucket kernels; every one has the three
# variable-node bucket kernels.
CHECK_BUCKETS = ((1, 8), (9, 16), (17, 24), (25, 32))
VAR_BUCKETS = ((1, 4), (5, 8), (9, 16))
MAX_VAR_UNROLLED = 16
TABLE_MS = dict(max_check_unrolled=32, check_group=(True, True, True, True), var_group=(True, True, True))
TABLES = {a: TABLE_MS for a in FIRST_ROUND_ARITHS}


def solo_launches(arith, row_degs, col_degs, V):
    """One launch per class (merge off): check_kernel<a,d,V> for every row degree d > 0 -- above the unrolled limit the
    generic kernel reports under the class's degree as well -- and var_kernel<a,d,V> for every column degree."""
    return ({"check_kernel<%s,%d,%d>" % (arith, d, V) for d in row_degs if d > 0} |
            {"var_kernel<%s,%d,%d>" % (arith, d, V) for d in col_degs})


def default_launches(arith, row_degs, col_degs, V):
    """(names, lacking): plan_launches of csrc/engine_flood.hip with merging on and no linked class, restated.  A class goes
    to the bucket of its degree if the arithmetic's table has that bucket's kernel (rows: and an unrolled body of that
    degree); a bucket with two or more classes is one launch, every other class is launched alone.  lacking: the bucket
    kernels with classes in their range that the table does not have, by name."""
    t = TABLES[arith]
    names, lacking = set(), []

    def plan(degs, buckets, have, group, solo, limit):
        members = {k: [] for k in range(len(buckets))}
        for d in degs:
            k = next((k for k, (lo, hi) in enumerate(buckets) if lo <= d <= hi and d <= limit), None)
            if k is not None and not have[k]:
                lacking.append(group % (arith, buckets[k][0], buckets[k][1], V))
                k = None
            if k is None:
                names.add(solo % (arith, d, V))
            else:
                members[k].append(d)
        for k, m in members.items():
            if len(m) >= 2:
                names.add(group % (arith, buckets[k][0], buckets[k][1], V))
            else:
                names.update(solo % (arith, d, V) for d in m)

    plan([d for d in row_degs if d > 0], CHECK_BUCKETS, t["check_group"], "check_group_kernel<%s,%d-%d,%d>", "check_kernel<%s,%d,%d>",
         t["max_check_unrolled"])
    plan(list(col_degs), VAR_BUCKETS, t["var_group"], "var_group_kernel<%s,%d-%d,%d>", "var_kernel<%s,%d,%d>", MAX_VAR_UNROLLED)
    return names, sorted(set(lacking))
