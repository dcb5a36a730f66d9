"""fp8 (E4M3) messages, the reference of tests/test_fp8_cpu.py and tests/test_gpu_fp8.py (a helper, not a test module).

msg_dtype = f8 is this repository's own definition (include/ldpc_hip.h: LDPC_MSG_F8): flooding min-sum with fp32
arithmetic whose channel values, variable->check messages and check->variable messages are OCP E4M3 values.

    s8(x): NaN stays NaN; anything else is clamped to [-448, 448] and rounded to the nearest E4M3 value (1-4-3, bias 7,
           subnormals down to 2^-9, no infinities), ties to the even code, the sign of zero kept.

flood() restates flooding min-sum in numpy from the CPU oracle's semantics (as ms_correction_ref.flood_ms does) with the
storage rounding as a PARAMETER: `rnd` is applied to the channel values where they are stored, to the variable->check
messages where they are stored, and to a row's two magnitude candidates where the check->variable message is produced --
after the correction fmaxf(m - offset, 0) * scale if there is one.  With the identity it is the oracle's fp32 min-sum,
with binary16 rounding flood_ms(f16=True) (there every candidate is a binary16 value or 1000 already, so rounding the
plain candidates changes nothing); tests/test_fp8_cpu.py holds it to both.  With s8 the plain candidates change in one
place: the start value 1000 reads 448."""
import numpy as np

from ms_correction_ref import Code  # noqa: F401  (the code object flood() takes)

F32 = np.float32
F8_MAX = 448.0


def identity(x):
    return x


def f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, F32).astype(np.float16).astype(F32)


def s8(x):
    """float32 in and out.  The grid of E4M3 around x is 2^(e - 3) with e = max(floor(log2 |x|), -6); np.rint rounds halves
    to even multiples of it, which are the even codes (a mantissa that rounds up to 16 quanta is the next binade's
    first, even, code).  All of it is exact in float64."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        c = np.clip(x.astype(np.float64), -F8_MAX, F8_MAX)              # NaN stays NaN
        _, ex = np.frexp(c)                                            # |c| = m * 2^ex, m in [0.5, 1)
        quantum = np.ldexp(1.0, np.maximum(ex - 1, -6) - 3)
        return (np.rint(c / quantum) * quantum).astype(F32)             # rint keeps -0


def _check(code, Q, scale, offset, rnd):
    """R_e = sign * rnd(corrected min over the row's other |q|, from 1000); a NaN message is skipped, its sign is +."""
    frames = Q.shape[0]
    Qx = np.concatenate([Q, np.full((frames, 1), np.inf, F32)], axis=1)
    x = Qx[:, code.row_edges]                               # [F, M, dmax]
    a = np.abs(x)
    a = np.where(np.isnan(a), F32(np.inf), a)
    idx = np.argmin(a, axis=2)
    m1 = np.minimum(np.take_along_axis(a, idx[..., None], 2)[..., 0], F32(1000))
    a2 = a.copy()
    np.put_along_axis(a2, idx[..., None], np.inf, 2)
    m2 = np.minimum(a2.min(axis=2), F32(1000))
    if scale != 0 or offset != 0:
        al = F32(scale if scale != 0 else 1.0)
        m1 = (np.maximum(m1 - F32(offset), F32(0)) * al).astype(F32)
        m2 = (np.maximum(m2 - F32(offset), F32(0)) * al).astype(F32)
    m1, m2 = rnd(m1), rnd(m2)
    neg = (x < 0) & code.row_valid[None]
    par = np.bitwise_xor.reduce(neg, axis=2)
    k = np.arange(code.dmax)
    b = np.where(k[None, None, :] == idx[..., None], m2[..., None], m1[..., None])
    r = np.where(par[..., None] ^ neg, -b, b).astype(F32)
    R = np.zeros((frames, code.E + 1), F32)
    R[:, code.row_edges[code.row_valid]] = r[:, code.row_valid]
    return R[:, :code.E]


def flood(code, y, max_iter, scale=0.0, offset=0.0, rnd=s8, tap_iter=0, pack_mode=0, raw_cols=None, stop=None):
    """dict(out, iters, hard, r_tap, q_tap, hard_tap as ms_correction_ref.flood_ms gives them;
            y8 = the stored channel values, post = float32 [frames, N]: the posterior y8 + R_e1 + R_e2 + ... (fp32, ascending
            edge id) of the round each frame stopped in, by_stop = frames stopped by `stop` in a round in which their
            syndrome was not clean).

    stop(hard uint8 [n, N]) -> bool [n], optional: a frame also stops in the first round whose hard bits it passes (the
    CRC rule of include/ldpc_hip.h), OR-ed with the syndrome.
    raw_cols (bool [N]) is no part of the definition: the model of a WRONG kernel in which the marked columns see the
    check->variable messages as they are BEFORE rnd -- a column-fused check kernel that rounds R only where it stores it."""
    y = np.ascontiguousarray(y, F32).reshape(-1, code.N)
    with np.errstate(invalid="ignore", over="ignore"):
        return _flood(code, y, max_iter, scale, offset, rnd, tap_iter, pack_mode, raw_cols, stop)


def _flood(code, y, max_iter, scale, offset, rnd, tap_iter, pack_mode, raw_cols, stop):
    frames = y.shape[0]
    yf = rnd(y).astype(F32)
    Q = yf[:, code.cols].copy()
    hard = np.zeros((frames, code.N), np.uint8)
    post = np.zeros((frames, code.N), F32)
    iters = np.zeros(frames, np.int32)
    by_stop = np.zeros(frames, bool)
    r_tap = np.full((frames, code.E), np.nan, F32) if tap_iter else None
    q_tap = np.full((frames, code.E), np.nan, F32) if tap_iter else None
    hard_tap = np.zeros((frames, code.N), np.uint8) if tap_iter else None
    raw_edges = None if raw_cols is None else np.asarray(raw_cols, bool)[code.cols]
    A = np.arange(frames)
    for t in range(1, max_iter + 1):
        R = _check(code, Q[A], scale, offset, rnd)
        R_stored = R
        if raw_edges is not None:
            R = np.where(raw_edges[None, :], _check(code, Q[A], scale, offset, identity), R)
        Rx = np.concatenate([R, np.full((len(A), 1), -0.0, F32)], axis=1)
        P = yf[A].copy()
        for k in range(code.col_edges.shape[1]):             # ascending edge id along every column
            P = P + Rx[:, code.col_edges[:, k]]
        h = (~(P > 0)).astype(np.uint8)
        hard[A] = h
        post[A] = P
        ok = code.syndrome_ok(h)
        if stop is not None:
            extra = np.asarray(stop(h), bool)
            by_stop[A[extra & ~ok]] = True
            ok = ok | extra
        iters[A] = t
        if tap_iter == t:
            r_tap[A] = R_stored
            hard_tap[A] = h
        if t == max_iter:
            break
        keep = ~ok
        A, P, R = A[keep], P[keep], R[keep]
        if len(A) == 0:
            break
        Q[A] = rnd((P[:, code.cols] - R).astype(F32))
        if tap_iter == t:
            q_tap[A] = Q[A]
    return dict(out=code.pack(hard, pack_mode), iters=iters, hard=hard, r_tap=r_tap, q_tap=q_tap, hard_tap=hard_tap,
                y8=yf, post=post, by_stop=np.nonzero(by_stop)[0])


# ---- the 256 codes, for a rounding built independently of s8 --------------------------------------------------------

def e4m3_table():
    """float64 [256]: the value of every code byte (S.EEEE.MMM, bias 7; E = 0: M * 2^-9; S.1111.111: NaN)"""
    b = np.arange(256)
    e, m = (b >> 3) & 15, b & 7
    v = np.where(e == 0, m * 2.0 ** -9, (1 + m / 8.0) * 2.0 ** (e.astype(np.float64) - 7))
    v = np.where((e == 15) & (m == 7), np.nan, v)
    return np.where(b & 128, -v, v)


def edge_inputs():
    """The inputs of the conversion tests, float32 [n]: all finite code values, the midpoint of every neighbouring pair
    and the fp32 neighbours of each midpoint (both signs), and the edge list of the definition."""
    t = e4m3_table()
    pos = np.sort(t[:127])                                   # 0 ... 448
    mid = ((pos[:-1] + pos[1:]) / 2).astype(F32)             # exact in fp32: one more mantissa bit
    near = np.concatenate([mid, np.nextafter(mid, F32(np.inf)), np.nextafter(mid, F32(-np.inf))])
    extra = np.array([464, 1000, np.inf, 2.0 ** -10, 1.5 * 2.0 ** -10, 3 * 2.0 ** -10, 1.0625, 1.1875, 15.5, 1e-6, 1e-41, 1e-8,
                      448, 449, 463.99, 480, 3.4e38, 0.0], F32)
    half = np.concatenate([pos.astype(F32), near, extra])
    return np.concatenate([half, -half, [F32(np.nan)]]).astype(F32)
