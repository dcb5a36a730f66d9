"""Fixed-point messages (msg_dtype = i8, msg_bits = q), the reference of tests/test_fixed_cpu.py and
tests/test_gpu_fixed.py (a helper, not a test module).

LDPC_MSG_I8 is this repository's own definition (include/ldpc_hip.h): flooding min-sum on saturating q-bit integers,
q one of 4, 5, 6, 8, L = 2^(q-1) - 1.  The rule is restated here in numpy int32 ONLY, apart from the two places the
definition itself states in float32: the channel multiply, c = sq(llr_scale * y), and the corrected magnitude,
m' = fminf(truncf(fmaxf(m - ms_offset, 0) * ms_scale), L).

    sq(x) = clamp(rintf(x), -L, L): ties to even, NaN gives 0, +-inf gives +-L.

Same interface as fp8_ref.flood.  Messages and posteriors are int32 arrays; a tap that was never written holds TAP_UNSET."""
import numpy as np

from ms_correction_ref import Code  # noqa: F401  (the code object flood() takes)

F32 = np.float32
I32 = np.int32
WIDTHS = (4, 5, 6, 8)
START = 1000                       # the start value of a row's minimum chain: reads L
TAP_UNSET = np.iinfo(np.int32).min


def limit(q):
    assert q in WIDTHS, q
    return (1 << (q - 1)) - 1


def sq(x, q):
    """float32 (or integer) in, int32 out"""
    L = limit(q)
    x = np.asarray(x)
    if x.dtype.kind in "iu":
        return np.clip(x.astype(np.int64), -L, L).astype(I32)
    x = x.astype(F32)
    with np.errstate(invalid="ignore"):
        r = np.rint(x)                                           # ties to even
        r = np.where(np.isnan(r), F32(0), np.clip(r, F32(-L), F32(L)))
    return r.astype(I32)


def channel_values(y, llr_scale, q):
    """c = sq(llr_scale * y): one float32 multiply"""
    with np.errstate(invalid="ignore", over="ignore"):
        return sq((F32(llr_scale) * np.asarray(y, F32)).astype(F32), q)


def corrected(m, scale, offset, q):
    """int magnitudes (or START) in, int32 out: fminf(truncf(fmaxf(m - offset, 0) * scale), L) in float32, in this order"""
    al = F32(scale if scale != 0 else 1.0)
    t = (np.maximum(np.asarray(m).astype(F32) - F32(offset), F32(0)) * al).astype(F32)
    return np.minimum(np.trunc(t), F32(limit(q))).astype(I32)


def _minima(code, Q):
    """(m1, m2, idx, neg, par) of every row: the two smallest |q| from START, the position of the first smallest, the
    signs and their parity -- all integers"""
    frames = Q.shape[0]
    big = I32(1 << 20)
    Qx = np.concatenate([Q, np.zeros((frames, 1), I32)], axis=1)
    x = Qx[:, code.row_edges]                               # [F, M, dmax]
    a = np.where(code.row_valid[None], np.abs(x), big)
    idx = np.argmin(a, axis=2)
    m1 = np.minimum(np.take_along_axis(a, idx[..., None], 2)[..., 0], I32(START))
    a2 = a.copy()
    np.put_along_axis(a2, idx[..., None], big, 2)
    m2 = np.minimum(a2.min(axis=2), I32(START))
    neg = (x < 0) & code.row_valid[None]
    par = np.bitwise_xor.reduce(neg, axis=2)
    return m1, m2, idx, neg, par


def _spread(code, m1, m2, idx, neg, par, dtype):
    frames = m1.shape[0]
    k = np.arange(code.dmax)
    b = np.where(k[None, None, :] == idx[..., None], m2[..., None], m1[..., None])
    r = np.where(par[..., None] ^ neg, -b, b).astype(dtype)
    R = np.zeros((frames, code.E + 1), dtype)
    R[:, code.row_edges[code.row_valid]] = r[:, code.row_valid]
    return R[:, :code.E]


def _check(code, Q, scale, offset, q):
    """R_e = sign * m over the row's other |q|: plain, min(m, L); corrected, corrected(m)"""
    m1, m2, idx, neg, par = _minima(code, Q)
    if scale != 0 or offset != 0:
        m1, m2 = corrected(m1, scale, offset, q), corrected(m2, scale, offset, q)
    else:
        m1, m2 = np.minimum(m1, I32(limit(q))), np.minimum(m2, I32(limit(q)))
    return _spread(code, m1, m2, idx, neg, par, I32)


def _check_raw(code, Q, scale, offset):
    """The check->variable messages of a WRONG kernel, float32: the corrected product neither truncated nor saturated,
    the plain start value not read as L"""
    m1, m2, idx, neg, par = _minima(code, Q)
    m1, m2 = m1.astype(F32), m2.astype(F32)
    if scale != 0 or offset != 0:
        al = F32(scale if scale != 0 else 1.0)
        m1 = (np.maximum(m1 - F32(offset), F32(0)) * al).astype(F32)
        m2 = (np.maximum(m2 - F32(offset), F32(0)) * al).astype(F32)
    return _spread(code, m1, m2, idx, neg, par, F32)


def flood(code, y, max_iter, scale=0.0, offset=0.0, q=8, llr_scale=1.0, tap_iter=0, pack_mode=0, raw_cols=None, stop=None):
    """dict(out, iters, hard as ms_correction_ref.flood_ms gives them; r_tap, q_tap int32 [frames, E] and hard_tap after
            round tap_iter; c = the stored channel values, int32 [frames, N]; post = int32 [frames, N]: the posterior
            c + R_e1 + R_e2 + ... of the round each frame stopped in; by_stop = frames stopped by `stop` in a round in which
            their syndrome was not clean; peak = int64 [frames]: the largest |P - R| in front of the store rule that the
            frame saw in any round, peak_deg3 the same over the columns of degree 3 and more).

    stop(hard uint8 [n, N]) -> bool [n], optional: the CRC rule, OR-ed with the syndrome.
    raw_cols (bool [N]) is no part of the definition: the model of a WRONG kernel in which the marked columns see the
    check->variable messages as _check_raw gives them -- a column-fused check kernel that forgets MsgRound / MsgStart in
    its registers.  Their posterior and the Q stored from it are then computed in float32."""
    y = np.ascontiguousarray(y, F32).reshape(-1, code.N)
    frames = y.shape[0]
    L = limit(q)
    c = channel_values(y, llr_scale, q)
    Q = c[:, code.cols].copy()
    hard = np.zeros((frames, code.N), np.uint8)
    post = np.zeros((frames, code.N), I32)
    iters = np.zeros(frames, I32)
    by_stop = np.zeros(frames, bool)
    r_tap = np.full((frames, code.E), TAP_UNSET, I32) if tap_iter else None
    q_tap = np.full((frames, code.E), TAP_UNSET, I32) if tap_iter else None
    hard_tap = np.zeros((frames, code.N), np.uint8) if tap_iter else None
    raw_edges = None if raw_cols is None else np.asarray(raw_cols, bool)[code.cols]
    peak, peak_deg3 = np.zeros(frames, np.int64), np.zeros(frames, np.int64)
    deg3_edges = (np.bincount(code.cols, minlength=code.N) >= 3)[code.cols]
    A =np.arange(frames)
    for t in range(1, max_iter + 1):
        R = _check(code, Q[A], scale, offset, q)
        R_stored = R
        if raw_edges is not None:
            R = np.where(raw_edges[None, :], _check_raw(code, Q[A], scale, offset), R.astype(F32)).astype(F32)
        Rx = np.concatenate([R, np.zeros((len(A), 1), R.dtype)], axis=1)
        P = c[A].astype(R.dtype)
        for k in range(code.col_edges.shape[1]):             # ascending edge id along every column
            P = P + Rx[:, code.col_edges[:, k]]
        h = (~(P > 0)).astype(np.uint8)
        hard[A] = h
        post[A] = P if raw_edges is None else np.rint(P).astype(I32)
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
        wide = np.abs(np.rint(P[:, code.cols] - R)).astype(np.int64)
        peak[A] = np.maximum(peak[A], wide.max(axis=1))
        peak_deg3[A] = np.maximum(peak_deg3[A], wide[:, deg3_edges].max(axis=1))
        Q[A] = sq(P[:, code.cols] - R, q)
        assert np.abs(Q[A]).max() <= L
        if tap_iter == t:
            q_tap[A] = Q[A]
    return dict(out=code.pack(hard, pack_mode), iters=iters, hard=hard, r_tap=r_tap, q_tap=q_tap, hard_tap=hard_tap,
                c=c, post=post, by_stop=np.nonzero(by_stop)[0], peak=peak, peak_deg3=peak_deg3)


def edge_inputs(q):
    """The inputs of the conversion tests, float32 [n]: every integer of [-L - 2, L + 2], every half-integer tie in that range
    and its two float32 neighbours, and the edge list of the definition."""
    L = limit(q)
    ints = np.arange(-L - 2, L + 3).astype(F32)
    ties = (ints[:-1] + F32(0.5)).astype(F32)
    near = np.concatenate([ties, np.nextafter(ties, F32(np.inf)), np.nextafter(ties, F32(-np.inf))])
    extra = np.array([L + 0.49, L + 0.5, 1000, np.inf, 0.0, 1e-41, 1e-8, 0.49999997, 3.4e38, 128, 129, 255, 256, 257], F32)
    return np.concatenate([ints, near, extra, -extra, [F32(np.nan)]]).astype(F32)
