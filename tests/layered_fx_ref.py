"""Fixed-point layered min-sum (LDPC_ALGO_LAYERED_FX), the reference of tests/test_layered_fx_cpu.py and
tests/test_gpu_layered_fx.py (a helper, not a test module).

algo = layered_fx is this repository's own definition (include/ldpc_hip.h: LDPC_ALGO_LAYERED_FX): the layered schedule on
saturating integers, q-bit messages (L = 2^(q-1) - 1) and a posterior MEMORY of p bits (LP = 2^(p-1) - 1).  The rule is
restated here in numpy int32 ONLY, apart from the two places the definition itself states in float32, both imported from
fixed_ref, not copied: the channel multiply, c = sq(llr_scale * y), and the corrected magnitude,
m' = fminf(truncf(fmaxf(m - ms_offset, 0) * ms_scale), L).

    P = c, R = 0, bit = (c < 0)
    layer by layer, every row of the layer independently (its columns are distinct, rows of a layer share none):
        t_k = P[col_k] - R_k                      exact
        x_k = clamp(t_k, -L, L)
        the check row of LDPC_MSG_I8 on x: sign = XOR of (x < 0), the two smallest |x| from a start value that reads L,
            corrected if asked, edge k takes the second minimum iff it holds the first
        R_k = that message ;  P[col_k] = clamp(t_k + R_k, -LP, LP)
    after the last layer: bit = P < 0, syndrome, freeze, iters -- as layered_bp_ref.layered_bp

Same interface as layered_bp_ref.layered_bp.  Messages and posteriors are int32 arrays; a tap that was never written holds
TAP_UNSET."""
import numpy as np

from fixed_ref import START, TAP_UNSET, channel_values, corrected, limit, sq  # noqa: F401  (sq: for the callers)
from ms_correction_ref import Code  # noqa: F401  (the code object layered_fx() takes)

F32 = np.float32
I32 = np.int32


def post_limit(p):
    assert 4 <= p <= 16, p
    return (1 << (p - 1)) - 1


def _layers(code, z):
    """per layer: (ev, cv, valid): the valid edge ids in row-major order, their columns, the [z, dmax] mask they fill"""
    key = "_layered_fx_%d" % z
    g = getattr(code, key, None)
    if g is None:
        g = []
        for l in range(code.M // z):
            valid = code.row_valid[l * z:(l + 1) * z]
            ev = code.row_edges[l * z:(l + 1) * z][valid]
            cv = code.cols[ev]
            assert len(np.unique(cv)) == len(cv), "rows of a layer share a column"
            g.append((ev, cv, valid))
        setattr(code, key, g)
    return g


def row(x, valid, scale, offset, q):
    """The check row on x int32 [n, z, dmax] (entries outside `valid` ignored): the messages out, int32 [n, z, dmax]"""
    big = I32(1 << 20)
    a = np.where(valid[None], np.abs(x), big)
    idx = np.argmin(a, axis=2)                                  # the first smallest
    m1 = np.minimum(np.take_along_axis(a, idx[..., None], 2)[..., 0], I32(START))
    a2 = a.copy()
    np.put_along_axis(a2, idx[..., None], big, 2)
    m2 = np.minimum(a2.min(axis=2), I32(START))
    if scale != 0 or offset != 0:
        m1, m2 = corrected(m1, scale, offset, q), corrected(m2, scale, offset, q)
    else:
        m1, m2 = np.minimum(m1, I32(limit(q))), np.minimum(m2, I32(limit(q)))     # the start value reads L
    neg = (x < 0) & valid[None]
    par = np.bitwise_xor.reduce(neg, axis=2)
    k = np.arange(x.shape[2])
    b = np.where(k[None, None, :] == idx[..., None], m2[..., None], m1[..., None])
    return np.where(par[..., None] ^ neg, -b, b).astype(I32)


def layered_fx(code, y, layer_rows, max_iter, scale=0.0, offset=0.0, q=8, p=16, llr_scale=1.0, tap_iter=0, pack_mode=0,
               stop=None, early_term=True):
    """dict(out, iters, hard, r_tap, hard_tap as ms_correction_ref.layered_ms gives them, r_tap int32; p_tap = int32
            [frames, N]: P after the last layer of round tap_iter; c = the stored channel values; post = int32 [frames, N]:
            P after the last layer of the round each frame stopped in; by_stop = frames stopped by `stop` in a round in
            which their syndrome was not clean; and what the premises of the tests ask about, per frame over all rounds:
            peak_t = largest |t_k|, peak_sum = largest |t_k + R_k| in front of the posterior clamp, sat = writes of P that
            the clamp changed, at_limit = writes of P that gave +-LP, zero_t = t_k that were exactly 0).

    stop(hard uint8 [n, N]) -> bool [n], optional: the CRC rule, OR-ed with the syndrome.
    early_term False: no frame stops before max_iter."""
    y = np.ascontiguousarray(y, F32).reshape(-1, code.N)
    frames, z = y.shape[0], int(layer_rows)
    assert z > 0 and code.M % z == 0
    L, LP = limit(q), post_limit(p)
    assert q <= p
    c = channel_values(y, llr_scale, q)
    P_all = c.copy()
    R_all = np.zeros((frames, code.E), I32)
    hard = (c < 0).astype(np.uint8)
    post = c.copy()
    iters = np.zeros(frames, I32)
    by_stop = np.zeros(frames, bool)
    r_tap = np.full((frames, code.E), TAP_UNSET, I32) if tap_iter else None
    p_tap = np.full((frames, code.N), TAP_UNSET, I32) if tap_iter else None
    hard_tap = np.zeros((frames, code.N), np.uint8) if tap_iter else None
    peak_t, peak_sum = np.zeros(frames, np.int64), np.zeros(frames, np.int64)
    sat, at_limit, zero_t = np.zeros(frames, np.int64), np.zeros(frames, np.int64), np.zeros(frames, np.int64)
    layers = _layers(code, z)
    A = np.arange(frames)
    for it in range(1, max_iter + 1):
        P, R = P_all[A], R_all[A]
        n = len(A)
        for ev, cv, valid in layers:
            if len(ev) == 0:
                continue
            t = P[:, cv] - R[:, ev]                              # exact, not clamped
            x = np.zeros((n,) + valid.shape, I32)
            x[:, valid] = np.clip(t, -L, L)
            rn = row(x, valid, scale, offset, q)[:, valid]
            s = t + rn
            pn = np.clip(s, -LP, LP)
            R[:, ev] = rn
            P[:, cv] = pn
            peak_t[A] = np.maximum(peak_t[A], np.abs(t).max(axis=1))
            peak_sum[A] = np.maximum(peak_sum[A], np.abs(s).max(axis=1))
            sat[A] += (pn != s).sum(axis=1)
            at_limit[A] += (np.abs(pn) == LP).sum(axis=1)
            zero_t[A] += (t == 0).sum(axis=1)
        assert np.abs(R).max() <= L and np.abs(P).max() <= LP
        P_all[A], R_all[A] = P, R
        h = (P < 0).astype(np.uint8)
        hard[A] = h
        post[A] = P
        ok = code.syndrome_ok(h)
        if stop is not None:
            extra = np.asarray(stop(h), bool)
            by_stop[A[extra & ~ok]] = True
            ok = ok | extra
        iters[A] = it
        if tap_iter == it:
            r_tap[A] = R
            p_tap[A] = P
            hard_tap[A] = h
        if it == max_iter:
            break
        if early_term:
            A = A[~ok]
        if len(A) == 0:
            break
    return dict(out=code.pack(hard, pack_mode), iters=iters, hard=hard, r_tap=r_tap, p_tap=p_tap, hard_tap=hard_tap, c=c,
                post=post, by_stop=np.nonzero(by_stop)[0], peak_t=peak_t, peak_sum=peak_sum, sat=sat, at_limit=at_limit,
                zero_t=zero_t)


def soft_of(w, kind):
    """float32 [frames, N]: the stop-round posterior, or that minus the stored channel value, in LSBs"""
    return (w["post"] if kind == "posterior" else w["post"] - w["c"]).astype(F32)
