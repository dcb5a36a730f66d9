"""Fixed-point layered box-plus (LDPC_ALGO_LAYERED_BP_FX), the reference of tests/test_layered_bp_fx_cpu.py and
tests/test_gpu_layered_bp_fx.py (a helper, not a test module).

algo = layered_bp_fx is this repository's own definition (include/ldpc_hip.h: LDPC_ALGO_LAYERED_BP_FX): the schedule, the
widths and the clamps of layered_fx (tests/layered_fx_ref.py) with a box-plus row computed the way hardware does, the
minimum plus a correction read from a table T of f fractional bits.  The rule is restated here in numpy int32 ONLY, as the
header states it -- signs and all, with no shortcut the kernels take --, apart from the channel multiply c = sq(llr_scale * y),
which the definition states in float32 and which is imported from fixed_ref, not copied.  The table is an ARGUMENT: the
tests hand in what the library's ldpc_bp_fx_table returns, so no libm stands between the kernels and this file.

    a [+] b = s ? -g : g,  s = (a < 0) XOR (b < 0),  m = min(|a|, |b|),  g = max(0, m + T[|a| + |b|] - T[||a| - |b||])
    row of degree D >= 2:  F_0 = x_0, F_k = F_{k-1} [+] x_k;  B_{D-1} = x_{D-1}, B_k = x_k [+] B_{k+1};
                           R_0 = B_1, R_{D-1} = F_{D-2}, R_k = F_{k-1} [+] B_{k+1} otherwise
    row of degree 1:       R_0 = +L
    P = c, R = 0; t_k = P[col_k] - R_k; x_k = clamp(t_k, -L, L); P[col_k] = clamp(t_k + R_k, -LP, LP)

Same interface as layered_fx_ref.layered_fx with the table in place of the min-sum correction."""
import numpy as np

from fixed_ref import TAP_UNSET, channel_values, limit  # noqa: F401
from layered_fx_ref import _layers, post_limit, soft_of  # noqa: F401  (soft_of: for the callers)
from ms_correction_ref import Code  # noqa: F401  (the code object layered_bp_fx() takes)

F32 = np.float32
I32 = np.int32


def padded(table, q):
    """T as the rule reads it: int32, zeros behind its last entry, long enough for |a| + |b| <= 2 L"""
    t = np.asarray(table, I32)
    assert t.ndim == 1 and t.size >= 1 and t[-1] == 0 and (t >= 0).all(), t
    out = np.zeros(max(t.size, 2 * limit(q) + 1), I32)
    out[:t.size] = t
    return out


def boxplus(a, b, T, stats=None):
    """a [+] b on int32 arrays, T from padded().  stats, a dict, counts in "clipped" the results the max with 0 changed and
    in "zero_g" those that are 0 although neither input is."""
    a, b = np.asarray(a, I32), np.asarray(b, I32)
    ma, mb = np.abs(a), np.abs(b)
    m = np.minimum(ma, mb)
    raw = m + T[ma + mb] - T[np.abs(ma - mb)]
    g = np.maximum(raw, 0)
    if stats is not None:
        stats["clipped"] = stats.get("clipped", 0) + int((raw < 0).sum())
        stats["zero_g"] = stats.get("zero_g", 0) + int(((g == 0) & (m > 0)).sum())
    return np.where((a < 0) ^ (b < 0), -g, g).astype(I32)


def row(x, valid, T, q, stats=None):
    """The row on x int32 [n, z, dmax] (row j has its deg_j = valid[j].sum() entries in front; the others are ignored): the
    messages out, int32 [n, z, dmax], 0 outside `valid`."""
    n, z, dmax = x.shape
    deg = valid.sum(axis=1)                                     # [z]
    L = I32(limit(q))
    out = np.zeros_like(x)
    if dmax == 0:
        return out
    # rows are handled by degree: every row of one degree runs the same association
    for D in np.unique(deg):
        D = int(D)
        rows = np.nonzero(deg == D)[0]
        if D == 0:
            continue
        xs = x[:, rows, :D]                                     # [n, r, D]
        if D == 1:
            o = np.full_like(xs, L)
        elif D == 2:
            o = xs[:, :, ::-1].copy()
        else:
            F = np.zeros_like(xs)
            F[:, :, 0] = xs[:, :, 0]
            for k in range(1, D - 1):
                F[:, :, k] = boxplus(F[:, :, k - 1], xs[:, :, k], T, stats)
            B = np.zeros_like(xs)
            B[:, :, D - 1] = xs[:, :, D - 1]
            for k in range(D - 2, 0, -1):
                B[:, :, k] = boxplus(xs[:, :, k], B[:, :, k + 1], T, stats)
            o = np.zeros_like(xs)
            o[:, :, 0] = B[:, :, 1]
            o[:, :, D - 1] = F[:, :, D - 2]
            for k in range(1, D - 1):
                o[:, :, k] = boxplus(F[:, :, k - 1], B[:, :, k + 1], T, stats)
        out[:, rows, :D] = o
    return out


def layered_bp_fx(code, y, layer_rows, max_iter, table, q=8, p=16, llr_scale=1.0, tap_iter=0, pack_mode=0, stop=None,
                  early_term=True):
    """dict(out, iters, hard, r_tap, p_tap, hard_tap, c, post, by_stop, peak_t, peak_sum, sat, at_limit, zero_t as
            layered_fx_ref.layered_fx gives them, and per call: clipped = box-plus results the max with 0 changed, zero_g =
            box-plus results that are 0 although neither input is).

    table: T_f as ldpc_bp_fx_table returns it.  stop, early_term: as layered_fx_ref.layered_fx."""
    y = np.ascontiguousarray(y, F32).reshape(-1, code.N)
    frames, z = y.shape[0], int(layer_rows)
    assert z > 0 and code.M % z == 0
    L, LP = limit(q), post_limit(p)
    assert q <= p
    T = padded(table, q)
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
    stats = {"clipped": 0, "zero_g": 0}
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
            rn = row(x, valid, T, q, stats)[:, valid]
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
                zero_t=zero_t, clipped=stats["clipped"], zero_g=stats["zero_g"])
