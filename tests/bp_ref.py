"""Log-domain sum-product (LDPC_ALGO_BP), the reference of tests/test_bp_cpu.py and tests/test_gpu_bp.py (a helper, not a
test module).

algo = bp is this repository's own definition (include/ldpc_hip.h: LDPC_ALGO_BP): min-sum's variable node with a
box-plus check node, every operation fp32 and one at a time.

    chan  = llr_scale * y                                      one multiply, rounded where stored
    t_j   = sign(x_j) * fminf(|x_j|, 1000)                     NaN reads +1000, -0 reads +0, +-inf read +-1000
    c(x)  = fmaxf(0.6931472f - 0.25f * x, 0)
    u[+]v = sign * fmaxf((fminf(|u|, |v|) + c(|u| + |v|)) - c(||u| - |v||), 0),   sign = -1 iff (u < 0) != (v < 0)
    row:    f_0 = t_0, f_j = f_{j-1} [+] t_j;  b_{D-1} = t_{D-1}, b_j = t_j [+] b_{j+1};
            out_0 = b_1, out_{D-1} = f_{D-2}, out_k = f_{k-1} [+] b_{k+1};  D = 2: the other input;  D = 1: +1000
    R_k   = rnd(out_k), where it is produced

flood() restates it in numpy, modelled on fp8_ref.flood, with the correction `c`, the storage rounding `rnd` (identity /
binary16) and llr_scale as PARAMETERS.  With c = zero it is flooding min-sum: tests/test_bp_cpu.py holds it to the C oracle
with the identity and to the fp16 oracle with binary16 rounding, bit for bit.  numpy's float32 operations are IEEE
operations one at a time, so nothing else is needed for 0 ulp."""
import numpy as np

from ms_correction_ref import Code  # noqa: F401  (the code object flood() takes)

F32 = np.float32
LN2 = F32(0.6931472)
assert LN2.view(np.uint32) == 0x3F317218
CLAMP = F32(1000.0)


def identity(x):
    return x


def f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, F32).astype(np.float16).astype(F32)


def linear(x):
    """the correction of the definition"""
    return np.maximum(LN2 - F32(0.25) * x, F32(0))


def zero(x):
    """c == 0: box-plus is min with the sign product -- min-sum"""
    return np.zeros_like(x)


def clamp(x):
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        a = np.fmin(np.abs(x), CLAMP)                           # fminf drops a NaN
        return np.where(x < 0, -a, a).astype(F32)


def boxplus(u, v, c=linear):
    """float32 arrays of clamped values (finite)"""
    au, av = np.abs(u), np.abs(v)
    m = np.fmin(au, av)
    s = (au + av).astype(F32)
    d = np.abs((au - av).astype(F32))
    g = np.maximum(((m + c(s)).astype(F32) - c(d)).astype(F32), F32(0))
    return np.where((u < 0) != (v < 0), -g, g).astype(F32)


def _row_groups(code):
    """[(D, edges int64 [n, D])]: the rows of every degree D >= 1 with their edge ids, ascending"""
    g = getattr(code, "_bp_groups", None)
    if g is None:
        deg = np.diff(code.row_ptr)
        g = []
        for D in np.unique(deg):
            if D == 0:
                continue
            r = np.nonzero(deg == D)[0]
            g.append((int(D), code.row_ptr[r][:, None] + np.arange(D)[None, :]))
        code._bp_groups = g
    return g


def check(code, Q, c=linear, rnd=identity):
    """R float32 [frames, E] from Q float32 [frames, E]"""
    R = np.zeros_like(Q)
    for D, edges in _row_groups(code):
        t = clamp(Q[:, edges])                                  # [F, n, D]
        out = np.empty_like(t)
        if D == 1:
            out[..., 0] = CLAMP
        elif D == 2:
            out[..., 0], out[..., 1] = t[..., 1], t[..., 0]
        else:
            b = [None] * D
            b[D - 1] = t[..., D - 1]
            for j in range(D - 2, 0, -1):
                b[j] = boxplus(t[..., j], b[j + 1], c)
            out[..., 0] = b[1]
            f = t[..., 0]
            for k in range(1, D - 1):
                out[..., k] = boxplus(f, b[k + 1], c)
                f = boxplus(f, t[..., k], c)
            out[..., D - 1] = f
        R[:, edges] = rnd(out)
    return R


def flood(code, y, max_iter, c=linear, rnd=identity, llr_scale=1.0, tap_iter=0, pack_mode=0, raw_cols=None, stop=None):
    """dict(out, iters, hard, r_tap, q_tap, hard_tap as ms_correction_ref.flood_ms gives them;
            chan = the stored channel values rnd(llr_scale * y), post = float32 [frames, N]: the posterior
            chan + R_e1 + R_e2 + ... (fp32, ascending edge id) of the round each frame stopped in, by_stop = frames
            stopped by `stop` in a round in which their syndrome was not clean).

    stop(hard uint8 [n, N]) -> bool [n], optional: a frame also stops in the first round whose hard bits it passes (the
    CRC rule of include/ldpc_hip.h), OR-ed with the syndrome.
    raw_cols (bool [N]) is no part of the definition: the model of a WRONG kernel in which the marked columns see the
    check->variable messages as they are BEFORE rnd -- a column-fused check kernel that rounds R only where it stores it."""
    y = np.ascontiguousarray(y, F32).reshape(-1, code.N)
    with np.errstate(invalid="ignore", over="ignore"):
        return _flood(code, y, max_iter, c, rnd, F32(llr_scale), tap_iter, pack_mode, raw_cols, stop)


def _flood(code, y, max_iter, c, rnd, llr_scale, tap_iter, pack_mode, raw_cols, stop):
    frames = y.shape[0]
    yf = rnd((llr_scale * y).astype(F32)).astype(F32)
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
        R = check(code, Q[A], c, rnd)
        R_stored = R
        if raw_edges is not None:
            R = np.where(raw_edges[None, :], check(code, Q[A], c, identity), R)
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
                chan=yf, post=post, by_stop=np.nonzero(by_stop)[0])


def soft_of(w, kind):
    """float32 [frames, N]: the stop-round posterior, or that minus the stored channel value (one fp32 subtraction)"""
    with np.errstate(invalid="ignore"):
        return w["post"] if kind == "posterior" else (w["post"] - w["chan"]).astype(F32)
