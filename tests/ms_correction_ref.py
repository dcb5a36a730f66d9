"""Normalized / offset min-sum, restated in numpy from the CPU oracle's semantics (oracle/ldpc_oracle.c:
oracle_decode_ms and oracle_decode_layered), vectorised over frames, fp32 throughout.

With scale = offset = 0 both decoders are the oracle's own min-sum decoders; otherwise each check row's two
magnitude candidates m become

    m' = fmaxf(m - offset, 0) * scale        (fp32, scale 0 meaning 1)

once per row and frame, before the per-edge selection and sign (include/ldpc_hip.h: ms_scale / ms_offset).
With fp16 messages (flooding only) the channel values and the variable->check messages are rounded to binary16
where they are stored, and so is the corrected magnitude where the check->variable message is produced.

Each decoder returns dict(out=packed bytes, iters=int32[frames], hard=uint8[frames, N], r_tap=float32[frames, E]
or None, hard_tap=uint8[frames, N] (the hard bits at iteration tap_iter) or None, and for layered undefined=uint8[frames]: a row none of whose |q| is <= 1000 -- the oracle's "undefined
frame", where the reference reads an uninitialised index).  flood_ms also returns q_tap=float32[frames, E] or None: the
variable->check messages after round tap_iter, NaN-filled for the frames that had stopped by then (the oracle's taps["q"])."""
import numpy as np

F32 = np.float32


def _f16(x):
    with np.errstate(over="ignore"):                        # |x| >= 65520 rounds to infinity: that is the definition
        return x.astype(np.float16).astype(F32)


def _corr(m, scale, offset, f16=False):
    """The corrected candidate, fp32: fmaxf(m - offset, 0) * scale; fp16: rounded where R is produced."""
    if scale == 0 and offset == 0:
        return m
    a = F32(scale if scale != 0 else 1.0)
    r = (np.maximum(m - F32(offset), F32(0)) * a).astype(F32)
    return _f16(r) if f16 else r


class Code:
    """H as its nonzeros in row-major order (edge id = rank), as the C ABI takes it."""

    def __init__(self, rows, cols, M, N, K):
        self.rows = np.asarray(rows, np.int64)
        self.cols = np.asarray(cols, np.int64)
        self.M, self.N, self.K, self.E = int(M), int(N), int(K), len(self.cols)
        self.row_ptr = np.zeros(self.M + 1, np.int64)
        np.add.at(self.row_ptr, self.rows + 1, 1)
        self.row_ptr = np.cumsum(self.row_ptr)
        deg = np.diff(self.row_ptr)
        self.dmax = int(deg.max())
        # [M, dmax] edge ids of every row, ascending; padding points at edge E (a sentinel slot)
        k = np.arange(self.dmax)
        self.row_edges = np.where(k[None, :] < deg[:, None], self.row_ptr[:-1, None] + k[None, :], self.E)
        self.row_valid = k[None, :] < deg[:, None]
        # columns: [N, cmax] edge ids in ascending order, padding = E
        order = np.lexsort((np.arange(self.E), self.cols))
        cdeg = np.bincount(self.cols, minlength=self.N)
        cptr = np.concatenate([[0], np.cumsum(cdeg)])
        cmax = int(cdeg.max())
        k = np.arange(cmax)
        pos = np.where(k[None, :] < cdeg[:, None], cptr[:-1, None] + k[None, :], 0)
        self.col_edges = np.where(k[None, :] < cdeg[:, None], order[pos], self.E)

    def syndrome_ok(self, hard):
        """hard: uint8 [F, N] -> bool [F]: every row of even parity."""
        h = np.concatenate([hard, np.zeros((hard.shape[0], 1), np.uint8)], axis=1)
        cols = np.where(self.row_valid, self.cols[np.minimum(self.row_edges, self.E - 1)], self.N)
        par = np.bitwise_xor.reduce(h[:, cols], axis=2)
        return ~np.any(par, axis=1)

    def pack(self, hard, pack_mode=0):
        """oracle pack_frame: pack_mode 0 = toChar (K/8 whole bytes at frame*K/8), 1 = bit offsets."""
        frames, K = hard.shape[0], self.K
        if pack_mode == 0:
            n = (frames - 1) * K // 8 + K // 8 if frames else 0
            out = np.zeros(n, np.uint8)
            nb = K // 8
            w = (hard[:, :nb * 8].reshape(frames, nb, 8).astype(np.uint32) << np.arange(8, dtype=np.uint32)).sum(axis=2)
            for f in range(frames):
                base = f * K // 8
                out[base:base + nb] = w[f]
            return out
        bits = hard[:, :K].reshape(-1)
        out = np.zeros((frames * K + 7) // 8, np.uint8)
        idx = np.nonzero(bits)[0]
        np.bitwise_or.at(out, idx // 8, (1 << (idx % 8)).astype(np.uint8))
        return out


def _check_ms(code, Q, scale, offset, f16):
    """refreshRMS over all rows: R_e = sign * (min over the row's other |q|, from 1000), corrected."""
    frames = Q.shape[0]
    Qx = np.concatenate([Q, np.full((frames, 1), np.inf, F32)], axis=1)
    x = Qx[:, code.row_edges]                               # [F, M, dmax]
    a = np.abs(x)
    a = np.where(np.isnan(a), F32(np.inf), a)               # fminf skips a NaN message (its sign test x < 0 is false)
    idx = np.argmin(a, axis=2)
    m1 = np.minimum(np.take_along_axis(a, idx[..., None], 2)[..., 0], F32(1000))
    a2 = a.copy()
    np.put_along_axis(a2, idx[..., None], np.inf, 2)
    m2 = np.minimum(a2.min(axis=2), F32(1000))
    m1, m2 = _corr(m1, scale, offset, f16), _corr(m2, scale, offset, f16)
    neg = (x < 0) & code.row_valid[None]
    par = np.bitwise_xor.reduce(neg, axis=2)
    k = np.arange(code.dmax)
    b = np.where(k[None, None, :] == idx[..., None], m2[..., None], m1[..., None])
    s = par[..., None] ^ neg
    r = np.where(s, -b, b).astype(F32)
    R = np.zeros((frames, code.E + 1), F32)
    R[:, code.row_edges[code.row_valid]] = r[:, code.row_valid]
    return R[:, :code.E]


def flood_ms(code, y, max_iter, scale=0.0, offset=0.0, f16=False, tap_iter=0, pack_mode=0, raw_cols=None):
    """oracle_decode_ms with the correction.

    raw_cols (bool [N], fp16 with a correction only) is no part of the definition: it is the model of a WRONG kernel
    for tests/test_fp16_cpu.py.  The marked columns see the corrected check->variable messages as they are before
    their rounding to binary16 -- what a column-fused check kernel would compute if it rounded R only where it
    stores it, since the fused columns' R stay in registers.  Every stored R (the tap included) is still rounded."""
    y = np.ascontiguousarray(y, F32).reshape(-1, code.N)
    frames = y.shape[0]
    with np.errstate(invalid="ignore"):                     # inf - inf and NaN inputs are part of what is defined
        return _flood_ms(code, y, frames, max_iter, scale, offset, f16, tap_iter, pack_mode, raw_cols)


def _flood_ms(code, y, frames, max_iter, scale, offset, f16, tap_iter, pack_mode, raw_cols):
    yf = _f16(y) if f16 else y.copy()
    Q = yf[:, code.cols].copy()
    hard = np.zeros((frames, code.N), np.uint8)
    iters = np.zeros(frames, np.int32)
    r_tap = np.full((frames, code.E), np.nan, F32) if tap_iter else None
    q_tap = np.full((frames, code.E), np.nan, F32) if tap_iter else None
    hard_tap = np.zeros((frames, code.N), np.uint8) if tap_iter else None
    raw_edges = None if raw_cols is None else np.asarray(raw_cols, bool)[code.cols]
    A = np.arange(frames)
    for t in range(1, max_iter + 1):
        R = _check_ms(code, Q[A], scale, offset, f16)
        R_stored = R
        if raw_edges is not None:
            R = np.where(raw_edges[None, :], _check_ms(code, Q[A], scale, offset, False), R)
        Rx = np.concatenate([R, np.full((len(A), 1), -0.0, F32)], axis=1)
        P = yf[A].copy()
        for k in range(code.col_edges.shape[1]):             # ascending edge id along every column
            P = P + Rx[:, code.col_edges[:, k]]
        h = (~(P > 0)).astype(np.uint8)
        hard[A] = h
        ok = code.syndrome_ok(h)
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
        Qn = P[:, code.cols] - R
        Q[A] = _f16(Qn) if f16 else Qn
        if tap_iter == t:
            q_tap[A] = Q[A]
    return dict(out=code.pack(hard, pack_mode), iters=iters, hard=hard, r_tap=r_tap, q_tap=q_tap, hard_tap=hard_tap)


def _cl_sign(x):
    return np.where(x > 0, F32(1), np.where(x < 0, F32(-1), np.where(x == 0, x, F32(0)))).astype(F32)


def layered_ms(code, y, layer_rows, max_iter, scale=0.0, offset=0.0, tap_iter=0, pack_mode=0):
    """oracle_decode_layered (the fused TDMP kernel's semantics, 1000 / 1001 start values, <=) with the
    correction applied to b and c of every row."""
    y = np.ascontiguousarray(y, F32).reshape(-1, code.N)
    frames, z = y.shape[0], int(layer_rows)
    assert z > 0 and code.M % z == 0
    P_all = y.copy()
    R_all = np.zeros((frames, code.E + 1), F32)
    hard = np.zeros((frames, code.N), np.uint8)
    iters = np.zeros(frames, np.int32)
    undefined = np.zeros(frames, np.uint8)
    r_tap = np.full((frames, code.E), np.nan, F32) if tap_iter else None
    hard_tap = np.zeros((frames, code.N), np.uint8) if tap_iter else None
    A = np.arange(frames)
    colx = np.concatenate([code.cols, [0]])
    with np.errstate(over="ignore", under="ignore"):       # the sign product may overflow: only its sign is used
        return _layered(code, P_all, R_all, hard, iters, undefined, r_tap, hard_tap, A, colx, z, max_iter, scale,
                        offset, tap_iter, pack_mode)


def _layered(code, P_all, R_all, hard, iters, undefined, r_tap, hard_tap, A, colx, z, max_iter, scale, offset,
             tap_iter, pack_mode):
    for t in range(1, max_iter + 1):
        P, R = P_all[A], R_all[A]
        n = len(A)
        for l in range(code.M // z):
            edges = code.row_edges[l * z:(l + 1) * z]           # [z, dmax]
            valid = code.row_valid[l * z:(l + 1) * z]
            cols = colx[edges]
            a = np.ones((n, z), F32)
            b = np.full((n, z), 1000, F32)
            c = np.full((n, z), 1001, F32)
            bind = np.full((n, z), -1, np.int64)
            sg = np.zeros((n, z, code.dmax), F32)
            for k in range(code.dmax):                          # edge by edge along every row of the layer
                rv = np.nonzero(valid[:, k])[0]                 # rows that have a k-th edge (distinct columns)
                ck, ek = cols[rv, k], edges[rv, k]
                tmp = P[:, ck] - R[:, ek]
                sg[:, rv, k] = _cl_sign(tmp)
                a[:, rv] = a[:, rv] * tmp
                P[:, ck] = tmp
                mag = np.abs(tmp)
                bb, cc = b[:, rv], c[:, rv]
                le_b = mag <= bb
                in_c = ~le_b & (mag > bb) & (mag <= cc)
                c[:, rv] = np.where(le_b, bb, np.where(in_c, mag, cc))
                bind[:, rv] = np.where(le_b, k, bind[:, rv])
                b[:, rv] = np.where(le_b, mag, bb)
            und = np.any((bind < 0) & valid.any(axis=1)[None, :], axis=1)
            undefined[A[und]] = 1
            b, c = _corr(b, scale, offset), _corr(c, scale, offset)
            a = _cl_sign(a)
            ab, ac = a * b, a * c
            for k in range(code.dmax):
                rv = np.nonzero(valid[:, k])[0]
                ck, ek = cols[rv, k], edges[rv, k]
                rn = (sg[:, rv, k] * np.where(bind[:, rv] == k, ac[:, rv], ab[:, rv])).astype(F32)
                R[:, ek] = rn
                P[:, ck] = P[:, ck] + rn
        P_all[A], R_all[A] = P, R
        h = (P < 0).astype(np.uint8)
        hard[A] = h
        ok = code.syndrome_ok(h)
        iters[A] = t
        if tap_iter == t:
            r_tap[A] = R[:, :code.E]
            hard_tap[A] = h
        if t == max_iter:
            break
        A = A[~ok]
        if len(A) == 0:
            break
    return dict(out=code.pack(hard, pack_mode), iters=iters, hard=hard, r_tap=r_tap, hard_tap=hard_tap,
                undefined=undefined)
