"""Fixed-point layered min-sum with the 8-byte check record as the only row state: the data layout of
layered_ldsp_fx_kernel (LDPC_TUNE_FX_RECORD, include/ldpc_hip.h) restated in numpy, the helper of
tests/test_layered_fx_record_cpu.py (not a test module).

layered_fx_ref.layered_fx keeps E messages per frame.  Here a row keeps two uint32 words and nothing else:

    word 0: signs of R_0 .. R_{D-1} in bits 0 .. 23, argmin in bits 24 .. 28
    word 1: m1' in bits 0 .. 7, m2' in bits 8 .. 15 (after correction and the clamp to L), the int16 posterior of the row's
            single-layer ("external") column in bits 16 .. 31

and R_k = (sign_k ? -1 : 1) * (k == argmin ? m2' : m1') is rebuilt from them in the next round.  The posterior of a column
that one row only meets -- that row's last entry, not an information column -- lives in word 1 and not in P.  The two minima
are taken from the unclamped |t_k|, the start value 1000 among them, and clamped to L afterwards (a degree-1 row keeps the
start value as its second candidate), as the kernel does; the argmin is the first smallest.  Everything else -- the channel
values, the correction, rounds, syndrome, freezing, taps -- is layered_fx_ref's, imported and not copied."""
import numpy as np

from fixed_ref import START, TAP_UNSET, channel_values, corrected, limit
from layered_fx_ref import _layers, post_limit

I32 = np.int32
U32 = np.uint32
MAX_DEG = 24


def pack(signs, argmin, m1, m2, ext):
    """the two words (uint32 arrays) from their fields; ext is a signed 16-bit value"""
    signs, argmin, m1, m2, ext = (np.asarray(a).astype(np.int64) for a in (signs, argmin, m1, m2, ext))
    assert (signs >= 0).all() and (signs < 1 << 24).all() and (argmin >= 0).all() and (argmin < MAX_DEG).all()
    assert (m1 >= 0).all() and (m1 <= 127).all() and (m2 >= 0).all() and (m2 <= 127).all()
    assert (ext >= -32768).all() and (ext <= 32767).all()
    return (signs | argmin << 24).astype(U32), (m1 | m2 << 8 | (ext & 0xffff) << 16).astype(U32)


def unpack(w0, w1):
    """(signs, argmin, m1, m2, ext) as int32 arrays"""
    w0, w1 = np.asarray(w0, U32).astype(np.int64), np.asarray(w1, U32).astype(np.int64)
    ext = w1 >> 16
    ext = np.where(ext >= 32768, ext - 65536, ext)
    return ((w0 & 0xffffff).astype(I32), ((w0 >> 24) & 31).astype(I32), (w1 & 255).astype(I32), ((w1 >> 8) & 255).astype(I32),
            ext.astype(I32))


def messages(w0, w1, dmax):
    """R_k of every row for k < dmax, int32 [..., dmax] (entries beyond the row's degree are meaningless)"""
    signs, argmin, m1, m2, _ = unpack(w0, w1)
    k = np.arange(dmax)
    mag = np.where(k == argmin[..., None], m2[..., None], m1[..., None])
    return np.where((signs[..., None] >> k) & 1, -mag, mag).astype(I32)


def external_rows(code):
    """bool [M]: the row's last entry is a column of degree 1 that is no information column"""
    cdeg = np.bincount(code.cols, minlength=code.N)
    deg = np.diff(code.row_ptr)
    last = code.cols[np.maximum(code.row_ptr[1:] - 1, 0)]
    return (deg > 0) & (cdeg[last] == 1) & (last >= code.K)


def layered_fx_record(code, y, layer_rows, max_iter, scale=0.0, offset=0.0, q=8, p=16, llr_scale=1.0, tap_iter=0, pack_mode=0,
                      early_term=True, ext=True):
    """layered_fx_ref.layered_fx's interface (no stop predicate) and its out, iters, hard, r_tap, p_tap, hard_tap, c, post.
    ext False: every column in P, as LDPC_TUNE_OFF(LDPC_TUNE_LDSP_EXT)."""
    y = np.ascontiguousarray(y, np.float32).reshape(-1, code.N)
    frames, z = y.shape[0], int(layer_rows)
    assert z > 0 and code.M % z == 0 and code.dmax <= MAX_DEG
    L, LP = limit(q), post_limit(p)
    c = channel_values(y, llr_scale, q)
    deg = np.diff(code.row_ptr)
    is_ext = external_rows(code) if ext else np.zeros(code.M, bool)
    last = code.cols[np.maximum(code.row_ptr[1:] - 1, 0)]
    ext_cols = last[is_ext]
    in_p = np.ones(code.N, bool)
    in_p[ext_cols] = False
    k = np.arange(code.dmax)
    # an entry reads P unless it is the external one: the row's last
    from_rec = is_ext[:, None] & (k[None, :] == deg[:, None] - 1)            # [M, dmax]
    col = np.where(code.row_valid, code.cols[np.minimum(code.row_edges, code.E - 1)], 0)      # [M, dmax]

    P_all = np.where(in_p[None], c, TAP_UNSET).astype(I32)                      # external columns never live here
    W0 = np.zeros((frames, code.M), U32)
    W1 = np.zeros((frames, code.M), U32)
    W0[:, is_ext], W1[:, is_ext] = pack(0, 0, 0, 0, c[:, ext_cols])             # R = 0; the column starts from its channel value

    def posterior(P, w1):
        full = P.copy()
        full[:, ext_cols] = unpack(0, w1[:, is_ext])[4]
        return full

    def edge_order(w0, w1):
        R = np.zeros((w0.shape[0], code.E), I32)
        R[:, code.row_edges[code.row_valid]] = messages(w0, w1, code.dmax)[:, code.row_valid]
        return R

    hard = (c < 0).astype(np.uint8)
    post = c.copy()
    iters = np.zeros(frames, I32)
    r_tap = np.full((frames, code.E), TAP_UNSET, I32) if tap_iter else None
    p_tap = np.full((frames, code.N), TAP_UNSET, I32) if tap_iter else None
    hard_tap = np.zeros((frames, code.N), np.uint8) if tap_iter else None
    _layers(code, z)                                                            # its assertion: rows of a layer share no column
    A = np.arange(frames)
    big = I32(1 << 20)
    for it in range(1, max_iter + 1):
        P, w0a, w1a = P_all[A], W0[A], W1[A]
        for l in range(code.M // z):
            rows = slice(l * z, (l + 1) * z)
            valid, frec, cl, d = code.row_valid[rows], from_rec[rows], col[rows], deg[rows]
            w0, w1 = w0a[:, rows], w1a[:, rows]
            pin = np.where(frec[None], unpack(w0, w1)[4][..., None], P[:, cl])      # [n, z, dmax]
            t = pin - messages(w0, w1, code.dmax)
            a = np.where(valid[None], np.abs(t), big)
            idx = np.argmin(a, axis=2)
            m1 = np.minimum(np.take_along_axis(a, idx[..., None], 2)[..., 0], I32(START))
            a2 = a.copy()
            np.put_along_axis(a2, idx[..., None], big, 2)
            m2 = np.minimum(a2.min(axis=2), I32(START))
            idx = np.where(m1 < START, idx, 0)                                  # nothing below the start value: entry 0
            m1 = np.where(d[None] >= 1, np.minimum(m1, L), m1)
            m2 = np.where(d[None] >= 2, np.minimum(m2, L), m2)
            m1, m2 = corrected(m1, scale, offset, q), corrected(m2, scale, offset, q)   # scale 0 reads 1: plain is the identity
            neg = (t < 0) & valid[None]
            par = np.bitwise_xor.reduce(neg, axis=2)
            sign = (par[..., None] ^ neg) & valid[None]
            b = np.where(k == idx[..., None], m2[..., None], m1[..., None])
            pn = np.clip(t + np.where(sign, -b, b), -LP, LP).astype(I32)
            e = np.where(frec, pn, 0).sum(axis=2)                               # the external entry's posterior, if any
            e = np.where(frec.any(axis=1)[None], e, 0)
            n0, n1 = pack((sign << k).sum(axis=2), idx, m1, m2, e)
            w0a[:, rows], w1a[:, rows] = n0, n1
            to_p = valid & ~frec
            P[:, cl[to_p]] = pn[:, to_p]
        P_all[A], W0[A], W1[A] = P, w0a, w1a
        full = posterior(P, w1a)
        h = (full < 0).astype(np.uint8)
        hard[A], post[A] = h, full
        ok = code.syndrome_ok(h)
        iters[A] = it
        if tap_iter == it:
            r_tap[A], p_tap[A], hard_tap[A] = edge_order(w0a, w1a), full, h
        if it == max_iter:
            break
        if early_term:
            A = A[~ok]
        if len(A) == 0:
            break
    return dict(out=code.pack(hard, pack_mode), iters=iters, hard=hard, r_tap=r_tap, p_tap=p_tap, hard_tap=hard_tap, c=c,
                post=post)
