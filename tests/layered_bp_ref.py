"""Layered log-domain sum-product (LDPC_ALGO_LAYERED_BP), the reference of tests/test_layered_bp_cpu.py and
tests/test_gpu_layered_bp.py (a helper, not a test module).

algo = layered_bp is this repository's own definition (include/ldpc_hip.h: LDPC_ALGO_LAYERED_BP): the schedule and the
bookkeeping of the layered min-sum decoder (ms_correction_ref.layered_ms) with the row of the log-domain sum-product
(bp_ref.check / bp_ref.boxplus, imported here, not copied), every operation fp32 and one at a time.

    chan = llr_scale * y                 one multiply
    P = chan, R = 0
    layer by layer, every row of the layer independently (its columns are distinct, rows of a layer share none):
        q_k = P[col_k] - R_k ;  out = bp row of (q_0 .. q_{D-1}) ;  R_k = out_k ;  P[col_k] = q_k + R_k
    after the last layer: bit = P < 0, syndrome, freeze, iters -- as layered_ms

The correction `c` is a parameter: with c = bp_ref.zero the row is min with the sign parity, and the decoder is layered
min-sum except where layered_ms's running sign PRODUCT differs from a parity of (q < 0): a zero, a NaN, an underflow
(tests/test_layered_bp_cpu.py)."""
import types

import numpy as np

import bp_ref as RB
from ms_correction_ref import Code  # noqa: F401  (the code object layered_bp() takes)

F32 = np.float32


def _layers(code, z):
    """[(e_lo, e_hi, rows)]: the contiguous edge range of every layer and a row_ptr relative to it, as bp_ref.check reads it"""
    key = "_layered_bp_%d" % z
    g = getattr(code, key, None)
    if g is None:
        g = []
        for l in range(code.M // z):
            rp = code.row_ptr[l * z:(l + 1) * z + 1]
            g.append((int(rp[0]), int(rp[-1]), types.SimpleNamespace(row_ptr=rp - rp[0])))
        setattr(code, key, g)
    return g


def layered_bp(code, y, layer_rows, max_iter, c=RB.linear, llr_scale=1.0, tap_iter=0, pack_mode=0, stop=None,
               early_term=True):
    """dict(out, iters, hard, r_tap, hard_tap as ms_correction_ref.layered_ms gives them; p_tap = float32 [frames, N]: P
            after the last layer of round tap_iter (NaN-filled, like r_tap, for the frames that had stopped by then);
            chan = llr_scale * y; post = float32 [frames, N]: P after the last layer of the round each frame stopped in;
            by_stop = frames stopped by `stop` in a round in which their syndrome was not clean).  bp_ref.soft_of(result,
            kind) gives the soft values of either kind from it.

    stop(hard uint8 [n, N]) -> bool [n], optional: the CRC rule of include/ldpc_hip.h, OR-ed with the syndrome.
    early_term False: no frame stops before max_iter (iters = max_iter everywhere, the last round's bits)."""
    y = np.ascontiguousarray(y, F32).reshape(-1, code.N)
    z = int(layer_rows)
    assert z > 0 and code.M % z == 0
    with np.errstate(invalid="ignore", over="ignore"):
        return _layered_bp(code, y, z, max_iter, c, F32(llr_scale), tap_iter, pack_mode, stop, early_term)


def _layered_bp(code, y, z, max_iter, c, llr_scale, tap_iter, pack_mode, stop, early_term):
    frames = y.shape[0]
    chan = (llr_scale * y).astype(F32)
    P_all = chan.copy()
    R_all = np.zeros((frames, code.E), F32)
    hard = (chan < 0).astype(np.uint8)
    post = chan.copy()
    iters = np.zeros(frames, np.int32)
    by_stop = np.zeros(frames, bool)
    r_tap = np.full((frames, code.E), np.nan, F32) if tap_iter else None
    p_tap = np.full((frames, code.N), np.nan, F32) if tap_iter else None
    hard_tap = np.zeros((frames, code.N), np.uint8) if tap_iter else None
    layers = _layers(code, z)
    A = np.arange(frames)
    for t in range(1, max_iter + 1):
        P, R = P_all[A], R_all[A]
        for e_lo, e_hi, rows in layers:
            if e_hi == e_lo:
                continue
            cols = code.cols[e_lo:e_hi]                         # distinct within a layer
            q = (P[:, cols] - R[:, e_lo:e_hi]).astype(F32)
            out = RB.check(rows, q, c)
            R[:, e_lo:e_hi] = out
            P[:, cols] = (q + out).astype(F32)
        P_all[A], R_all[A] = P, R
        h = (P < 0).astype(np.uint8)
        hard[A] = h
        post[A] = P
        ok = code.syndrome_ok(h)
        if stop is not None:
            extra = np.asarray(stop(h), bool)
            by_stop[A[extra & ~ok]] = True
            ok = ok | extra
        iters[A] = t
        if tap_iter == t:
            r_tap[A] = R
            p_tap[A] = P
            hard_tap[A] = h
        if t == max_iter:
            break
        if early_term:
            A = A[~ok]
        if len(A) == 0:
            break
    return dict(out=code.pack(hard, pack_mode), iters=iters, hard=hard, r_tap=r_tap, p_tap=p_tap, hard_tap=hard_tap,
                chan=chan, post=post, by_stop=np.nonzero(by_stop)[0])
