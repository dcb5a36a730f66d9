"""What ldpc_decode_soft must return, from the CPU oracle alone (a helper, not a test module; never from the library
under test).

The rule (include/ldpc_hip.h): frame f's soft values are those of round i_f = iters[f], the round it stopped in.  The
oracle's taps are taken in ONE fixed round of a run, so expected() runs oracle.decode(..., tap_iter = i) once per distinct
value i of the oracle's iters, on the frames with iters[f] = i (frames are decoded independently of each other), and takes
their rows of taps["post"].  With the min-sum
correction (ms_scale / ms_offset), which the oracle does not have, the same is done with ms_correction_ref.flood_ms: its
r_tap of round i, and y + sum R formed here in np.float32, one add at a time in ascending edge id along the column.
Extrinsic = posterior - y in fp32 (y rounded to binary16 for the fp16 form).  Comparison is on the uint32 bit patterns:
0 ulp, the sign of zeros included."""
import numpy as np

import oracle

import ms_correction_ref as MC

F32 = np.float32


def f16_round(y):
    with np.errstate(over="ignore"):
        return np.asarray(y, F32).astype(np.float16).astype(F32)


def expected(g, y, algo, max_iter, layer_rows=0, llr_scale=8.0, f16=False, scale=0.0, offset=0.0, code=None):
    """g: oracle.Graph.  algo in {"ms", "layered", "layered_host", "ms_fused"}; f16 / scale / offset: flooding "ms" only
    (code: the ms_correction_ref.Code of the same matrix, needed with scale / offset).
    Returns dict(out, iters, hard uint8 [frames, N], post, ext float32 [frames, N], undefined bool [frames],
    filled int32 [frames]: how many of the per-round runs supplied the frame's row -- exactly one each)."""
    y = np.ascontiguousarray(y, F32).reshape(-1, g.N)
    frames = y.shape[0]
    corrected = scale != 0.0 or offset != 0.0
    assert algo == "ms" or not (f16 or corrected)
    if corrected:
        base = MC.flood_ms(code, y, max_iter, scale, offset, f16)
        undefined = np.zeros(frames, bool)
    else:
        base = oracle.decode(g, y, algo, max_iter=max_iter, llr_scale=llr_scale, layer_rows=layer_rows, msg_f16=f16)
        undefined = np.asarray(base.get("undefined", np.zeros(frames, np.uint8))).astype(bool)
    iters = np.asarray(base["iters"], np.int32)
    yd = f16_round(y) if f16 else y
    post = np.full((frames, g.N), np.nan, F32)
    filled = np.zeros(frames, np.int32)
    for i in np.unique(iters):
        sel = iters == i                # frames are independent: the run with tap_iter = i decodes these frames alone
        if corrected:
            run = MC.flood_ms(code, y[sel], max_iter, scale, offset, f16, tap_iter=int(i))
            r = run["r_tap"]
            rx = np.concatenate([r, np.full((r.shape[0], 1), -0.0, F32)], axis=1)        # x + (-0.0) == x, bit for bit
            p = yd[sel].copy()
            with np.errstate(invalid="ignore", over="ignore"):
                for k in range(code.col_edges.shape[1]):
                    p = (p + rx[:, code.col_edges[:, k]]).astype(F32)
        else:
            run = oracle.decode(g, y[sel], algo, max_iter=max_iter, llr_scale=llr_scale, layer_rows=layer_rows, tap_iter=int(i),
                                msg_f16=f16)
            p = run["taps"]["post"]
        assert (np.asarray(run["iters"]) == i).all() and np.array_equal(run["hard"], np.asarray(base["hard"])[sel])
        post[sel] = p
        filled[sel] += 1
    with np.errstate(invalid="ignore", over="ignore"):
        ext = (post - yd).astype(F32)
    res = dict(out=np.asarray(base["out"], np.uint8), iters=iters, hard=np.asarray(base["hard"], np.uint8), post=post, ext=ext,
               undefined=undefined, filled=filled)
    for v in res.values():
        v.setflags(write=False)
    return res


def bits(a):
    """The uint32 bit patterns of a float32 array."""
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_same_bits(got, want, keep=None, what=""):
    """0 ulp, the sign of zeros included; keep: bool [frames] of the rows that are compared (default: all)."""
    got, want = np.asarray(got, F32).reshape(want.shape), np.asarray(want, F32)
    if keep is not None:
        got, want = got[keep], want[keep]
    bad = np.nonzero(bits(got) != bits(want))
    assert bad[0].size == 0, "%s: %d of %d soft values differ from the oracle, first at row %d column %d: %r != %r" % (
        what, bad[0].size, want.size, bad[0][0], bad[1][0], got[bad[0][0], bad[1][0]], want[bad[0][0], bad[1][0]])


def sign_disagreements(post, hard):
    """Number of finite, non-zero posteriors whose sign is not the output bit (positive <-> 0)."""
    post = np.asarray(post, F32)
    hard = np.asarray(hard).reshape(post.shape)
    ok = np.isfinite(post) & (post != 0)
    return int(np.count_nonzero(ok & ((post < 0) != (hard != 0))))
