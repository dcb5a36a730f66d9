"""The ordered-statistics rule of include/ldpc_hip.h ("ordered-statistics post-processing") restated in numpy -- nothing
of the library is used here.  H is a dense uint8 [M, N] matrix; a frame is a float32 row of posteriors, positive <-> 0.

frame(H, p, scale) gives everything about one frame at both orders (the candidates are written out as codewords, one
column per free position); run(H, soft, order, scale, K) gives the four outputs of ldpc_osd_device."""
import numpy as np

F32 = np.float32
CAP = 65535


def dense(rows, cols, M, N):
    H = np.zeros((M, N), np.uint8)
    H[np.asarray(rows), np.asarray(cols)] = 1
    return H


def hard_bits(p):
    with np.errstate(invalid="ignore"):
        return (np.asarray(p, F32) < 0).astype(np.uint8)


def weights(p, scale):
    """int64 [..]: floorf(fminf(fabsf(p) * scale, 65535)), one fp32 multiply; NaN -> 0"""
    p = np.asarray(p, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.abs(p) * F32(scale)).astype(F32)
        w = np.floor(np.fmin(t, F32(CAP)))
    return np.where(np.isnan(p), 0, w).astype(np.int64)


def order_of(w):
    """positions, the least reliable first, ties to the index"""
    return np.lexsort((np.arange(w.size), w))


def syndrome(H, bits):
    return (H.astype(np.int64) @ np.asarray(bits, np.int64).T) & 1


def basis(H, perm):
    """(A, pivcol): H fully reduced on the pivot set the scan of `perm` finds; pivcol int [M], the pivot column of each
    row, -1 for a row that ended up zero"""
    A = H.copy()
    M = A.shape[0]
    pivcol = -np.ones(M, np.int64)
    left = M
    for c in perm:
        have = np.flatnonzero(A[:, c])
        free_rows = have[pivcol[have] < 0]
        if free_rows.size == 0:
            continue
        r = free_rows[0]
        others = have[have != r]
        A[others] ^= A[r]
        pivcol[r] = c
        left -= 1
        if left == 0:
            break
    return A, pivcol


def metric(w, c, h):
    return int(w[np.asarray(c) != np.asarray(h)].sum())


def frame(H, p, scale):
    """dict: h, w, clean, P (pivot positions in scan order), F (free positions ascending), c0, D0, and the order-1 choice
    c1, D1, flip (the flipped position or -1)"""
    p = np.asarray(p, F32)
    N = H.shape[1]
    h, w = hard_bits(p), weights(p, scale)
    res = dict(h=h, w=w, clean=not syndrome(H, h).any())
    if res["clean"]:
        return res
    perm = order_of(w)
    A, pivcol = basis(H, perm)
    used = np.flatnonzero(pivcol >= 0)
    P = pivcol[used]
    isP = np.zeros(N, bool)
    isP[P] = True
    Fp = np.flatnonzero(~isP)
    AF = A[used][:, Fp].astype(np.int64)               # pivot bit i = XOR of the free bits AF[i] selects
    c0 = h.copy()
    c0[P] = (AF @ h[Fp].astype(np.int64)) & 1
    D0 = metric(w, c0, h)
    rank_in_scan = np.empty(N, np.int64)
    rank_in_scan[perm] = np.arange(N)
    res.update(P=P[np.argsort(rank_in_scan[P])], F=Fp, c0=c0, D0=D0, c1=c0, D1=D0, flip=-1)
    # every single flip: column k of CP holds the pivot bits of the codeword that has h on F except at F[k]
    CP = c0[P][:, None].astype(np.int64) ^ AF
    D = w[Fp] + (w[P][:, None] * (CP ^ h[P][:, None])).sum(axis=0)
    if D.size:
        k = int(np.argmin(D))                          # the first minimum: the smallest position among equals
        if D[k] < D0:                                  # on a tie c0 wins
            c1 = h.copy()
            c1[Fp[k]] ^= 1
            c1[P] = CP[:, k]
            res.update(c1=c1.astype(np.uint8), D1=int(D[k]), flip=int(Fp[k]))
            assert metric(w, c1, h) == int(D[k])
    return res


def pack(code, K):
    """uint8 [frames, K/8]: the first K bits, LSB first"""
    return np.packbits(np.asarray(code, np.uint8)[:, :K], axis=1, bitorder="little")


def run(H, soft, order, scale, K=None):
    """dict(code uint8 [frames, N], status, metric int32 [frames], out uint8 [frames, K/8] when K % 8 == 0, flip int [frames])"""
    soft = np.asarray(soft, F32).reshape(-1, H.shape[1])
    frames = soft.shape[0]
    code = np.zeros((frames, H.shape[1]), np.uint8)
    status, met, flip = np.zeros(frames, np.int32), np.zeros(frames, np.int32), -np.ones(frames, np.int64)
    for f in range(frames):
        r = frame(H, soft[f], scale)
        if r["clean"]:
            code[f] = r["h"]
        elif order == 0 or r["flip"] < 0:
            code[f], status[f], met[f] = r["c0"], 1, r["D0"]
        else:
            code[f], status[f], met[f], flip[f] = r["c1"], 2, r["D1"], r["flip"]
    res = dict(code=code, status=status, metric=met, flip=flip)
    if K is not None and K % 8 == 0:
        res["out"] = pack(code, K)
    return res
