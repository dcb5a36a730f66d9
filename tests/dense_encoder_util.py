"""Helpers of the dense-encoder tests: GF(2) rank / pivot selection by a plain numpy elimination (never the code under
test), the two seeded test matrices of unstructured codes, the swapped 802.16e matrix, and the checks of a codeword."""
import numpy as np

from myldpccppapi_amd import codes


def dense(rows, cols, M, N):
    H = np.zeros((M, N), np.uint8)
    H[np.asarray(rows), np.asarray(cols)] = 1
    return H


def pivots(A, order):
    """Columns of A, visited in `order`, that are independent over GF(2) of the ones taken before them."""
    A = A.copy().astype(np.uint8)
    M = A.shape[0]
    used = np.zeros(M, bool)
    out = []
    for c in order:
        hit = np.nonzero((A[:, c] != 0) & ~used)[0]
        if hit.size == 0:
            continue
        p = hit[0]
        used[p] = True
        others = np.nonzero(A[:, c])[0]
        others = others[others != p]
        A[others] ^= A[p]
        out.append(int(c))
    return out


def rank(A):
    return len(pivots(A, range(A.shape[1])))


def systematic_order(H):
    """(perm, rank) by the rule of include/ldpc_hip.h: pivots from column N-1 down, non-pivots then pivots, ascending."""
    N = H.shape[1]
    piv = sorted(pivots(H, range(N - 1, -1, -1)))
    rest = sorted(set(range(N)) - set(piv))
    return np.array(rest + piv, np.int32), len(piv)


def matrix_r():
    """R: 100 x 200, three ones per column in rows drawn column by column from default_rng(1)."""
    rng = np.random.default_rng(1)
    rows, cols = [], []
    for c in range(200):
        for r in rng.choice(100, 3, replace=False):
            rows.append(int(r))
            cols.append(c)
    r, c = codes.row_major(rows, cols)
    return r, c, 100, 200


def matrix_g():
    """G: Gallager (3, 6), N = 204, three bands of 34 rows; band 0 in the identity order, bands 1 and 2 in
    default_rng(1).permutation(204) each, in turn.  Row b * 34 + i holds the six columns order_b[6 i .. 6 i + 6)."""
    rng = np.random.default_rng(1)
    rows, cols = [], []
    for b in range(3):
        order = np.arange(204) if b == 0 else rng.permutation(204)
        for i in range(34):
            for c in order[6 * i:6 * i + 6]:
                rows.append(b * 34 + i)
                cols.append(int(c))
    r, c = codes.row_major(rows, cols)
    return r, c, 102, 204


def matrix_w648s():
    """802.16e rate 1/2 (648, 324) with parity columns K + 3 and K + 2 z + 5 swapped: no circulants any more."""
    K, M, z = codes.wimax_dims(codes.RATE_1_2, 648)
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 648)
    c2 = cols.astype(np.int64).copy()
    p, q = K + 3, K + 2 * z + 5
    c2[cols == p], c2[cols == q] = q, p
    r2, c2 = codes.row_major(rows, c2)
    return r2, c2, M, 648


def t_bits(t_words, M):
    """uint64 [rows, ceil(M / 64)] -> uint8 [rows, M]; asserts that the tail bits are zero."""
    t_words = np.ascontiguousarray(t_words, np.uint64)
    bits = np.unpackbits(t_words.view(np.uint8), axis=1, bitorder="little")
    assert not bits[:, M:].any(), "tail bits of T are set"
    return bits[:, :M]


def syndrome_weight_dense(H, bits):
    """Unsatisfied checks over all frames: bits uint8 [frames, N]."""
    return int(((bits.astype(np.int64) @ H.T.astype(np.int64)) & 1).sum())
