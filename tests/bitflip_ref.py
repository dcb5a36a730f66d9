"""Hard-decision parallel bit flipping (algo = bitflip, include/ldpc_hip.h: LDPC_ALGO_BITFLIP) restated in integers with
numpy, from the header's text alone.

    r_n = (y_n < 0)                      NaN and -0 read 0
    x = r
    round i = 1 .. max_iter:
        s_m = XOR of x over row m
        a frame with s == 0 is done: frozen, iters = i - 1
        u_n = sum of s over the rows of column n,  E_n = u_n + (x_n != r_n)
        hit_n = (E_n >= T(d_n, i))
        a frame with a hit flips its hit columns; a frame without flips the columns whose E is the frame's largest,
        if that is >= 2                          (every flip of a round from the same s)
    frames never done: iters = max_iter

    T(d, i) = max(floor((d + 1) / 2) + 1, d + 1 - off(i))
    off(i)  = i - 1                              with bf_threshold all zero (the default)
            = bf_threshold[min(i - 1, 15)]       otherwise

Three other schedules, for the comparison the CPU test prints: "threshold" (the hits alone, no fall-back), "majority" (the
hits alone with T = floor((d + 1) / 2) + 1 from round 1, which is bf_threshold = [62] * 16) and "max" (only the columns
whose E is the frame's largest, if that is >= 2, in every round)."""
import numpy as np

MAX_DEGREE = 62
THRESHOLDS = 16


def offset(i, bf_threshold=None):
    """off(i) of round i >= 1."""
    if bf_threshold is None or not any(int(t) for t in bf_threshold):
        return i - 1
    assert len(bf_threshold) == THRESHOLDS and all(0 <= int(t) <= MAX_DEGREE for t in bf_threshold)
    return int(bf_threshold[min(i - 1, THRESHOLDS - 1)])


def threshold(d, i, bf_threshold=None):
    """T(d, i): votes of d + 1 (the d checks and the received bit) a column of degree d needs in round i to flip."""
    return max((d + 1) // 2 + 1, d + 1 - offset(i, bf_threshold))


class Code:
    """The edges of H in row-major order (edge id = rank), and the same edges sorted by column."""

    def __init__(self, rows, cols, M, N):
        self.rows, self.cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        self.M, self.N = int(M), int(N)
        self.row_deg = np.bincount(self.rows, minlength=self.M)
        self.col_deg = np.bincount(self.cols, minlength=self.N)
        assert self.col_deg.max() <= MAX_DEGREE
        order = np.argsort(self.cols, kind="stable")
        self.rows_by_col = self.rows[order]
        # reduceat wants a start inside the array for every segment; empty segments are zeroed afterwards
        self.row_start = np.minimum(np.concatenate(([0], np.cumsum(self.row_deg)[:-1])), self.rows.size - 1)
        self.col_start = np.minimum(np.concatenate(([0], np.cumsum(self.col_deg)[:-1])), self.rows.size - 1)

    # bits are held column-major here, x[n, frame], so that a gather copies whole rows

    def syndrome(self, x):
        """x uint8 [N, frames] -> uint8 [M, frames]"""
        s = np.bitwise_xor.reduceat(x[self.cols], self.row_start, axis=0)
        s[self.row_deg == 0] = 0
        return s

    def unsatisfied(self, s):
        """s uint8 [M, frames] -> int8 [N, frames]: u_n <= 62"""
        u = np.add.reduceat(s[self.rows_by_col], self.col_start, axis=0, dtype=np.int8)
        u[self.col_deg == 0] = 0
        return u


def received(y):
    """r = (y < 0): NaN compares false, -0.0 is not below 0."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(y, np.float32) < 0).astype(np.uint8)


SCHEDULES = ("default", "threshold", "majority", "max")


def decode(code, y, max_iter, bf_threshold=None, schedule="default"):
    """dict(hard uint8 [frames, N], iters int32 [frames], done bool [frames], syndrome uint8 [frames, M] = s of the last
    round run (all zero with max_iter = 0)).  y: float [frames, N], the values the decoder reads."""
    y = np.asarray(y, np.float32).reshape(-1, code.N)
    frames = y.shape[0]
    r = np.ascontiguousarray(received(y).T)
    x = r.copy()
    iters = np.full(frames, max_iter, np.int32)
    done = np.zeros(frames, bool)
    s = np.zeros((code.M, frames), np.uint8)
    for i in range(1, max_iter + 1):
        run = np.nonzero(~done)[0]                # a done frame has s = 0 and flips nothing: only the others are worked on
        if run.size == 0:
            break
        xr, rr = x[:, run], r[:, run]
        sr = code.syndrome(xr)
        clean = ~sr.any(axis=0)
        s[:, run] = sr
        iters[run[clean]] = i - 1
        done[run[clean]] = True
        E = code.unsatisfied(sr) + (xr != rr)
        top = (E == E.max(axis=0, keepdims=True)) & (E >= 2)
        table = [MAX_DEGREE] * THRESHOLDS if schedule == "majority" else bf_threshold
        T = np.maximum((code.col_deg + 1) // 2 + 1, code.col_deg + 1 - offset(i, table))      # threshold(d, i, table), all columns
        hit = E >= T[:, None]
        if schedule == "max":
            flip = top
        elif schedule == "default":
            flip = np.where(hit.any(axis=0, keepdims=True), hit, top)
        else:
            flip = hit
        flip = flip & ~clean[None, :]
        x[:, run] = xr ^ flip.astype(np.uint8)
    return dict(hard=np.ascontiguousarray(x.T), iters=iters, done=done, syndrome=np.ascontiguousarray(s.T))


def pack_bytes(hard, K):
    """LDPC_PACK_BYTES: the K / 8 whole bytes of frame b, LSB first, at (b * K) / 8; (frames - 1) * K / 8 + K / 8 bytes in
    all, the others 0 (K = 4: no frame has a whole byte)."""
    frames, kb = hard.shape[0], K // 8
    out = np.zeros((frames - 1) * K // 8 + kb if frames else 0, np.uint8)
    rows = np.packbits(hard[:, :kb * 8], axis=1, bitorder="little")
    for b in range(frames):
        out[b * K // 8:b * K // 8 + kb] = rows[b]
    return out


def pack_bits(hard, K):
    """LDPC_PACK_BITS: bit i of frame b at bit b * K + i."""
    return np.packbits(np.ascontiguousarray(hard[:, :K]).reshape(-1), bitorder="little")


def bsc(frames, N, crossover, seed, code_bits=None):
    """+-1 channel values of `code_bits` (default: the all-zero codeword) through a binary symmetric channel: float32
    [frames, N], +1 <-> bit 0."""
    rng = np.random.default_rng(seed)
    flips = (rng.random((frames, N)) < crossover).astype(np.uint8)
    bits = flips if code_bits is None else (np.asarray(code_bits, np.uint8).reshape(frames, N) ^ flips)
    return (1.0 - 2.0 * bits).astype(np.float32)


def schedule_table(code_of, sizes=((576, 288), (2304, 1152)), crossovers=(0.01, 0.02, 0.03), frames=512, max_iter=30, seed=11):
    """Frame errors of the schedules on the all-zero codeword: rows of (N, K, p, dirty frames at the input, then the frames
    left dirty by each of SCHEDULES).  code_of(N) -> Code."""
    out = []
    for N, K in sizes:
        code = code_of(N)
        for p in crossovers:
            y = bsc(frames, N, p, seed)
            row = [N, K, p, int(received(y).any(axis=1).sum())]
            for schedule in SCHEDULES:
                row.append(int(decode(code, y, max_iter, schedule=schedule)["hard"].any(axis=1).sum()))
            out.append(tuple(row))
    return out
