"""numpy restatement of the modem contract of include/ldpc_hip.h, for the tests only: float32 element-wise operations,
nothing from the library under test.  The noise is the double-precision normal stream of csrc/ldpc_channel.h compiled
for the host (tests/util.host_channel_lib), combined as np.float32(np.float64(x) + np.float64(np.float32(sd)) * z)."""
import ctypes

import numpy as np

NORM = {2: 2, 4: 10, 6: 42, 8: 170}


def default_interleave(Qm):
    return Qm >= 2


def symbol_floats(Qm, E):
    assert E % Qm == 0
    return E if Qm == 1 else 2 * (E // Qm)


def index(Qm, interleave, E):
    """int32 [E]: entry j * Qm + i = tx bit behind bit i of symbol j."""
    S = E // Qm
    out = np.empty(E, np.int32)
    for j in range(S):
        for i in range(Qm):
            out[j * Qm + i] = i * S + j if (interleave and Qm > 1) else j * Qm + i
    return out


def scale(Qm):
    return np.float32(1.0) if Qm == 1 else np.float32(1.0 / np.sqrt(np.float64(NORM[Qm])))


def amp(c):
    """Integer level of axis bits c[0], c[1], ... (arrays of 0/1, last axis = bit): the recurrence of the header."""
    c = np.asarray(c, np.int64)
    k = c.shape[-1]
    if k == 0:
        return np.zeros(c.shape[:-1], np.int64)
    return (1 - 2 * c[..., 0]) * (2 ** (k - 1) - amp(c[..., 1:]))


def axis_levels(Qm):
    """(labels int [2^m, m] with c0 first, float32 levels [2^m]) of one axis."""
    m = Qm // 2
    lab = np.array([[(v >> (m - 1 - k)) & 1 for k in range(m)] for v in range(1 << m)], np.int64).reshape(1 << m, m)
    return lab, amp(lab).astype(np.float32) * scale(Qm)


def points(Qm):
    """float32 [2^Qm, 2]: label v = sum b_i 2^(Qm-1-i)."""
    if Qm == 1:
        return np.array([[1, 0], [-1, 0]], np.float32)
    b = np.array([[(v >> (Qm - 1 - i)) & 1 for i in range(Qm)] for v in range(1 << Qm)], np.int64)
    out = np.empty((1 << Qm, 2), np.float32)
    out[:, 0] = amp(b[:, 0::2]).astype(np.float32) * scale(Qm)
    out[:, 1] = amp(b[:, 1::2]).astype(np.float32) * scale(Qm)
    return out


def clean_symbols(Qm, interleave, bits):
    """bits uint8 [frames, E] -> noise-free float32 [frames, symbol_floats]."""
    bits = np.asarray(bits, np.uint8) & 1
    frames, E = bits.shape
    if Qm == 1:
        return (np.float32(1.0) - np.float32(2.0) * bits.astype(np.float32)).astype(np.float32)
    S = E // Qm
    b = bits[:, index(Qm, interleave, E)].reshape(frames, S, Qm)          # [f, j, i]
    x = np.empty((frames, S, 2), np.float32)
    x[:, :, 0] = amp(b[:, :, 0::2]).astype(np.float32) * scale(Qm)
    x[:, :, 1] = amp(b[:, :, 1::2]).astype(np.float32) * scale(Qm)
    return x.reshape(frames, 2 * S)


def normals(chlib, seed, frame, count):
    """float64 [count]: z(seed, frame, n) for n < count."""
    groups = (count + 3) // 4
    z = np.empty(4 * groups, np.float64)
    chlib.normals(ctypes.c_uint64(seed), ctypes.c_uint64(frame), groups, z.ctypes.data)
    return z[:count]


def transmit(Qm, interleave, bits, sd, seed, first_frame, chlib):
    x = clean_symbols(Qm, interleave, bits)
    if sd == 0:
        return x
    out = np.empty_like(x)
    for f in range(x.shape[0]):
        z = normals(chlib, seed, first_frame + f, x.shape[1])
        out[f] = (np.float64(x[f]) + np.float64(np.float32(sd)) * z).astype(np.float32)
    return out


def demap(Qm, interleave, sym, E):
    """sym float32 [frames, symbol_floats] -> float32 [frames, E]: y = (D1 - D0) * 0.25f per bit, de-interleaved."""
    sym = np.asarray(sym, np.float32)
    frames = sym.shape[0]
    if Qm == 1:
        return sym.reshape(frames, E).copy()
    S, m = E // Qm, Qm // 2
    lab, lev = axis_levels(Qm)
    r = sym.reshape(frames, S, 2)
    t = r[..., None] - lev                                                 # [f, j, axis, level], float32
    d = t * t
    assert d.dtype == np.float32
    y = np.empty((frames, S, Qm), np.float32)
    for k in range(m):
        d0 = d[..., lab[:, k] == 0].min(axis=-1)
        d1 = d[..., lab[:, k] == 1].min(axis=-1)
        v = (d1 - d0) * np.float32(0.25)                                   # [f, j, axis]
        y[:, :, 2 * k] = v[:, :, 0]
        y[:, :, 2 * k + 1] = v[:, :, 1]
    out = np.empty((frames, E), np.float32)
    out[:, index(Qm, interleave, E)] = y.reshape(frames, E)
    return out
