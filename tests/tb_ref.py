"""Independent numpy reference of the transport-block stage (include/ldpc_hip.h, "transport block"): the CRC of TS 38.212
section 5.1 by long division, and attach / check as literal loops over the bits of a transport block -- vectorised over
the transport blocks of a batch only.  Never calls the library under test.

Bit order everywhere: LSB first, bit i of a row is bit i % 8 of byte i / 8."""
import numpy as np

#: kind -> (generator with its top bit, degree); 24 is CRC24A, 25 is CRC24B
POLY = {16: (0x11021, 16), 24: (0x1864CFB, 24), 25: (0x1800063, 24)}


def bits_of(rows):
    """uint8 [n, bytes] -> uint8 [n, 8 bytes] of 0/1."""
    return np.unpackbits(np.ascontiguousarray(rows, np.uint8), axis=-1, bitorder="little")


def bytes_of(bits):
    return np.packbits(np.ascontiguousarray(bits, np.uint8), axis=-1, bitorder="little")


def parity(kind, bits):
    """bits uint8 [n, m] (a_0 first) -> parity uint8 [n, L], p_0 first: the remainder of a(x) x^L by long division."""
    g, L = POLY[kind]
    gbits = np.array([(g >> (L - k)) & 1 for k in range(L + 1)], np.uint8)       # x^L first
    bits = np.atleast_2d(np.asarray(bits, np.uint8))
    n, m = bits.shape
    reg = np.concatenate([bits, np.zeros((n, L), np.uint8)], axis=1)
    for i in range(m):
        rows = np.nonzero(reg[:, i])[0]
        if rows.size:
            reg[rows, i:i + L + 1] ^= gbits
    return reg[:, m:]


def crc(kind, bits):
    """The CRC of one row of bits as an integer, p_0 its top bit."""
    p = parity(kind, np.asarray(bits, np.uint8).reshape(1, -1))[0]
    v = 0
    for b in p:
        v = (v << 1) | int(b)
    return v


class Spec:
    def __init__(self, A, K, C=None, tb_crc=None, cb_crc=None):
        """None: the rule of TS 38.212 section 5.2.2 with K in place of Kcb."""
        rule_tb = 24 if A > 3824 else 16
        B = A + rule_tb
        if B <= K:
            rule_C, rule_cb = 1, 0
        else:
            rule_C, rule_cb = -(-B // (K - 24)), 24
        self.A, self.K = A, K
        self.tb_crc = rule_tb if tb_crc is None else tb_crc
        self.C = rule_C if C is None else C
        self.cb_crc = rule_cb if cb_crc is None else cb_crc
        self.B = self.A + self.tb_crc
        self.valid = self.B % self.C == 0
        self.S = self.B // self.C
        self.Kp = self.S + self.cb_crc
        self.valid = self.valid and self.Kp <= K

    def layout(self):
        return (self.B, self.S, self.Kp, self.Kp, self.K, self.C)


def attach(spec, payload):
    """payload uint8 [tbs, A/8] -> frames uint8 [tbs * C, K/8]."""
    a = bits_of(np.asarray(payload, np.uint8).reshape(-1, spec.A // 8))
    tbs = a.shape[0]
    stream = np.zeros((tbs, spec.B), np.uint8)
    for i in range(spec.A):
        stream[:, i] = a[:, i]
    if spec.tb_crc:
        p = parity(spec.tb_crc, a)
        for i in range(spec.tb_crc):
            stream[:, spec.A + i] = p[:, i]
    frames = np.zeros((tbs, spec.C, spec.K), np.uint8)
    for c in range(spec.C):
        for i in range(spec.S):
            frames[:, c, i] = stream[:, c * spec.S + i]
        if spec.cb_crc:
            p = parity(25, frames[:, c, :spec.S])
            for i in range(24):
                frames[:, c, spec.S + i] = p[:, i]
    return bytes_of(frames.reshape(tbs * spec.C, spec.K))


def check(spec, dec):
    """dec uint8 [tbs * C, K/8] -> (payload uint8 [tbs, A/8], cb_ok uint8 [tbs * C], tb_ok uint8 [tbs])."""
    f = bits_of(np.asarray(dec, np.uint8).reshape(-1, spec.K // 8)).reshape(-1, spec.C, spec.K)
    tbs = f.shape[0]
    cb_ok = np.ones((tbs, spec.C), np.uint8)
    stream = np.zeros((tbs, spec.B), np.uint8)
    for c in range(spec.C):
        if spec.cb_crc:
            cb_ok[:, c] = ~parity(25, f[:, c, :spec.Kp]).any(axis=1)
        for i in range(spec.S):
            stream[:, c * spec.S + i] = f[:, c, i]
    tb_ok = cb_ok.all(axis=1)
    if spec.tb_crc:
        tb_ok = tb_ok & ~parity(spec.tb_crc, stream).any(axis=1)
    return bytes_of(stream[:, :spec.A]), cb_ok.reshape(-1), tb_ok.astype(np.uint8)


def tally(tb_ok, payload, ref):
    """(failed, wrong, undetected, parity_only)."""
    tb_ok = np.asarray(tb_ok).astype(bool)
    payload = np.asarray(payload).reshape(tb_ok.size, -1)
    differs = (payload != (np.asarray(ref).reshape(tb_ok.size, -1) if ref is not None else 0)).any(axis=1)
    return (int((~tb_ok).sum()), int(differs.sum()), int((differs & tb_ok).sum()), int((~differs & ~tb_ok).sum()))
