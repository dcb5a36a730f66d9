"""The outer code of include/ldpc_hip.h ("outer code") restated in numpy and plain integers, from the definition and not
from the library: the field tables, the cyclotomic cosets and the generator, long-division encoding, syndromes,
Berlekamp-Massey with a Chien search and its range and count checks, the tally.  Polynomials over GF(2) are Python
integers, bit i = coefficient of x^i.  For batches the two linear maps (message -> parity, word -> syndromes) are also
available as bit matrices built row by row from the same definitions; tests/test_bch_cpu.py holds them to the bitwise
forms."""
import functools

import numpy as np

DEFAULT = {14: 0x402B, 16: 0x1002D}


def bits_of(rows):
    """uint8 [..., B] -> uint8 [..., 8 B] of 0/1, bit i of a row = bit i % 8 of byte i / 8."""
    return np.unpackbits(np.asarray(rows, np.uint8), axis=-1, bitorder="little")


def bytes_of(bits):
    return np.packbits(np.asarray(bits, np.uint8), axis=-1, bitorder="little")


def order_of_x(m, prim):
    """The multiplicative order of x modulo prim (0 if x never returns to 1 within 2^m - 1 steps)."""
    v = 1
    for i in range(1, (1 << m)):
        v <<= 1
        if v >> m:
            v ^= prim
        if v == 1:
            return i
    return 0


def is_primitive(m, prim):
    return (prim >> m) == 1 and order_of_x(m, prim) == (1 << m) - 1


class Field:
    def __init__(self, m, prim):
        assert is_primitive(m, prim)
        self.m, self.prim, self.N = m, prim, (1 << m) - 1
        exp = np.zeros(2 * self.N, np.int64)
        v = 1
        for i in range(self.N):
            exp[i] = v
            v <<= 1
            if v >> m:
                v ^= prim
        exp[self.N:] = exp[:self.N]
        self.exp = exp
        self.log = np.zeros(1 << m, np.int64)
        self.log[exp[:self.N]] = np.arange(self.N)

    def mul(self, a, b):
        return 0 if a == 0 or b == 0 else int(self.exp[self.log[a] + self.log[b]])

    def inv(self, a):
        assert a != 0
        return int(self.exp[(self.N - self.log[a]) % self.N])

    def alpha(self, e):
        return int(self.exp[e % self.N])


@functools.lru_cache(maxsize=None)
def field(m, prim):
    return Field(m, prim)


def cosets(m, t):
    """([coset of the first new j, ...], cls) with cls[j - 1] = index of the coset that holds j, j = 1 .. 2t."""
    N = (1 << m) - 1
    found, cls = [], []
    for j in range(1, 2 * t + 1):
        c, e = [], j
        while e not in c:
            c.append(e)
            e = (2 * e) % N
        key = min(c)
        for i, other in enumerate(found):
            if min(other) == key:
                cls.append(i)
                break
        else:
            cls.append(len(found))
            found.append(c)
    return found, cls


def min_poly(F, coset):
    """prod (x + alpha^e) over the coset; its coefficients lie in GF(2)."""
    co = [1]
    for e in coset:
        beta = F.alpha(e)
        co = [(co[k - 1] if k else 0) ^ (F.mul(co[k], beta) if k < len(co) else 0) for k in range(len(co) + 1)]
    assert all(c in (0, 1) for c in co)
    return sum(c << k for k, c in enumerate(co))


def poly_mul(a, b):
    out = 0
    while b:
        if b & 1:
            out ^= a
        a <<= 1
        b >>= 1
    return out


def poly_mod(a, q):
    d = q.bit_length() - 1
    while a and a.bit_length() - 1 >= d:
        a ^= q << (a.bit_length() - 1 - d)
    return a


@functools.lru_cache(maxsize=None)
def generator(m, prim, t):
    """(g, [minimal polynomials])."""
    F = field(m, prim)
    polys = [min_poly(F, c) for c in cosets(m, t)[0]]
    g = 1
    for p in polys:
        g = poly_mul(g, p)
    return g, polys


def tally(status, payload, ref):
    status = np.asarray(status)
    payload = np.asarray(payload)
    differs = (payload != (0 if ref is None else np.asarray(ref))).reshape(len(status), -1).any(axis=1)
    pos = status[status > 0]
    return (int((status < 0).sum()), int(differs.sum()), int((differs & (status >= 0)).sum()), int(len(pos)), int(pos.sum()),
            int((~differs & (status < 0)).sum()))


class Code:
    def __init__(self, n, t, row_bytes=None, m=None, prim=None):
        if m is None:
            m = 14 if n <= 16383 else 16
        if prim is None:
            prim = DEFAULT[m]
        self.n, self.t, self.m, self.prim = n, t, m, prim
        self.row_bytes = n // 8 if row_bytes is None else row_bytes
        self.F = field(m, prim)
        self.g, self.polys = generator(m, prim, t)
        self.r = self.g.bit_length() - 1
        self.k = n - self.r
        self.valid = n % 8 == 0 and 0 < n <= self.F.N and self.k >= 8 and self.k % 8 == 0 and 8 * self.row_bytes >= n

    # ---- bitwise forms: the definition ------------------------------------------------------------------------------
    def parity_long_division(self, a):
        """bits a_0 .. a_(k-1) -> bits p_0 .. p_(r-1): x^r a(x) mod g, one bit at a time through an r-bit register."""
        reg, r, low = 0, self.r, self.g ^ (1 << self.r)
        for bit in a:
            fb = ((reg >> (r - 1)) & 1) ^ int(bit)
            reg = (reg << 1) & ((1 << r) - 1)
            if fb:
                reg ^= low
        return np.array([(reg >> (r - 1 - j)) & 1 for j in range(r)], np.uint8)

    def syndromes_direct(self, v):
        """bits v_0 .. v_(n-1) -> [S_1 .. S_2t], S_j = sum v_i alpha^(j (n - 1 - i))."""
        F, out = self.F, []
        idx = np.nonzero(np.asarray(v)[:self.n])[0]
        for j in range(1, 2 * self.t + 1):
            s = 0
            for i in idx:
                s ^= F.alpha(j * (self.n - 1 - int(i)))
            out.append(s)
        return out

    # ---- the same two maps as bit matrices, for batches ------------------------------------------------------------------
    @functools.cached_property
    def parity_matrix(self):
        """float32 [k, r]: row i = the parity bits of the unit message e_i, that is x^(r + k - 1 - i) mod g."""
        rows, v, r = [], poly_mod(1 << self.r, self.g), self.r
        for _ in range(self.k):
            rows.append(v)
            v <<= 1
            if v >> r:
                v ^= self.g
        nb = (r + 7) // 8
        raw = np.frombuffer(b"".join(x.to_bytes(nb, "little") for x in rows[::-1]), np.uint8).reshape(self.k, nb)
        coeff = np.unpackbits(raw, axis=1, bitorder="little")[:, :r]          # column c = coefficient of x^c
        return coeff[:, ::-1].astype(np.float32)                              # column j = p_j = coefficient of x^(r-1-j)

    @functools.cached_property
    def syndrome_matrix(self):
        """float32 [n, t m]: row i = the bits of alpha^(j (n - 1 - i)) for the odd j = 1, 3 .. 2t - 1."""
        F = self.F
        e = self.n - 1 - np.arange(self.n, dtype=np.int64)
        cols = []
        for j in range(1, 2 * self.t, 2):
            val = F.exp[(j * e) % F.N]
            cols.append(((val[:, None] >> np.arange(self.m)) & 1))
        return np.concatenate(cols, axis=1).astype(np.float32)

    def parity(self, abits):
        abits = np.asarray(abits, np.uint8).reshape(-1, self.k)
        return (np.rint(abits.astype(np.float32) @ self.parity_matrix).astype(np.int64) & 1).astype(np.uint8)

    def syndromes(self, vbits):
        """uint8 [F, >= n] -> int64 [F, 2t]; the even ones by S_2j = S_j^2, which holds for every binary word."""
        F = self.F
        vbits = np.asarray(vbits, np.uint8).reshape(len(vbits), -1)[:, :self.n]
        sbits = np.rint(vbits.astype(np.float32) @ self.syndrome_matrix).astype(np.int64) & 1
        odd = (sbits.reshape(len(vbits), self.t, self.m) << np.arange(self.m)).sum(axis=2)
        S = np.zeros((len(vbits), 2 * self.t + 1), np.int64)
        S[:, 1::2] = odd
        for j in range(2, 2 * self.t + 1, 2):
            h = S[:, j // 2]
            S[:, j] = np.where(h == 0, 0, F.exp[(2 * F.log[h]) % F.N])
        return S[:, 1:]

    # ---- encode and decode -----------------------------------------------------------------------------------------------
    def encode(self, payload):
        payload = np.asarray(payload, np.uint8).reshape(-1, self.k // 8)
        a = bits_of(payload)
        rows = np.zeros((len(payload), 8 * self.row_bytes), np.uint8)
        rows[:, :self.k] = a
        rows[:, self.k:self.n] = self.parity(a)
        return bytes_of(rows)

    def locate(self, S):
        """S_1 .. S_2t (not all zero) -> sorted error positions, or None: Berlekamp-Massey, then the roots of the
        locator among the positions [0, n) only; fails if deg sigma > t, if the number of such roots differs from
        deg sigma, or if flipping them would not cancel every syndrome."""
        F, t, n = self.F, self.t, self.n
        C, B, L, shift, b = [1], [1], 0, 1, 1
        for i in range(2 * t):
            d = S[i]
            for q in range(1, L + 1):
                if q < len(C):
                    d ^= F.mul(C[q], S[i - q])
            if d == 0:
                shift += 1
                continue
            coef = F.mul(d, F.inv(b))
            T = list(C)
            C = C + [0] * max(0, len(B) + shift - len(C))
            for q, v in enumerate(B):
                C[q + shift] ^= F.mul(coef, v)
            if 2 * L <= i:
                L, B, b, shift = i + 1 - L, T, d, 1
            else:
                shift += 1
        while len(C) > 1 and C[-1] == 0:
            C.pop()
        if L > t or len(C) - 1 != L:
            return None
        # sigma(x) = prod (1 + X x): position i is in error iff sigma(alpha^-(n - 1 - i)) = 0
        e = (-(n - 1 - np.arange(n, dtype=np.int64))) % F.N
        acc = np.full(n, C[0], np.int64)
        for q in range(1, len(C)):
            if C[q]:
                acc ^= F.exp[(F.log[C[q]] + q * e) % F.N]
        pos = np.nonzero(acc == 0)[0]
        if len(pos) != L:
            return None
        for j in range(1, 2 * t + 1):
            s = 0
            for i in pos:
                s ^= F.alpha(j * (n - 1 - int(i)))
            if s != S[j - 1]:
                return None
        return [int(i) for i in pos]

    def decode_bits(self, vbits):
        """uint8 [F, >= n] -> (corrected bits uint8 [F, n], status int32 [F])."""
        v = np.array(np.asarray(vbits, np.uint8).reshape(len(vbits), -1)[:, :self.n])
        S = self.syndromes(v)
        status = np.zeros(len(v), np.int32)
        for f in np.nonzero(S.any(axis=1))[0]:
            pos = self.locate([int(s) for s in S[f]])
            if pos is None:
                status[f] = -1
            else:
                v[f, pos] ^= 1
                status[f] = len(pos)
        return v, status

    def decode(self, rows):
        """uint8 [F, row_bytes] -> (payload uint8 [F, k / 8], status)."""
        rows = np.asarray(rows, np.uint8).reshape(-1, self.row_bytes)
        v, status = self.decode_bits(bits_of(rows))
        return bytes_of(v[:, :self.k]), status
