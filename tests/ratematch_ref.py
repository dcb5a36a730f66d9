"""numpy restatement of the rate-matching contract of include/ldpc_hip.h, for the tests only.

index() is the literal walk over the circular buffer (position by position, fillers skipped), NOT the closed form the
library uses; recover() sums in ascending e with float32, one addition at a time, as the contract prescribes."""
import numpy as np


class Spec:
    def __init__(self, N, punctured=0, filler=(0, 0), fill_llr=10.0, erasure_llr=0.0):
        self.N, self.P = int(N), int(punctured)
        self.lo, self.hi = (int(filler[0]), int(filler[1])) if filler[0] != filler[1] else (self.P, self.P)
        self.fill_llr, self.erasure_llr = np.float32(fill_llr), np.float32(erasure_llr)

    @property
    def Ncb(self):
        return self.N - self.P

    @property
    def L(self):
        return self.Ncb - (self.hi - self.lo)

    def kwargs(self):
        """The arguments of myldpccppapi_amd.RateMatcher for the same spec."""
        return dict(N=self.N, punctured=self.P, filler=(self.lo, self.hi), fill_llr=float(self.fill_llr),
                    erasure_llr=float(self.erasure_llr))


def index(spec, k0, E):
    """int32 [E]: walk the buffer (code bits P .. N-1) from position k0, wrap at Ncb, skip fillers, emit E bits."""
    out = np.empty(E, np.int32)
    pos, e = k0, 0
    while e < E:
        n = spec.P + pos
        if not (spec.lo <= n < spec.hi):
            out[e] = n
            e += 1
        pos += 1
        if pos == spec.Ncb:
            pos = 0
    return out


def match(spec, code_bits, k0, E):
    """code_bits: uint8 [frames, N] of 0/1 -> uint8 [frames, E]."""
    return np.ascontiguousarray(np.asarray(code_bits, np.uint8)[:, index(spec, k0, E)])


def erasure_values(N, erasure_llr):
    """float32 [N]: eps * (1 + n / N), every operation in float32."""
    n = np.arange(N, dtype=np.float32)              # exact up to 2^24
    return np.float32(erasure_llr) * (np.float32(1.0) + n / np.float32(N))


def recover(spec, rx, k0, E, soft=None):
    """rx: float32 [frames, E]; soft: float32 [frames, N] of earlier sums or None.  Returns (soft, y), new arrays."""
    rx = np.asarray(rx, np.float32).reshape(-1, E)
    frames, N = rx.shape[0], spec.N
    s = np.zeros((frames, N), np.float32) if soft is None else np.array(soft, np.float32).reshape(frames, N)
    idx = index(spec, k0, E)
    L = spec.L
    # position e and e + L hit the same code bit: pass p adds the e in [p L, (p + 1) L), each code bit at most once per
    # pass, so every code bit receives its values one float32 addition at a time in ascending e
    for p0 in range(0, E, L):
        cols = idx[p0:p0 + L]
        s[:, cols] = s[:, cols] + rx[:, p0:p0 + L]
    s[:, spec.lo:spec.hi] = np.float32(0.0)
    erased = erasure_values(N, spec.erasure_llr) if spec.erasure_llr > 0 else np.zeros(N, np.float32)
    y = np.where(s != np.float32(0.0), s, erased[None, :]).astype(np.float32)
    y[:, spec.lo:spec.hi] = spec.fill_llr
    return s, y
