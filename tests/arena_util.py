"""One device allocation carved into sub-buffers at chosen address phases, with guard bands (a helper, not a test module).

A caller of the device entry points cuts one arena into buffers at whatever offsets its sizes produce.  Arena does the
same for the tests: every buffer a call gets lies at an address of a chosen phase (say 4 modulo 16, or odd), has exactly
the size the call states, and is surrounded by bytes that still hold 0xEE when the call has finished -- or the call
wrote outside its buffers."""
import numpy as np
import torch

FILL = 0xEE
NAN_WORD = 0x7FC0BEEF          # a quiet NaN with a recognisable payload: rows that are not part of a call


class Arena:
    def __init__(self, nbytes, device="cuda"):
        self.buf = torch.full((int(nbytes),), FILL, dtype=torch.uint8, device=device)
        self.base = self.buf.data_ptr()
        self.size = int(nbytes)
        self.cursor = 0                    # first byte no carved buffer or guard band has claimed
        self.carved = []                   # (offset, nbytes, name) in ascending offset order

    # ------------------------------------------------------------------ carving
    def carve(self, nbytes, align=1, phase=0, guard=64, name=None):
        """Device pointer p of a buffer of `nbytes` bytes with p % align == phase; at least `guard` bytes that belong to
        no buffer lie on both sides of it."""
        nbytes, align, phase, guard = int(nbytes), int(align), int(phase), int(guard)
        if not (align >= 1 and 0 <= phase < align and nbytes >= 0 and guard >= 0):
            raise ValueError("carve(%d, align=%d, phase=%d, guard=%d)" % (nbytes, align, phase, guard))
        off = self.cursor + guard
        off += (phase - (self.base + off)) % align
        if off + nbytes + guard > self.size:
            raise MemoryError("arena of %d bytes is full (%d carved, %d more asked for)" % (self.size, self.cursor, nbytes))
        self.carved.append((off, nbytes, name or "buffer %d" % len(self.carved)))
        self.cursor = off + nbytes
        return self.base + off

    def _off(self, ptr, nbytes):
        off = int(ptr) - self.base
        for lo, n, _ in self.carved:
            if lo <= off and off + nbytes <= lo + n:
                return off
        raise ValueError("[%d, %d) is not inside a carved buffer" % (off, off + nbytes))

    # ------------------------------------------------------------------ data in and out
    def put(self, ptr, array):
        """the bytes of a numpy array to ptr"""
        a = np.ascontiguousarray(array)
        raw = torch.from_numpy(a.reshape(-1).view(np.uint8).copy())
        off = self._off(ptr, raw.numel())
        self.buf[off:off + raw.numel()].copy_(raw)

    def put_floats(self, ptr, array):
        self.put(ptr, np.ascontiguousarray(array, np.float32))

    def get(self, ptr, n, dtype=np.uint8):
        """numpy array of n items of dtype read from ptr"""
        nb = int(n) * np.dtype(dtype).itemsize
        off = self._off(ptr, nb)
        return self.buf[off:off + nb].cpu().numpy().copy().view(dtype)

    def fill(self, ptr, nbytes, value=FILL):
        off = self._off(ptr, int(nbytes))
        self.buf[off:off + int(nbytes)].fill_(value)

    def poison(self, ptr, nfloats):
        """nfloats quiet NaNs of the pattern 0x7fc0beef from ptr on"""
        if nfloats > 0:
            self.put(ptr, np.full(int(nfloats), NAN_WORD, np.uint32))

    # ------------------------------------------------------------------ checks
    def outside_mask(self):
        """bool [size]: bytes that belong to no carved buffer"""
        m = np.ones(self.size, bool)
        for lo, n, _ in self.carved:
            m[lo:lo + n] = False
        return m

    def assert_untouched(self, what=""):
        """Every byte outside the carved buffers still holds 0xEE (one device-to-host copy)."""
        host = self.buf.cpu().numpy()
        bad = np.nonzero(self.outside_mask() & (host != FILL))[0]
        if bad.size:
            at = int(bad[0])
            # the nearest carved buffer: the distance to its interval
            lo, n, name = min(self.carved, key=lambda c: max(c[0] - at, at - (c[0] + c[1] - 1), 0)) if self.carved else (0, 0, "arena")
            where = "%d bytes before its start" % (lo - at) if at < lo else "%d bytes past its end" % (at - (lo + n) + 1)
            raise AssertionError("%s: %d bytes outside every buffer were written; the first at arena offset %d, %s of %r "
                                 "(offset %+d from its first byte), now 0x%02x"
                                 % (what, bad.size, at, where, name, at - lo, int(host[at])))

    def assert_all_untouched(self, what=""):
        """The whole arena, carved buffers included, still holds 0xEE (after a refused call)."""
        host = self.buf.cpu().numpy()
        bad = np.nonzero(host != FILL)[0]
        assert bad.size == 0, "%s: %d bytes written, the first at arena offset %d" % (what, bad.size, int(bad[0]))

    def assert_tail_untouched(self, ptr, written, size, what=""):
        """Bytes [written, size) of the carved buffer at ptr, which a call was to write only in part, still hold 0xEE."""
        tail = self.get(int(ptr) + int(written), int(size) - int(written))
        bad = np.nonzero(tail != FILL)[0]
        assert bad.size == 0, "%s: byte %d of the buffer (behind the %d the call may write) is 0x%02x" % (
            what, int(written) + int(bad[0]) if bad.size else -1, int(written), int(tail[bad[0]]) if bad.size else 0)
