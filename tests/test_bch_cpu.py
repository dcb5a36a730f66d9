"""The outer code without a GPU: primitivity and the table of generator degrees, ldpc_bch_generator and ldpc_bch_layout
against the restatement of bch_ref on a grid of fields, every refusal, the restatement's decoder against the definition
by exhaustion on a small code, csrc/bch_host.hpp in a stand-alone program under the host sanitizers, and -- with bch_ref
and the oracle alone -- the premises of the chain test on the GPU."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib

import bch_ref
import bch_util as BU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _coeffs(g):
    return np.array([(g >> i) & 1 for i in range(g.bit_length())], np.uint8)


def test_default_polynomials_are_primitive_and_the_degrees_hold(built):
    assert bch_ref.DEFAULT == {14: 0x402B, 16: 0x1002D}
    for m, prim in BU.PRIM.items():
        assert bch_ref.is_primitive(m, prim), m
    want = {(16, 12): 192, (16, 10): 160, (16, 8): 128, (14, 12): 168, (14, 10): 140, (14, 8): 112}
    for (m, t), r in want.items():
        g, polys = bch_ref.generator(m, bch_ref.DEFAULT[m], t)
        assert g.bit_length() - 1 == r and len(polys) == t, (m, t)
        got = L.BchCode.generator_of(m, bch_ref.DEFAULT[m], t)
        assert len(got) - 1 == r and np.array_equal(got, _coeffs(g)), (m, t)
    # the rule of ldpc_bch_spec_init
    for n, (m, prim) in ((16376, (14, 0x402B)), (16384, (16, 0x1002D)), (1152, (14, 0x402B)), (58320, (16, 0x1002D))):
        s = _lib.BchSpec()
        _lib.load().ldpc_bch_spec_init(ctypes.byref(s), n, 8, n // 8 + 1)
        assert (s.struct_size, s.m, s.prim, s.t, s.n, s.row_bytes) == (ctypes.sizeof(_lib.BchSpec), m, prim, 8, n, n // 8 + 1)
        assert ctypes.sizeof(_lib.BchSpec) == 24


def test_generator_equals_the_restatement_on_a_grid_of_fields(built):
    """m = 4 .. 16, several t each, among them fields where a minimal polynomial has a degree below m: m = 6 with
    alpha^9 (degree 3) and alpha^21 (degree 2), m = 4 with alpha^5, m = 8 with alpha^17, m = 10 with alpha^33."""
    small = {(6, 9): 3, (6, 21): 2, (4, 5): 2, (8, 17): 4, (10, 33): 5, (12, 65): 6}
    for (m, j), d in small.items():
        F = bch_ref.field(m, BU.PRIM[m])
        c = [e for e in bch_ref.cosets(m, (j + 1) // 2)[0] if j in e][0]
        assert bch_ref.min_poly(F, c).bit_length() - 1 == d == len(c), (m, j)
    for m, prim in BU.PRIM.items():
        N = (1 << m) - 1
        for t in (1, 2, 3, 5, 8, 11, 12):
            if 2 * t >= N:
                continue
            g, polys = bch_ref.generator(m, prim, t)
            got = L.BchCode.generator_of(m, prim, t)
            assert np.array_equal(got, _coeffs(g)), (m, t)
            # g divides x^(2^m - 1) + 1, and alpha^j is a root of g for j = 1 .. 2t and g has no repeated factor
            assert bch_ref.poly_mod((1 << N) | 1, g) == 0, (m, t)
            assert len(set(polys)) == len(polys)
            r = ctypes.c_int32()
            assert _lib.load().ldpc_bch_generator(m, prim, t, None, 0, ctypes.byref(r)) == 0 and r.value == g.bit_length() - 1
    # roots: g(alpha^j) = 0 for j = 1 .. 2t, g(alpha^(2t + 1)) != 0 where 2t + 1 lies in no coset of 1 .. 2t
    F = bch_ref.field(8, 0x11D)
    g, _ = bch_ref.generator(8, 0x11D, 3)
    def at(j):
        v = 0
        for i in range(g.bit_length()):
            if (g >> i) & 1:
                v ^= F.alpha(i * j)
        return v
    assert [at(j) for j in range(1, 7)] == [0] * 6 and at(7) != 0


def test_layout_is_right(built):
    for shape in BU.SHAPES:
        m, t, n = shape
        ref = BU.ref_code(shape)
        for extra in (0, 5):
            c = L.BchCode(n, t, row_bytes=n // 8 + extra, m=m, prim=BU.PRIM[m])
            assert c.layout() == (ref.k, ref.r, len(ref.polys), m), shape
            assert (c.k, c.r, c.n, c.t, c.row_bytes) == (ref.k, ref.r, n, t, n // 8 + extra)
            assert np.array_equal(c.generator(), _coeffs(ref.g))
    c = L.BchCode(32400, 12)
    assert (c.m, c.prim, c.k, c.r, c.row_bytes) == (16, 0x1002D, 32208, 192, 4050)
    c = L.BchCode(7200, 12)
    assert (c.m, c.prim, c.k, c.r) == (14, 0x402B, 7032, 168)


def _spec(n=248, t=3, row_bytes=31, m=8, prim=0x11D):
    s = _lib.BchSpec()
    _lib.load().ldpc_bch_spec_init(ctypes.byref(s), n, t, row_bytes)
    s.m, s.prim = m, prim
    return s


def test_every_refusal_names_the_field(built):
    """Judged before a device is touched: the pointers here are never dereferenced."""
    lib = _lib.load()
    p, q, r = 1 << 20, 1 << 24, 1 << 26
    ok = _spec()                     # k = 224: 28 payload bytes, rows of 31 bytes
    out = (ctypes.c_int32 * 4)()
    assert lib.ldpc_bch_layout(ctypes.byref(ok), out) == 0 and tuple(out) == (224, 24, 3, 8)

    def layout(spec):
        return lib.ldpc_bch_layout(ctypes.byref(spec), out)

    def encode(spec=ok, pay=p, frames=4, src=q, cap=4 * 31):
        return lib.ldpc_bch_encode_device(ctypes.byref(spec), pay, frames, src, cap, 0, None)

    def decode(spec=ok, dec=p, frames=4, pay=q, st=r):
        return lib.ldpc_bch_decode_device(ctypes.byref(spec), dec, frames, pay, st, 0, None)

    def tally(st=p, pay=q, ref=r, frames=4, per=28, counts=True):
        c = (ctypes.c_int64 * 6)()
        return lib.ldpc_bch_tally_device(st, pay, ref, frames, per, c if counts else None, 0, None)

    bad_size = _spec()
    bad_size.struct_size += 4
    cases = [(_spec(prim=0x11B), "spec.prim"),            # irreducible, not primitive
             (_spec(prim=0x101), "spec.prim"),            # reducible
             (_spec(prim=0x1D), "spec.prim"),             # degree 4 in a field declared with m = 8
             (_spec(prim=0x31D), "spec.prim"),            # degree 9
             (_spec(m=3, prim=0xB), "spec.m"), (_spec(m=17, prim=0x20009), "spec.m"),
             (_spec(n=256), "spec.n"),                    # n > 2^m - 1
             (_spec(n=244), "spec.n"), (_spec(n=0), "spec.n"), (_spec(n=-8), "spec.n"),
             (_spec(t=0), "spec.t"), (_spec(t=13), "spec.t"), (_spec(t=-1), "spec.t"),
             (_spec(m=4, prim=0x13, t=8, n=8, row_bytes=1), "spec.t"),     # 2t >= 2^m - 1
             (_spec(m=6, prim=0x43, t=5, n=56, row_bytes=7), "k = spec.n"),  # r = 27: k % 8 != 0
             (_spec(n=24, row_bytes=3), "k = spec.n"),   # k = 0
             (_spec(m=4, prim=0x13, t=2, n=8, row_bytes=1), "k = spec.n"),  # r = 8: k = 0
             (_spec(row_bytes=30), "spec.row_bytes"), (_spec(row_bytes=0), "spec.row_bytes"),
             (bad_size, "spec.struct_size")]
    for spec, word in cases:
        for call in (layout, lambda s: encode(spec=s), lambda s: decode(spec=s)):
            assert call(spec) == 1, word
            assert word in lib.ldpc_last_error().decode(), (word, lib.ldpc_last_error().decode())
    g = (ctypes.c_uint8 * 64)()
    rr = ctypes.c_int32()
    for (m, prim, t, buf, cap, deg), word in (((8, 0x11B, 3, g, 64, ctypes.byref(rr)), "prim"), ((8, 0x11D, 0, g, 64, ctypes.byref(rr)), "t"),
                                              ((3, 0xB, 1, g, 64, ctypes.byref(rr)), "m"), ((8, 0x11D, 3, g, 24, ctypes.byref(rr)), "cap"),
                                              ((8, 0x11D, 3, None, 0, None), "NULL")):
        assert lib.ldpc_bch_generator(m, prim, t, buf, cap, deg) == 1, word
        assert word in lib.ldpc_last_error().decode(), word
    for call, word in ((lambda: lib.ldpc_bch_layout(None, out), "NULL"),
                       (lambda: lib.ldpc_bch_layout(ctypes.byref(ok), None), "NULL"),
                       (lambda: encode(frames=-1), "frames"), (lambda: decode(frames=-1), "frames"), (lambda: tally(frames=-1), "frames"),
                       (lambda: encode(cap=4 * 31 - 1), "src_bytes"),
                       (lambda: encode(pay=None), "NULL"), (lambda: encode(src=None), "NULL"), (lambda: decode(dec=None), "NULL"),
                       (lambda: decode(pay=None, st=None), "NULL"), (lambda: tally(st=None), "NULL"), (lambda: tally(pay=None), "NULL"),
                       (lambda: tally(counts=False), "NULL"), (lambda: tally(per=0), "bytes_per_frame"),
                       (lambda: decode(st=r + 2), "aligned"), (lambda: tally(st=p + 1), "aligned"),
                       (lambda: encode(src=p + 4 * 28 - 1), "overlap"), (lambda: encode(pay=q + 4 * 31 - 1), "overlap"),
                       (lambda: decode(pay=p + 4 * 31 - 1), "overlap"), (lambda: decode(st=p + 120), "overlap"),
                       (lambda: decode(st=q + 108), "overlap"), (lambda: decode(dec=q + 4 * 28 - 1), "overlap")):
        assert call() == 1, word
        assert word in lib.ldpc_last_error().decode(), (word, lib.ldpc_last_error().decode())
    # adjacent buffers and frames == 0 are fine (frames == 0 enqueues nothing and touches no device)
    assert encode(frames=0, cap=0) == 0 and decode(frames=0) == 0 and tally(frames=0) == 0
    assert decode(frames=0, pay=None) == 0 and decode(frames=0, st=None) == 0
    with pytest.raises(L.LdpcError) as e:
        L.BchCode(248, 3, m=8, prim=0x11B)
    assert e.value.code == 1


def test_compute_entry_points_have_no_cpu_path(built):
    """Host buffers: without a device LDPC_ERR_HIP, with one the call simply runs."""
    code = L.BchCode(248, 3, m=8, prim=0x11D)
    payload = np.arange(2 * 28, dtype=np.uint8).reshape(2, 28)
    if L.device_count() > 0:
        got, status = code.decode(code.encode(payload))
        assert np.array_equal(got, payload) and not status.any()
        return
    with pytest.raises(L.LdpcError) as e:
        code.encode(payload)
    assert e.value.code == 2
    with pytest.raises(L.LdpcError) as e:
        code.decode(np.zeros((2, 31), np.uint8))
    assert e.value.code == 2
    lib = _lib.load()
    s = _spec()
    counts = (ctypes.c_int64 * 6)()
    assert lib.ldpc_bch_encode_device(ctypes.byref(s), 1 << 20, 4, 1 << 24, 4 * 31, 0, None) == 2
    assert lib.ldpc_bch_decode_device(ctypes.byref(s), 1 << 20, 4, 1 << 24, None, 0, None) == 2
    assert lib.ldpc_bch_tally_device(1 << 20, 1 << 24, None, 4, 28, counts, 0, None) == 2


def test_coder_exports_set_outer_bch(built):
    so = os.path.join(ROOT, "myldpccppapi_amd", "libmyldpc.so")
    syms = subprocess.run("nm -D --defined-only %s | c++filt" % so, shell=True, capture_output=True, text=True).stdout
    assert "Coder::setOuterBch(int, int)" in syms


def test_coder_set_outer_bch_refusals_and_lengths(built, tmp_path):
    """tests/cpp/coder_outer_bch.cpp, the parts that need no device: t, n and k out of range are refused, a refused call
    changes nothing, setOuterBch and setTransportBlock exclude one another, the length helpers count payload bytes."""
    out = subprocess.run([BU.coder_outer_bch_exe(tmp_path), "host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "refused=ok lengths=ok" in out.stdout, out.stdout + out.stderr


def test_bch_host_unit_under_host_sanitizers(tmp_path):
    """csrc/bch_host.hpp in a stand-alone program built with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "bch_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "bch_host_test.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout + p.stderr


# ---- the restatement against the definition ----------------------------------------------------------------------------

def _small():
    c = bch_ref.Code(40, 2, m=8, prim=0x11D)
    assert c.valid and (c.k, c.r) == (24, 16)
    return c


def test_restated_maps_equal_their_bitwise_forms():
    """The bit matrices used for batches against long division and the direct syndrome sum, on whole random words."""
    rng = np.random.default_rng(500)
    for shape in ((8, 3, 248), (10, 4, 1000), (6, 4, 56), (14, 12, 7200)):
        c = BU.ref_code(shape)
        a = rng.integers(0, 2, (3, c.k), dtype=np.uint8)
        par = c.parity(a)
        v = rng.integers(0, 2, (3, c.n), dtype=np.uint8)
        S = c.syndromes(v)
        for f in range(3 if c.n < 2000 else 1):
            assert np.array_equal(par[f], c.parity_long_division(a[f])), shape
            assert list(S[f]) == c.syndromes_direct(v[f]), shape
        # a code word has zero syndromes; its parity is that of the definition p(x) = x^r a(x) mod g(x)
        word = np.concatenate([a, par], axis=1)
        assert not c.syndromes(word).any(), shape
        ax = sum(int(b) << (c.k - 1 - i) for i, b in enumerate(a[0]))
        px = sum(int(b) << (c.r - 1 - j) for j, b in enumerate(par[0]))
        assert bch_ref.poly_mod(ax << c.r, c.g) == px, shape


def test_decode_rule_by_exhaustion_on_the_small_code():
    """(m = 8, t = 2, n = 40, k = 24).  Every pattern of weight <= 2 is corrected exactly.  For every pattern of weight 3
    and a seeded sample of heavier ones the result is -1 with the bits unchanged -- and then no set of at most t flips
    has the word's syndromes -- or a word with all-zero syndromes at distance <= t from the input."""
    c = _small()
    n, t = c.n, c.t
    rng = np.random.default_rng(501)
    word = bch_ref.bits_of(c.encode(rng.integers(0, 256, (1, 3), dtype=np.uint8)))[0]
    assert c.syndromes_direct(word) == [0] * 4
    light = [p for w in (1, 2) for p in itertools.combinations(range(n), w)]
    rows = np.tile(word, (len(light), 1))
    for f, p in enumerate(light):
        rows[f, list(p)] ^= 1
    fixed, status = c.decode_bits(rows)
    assert (fixed == word).all() and list(status) == [len(p) for p in light]
    table = {tuple(s) for s in c.syndromes(rows)}                  # the syndromes of every set of 1 .. t flips
    assert len(table) == len(light) and (0, 0, 0, 0) not in table  # all distinct: d >= 2t + 1
    heavy = [p for p in itertools.combinations(range(n), 3)]
    for w in (4, 5, 7, 12, 20):
        heavy += [tuple(sorted(rng.choice(n, w, replace=False))) for _ in range(300)]
    rows = np.tile(word, (len(heavy), 1))
    for f, p in enumerate(heavy):
        rows[f, list(p)] ^= 1
    fixed, status = c.decode_bits(rows)
    S_in, S_out = c.syndromes(rows), c.syndromes(fixed)
    seen = set()
    for f in range(len(heavy)):
        if status[f] == -1:
            assert np.array_equal(fixed[f], rows[f]) and tuple(S_in[f]) not in table
        elif status[f] == 0:
            assert not S_in[f].any() and np.array_equal(fixed[f], rows[f])
        else:
            assert 1 <= status[f] <= t and int((fixed[f] ^ rows[f]).sum()) == status[f] and not S_out[f].any()
        seen.add(int(status[f]))
    assert {-1, 1, 2} <= seen                                       # failures and miscorrections both occur
    assert (status[:len(heavy) - 1500] != 0).all()                   # weight 3 < d never lands on a code word


def test_a_root_outside_the_shortened_code_is_a_failure():
    """A code word of the (m = 8, t = 2, n = 48) code with one wrong bit among its first 8 bits, such that those 8 bits
    are zero, and the word then shortened by them: as polynomials the two words are the same, so the n = 40 word has the
    syndromes of the locator alpha^e with e = 47 - bit >= 40, which is no position of it.  No other set of at most t
    positions has them (it would make a code word of weight <= 3), so the result must be -1."""
    long_, short = bch_ref.Code(48, 2, m=8, prim=0x11D), _small()
    rng = np.random.default_rng(502)
    for bit in (0, 3, 7):
        payload = rng.integers(0, 256, (1, 4), dtype=np.uint8)
        payload[0, 0] = 1 << bit
        word = bch_ref.bits_of(long_.encode(payload))[0]
        bad = word.copy()
        bad[bit] ^= 1                                               # the one wrong bit; the first 8 bits are now zero
        assert not bad[:8].any()
        fixed, st = long_.decode_bits(bad[None])
        assert list(st) == [1] and np.array_equal(fixed[0], word)   # the long code repairs it
        cut = bad[8:]
        assert short.syndromes_direct(cut) == [short.F.alpha(j * (47 - bit)) for j in range(1, 5)]
        fixed, st = short.decode_bits(cut[None])
        assert list(st) == [-1] and np.array_equal(fixed[0], cut)


def test_tally_restated():
    status = np.array([0, 0, 1, 2, -1, -1, 3], np.int32)
    ref = np.arange(7 * 3, dtype=np.uint8).reshape(7, 3)
    payload = ref.copy()
    payload[1, 2] ^= 1      # undetected
    payload[3, 0] ^= 4      # miscorrected
    payload[4, 1] ^= 8      # failed and wrong; frame 5 failed although equal
    assert bch_ref.tally(status, payload, ref) == (2, 3, 2, 3, 6, 1)


# ---- bch_ref and the oracle alone: what the chain test on the GPU leans on ---------------------------------------------

@pytest.mark.parametrize("algo", sorted(BU.BUDGET))
def test_chain_scenario_has_all_three_kinds_of_frame(algo):
    """WiMAX (2304, 1152), 96 frames, sd = 0.74, the round budget of bch_util: the oracle's decoder leaves at least three
    clean frames, at least three with 1 .. t wrong bits and at least three with more than t."""
    out, residual, want_payload, want_status, counts = BU.chain_oracle(algo)
    t = BU.T
    kinds = (int((residual == 0).sum()), int(((residual > 0) & (residual <= t)).sum()), int((residual > t).sum()))
    print("%s max_iter %d: clean %d, 1..t %d, > t %d; tally %s" % ((algo, BU.BUDGET[algo]) + kinds + (counts,)))
    assert min(kinds) >= 3, kinds
    # frames with at most t wrong bits are repaired to the payload that was sent, with status = their number
    payload = BU.chain_sent()[0]
    few = residual <= t
    assert np.array_equal(want_status[few], residual[few]) and np.array_equal(want_payload[few], payload[few])
    # beyond t the stage fails or miscorrects; it never reports a clean frame
    assert (want_status[~few] != 0).all()
