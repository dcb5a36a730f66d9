"""The transport-block stage without a GPU: the CRC's known answers for tb_ref and ldpc_crc_bits, CRC16 against binascii,
the rule of ldpc_tb_spec_init, ldpc_tb_layout, the argument checks, csrc/tb_host.hpp in a stand-alone program under the host
sanitizers, and -- with tb_ref and the oracle alone -- the window the GPU chain test leans on."""
import binascii
import ctypes
import os
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib

import tb_ref
import tb_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = {24: 0xCDE703, 25: 0x23EF52, 16: 0x31C3}


def _msb_first(data):
    """bytes -> the row whose project-order bits a_0, a_1, ... are the bytes' bits MSB first."""
    return np.packbits(np.unpackbits(np.frombuffer(data, np.uint8), bitorder="big"), bitorder="little")


def test_known_answers(built):
    row = _msb_first(b"123456789")
    for kind, want in KNOWN.items():
        assert tb_ref.crc(kind, tb_ref.bits_of(row)) == want, kind
        assert L.TransportBlock.crc_bits(kind, row) == want, kind
    assert L.TransportBlock.crc_bits("24a", row) == KNOWN[24] and L.TransportBlock.crc_bits("24b", row, 72) == KNOWN[25]
    assert binascii.crc_hqx(b"123456789", 0) == KNOWN[16]
    # p_0 is the top bit: the parity bits as tb_ref lists them
    p = tb_ref.parity(24, tb_ref.bits_of(row).reshape(1, -1))[0]
    assert [int(b) for b in p] == [(KNOWN[24] >> (23 - i)) & 1 for i in range(24)]


def test_crc16_equals_binascii_on_random_rows(built):
    rng = np.random.default_rng(70)
    for n in (1, 2, 3, 39, 64, 257):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        row = _msb_first(data)
        assert L.TransportBlock.crc_bits(16, row) == binascii.crc_hqx(data, 0), n
        assert tb_ref.crc(16, tb_ref.bits_of(row)) == binascii.crc_hqx(data, 0), n


def test_crc_bits_equals_the_reference_at_any_length(built):
    rng = np.random.default_rng(71)
    row = rng.integers(0, 256, 300, dtype=np.uint8)
    bits = tb_ref.bits_of(row)
    for kind in (16, 24, 25):
        for n in (0, 1, 7, 9, 23, 24, 25, 129, 258, 516, 1031, 2399):
            assert L.TransportBlock.crc_bits(kind, row, n) == tb_ref.crc(kind, bits[:n]), (kind, n)
    # bits behind nbits do not matter
    other = row.copy()
    other[2] ^= 0x80
    assert L.TransportBlock.crc_bits(24, other, 23) == L.TransportBlock.crc_bits(24, row, 23)
    assert L.TransportBlock.crc_bits(24, other, 24) != L.TransportBlock.crc_bits(24, row, 24)


def _init(A, K):
    s = _lib.TbSpec()
    _lib.load().ldpc_tb_spec_init(ctypes.byref(s), A, K)
    assert s.struct_size == ctypes.sizeof(_lib.TbSpec) == 24 and s.A == A and s.K == K
    return s


def test_spec_init_follows_the_rule(built):
    lib = _lib.load()
    K = 8448
    #        A, K -> tb_crc, C, cb_crc
    cases = [(3824, K, 16, 1, 0), (3832, K, 24, 1, 0),
             (K - 24, K, 24, 1, 0),                      # B = K
             (K - 16, K, 24, 2, 24),                     # B = K + 8
             (312, 352, 16, 1, 0), (8 * 8424 - 24, K, 24, 8, 24), (1000, 352, 16, 4, 24)]
    for A, k, tb_crc, C, cb_crc in cases:
        s = _init(A, k)
        assert (s.tb_crc, s.C, s.cb_crc) == (tb_crc, C, cb_crc), (A, k)
        r = tb_ref.Spec(A, k)
        assert (r.tb_crc, r.C, r.cb_crc) == (tb_crc, C, cb_crc), (A, k)
        out = (ctypes.c_int32 * 6)()
        if r.valid:
            assert lib.ldpc_tb_layout(ctypes.byref(s), out) == 0 and tuple(out) == r.layout(), (A, k)
    # a case the rule leaves with B % C != 0: B = 8456 into C = 3 code blocks (K = 4248)
    s = _init(8432, 4248)
    assert (s.tb_crc, s.C, s.cb_crc) == (24, 3, 24) and 8456 % 3 != 0
    out = (ctypes.c_int32 * 6)()
    assert lib.ldpc_tb_layout(ctypes.byref(s), out) == 1 and "B % C" in lib.ldpc_last_error().decode()
    with pytest.raises(L.LdpcError) as e:
        L.TransportBlock(8432, 4248)
    assert e.value.code == 1


def test_layout_equals_the_reference(built):
    for shape in TU.SHAPES:
        A, tb_crc, C, cb_crc, K = shape
        tb = L.TransportBlock(A, K, C=C, tb_crc=tb_crc, cb_crc=cb_crc)
        r = TU.ref_spec(shape)
        assert r.valid and tb.layout() == r.layout(), shape
        assert (tb.B, tb.S, tb.Kp, tb.filler_lo, tb.filler_hi, tb.C) == r.layout()
    tb = L.TransportBlock(312, 352)
    assert tb.layout() == (328, 328, 328, 328, 352, 1) and (tb.tb_crc, tb.cb_crc) == (16, 0)


def _spec(A=1008, tb_crc=24, C=4, cb_crc=24, K=288):
    s = _init(A, K)
    s.tb_crc, s.C, s.cb_crc = tb_crc, C, cb_crc
    return s


def test_argument_errors_name_the_field(built):
    """Every refusal is judged before a device is touched: the pointers here are never dereferenced."""
    lib = _lib.load()
    p, q, r, t = 1 << 20, 1 << 24, 1 << 26, 1 << 27
    ok = _spec()                    # A/8 = 126 bytes per block, 4 frames of 36 bytes

    def attach(spec=ok, pay=p, tbs=4, src=q, cap=4 * 4 * 36):
        return lib.ldpc_tb_attach_device(ctypes.byref(spec), pay, tbs, src, cap, 0, None)

    def check(spec=ok, dec=p, tbs=4, pay=q, cb=r, tb=t):
        return lib.ldpc_tb_check_device(ctypes.byref(spec), dec, tbs, pay, cb, tb, 0, None)

    def tally(ok_ptr=p, pay=q, ref=r, tbs=4, per=126, counts=True):
        c = (ctypes.c_int64 * 4)()
        return lib.ldpc_tb_tally_device(ok_ptr, pay, ref, tbs, per, c if counts else None, 0, None)

    bad_size = _spec()
    bad_size.struct_size -= 4
    for call, word in ((lambda: attach(spec=_spec(A=1004)), "A"), (lambda: attach(spec=_spec(A=0)), "A"), (lambda: check(spec=_spec(A=-8)), "A"),
                       (lambda: attach(spec=_spec(tb_crc=8)), "tb_crc"), (lambda: check(spec=_spec(tb_crc=25)), "tb_crc"),
                       (lambda: attach(spec=_spec(C=0)), "C"), (lambda: check(spec=_spec(C=-1)), "C"),
                       (lambda: attach(spec=_spec(cb_crc=16)), "cb_crc"), (lambda: check(spec=_spec(cb_crc=25)), "cb_crc"),
                       (lambda: attach(spec=_spec(K=284)), "K"), (lambda: check(spec=_spec(K=0)), "K"),
                       (lambda: attach(spec=_spec(C=5)), "B % C"), (lambda: check(spec=_spec(C=7)), "B % C"),
                       (lambda: attach(spec=_spec(K=280)), "Kp"), (lambda: check(spec=_spec(C=3, K=352)), "Kp"),
                       (lambda: attach(spec=bad_size), "struct_size"), (lambda: check(spec=bad_size), "struct_size"),
                       (lambda: attach(tbs=-1), "tbs"), (lambda: check(tbs=-1), "tbs"), (lambda: tally(tbs=-1), "tbs"),
                       (lambda: attach(cap=4 * 4 * 36 - 1), "src_bytes"),
                       (lambda: attach(pay=None), "NULL"), (lambda: attach(src=None), "NULL"), (lambda: check(dec=None), "NULL"),
                       (lambda: check(pay=None, cb=None, tb=None), "NULL"), (lambda: tally(ok_ptr=None), "NULL"), (lambda: tally(pay=None), "NULL"),
                       (lambda: tally(counts=False), "NULL"), (lambda: tally(per=0), "bytes_per_tb"),
                       (lambda: attach(src=p + 4 * 126 - 1), "overlap"), (lambda: attach(pay=q + 4 * 4 * 36 - 1), "overlap"),
                       (lambda: check(pay=p + 4 * 4 * 36 - 1), "overlap"), (lambda: check(cb=p), "overlap"), (lambda: check(tb=p + 100), "overlap"),
                       (lambda: check(cb=q + 4 * 126 - 1), "overlap"), (lambda: check(tb=r + 15), "overlap")):
        assert call() == 1, word
        assert word in lib.ldpc_last_error().decode(), (word, lib.ldpc_last_error().decode())
    out = (ctypes.c_int32 * 6)()
    assert lib.ldpc_tb_layout(None, out) == 1 and lib.ldpc_tb_layout(ctypes.byref(bad_size), out) == 1
    assert lib.ldpc_tb_layout(ctypes.byref(ok), None) == 1 and "NULL" in lib.ldpc_last_error().decode()
    crc = ctypes.c_uint32()
    row = np.zeros(4, np.uint8)
    assert lib.ldpc_crc_bits(17, row.ctypes.data, 8, ctypes.byref(crc)) == 1 and "kind" in lib.ldpc_last_error().decode()
    assert lib.ldpc_crc_bits(24, row.ctypes.data, -1, ctypes.byref(crc)) == 1 and "nbits" in lib.ldpc_last_error().decode()
    assert lib.ldpc_crc_bits(24, None, 8, ctypes.byref(crc)) == 1 and lib.ldpc_crc_bits(24, row.ctypes.data, 8, None) == 1
    # adjacent buffers and tbs == 0 are fine (tbs == 0 enqueues nothing and touches no device)
    assert attach(tbs=0, cap=0) == 0 and check(tbs=0) == 0 and tally(tbs=0) == 0
    assert check(tbs=0, pay=None, cb=None) == 0 and check(tbs=0, cb=None, tb=None) == 0


def test_compute_entry_points_have_no_cpu_path(built):
    """Host buffers: without a device LDPC_ERR_HIP, with one the call simply runs."""
    tb = L.TransportBlock(312, 352)
    payload = np.arange(2 * 39, dtype=np.uint8).reshape(2, 39)
    if L.device_count() > 0:
        got, cb_ok, tb_ok = tb.check(tb.attach(payload))
        assert np.array_equal(got, payload) and cb_ok.all() and tb_ok.all()
        return
    with pytest.raises(L.LdpcError) as e:
        tb.attach(payload)
    assert e.value.code == 2
    with pytest.raises(L.LdpcError) as e:
        tb.check(np.zeros((2, 44), np.uint8))
    assert e.value.code == 2
    lib = _lib.load()
    s = _spec()
    counts = (ctypes.c_int64 * 4)()
    assert lib.ldpc_tb_attach_device(ctypes.byref(s), 1 << 20, 4, 1 << 24, 4 * 4 * 36, 0, None) == 2
    assert lib.ldpc_tb_check_device(ctypes.byref(s), 1 << 20, 4, 1 << 24, None, None, 0, None) == 2
    assert lib.ldpc_tb_tally_device(1 << 20, 1 << 24, None, 4, 126, counts, 0, None) == 2


def test_coder_exports_set_transport_block(built):
    so = os.path.join(ROOT, "myldpccppapi_amd", "libmyldpc.so")
    syms = subprocess.run("nm -D --defined-only %s | c++filt" % so, shell=True, capture_output=True, text=True).stdout
    assert "Coder::setTransportBlock(int, int)" in syms


def test_coder_set_transport_block_refusals_and_lengths(built, tmp_path):
    """tests/cpp/coder_transport_block.cpp, the parts that need no device: payload + CRC beyond K is refused, a refused call
    changes nothing, and the length helpers count payload bytes."""
    out = subprocess.run([TU.coder_transport_block_exe(tmp_path), "host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "refused=ok lengths=ok" in out.stdout, out.stdout + out.stderr


def test_tb_host_unit_under_host_sanitizers(tmp_path):
    """csrc/tb_host.hpp in a stand-alone program built with the address and undefined-behaviour sanitizers: mulmod and
    x^n mod g against repeated shifting, the combine identity against the bitwise CRC on random rows cut at random
    points, the plan's lane and segment weights, the known answers, the rule."""
    exe = str(tmp_path / "tb_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "tb_host_test.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout + p.stderr


def test_reference_attach_then_check_round_trips():
    """tb_ref alone: check(attach(x)) = x with every flag set; one flipped bit in front of the fillers clears tb_ok, one
    inside them changes nothing."""
    rng = np.random.default_rng(72)
    for shape in TU.SHAPES:
        spec = TU.ref_spec(shape)
        payload = rng.integers(0, 256, (3, spec.A // 8), dtype=np.uint8)
        frames = tb_ref.attach(spec, payload)
        assert frames.shape == (3 * spec.C, spec.K // 8)
        assert not tb_ref.bits_of(frames)[:, spec.Kp:].any()
        got, cb_ok, tb_ok = tb_ref.check(spec, frames)
        assert np.array_equal(got, payload) and cb_ok.all() and tb_ok.all(), shape
        bad = frames.copy()
        bit = int(rng.integers(0, spec.Kp))
        bad[spec.C + spec.C // 2, bit >> 3] ^= 1 << (bit & 7)
        _, cb_ok, tb_ok = tb_ref.check(spec, bad)
        assert list(tb_ok) == [1, 0, 1], shape
        assert int(cb_ok.sum()) == 3 * spec.C - (1 if spec.cb_crc else 0), shape
        if spec.Kp < spec.K:
            bad = frames.copy()
            bad[0, (spec.K - 1) >> 3] ^= 0x80
            _, cb_ok, tb_ok = tb_ref.check(spec, bad)
            assert cb_ok.all() and tb_ok.all(), shape


# ---- tb_ref and the oracle alone: what the chain test on the GPU leans on -------------------------------------------

@pytest.mark.parametrize("algo", ["layered", "ms", "sp"])
def test_chain_scenario_has_passing_and_failing_blocks(algo):
    """At 3.0 dB every one of the 64 transport blocks passes its CRC16; at the hard point (0.0 dB for layered and ms,
    1.5 dB for sp with llr_scale 8) between 8 and 56 of them fail."""
    out, iters, payload, cb_ok, tb_ok, counts = TU.chain_oracle(algo, TU.CLEAN_DB)
    print("%s %.1f dB: failed %d wrong %d undetected %d parity-only %d" % ((algo, TU.CLEAN_DB) + counts))
    assert counts == (0, 0, 0, 0) and tb_ok.all() and np.array_equal(payload, TU.chain_payload()[0])
    snr = TU.HARD[algo][0]
    out, iters, payload, cb_ok, tb_ok, counts = TU.chain_oracle(algo, snr)
    print("%s %.1f dB: failed %d wrong %d undetected %d parity-only %d" % ((algo, snr) + counts))
    assert TU.WINDOW[0] <= counts[0] <= TU.WINDOW[1], counts
    assert counts[0] == int((tb_ok == 0).sum()) and cb_ok.all()
