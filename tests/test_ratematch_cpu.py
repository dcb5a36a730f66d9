"""Rate matching without a GPU: the index arithmetic of ldpc_rate_index against the literal buffer walk, the argument
checks, the erasure values, and -- with ratematch_ref and the oracle alone -- the reference-only facts the GPU tests
and the documentation lean on (the layered arithmetic cannot take an exact erasure; the distinct-value rule repairs it)."""
import ctypes

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib

import ratematch_ref as ref
import ratematch_util as U


def test_index_equals_the_buffer_walk(built):
    cases = U.grid_cases()
    assert len(cases) >= 6 * 2 * 5
    for spec, k0, E in cases:
        rm = L.RateMatcher(**spec.kwargs())
        assert rm.lengths() == (spec.Ncb, spec.L)
        got = rm.index(k0, E)
        assert np.array_equal(got, ref.index(spec, k0, E)), (spec.P, spec.lo, spec.hi, k0, E)


def test_fillers_at_the_end_of_the_buffer_wrap_to_the_start(built):
    spec = ref.Spec(1001, 5, (990, 1001))
    rm = L.RateMatcher(**spec.kwargs())
    for k0 in (0, 984, 985, 990, spec.Ncb - 1):
        assert np.array_equal(rm.index(k0, 2 * spec.L + 3), ref.index(spec, k0, 2 * spec.L + 3)), k0


def _raw_spec(N=1088, P=32, lo=328, hi=352, fill=10.0, eps=0.0):
    lib = _lib.load()
    s = _lib.RateSpec()
    lib.ldpc_rate_spec_init(ctypes.byref(s), N)
    assert s.struct_size == ctypes.sizeof(_lib.RateSpec) and s.N == N and s.fill_llr == 10.0 and s.erasure_llr == 0.0
    assert (s.punctured, s.filler_lo, s.filler_hi) == (0, 0, 0)
    s.punctured, s.filler_lo, s.filler_hi, s.fill_llr, s.erasure_llr = P, lo, hi, fill, eps
    return s


def _index_rc(s, k0, E):
    lib = _lib.load()
    out = np.zeros(max(E, 1), np.int32)
    rc = lib.ldpc_rate_index(ctypes.byref(s), k0, E, out.ctypes.data)
    return rc, lib.ldpc_last_error().decode()


def test_argument_errors_name_the_field(built):
    ok = _raw_spec()
    assert _index_rc(ok, 0, 10)[0] == 0
    Ncb = 1088 - 32
    for s, k0, E, word in ((ok, Ncb, 10, "k0"), (ok, -1, 10, "k0"), (ok, 0, 0, "E"), (ok, 0, -4, "E"),
                           (_raw_spec(lo=31), 0, 10, "filler_lo"), (_raw_spec(hi=1089), 0, 10, "filler_hi"),
                           (_raw_spec(lo=352, hi=328), 0, 10, "filler_hi"),
                           (_raw_spec(P=32, lo=32, hi=1088), 0, 10, "L = 0"),
                           (_raw_spec(P=-1), 0, 10, "punctured"), (_raw_spec(N=0, P=0, lo=0, hi=0), 0, 10, "N"),
                           (_raw_spec(eps=-1e-6), 0, 10, "erasure_llr"), (_raw_spec(eps=float("nan")), 0, 10, "erasure_llr"),
                           (_raw_spec(eps=float("inf")), 0, 10, "erasure_llr"), (_raw_spec(fill=float("nan")), 0, 10, "fill_llr")):
        rc, msg = _index_rc(s, k0, E)
        assert rc == 1 and word in msg, (word, rc, msg)
    bad = _raw_spec()
    bad.struct_size -= 4
    rc, msg = _index_rc(bad, 0, 10)
    assert rc == 1 and "struct_size" in msg
    lib = _lib.load()
    assert lib.ldpc_rate_lengths(ctypes.byref(bad), None, None) == 1
    assert lib.ldpc_rate_lengths(None, None, None) == 1
    # the erasure values stop being pairwise distinct beyond 2^22 code bits
    big = _raw_spec(N=(1 << 22) + 8, P=0, lo=0, hi=0, eps=1e-6)
    rc, msg = _index_rc(big, 0, 10)
    assert rc == 1 and "erasure_llr" in msg
    assert _index_rc(_raw_spec(N=(1 << 22) + 8, P=0, lo=0, hi=0), 0, 10)[0] == 0
    assert _index_rc(_raw_spec(N=1 << 22, P=0, lo=0, hi=0, eps=1e-6), 0, 10)[0] == 0
    with pytest.raises(L.LdpcError) as e:
        L.RateMatcher(1088, punctured=32, filler=(8, 16))
    assert e.value.code == 1


def test_device_entry_points_check_their_arguments_first(built):
    """Formats, lengths, NULL and aliasing are judged before any device is touched."""
    lib = _lib.load()
    s = _raw_spec()
    sp = ctypes.byref(s)
    p = 4096        # never dereferenced
    for args, word in (((sp, p, 7, 4, 0, 64, p, 1 << 20, 1, 0, None), "code_format"),
                       ((sp, p, 1, 4, 0, 64, p, 1 << 20, 9, 0, None), "tx_format"),
                       ((sp, p, 1, 4, 0, 61, p, 1 << 20, 0, 0, None), "E % 8"),
                       ((sp, p, 1, 4, 0, 64, p, 4 * 64 - 1, 1, 0, None), "tx_bytes"),
                       ((sp, p, 1, 4, 0, 64, p, 4 * 8 - 1, 0, 0, None), "tx_bytes"),
                       ((sp, None, 1, 4, 0, 64, p, 1 << 20, 1, 0, None), "NULL"),
                       ((sp, p, 1, -1, 0, 64, p, 1 << 20, 1, 0, None), "frames")):
        assert lib.ldpc_rate_match_device(*args) == 1
        assert word in lib.ldpc_last_error().decode(), word
    odd = _raw_spec(N=1001, P=0, lo=0, hi=0)
    assert lib.ldpc_rate_match_device(ctypes.byref(odd), p, 0, 4, 0, 64, p, 1 << 20, 1, 0, None) == 1
    assert "N % 8" in lib.ldpc_last_error().decode()
    for args, word in (((sp, p, 4, 0, 64, None, 0, None, 0, None), "both NULL"),
                       ((sp, p, 4, 0, 64, None, 1, p, 0, None), "accumulate"),
                       ((sp, None, 4, 0, 64, p, 0, None, 0, None), "rx_dev"),
                       ((sp, p, 4, 0, 64, p, 0, p, 0, None), "alias"),
                       ((sp, p, 4, 0, 64, p, 0, p + 4 * 1088 * 4 - 4, 0, None), "alias")):
        assert lib.ldpc_rate_recover_device(*args) == 1
        assert word in lib.ldpc_last_error().decode(), word


@pytest.mark.parametrize("N", [26112, 64800])
def test_erasure_values_are_pairwise_distinct(N):
    v = ref.erasure_values(N, 1e-6)
    assert v.dtype == np.float32 and np.unique(v).size == N
    assert (np.diff(v) > 0).all() and v[0] == np.float32(1e-6) and v[-1] < np.float32(2e-6)


# ---- the oracle on reference-recovered channel values: entries of the table in DESIGN.md ----------------------------

def test_layered_fails_every_frame_with_exact_erasures():
    assert U.oracle_decode("S1", 0.0, 1, "layered")[2] == U.FRAMES


@pytest.mark.parametrize("name,transmissions", [("S1", 1), ("S2", 1), ("S4", 2)])
def test_distinct_erasure_values_repair_layered_and_leave_min_sum_alone(name, transmissions):
    assert U.oracle_decode(name, 1e-6, transmissions, "layered")[2] == 0
    assert U.oracle_decode(name, 1e-6, transmissions, "ms")[2] == 0
    assert U.oracle_decode(name, 0.0, transmissions, "ms")[2] == 0


def test_first_transmission_of_s4_alone_fails_for_every_algorithm():
    for algo in ("layered", "ms", "sp"):
        assert U.oracle_decode("S4", 1e-6, 1, algo)[2] == U.FRAMES, algo


def test_reference_recover_keeps_soft_sums_exact():
    """soft after tx1 + tx2 holds plain sums: erasure values and fill values never enter it."""
    spec = U.scenario_spec(1e-6)
    (k1, E1, _, rx1), (k2, E2, _, rx2) = U.received("S4")[0]
    s1, y1 = ref.recover(spec, rx1, k1, E1)
    s2, y2 = ref.recover(spec, rx2, k2, E2, s1)
    assert (s1[:, :U.P] == 0).all() and (y1[:, :U.P] > 0).all() and (y1[:, :U.P] < 2e-6).all()
    assert (s2[:, U.FILLER[0]:U.FILLER[1]] == 0).all() and (y2[:, U.FILLER[0]:U.FILLER[1]] == 10).all()
    i1, i2 = ref.index(spec, k1, E1), ref.index(spec, k2, E2)
    assert np.intersect1d(i1, i2).size == 0 and (np.diff(i2) > 0).all()        # two disjoint, unwrapped windows
    assert np.array_equal(s2[:, i1].view(np.uint32), s1[:, i1].view(np.uint32))
    assert np.array_equal(s2[:, i2].view(np.uint32), (np.float32(0) + rx2).view(np.uint32))


def test_coder_exports_set_rate_match(built):
    import os
    import subprocess
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "myldpccppapi_amd", "libmyldpc.so")
    syms = subprocess.run("nm -D --defined-only %s | c++filt" % so, shell=True, capture_output=True, text=True).stdout
    assert "Coder::setRateMatch(int, int, int, int, int, float)" in syms
