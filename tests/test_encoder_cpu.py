"""The encoder's host side without a GPU: ldpc_parity_structure on every code family the project builds, its
refusals, the byte arithmetic, argument checks that come before the device is touched, no CPU fall-back, and the
new Coder symbol.  Expected values are derived here from the seed tables, never from the library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, codes, wimax_seeds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _seed_expectation(rate, N):
    """(c, x, a, b) of the weight-3 parity block column, from the seed table and the reference's shift scaling."""
    seed = np.asarray(wimax_seeds.SEEDS[rate])
    z = N // wimax_seeds.NB
    mb = seed.shape[0]
    kb = wimax_seeds.NB - mb
    scale = (lambda p: p % z) if rate == codes.RATE_2_3_A else (lambda p: p * z // wimax_seeds.Z0)
    at = [i for i in range(mb) if seed[i, kb] >= 0]
    assert len(at) == 3 and at[0] == 0 and at[2] == mb - 1
    assert scale(int(seed[0, kb])) == scale(int(seed[mb - 1, kb]))
    return mb, at[1], scale(int(seed[0, kb])), scale(int(seed[at[1], kb]))


@pytest.mark.parametrize("N", [576, 648, 2304, 64800])
@pytest.mark.parametrize("rate", range(6))
def test_parity_structure_of_the_six_seeds(built, rate, N):
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    ps = L.parity_structure(L.Graph(rows, cols, M, N), K, z)
    c, x, a, b = _seed_expectation(rate, N)
    assert ps == dict(kind="dual_diagonal", c=c, x=x, a=a, b=b, ext_rows=0, z=z)
    if rate == codes.RATE_3_4_B:
        assert ps["a"] == 0 and ps["b"] == 80 * z // 96 and ps["b"] != 0     # the shape the host solve does not take
    else:
        assert ps["b"] == 0


def test_seed_order_of_the_middle_block_row():
    assert [_seed_expectation(r, 576)[1] for r in range(6)] == [5, 4, 6, 3, 2, 1]


@pytest.mark.parametrize("Z", [16, 384])
def test_parity_structure_of_the_bg1_profile(built, Z):
    rows, cols = codes.nr_bg1_profile_edges(Z)
    ps = L.parity_structure(L.Graph(rows, cols, 46 * Z, 68 * Z), 22 * Z, Z)
    assert ps == dict(kind="dual_diagonal", c=4, x=1, a=1 % Z, b=0, ext_rows=42, z=Z)


def test_parity_structure_of_the_dvbs2_profile(built):
    rows, cols = codes.dvbs2_profile_edges(12960, 6480)
    assert int((cols >= 6480).sum()) == 2 * 6480 - 1
    ps = L.parity_structure(L.Graph(rows, cols, 6480, 12960), 6480, 0)
    assert ps["kind"] == "staircase"
    # a circulant size is not needed, and is harmless
    assert L.parity_structure(L.Graph(rows, cols, 6480, 12960), 6480, 360)["kind"] == "staircase"


def _code(exc):
    return exc.value.code


def test_unsupported_structures_are_refused(built):
    K, M, z = codes.wimax_dims(codes.RATE_1_2, 648)
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 648)
    # two parity columns of different blocks swapped: the blocks are no circulants any more
    c2 = cols.astype(np.int64).copy()
    p, q = K + 3, K + 2 * z + 5
    c2[cols == p], c2[cols == q] = q, p
    r2, c2 = codes.row_major(rows, c2)
    with pytest.raises(L.LdpcError) as e:
        L.parity_structure(L.Graph(r2, c2, M, 648), K, z)
    assert _code(e) == 4 and "circulant" in str(e.value)
    g = L.Graph(rows, cols, M, 648)
    for bad_z in (0, 9, 54):
        with pytest.raises(L.LdpcError) as e:
            L.parity_structure(g, K, bad_z)
        assert _code(e) == 4, bad_z
    # a staircase with one edge moved
    rows, cols = codes.dvbs2_profile_edges(12960, 6480)
    r3 = rows.astype(np.int64).copy()
    hit = np.nonzero((cols == 6480 + 100) & (rows == 101))[0]
    assert hit.size == 1
    r3[hit[0]] = 103
    r3, c3 = codes.row_major(r3, cols)
    with pytest.raises(L.LdpcError) as e:
        L.parity_structure(L.Graph(r3, c3, 6480, 12960), 6480, 0)
    assert _code(e) == 4
    # ... and Encoder() says the same before it looks for a device
    with pytest.raises(L.LdpcError) as e:
        L.Encoder(L.Graph(r3, c3, 6480, 12960), 6480)
    assert _code(e) == 4


def test_bad_arguments_are_rejected_before_touching_the_device(built):
    K, M, z = codes.wimax_dims(codes.RATE_1_2, 648)
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 648)
    g = L.Graph(rows, cols, M, 648)
    for bad_k in (0, K - 8, K + 1, 648):
        with pytest.raises(L.LdpcError) as e:
            L.parity_structure(g, bad_k, z)
        assert _code(e) == 1, bad_k
        with pytest.raises(L.LdpcError) as e:
            L.Encoder(g, bad_k, z)
        assert _code(e) == 1, bad_k
    for bad_frames in (0, -3):
        with pytest.raises(L.LdpcError) as e:
            L.Encoder(g, K, z, max_frames=bad_frames)
        assert _code(e) == 1
    lib = _lib.load()
    # an unknown format is named before anything else is looked at
    assert lib.ldpc_encode_device(None, None, 0, 0, None, 0, 7, None) == 1
    assert b"format" in lib.ldpc_last_error()
    assert lib.ldpc_encode_device(None, None, 0, 0, None, 0, 1, None) == 1
    assert lib.ldpc_encode(None, None, 0, None, 0) == 1
    out = (ctypes.c_int32 * 8)()
    assert lib.ldpc_parity_structure(None, K, z, out) == 1
    assert lib.ldpc_encoder_destroy(None) == 0


def test_code_bytes(built):
    assert L.code_bytes(648, 70, "packed") == 70 * 81
    assert L.code_bytes(648, 70, "bits") == 70 * 648
    assert L.code_bytes(64800, 4096, "bits") == 4096 * 64800
    assert L.code_bytes(652, 3, "bits") == 3 * 652
    assert L.code_bytes(652, 3, "packed") == 0          # packed needs whole bytes per frame
    assert L.code_bytes(648, 0, "packed") == 0
    assert L.code_bytes(648, 3, 7) == 0                 # unknown format


def test_no_cpu_fallback_for_the_encoder(built):
    if L.device_count() > 0:
        pytest.skip("a HIP device is present")
    K, M, z = codes.wimax_dims(codes.RATE_1_2, 648)
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 648)
    with pytest.raises(L.LdpcError) as e:
        L.Encoder(L.Graph(rows, cols, M, 648), K, z)
    assert _code(e) == 2


def test_coder_exports_set_encode_on_device(built):
    so = os.path.join(ROOT, "myldpccppapi_amd", "libmyldpc.so")
    syms = subprocess.run("nm -D --defined-only %s | c++filt" % so, shell=True, capture_output=True, text=True).stdout
    assert "Coder::setEncodeOnDevice(bool)" in syms
