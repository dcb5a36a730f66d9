"""The dense encoder's host side without a GPU: the systematic column order, the analysis behind LDPC_PARITY_DENSE and its
refusals, the solve matrix T, argument checks that come before the device, no CPU fall-back, the new symbols.
Expected values come from the numpy elimination of dense_encoder_util, never from the library.  Everything is GF(2):
every comparison is exact."""
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, codes

import dense_encoder_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _code(exc):
    return exc.value.code


@pytest.fixture(scope="module")
def mats(built):
    """name -> dict(rows, cols, M, N, H, perm, rank, rows2, cols2, H2): the matrix, numpy's order, the re-ordered matrix."""
    out = {}
    for name, make in (("R", U.matrix_r), ("G", U.matrix_g)):
        rows, cols, M, N = make()
        H = U.dense(rows, cols, M, N)
        perm, rank = U.systematic_order(H)
        rows2, cols2 = codes.permute_columns(rows, cols, perm)
        out[name] = dict(rows=rows, cols=cols, M=M, N=N, H=H, perm=perm, rank=rank, rows2=rows2, cols2=cols2,
                         H2=U.dense(rows2, cols2, M, N))
    return out


def test_the_generators_make_the_matrices_the_tests_are_about(mats):
    R, G = mats["R"], mats["G"]
    assert (R["H"].sum(axis=0) == 3).all()
    assert U.rank(R["H"]) == 100 and U.rank(R["H"][:, 100:]) == 92
    assert (G["H"].sum(axis=0) == 3).all() and (G["H"].sum(axis=1) == 6).all()
    assert U.rank(G["H"]) == 100
    # the re-ordered matrix is the old one with its columns moved: column perm[i] of H is column i of H'
    for m in (R, G):
        assert np.array_equal(m["H2"], m["H"][:, m["perm"]])


@pytest.mark.parametrize("name", ["R", "G"])
def test_systematic_order_equals_the_numpy_elimination(mats, name):
    m = mats[name]
    perm, rank = L.systematic_order(L.Graph(m["rows"], m["cols"], m["M"], m["N"]))
    assert rank == m["rank"] == 100
    assert np.array_equal(perm, m["perm"])
    assert not np.array_equal(perm, np.arange(m["N"]))
    # the rule's shape: both halves ascend, and the order of the re-ordered matrix is the identity
    K = m["N"] - rank
    assert (np.diff(perm[:K]) > 0).all() and (np.diff(perm[K:]) > 0).all()
    again, rank2 = L.systematic_order(L.Graph(m["rows2"], m["cols2"], m["M"], m["N"]))
    assert rank2 == rank and np.array_equal(again, np.arange(m["N"]))


@pytest.mark.parametrize("rate", range(6))
def test_systematic_order_is_the_identity_on_the_six_seeds(built, rate):
    K, M, z = codes.wimax_dims(rate, 576)
    rows, cols = codes.wimax_edges(rate, 576)
    perm, rank = L.systematic_order(L.Graph(rows, cols, M, 576))
    assert rank == M and np.array_equal(perm, np.arange(576))


def test_systematic_order_is_the_identity_on_the_dvbs2_profile(built):
    """The whole (12960, 6480) matrix: 6480 x 12960 = 84.0 M bits, under the 2^27 = 134.2 M bit limit, not truncated."""
    rows, cols = codes.dvbs2_profile_edges(12960, 6480)
    perm, rank = L.systematic_order(L.Graph(rows, cols, 6480, 12960))
    assert rank == 6480 and np.array_equal(perm, np.arange(12960))


def test_systematic_order_limit(built):
    M, N = 8192, 16385            # one column over 2^27 bits; an identity-shaped edge list is enough
    g = L.Graph(np.arange(M), np.arange(M), M, N)
    with pytest.raises(L.LdpcError) as e:
        L.systematic_order(g)
    assert _code(e) == 4 and str(M * N) in str(e.value)


def test_dense_parity(mats):
    R, G = mats["R"], mats["G"]
    with pytest.raises(L.LdpcError) as e:
        L.dense_parity(L.Graph(R["rows"], R["cols"], 100, 200), 100)
    assert _code(e) == 4 and "singular" in str(e.value) and "92" in str(e.value)
    # ... and the C entry point has filled in what it computed
    out = (ctypes.c_int64 * 4)()
    assert _lib.load().ldpc_parity_dense(L.Graph(R["rows"], R["cols"], 100, 200)._h, 100, out) == 4
    assert list(out) == [100, 92, 100, 2]
    assert L.dense_parity(L.Graph(R["rows2"], R["cols2"], 100, 200), 100) == dict(rho=100, rank_hp=100, M=100, t_words=2)
    g2 = L.Graph(G["rows2"], G["cols2"], 102, 204)
    assert L.dense_parity(g2, 104) == dict(rho=100, rank_hp=100, M=102, t_words=2)
    with pytest.raises(L.LdpcError) as e:
        L.dense_parity(g2, 102)
    assert _code(e) == 4 and "singular" in str(e.value) and "100 of 102" in str(e.value)


def test_information_bits_that_are_not_free(mats):
    """R' plus a row with a single one in information column 0: rank(H_p) = rho = 100 but rank(H) = 101."""
    R = mats["R"]
    rows = np.concatenate([R["rows2"], [100]])
    cols = np.concatenate([R["cols2"], [0]])
    H = U.dense(rows, cols, 101, 200)
    assert U.rank(H[:, 100:]) == 100 and U.rank(H) == 101
    g = L.Graph(rows, cols, 101, 200)
    with pytest.raises(L.LdpcError) as e:
        L.dense_parity(g, 100)
    assert _code(e) == 4 and "not free" in str(e.value)
    with pytest.raises(L.LdpcError) as e:
        L.DenseEncoder(g, 100)
    assert _code(e) == 4


def _t_in_two_calls(g, K, rho):
    return np.concatenate([L.dense_parity_rows(g, K, 0, 64), L.dense_parity_rows(g, K, 64, rho - 64)])


@pytest.mark.parametrize("name", ["R", "G", "W648s"])
def test_solve_matrix_inverts_the_parity_part(mats, name):
    if name == "W648s":
        rows, cols, M, N = U.matrix_w648s()
        K, H = 324, U.dense(rows, cols, M, N)
        assert M == 5 * 64 + 4
    else:
        m = mats[name]
        rows, cols, M, N, H = m["rows2"], m["cols2"], m["M"], m["N"], m["H2"]
        K = N - m["rank"]
    rho = N - K
    g = L.Graph(rows, cols, M, N)
    T = U.t_bits(_t_in_two_calls(g, K, rho), M)
    assert T.shape == (rho, M)
    assert np.array_equal((T.astype(np.int64) @ H[:, K:].astype(np.int64)) & 1, np.eye(rho, dtype=np.int64))
    # and with it the codeword of a random word checks: p = T (H_s u)
    u = np.random.default_rng(3).integers(0, 2, K).astype(np.int64)
    p = (T.astype(np.int64) @ ((H[:, :K].astype(np.int64) @ u) & 1)) & 1
    assert not ((H.astype(np.int64) @ np.concatenate([u, p])) & 1).any()
    lib = _lib.load()
    buf = np.zeros(64 * ((M + 63) // 64), np.uint64)
    assert lib.ldpc_parity_dense_rows(g._h, K, 0, 64, buf.ctypes.data, buf.size - 1) == 1        # words too small
    assert lib.ldpc_parity_dense_rows(g._h, K, 0, 64, buf.ctypes.data, buf.size) == 0
    assert lib.ldpc_parity_dense_rows(g._h, K, rho - 63, 64, buf.ctypes.data, buf.size) == 1     # beyond row rho
    assert lib.ldpc_parity_dense_rows(g._h, K, -1, 2, buf.ctypes.data, buf.size) == 1
    assert lib.ldpc_parity_dense_rows(g._h, K, 0, 64, None, buf.size) == 1


def test_bad_arguments_are_rejected_before_touching_the_device(mats):
    R = mats["R"]
    g = L.Graph(R["rows2"], R["cols2"], 100, 200)
    for bad_k in (-1, 0, 99, 200, 201):
        with pytest.raises(L.LdpcError) as e:
            L.dense_parity(g, bad_k)
        assert _code(e) == 1, bad_k
        with pytest.raises(L.LdpcError) as e:
            L.DenseEncoder(g, bad_k)
        assert _code(e) == 1, bad_k
    for bad_frames in (0, -3):
        with pytest.raises(L.LdpcError) as e:
            L.DenseEncoder(g, 100, max_frames=bad_frames)
        assert _code(e) == 1
    lib = _lib.load()
    out = (ctypes.c_int64 * 4)()
    h = ctypes.c_void_p()
    perm = np.zeros(200, np.int32)
    rank = ctypes.c_int32()
    assert lib.ldpc_parity_dense(None, 100, out) == 1
    assert lib.ldpc_parity_dense(g._h, 100, None) == 1
    assert lib.ldpc_encoder_create_dense(None, 100, 64, 0, ctypes.byref(h)) == 1
    assert lib.ldpc_encoder_create_dense(g._h, 100, 64, 0, None) == 1
    assert lib.ldpc_graph_systematic_order(None, perm.ctypes.data, ctypes.byref(rank)) == 1
    assert lib.ldpc_graph_systematic_order(g._h, None, ctypes.byref(rank)) == 1
    assert lib.ldpc_graph_systematic_order(g._h, perm.ctypes.data, None) == 1
    assert lib.ldpc_parity_dense_rows(None, 100, 0, 1, perm.ctypes.data, 2) == 1


def test_more_than_16384_rows_are_refused_before_any_elimination(built):
    M = 16385
    m = np.arange(M)
    rows = np.concatenate([m, m, m[1:]])
    cols = np.concatenate([m, M + m, M + m[:-1]])          # information column m; staircase parity columns
    rows, cols = codes.row_major(rows, cols)
    g = L.Graph(rows, cols, M, 2 * M)
    t0 = time.perf_counter()
    with pytest.raises(L.LdpcError) as e:
        L.dense_parity(g, M)
    with pytest.raises(L.LdpcError) as e2:
        L.DenseEncoder(g, M)
    took = time.perf_counter() - t0
    for x in (e, e2):
        assert _code(x) == 4 and "16385" in str(x.value) and "16384" in str(x.value)
    assert took < 0.5, took            # an elimination of 16385 rows takes seconds
    # K out of range is named first
    with pytest.raises(L.LdpcError) as e:
        L.dense_parity(g, M - 1)
    assert _code(e) == 1


def test_no_cpu_fallback_for_the_dense_encoder(mats):
    R = mats["R"]
    # the host analysis comes first: a singular input is refused as such even where there is no device ...
    with pytest.raises(L.LdpcError) as e:
        L.DenseEncoder(L.Graph(R["rows"], R["cols"], 100, 200), 100)
    assert _code(e) == 4
    # ... and an encodable one gets as far as the device: without one that is LDPC_ERR_HIP, never a host encoder
    g2 = L.Graph(R["rows2"], R["cols2"], 100, 200)
    if L.device_count() > 0:
        L.DenseEncoder(g2, 100, max_frames=64).close()
        return
    with pytest.raises(L.LdpcError) as e:
        L.DenseEncoder(g2, 100)
    assert _code(e) == 2


def test_the_structured_encoder_still_refuses_unstructured_matrices(mats):
    R = mats["R"]
    g = L.Graph(R["rows2"], R["cols2"], 100, 200)
    with pytest.raises(L.LdpcError) as e:
        L.Encoder(g, 100)
    assert _code(e) == 4
    with pytest.raises(L.LdpcError) as e:
        L.parity_structure(g, 100, 0)
    assert _code(e) == 4


def test_library_exports_the_new_symbols(built):
    so = os.path.join(ROOT, "myldpccppapi_amd", "libldpc_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout.split()
    for name in ("ldpc_graph_systematic_order", "ldpc_parity_dense", "ldpc_parity_dense_rows", "ldpc_encoder_create_dense"):
        assert name in syms, name
    assert _lib.load().ldpc_abi_version() == 3


def test_permute_columns(built):
    rows, cols = np.array([0, 0, 1, 1]), np.array([0, 2, 1, 2])
    r2, c2 = codes.permute_columns(rows, cols, [2, 0, 1])      # column 2 of H becomes column 0
    assert r2.tolist() == [0, 0, 1, 1] and c2.tolist() == [0, 1, 0, 2]
