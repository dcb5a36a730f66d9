"""Ordered-statistics decoding without a GPU: the numpy restatement (tests/osd_ref.py) held to the rule by hand on the
Hamming code, by an independent construction of the free set from a generator matrix, and by enumeration of all codewords
on small codes; its properties on WiMAX frames and on the edge cases; the premise of the feature and of the GPU cases; the
bindings' refusals that precede device use; csrc/osd_host.hpp under the host sanitizers.  Every test prints its counts."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib

import osd_cases as OC
import osd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ---- helpers that share nothing with osd_ref ------------------------------------------------------------------------------

def gf2_rank(rows):
    """rank of a list of integers read as bit vectors"""
    basis = {}                                          # leading bit -> vector
    for v in rows:
        while v:
            top = v.bit_length()
            if top not in basis:
                basis[top] = v
                break
            v ^= basis[top]
    return len(basis)


def generator(H):
    """uint8 [k, N]: a basis of the null space of H, by an elimination of its own (column pivots from the left)"""
    A = H.copy().astype(np.uint8)
    M, N = A.shape
    piv, r = [], 0
    for c in range(N):
        rows = [i for i in range(r, M) if A[i, c]]
        if not rows:
            continue
        A[[r, rows[0]]] = A[[rows[0], r]]
        for i in range(M):
            if i != r and A[i, c]:
                A[i] ^= A[r]
        piv.append(c)
        r += 1
        if r == M:
            break
    free = [c for c in range(N) if c not in piv]
    G = np.zeros((len(free), N), np.uint8)
    for k, c in enumerate(free):
        G[k, c] = 1
        for i, p in enumerate(piv):
            G[k, p] = A[i, c]
    assert not ((H.astype(int) @ G.T.astype(int)) & 1).any()
    return G


def column_int(G, n):
    return int("".join(map(str, G[:, n])), 2) if G.shape[0] else 0


def all_codewords(G):
    k = G.shape[0]
    msgs = np.array(list(itertools.product((0, 1), repeat=k)), np.int64).reshape(-1, k)
    return ((msgs @ G.astype(np.int64)) & 1).astype(np.uint8)


def is_codeword(H, c):
    return not ((H.astype(np.int64) @ np.asarray(c, np.int64)) & 1).any()


# ---- by hand ----------------------------------------------------------------------------------------------------------------

def test_hamming_by_hand():
    """H: row 0 = {0, 2, 4, 6}, row 1 = {1, 2, 5, 6}, row 2 = {3, 4, 5, 6}; scale 4.

    A: p = (2, -.5, 1, 3, .25, 1.5, 2.5): w = (8, 2, 4, 12, 1, 6, 10), h = 0100000.  Order 4, 1, 2, 5, 0, 6, 3.  Columns
       4 = (1,0,1), 1 = (0,1,0), 2 = (1,1,0) are independent: P = {4, 1, 2}, F = {0, 3, 5, 6}.  h is 0 on F, so c0 = 0 and
       D0 = w_1 = 2; every flip costs at least its own w_j >= 6: c0 stays.
    B: p = (.25, .3, -.25, 2.25, 2.3, 2.4, 2.45): w = (1, 1, 1, 9, 9, 9, 9), h = 0010000.  Order 0, 1, 2, 3, ..; column 2 is
       column 0 + column 1, so P = {0, 1, 3}, F = {2, 4, 5, 6}.  c0 has c2 = 1, so c0 = c1 = 1, c3 = 0: c0 = 1110000,
       D0 = w_0 + w_1 = 2.  Flipping position 2 gives the zero word at D = w_2 = 1 < 2: the flip wins.
    C: as B with p_2 = -.5: w_2 = 2, the flip costs 2 = D0: a tie, c0 wins."""
    H = OC.HAMMING
    a = osd_ref.frame(H, np.array([2, -.5, 1, 3, .25, 1.5, 2.5], f32), 4.0)
    assert list(a["w"]) == [8, 2, 4, 12, 1, 6, 10] and list(a["h"]) == [0, 1, 0, 0, 0, 0, 0]
    assert list(a["P"]) == [4, 1, 2] and list(a["F"]) == [0, 3, 5, 6]
    assert not a["c0"].any() and a["D0"] == 2 and a["flip"] == -1 and a["D1"] == 2
    b = osd_ref.frame(H, np.array([.25, .3, -.25, 2.25, 2.3, 2.4, 2.45], f32), 4.0)
    assert list(b["w"]) == [1, 1, 1, 9, 9, 9, 9] and list(b["P"]) == [0, 1, 3] and list(b["F"]) == [2, 4, 5, 6]
    assert list(b["c0"]) == [1, 1, 1, 0, 0, 0, 0] and b["D0"] == 2 and b["flip"] == 2 and b["D1"] == 1 and not b["c1"].any()
    c = osd_ref.frame(H, np.array([.25, .3, -.5, 2.25, 2.3, 2.4, 2.45], f32), 4.0)
    assert list(c["P"]) == [0, 1, 3] and list(c["c0"]) == [1, 1, 1, 0, 0, 0, 0] and c["D0"] == 2 and c["flip"] == -1
    r = osd_ref.run(H, np.stack([[2, -.5, 1, 3, .25, 1.5, 2.5], [.25, .3, -.25, 2.25, 2.3, 2.4, 2.45], [.25, .3, -.5, 2.25, 2.3, 2.4, 2.45],
                                 [1, 1, 1, 1, 1, 1, 1]]).astype(f32), 1, 4.0)
    print("hamming: status", list(r["status"]), "metric", list(r["metric"]))
    assert list(r["status"]) == [1, 2, 1, 0] and list(r["metric"]) == [2, 1, 2, 0]


# ---- the basis, independently ---------------------------------------------------------------------------------------------

def test_free_set_is_the_most_reliable_basis_of_a_generator():
    """F is the set a greedy scan from the MOST reliable end picks as independent columns of a generator matrix (the
    matroid dual of the least reliable basis of H), the generator coming from an elimination of its own."""
    rng = np.random.default_rng(2026)
    dirty = 0
    for trial in range(40):
        N = int(rng.integers(24, 41))
        M = int(rng.integers(8, N - 6))
        H = OC.random_h(M, N, seed=trial)
        if trial % 5 == 0:
            H[M - 1] = H[0] ^ H[1]                       # a dependent row
        G = generator(H)
        p = (np.round(rng.normal(1.0, 1.2, N) * 4) / 4).astype(f32)        # many equal weights
        r = osd_ref.frame(H, p, 4.0)
        if r["clean"]:
            continue
        dirty += 1
        order = osd_ref.order_of(osd_ref.weights(p, 4.0))
        picked, vecs = [], []
        for n in order[::-1]:
            v = column_int(G, n)
            if gf2_rank(vecs + [v]) > len(vecs):
                vecs.append(v)
                picked.append(int(n))
        assert sorted(picked) == list(r["F"]) and len(r["P"]) == N - G.shape[0]
    print("basis: %d dirty frames of 40 checked" % dirty)
    assert dirty >= 30


# ---- the choice, independently --------------------------------------------------------------------------------------------

def test_choice_against_all_codewords():
    """On codes with K <= 10: among all 2^K codewords, those that differ from h on F in at most `order` positions; the
    smallest D wins, on a tie c0 (no difference on F), then the smallest differing position."""
    rng = np.random.default_rng(7)
    counts = np.zeros(3, int)
    ties = 0
    for trial in range(60):
        N = int(rng.integers(12, 21))
        k = int(rng.integers(3, 11))
        H = OC.random_h(N - k, N, seed=1000 + trial)
        words = all_codewords(generator(H))
        p = (np.round(rng.normal(0.6, 1.0, N) * 2) / 2).astype(f32)        # coarse: ties are common
        r = osd_ref.frame(H, p, 2.0)
        if r["clean"]:
            counts[0] += 1
            continue
        h, w, F = r["h"], r["w"], r["F"]
        diff = words[:, F] != h[F]
        for order in (0, 1):
            best = None
            for c, d in zip(words[diff.sum(axis=1) <= order], diff[diff.sum(axis=1) <= order]):
                key = (int(w[c != h].sum()), int(F[np.flatnonzero(d)[0]]) if d.any() else -1)
                if best is None or key < best[0]:
                    best = (key, c)
            got = (r["c0"], r["D0"], -1) if order == 0 or r["flip"] < 0 else (r["c1"], r["D1"], r["flip"])
            assert np.array_equal(got[0], best[1]) and (got[1], got[2]) == best[0], (trial, order)
        counts[1 if r["flip"] < 0 else 2] += 1
        D = [int(w[c != h].sum()) for c in words[diff.sum(axis=1) <= 1]]
        ties += sorted(D)[0] == sorted(D)[1] if len(D) > 1 else 0
    print("choice: clean / c0 / flip = %s, frames whose best two candidates tie: %d" % (counts, ties))
    assert counts[1] >= 5 and counts[2] >= 5 and ties >= 3


# ---- properties -----------------------------------------------------------------------------------------------------------

def check_properties(H, soft, scale, K=None):
    r0, r1 = osd_ref.run(H, soft, 0, scale, K), osd_ref.run(H, soft, 1, scale, K)
    h, w = osd_ref.hard_bits(soft), osd_ref.weights(soft, scale)
    for f in range(soft.shape[0]):
        clean = is_codeword(H, h[f])
        for r in (r0, r1):
            assert is_codeword(H, r["code"][f])
            assert r["metric"][f] == w[f][r["code"][f] != h[f]].sum()
            assert (r["status"][f] == 0) == clean
            if clean:
                assert np.array_equal(r["code"][f], h[f]) and r["metric"][f] == 0
        assert r0["status"][f] in (0, 1) and r1["metric"][f] <= r0["metric"][f]
        assert (r1["status"][f] == 2) == (r1["metric"][f] < r0["metric"][f])
    return np.bincount(r1["status"], minlength=3)


def test_properties_on_wimax_frames():
    c = OC.code(OC.WIMAX_HALF)
    soft = OC.noisy(OC.WIMAX_HALF, 200, (0.27, 0.8), seed=200)
    counts = check_properties(c["H"], soft, OC.SCALE, c["K"])
    print("properties: clean / c0 / flip =", counts)
    assert counts.min() >= 10


@pytest.mark.parametrize("kind", ["ties", "specials", "all_clean", "all_dirty"])
def test_edge_case_rows(kind):
    c = OC.code(OC.WIMAX_HALF)
    soft, scale = OC.synthetic(kind)
    counts = check_properties(c["H"], np.array(soft), scale, c["K"])
    print(kind, "clean / c0 / flip =", counts)
    if kind == "all_clean":
        assert counts[0] == soft.shape[0]
    if kind == "all_dirty":
        assert counts[0] == 0
    if kind == "ties":
        w = osd_ref.weights(soft, scale)
        assert w.max() <= 12 and all(np.unique(row).size <= 13 for row in w)


def test_special_values():
    w = osd_ref.weights(np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 300.0, 255.99, -256.0, 1e-40, 65535.0 / 256, -3.4e38, 1.0 / 512], f32), 256.0)
    assert list(w) == [0, 0, 0, 65535, 65535, 65535, 65533, 65535, 0, 65535, 65535, 0]
    assert list(osd_ref.hard_bits(np.array([0.0, -0.0, np.nan, -np.inf, np.inf, -1e-40], f32))) == [0, 0, 0, 1, 0, 1]
    soft, scale = OC.synthetic("specials")
    r = OC.want(OC.WIMAX_HALF, "specials", 1)
    assert r["status"][5] == 0 and not r["code"][5].any()                  # all NaN: h = 0, clean
    assert r["status"][6] > 0                                               # all ones is no codeword of this H
    # one confident one among zeros: the zero-weight pivots follow it at no cost
    assert r["status"][7] == 1 and r["code"][7][3] == 1 and r["metric"][7] == 0


@pytest.mark.parametrize("name", ["deficient", "n100"])
def test_odd_shapes(name):
    c = OC.code(name)
    H = c["H"]
    rank = gf2_rank([int("".join(map(str, row)), 2) for row in H])
    soft = np.array(OC.shape_rows(name, 12, seed=len(name)))
    counts = check_properties(H, soft, OC.SCALE, c["K"])
    for f in range(soft.shape[0]):
        r = osd_ref.frame(H, soft[f], OC.SCALE)
        if not r["clean"]:
            assert len(r["P"]) == rank and len(r["F"]) == c["N"] - rank
    print(name, "M", c["M"], "rank", rank, "clean / c0 / flip =", counts)
    assert counts[1] + counts[2] >= 3 and (name != "deficient" or rank <= c["M"] - 2)


# ---- premises ---------------------------------------------------------------------------------------------------------------

def test_premise_of_the_feature():
    """WiMAX (576, 288), 600 frames at 2.0 dB, 20 rounds of flooding BP: ordered statistics repair frames BP leaves wrong.
    Measured: 28 / 11 / 8 frame errors (BP alone, + order 0, + order 1)."""
    import bp_cases
    import bp_ref
    from ms_correction_ref import Code
    c = OC.code(OC.WIMAX_HALF)
    y, sd = bp_cases.wimax_frames(576, 600, 2.0, seed=5)
    w = bp_ref.flood(Code(c["rows"], c["cols"], c["M"], c["N"], c["K"]), y, 20, llr_scale=2.0 / (sd * sd))
    post = w["post"]
    bp = int(osd_ref.hard_bits(post).any(axis=1).sum())
    e0 = int(osd_ref.run(c["H"], post, 0, OC.SCALE)["code"].any(axis=1).sum())
    e1 = int(osd_ref.run(c["H"], post, 1, OC.SCALE)["code"].any(axis=1).sum())
    print("premise: frame errors of 600: BP %d, + OSD-0 %d, + OSD-1 %d" % (bp, e0, e1))
    assert e1 <= e0 < bp


@pytest.mark.parametrize("algo", ["ms", "bp"])
def test_premises_of_the_gpu_decoder_case(algo):
    c = OC.code(OC.WIMAX_HALF)
    st = osd_ref.run(c["H"], OC.decoder_post(algo), 1, OC.SCALE)["status"]
    counts = np.bincount(st, minlength=3)
    print("decoder case", algo, "clean / c0 / flip =", counts)
    assert st.size == 96 and counts[1] + counts[2] >= 12 and counts[1] >= 3 and counts[2] >= 3 and counts[0] >= 20


def test_premises_of_the_gpu_shape_cases():
    for name, frames in (("n100", 12), ("deficient", 12), ("hamming", 16), ("bg1", 8), (OC.WIMAX_LONG, 6), (OC.WIMAX_HIGH, 6)):
        c = OC.code(name)
        st = osd_ref.run(c["H"], OC.shape_rows(name, frames, seed=len(name)), 1, OC.SCALE)["status"]
        print(name, "clean / c0 / flip =", np.bincount(st, minlength=3))
        assert (st > 0).sum() >= 3


@pytest.mark.parametrize("name", sorted(OC.CRAFTED))
def test_premises_of_the_crafted_syndromes(name):
    """Every crafted frame's hard decision has exactly the unsatisfied checks it was made for, every one is processed, and
    the frames made of pairs are those a flag pass would lose that XORed the parities of the rows m, m + 256, m + 512 ..
    one lane owns before asking whether any is odd."""
    c = OC.code(name)
    soft, sets = OC.crafted(name)
    syn = osd_ref.syndrome(c["H"], osd_ref.hard_bits(soft)).T
    lost = 0
    for f, rows in enumerate(sets):
        assert sorted(np.flatnonzero(syn[f])) == sorted(rows)
        folded = np.zeros(OC.FLAG_LANES, np.int64)
        np.add.at(folded, np.arange(c["M"]) % OC.FLAG_LANES, syn[f])
        lost += not (folded & 1).any()
    st = OC.crafted_want(name, 1)["status"]
    print(name, "crafted frames", len(sets), "that cancel lane by lane", lost, "beyond row 255 alone",
          sum(len(r) == 1 and r[0] >= 256 for r in sets), "status", list(st))
    assert (st > 0).all() and lost >= 3 and any(len(r) == 1 and r[0] >= 256 for r in sets)


# ---- bindings ---------------------------------------------------------------------------------------------------------------

def _graph(name):
    c = OC.code(name)
    return c, L.Graph(c["rows"], c["cols"], c["M"], c["N"])


def test_symbols_are_exported(built):
    lib = _lib.load()
    for name in ("ldpc_osd_create", "ldpc_osd_destroy", "ldpc_osd_device", "ldpc_osd_run", "ldpc_osd_info"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    so = os.path.join(ROOT, "myldpccppapi_amd", "libmyldpc.so")
    syms = subprocess.run("nm -D --defined-only %s | c++filt" % so, shell=True, capture_output=True, text=True).stdout
    assert "Coder::setOsd(int)" in syms


def test_refusals_that_precede_device_use(built):
    """They give their codes on any machine: a handle is made without a device too, and the compute calls check their
    arguments before they ask for one."""
    c, g = _graph(OC.WIMAX_HALF)

    def refused(code, needles, fn):
        with pytest.raises(L.LdpcError) as e:
            fn()
        assert e.value.code == code and all(n in str(e.value) for n in needles), str(e.value)

    refused(1, ["K = 0"], lambda: L.Osd(g, 0))
    refused(1, ["K = 577"], lambda: L.Osd(g, 577))
    refused(1, ["max_frames"], lambda: L.Osd(g, c["K"], max_frames=0))
    big, gb = _graph("wimax_2304_1/2")
    refused(4, ["N = 2304", "82944", "28672", "4096"], lambda: L.Osd(gb, big["K"]))
    osd = L.Osd(g, c["K"], max_frames=8)
    assert osd.info() == dict(M=288, N=576, words_per_row=18, lds_bytes=osd.info()["lds_bytes"]) and 288 * 18 * 4 < osd.info()["lds_bytes"] <= 160 * 1024 - 512
    soft, out = np.zeros((9, c["N"]), f32), np.zeros(9 * c["K"] // 8, np.uint8)
    st = np.zeros(9, np.int32)
    args = lambda **kw: dict(dict(soft_ptr=soft.ctypes.data, frames=4, order=1, weight_scale=256.0, out_ptr=out.ctypes.data, out_nbytes=out.size), **kw)
    refused(1, ["order = 2"], lambda: osd.run_device(**args(order=2)))
    refused(1, ["order = -1"], lambda: osd.run_device(**args(order=-1)))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(1, ["weight_scale"], lambda: osd.run_device(**args(weight_scale=bad)))
    refused(1, ["frames = 9", "max_frames = 8"], lambda: osd.run_device(**args(frames=9)))
    refused(1, ["frames = -1"], lambda: osd.run_device(**args(frames=-1)))
    refused(1, ["out_bytes"], lambda: osd.run_device(**args(out_nbytes=4 * c["K"] // 8 - 1)))
    refused(1, ["all NULL"], lambda: osd.run_device(**args(out_ptr=None, out_nbytes=0)))
    refused(1, ["overlaps"], lambda: osd.run_device(**args(out_ptr=None, out_nbytes=0, status_ptr=soft.ctypes.data + 8)))
    refused(1, ["aligned"], lambda: osd.run_device(**args(status_ptr=st.ctypes.data + 2)))
    osd.run_device(**args(frames=0))                                        # enqueues nothing: no device is asked for
    # K % 8 != 0: every output but the packed one
    c7, g7 = _graph("hamming")
    o7 = L.Osd(g7, 4)
    s7 = np.zeros((2, 7), f32)
    refused(1, ["K % 8"], lambda: o7.run_device(s7.ctypes.data, 2, 1, 256.0, out.ctypes.data, 8))
    if L.device_count() == 0:
        refused(2, ["no usable HIP device"], lambda: osd.run_device(**args()))
        refused(2, ["no usable HIP device"], lambda: osd.run(soft))
    for h in (osd, o7, g, gb, g7):
        h.close()


def test_coder_refusals(built, tmp_path):
    """tests/cpp/coder_osd.cpp, the parts that need no device: orders that are not built, setRateMatch, DecodeSP and
    DecodeCPU, a code beyond the LDS limit with both numbers in the message"""
    import coder_osd_harness as H
    H.run_host(tmp_path)


def test_osd_host_unit_under_host_sanitizers(tmp_path):
    """csrc/osd_host.hpp in a stand-alone program built with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "osd_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "osd_host_test.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
