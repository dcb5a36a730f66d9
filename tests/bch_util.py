"""Shared set-up of the outer-code tests: the shapes, the program of tests/cpp/coder_outer_bch.cpp, one bch_ref.Code per
shape (its bit matrices are built once per process), the damaged batches of the decode test, and the chain scenario -- the WiMAX (2304, 1152) code carrying the
BCH(n = 1152, t = 8) code over GF(2^14) (r = 112, k = 1040) through 96 frames at sd = 0.74 with a round budget so short
that the decoder leaves clean frames, frames with a few wrong bits and frames with many.  Everything here comes from
bch_ref, codes.py and the oracle, never from the library under test; arrays are handed out read-only."""
import functools
import os
import subprocess

import numpy as np

import oracle
from oracle.gf2_encoder import Gf2Encoder
from myldpccppapi_amd import codes

import bch_ref

#: one primitive polynomial per degree (each is checked by test_bch_cpu)
PRIM = {4: 0x13, 5: 0x25, 6: 0x43, 7: 0x89, 8: 0x11D, 9: 0x211, 10: 0x409, 11: 0x805, 12: 0x1053, 13: 0x201B, 14: 0x402B,
        15: 0x8003, 16: 0x1002D}

#: (m, t, n).  The last two have minimal polynomials of degree 6 and 7: registers whose modulus is shifted furthest.
SHAPES = [(8, 3, 248), (10, 4, 1000), (14, 12, 7200), (16, 12, 32400), (16, 8, 58320), (6, 4, 56), (7, 8, 120)]


def coder_outer_bch_exe(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "coder_outer_bch")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "coder_outer_bch.cpp"), "-o", exe,
                           "-L" + os.path.join(root, "myldpccppapi_amd"), "-lmyldpc", "-lldpc_hip",
                           "-Wl,-rpath," + os.path.join(root, "myldpccppapi_amd")])
    return exe


def shape_id(s):
    return "m%d_t%d_n%d" % s


@functools.lru_cache(maxsize=None)
def ref_code(shape, extra=0):
    m, t, n = shape
    c = bch_ref.Code(n, t, row_bytes=n // 8 + extra, m=m, prim=PRIM[m])
    assert c.valid
    return c


def flip(rows, f, bit):
    rows[f, bit >> 3] ^= np.uint8(1 << (bit & 7))


def damaged(code, frames, seed, all_dirty=False):
    """(payload, clean rows, damaged rows).  Frame f gets weight (0, 1, t, t + 1, 3t)[f % 5] (all_dirty: weight
    1 .. t only), at random places plus, frame after frame, the places where the walk can go wrong: bit 0, bit n - 1,
    both sides of a byte boundary, both sides of the boundary between two lanes' runs of n / 8 bytes, inside the parity."""
    rng = np.random.default_rng(seed)
    n, t, k = code.n, code.t, code.k
    payload = rng.integers(0, 256, (frames, k // 8), dtype=np.uint8)
    rows = code.encode(payload)
    bad = rows.copy()
    run = 8 * ((n // 8 + 63) // 64)                      # bits of a lane's run in the decoder's walk
    runk = 8 * ((k // 8 + 63) // 64)
    special = [[0], [n - 1], [7, 8], [15, 16], [min(run, n - 1) - 1, min(run, n - 1)], [min(2 * run, n - 1) - 1],
               [k, n - 2], [k - 1, k], [min(runk, k - 1)], [0, n - 1]]
    weights = (0, 1, t, t + 1, 3 * t)
    for f in range(frames):
        w = 1 + (f % t) if all_dirty else weights[f % 5]
        if w == 0:
            continue
        want = [b for b in special[(f // 5) % len(special)] if 0 <= b < n][:w]
        pos = set(want)
        while len(pos) < min(w, n):
            pos.add(int(rng.integers(0, n)))
        for b in pos:
            flip(bad, f, b)
    if code.row_bytes > n // 8:                          # garbage behind bit n
        bad[:, n // 8:] = rng.integers(0, 256, (frames, code.row_bytes - n // 8), dtype=np.uint8)
    for a in (payload, rows, bad):
        a.setflags(write=False)
    return payload, rows, bad


@functools.lru_cache(maxsize=None)
def decode_case(shape, extra, frames, seed, all_dirty=False):
    """(payload, rows, damaged rows, expected payload, expected status) of bch_ref.Code.decode."""
    code = ref_code(shape, extra)
    payload, rows, bad = damaged(code, frames, seed, all_dirty)
    want_payload, want_status = code.decode(bad)
    want_payload.setflags(write=False)
    want_status.setflags(write=False)
    return payload, rows, bad, want_payload, want_status


# ---- the chain scenario ------------------------------------------------------------------------------------------
RATE, N, T, FRAMES, SD, PAYLOAD_SEED, NOISE_SEED = codes.RATE_1_2, 2304, 8, 96, 0.74, 600, 601
#: algo -> max_iter: a round budget at which all three kinds of frame occur
BUDGET = {"ms": 4, "layered": 3}


@functools.lru_cache(maxsize=None)
def chain_graph():
    K, M, z = codes.wimax_dims(RATE, N)
    rows, cols = codes.wimax_edges(RATE, N)
    return K, M, z, rows, cols


@functools.lru_cache(maxsize=None)
def chain_code():
    K = chain_graph()[0]
    c = bch_ref.Code(K, T)
    assert c.valid and (c.m, c.r, c.k) == (14, 112, 1040)
    return c


@functools.lru_cache(maxsize=None)
def chain_sent():
    """(payload uint8 [96, 130], source rows uint8 [96, 144], code bits uint8 [96, N], y float32 [96, N])."""
    K, M, z, rows, cols = chain_graph()
    payload = np.random.default_rng(PAYLOAD_SEED).integers(0, 256, (FRAMES, chain_code().k // 8), dtype=np.uint8)
    src = chain_code().encode(payload)
    ge = Gf2Encoder(rows, cols, M, N)
    packed = np.stack([np.frombuffer(ge.encode_bytes(src[f].tobytes()), np.uint8) for f in range(FRAMES)])
    bits = np.unpackbits(packed, axis=1, bitorder="little")
    y = oracle.awgn(N, 0, FRAMES, SD, seed=NOISE_SEED, codewords=bits)
    for a in (payload, src, bits, y):
        a.setflags(write=False)
    return payload, src, bits, y


@functools.lru_cache(maxsize=None)
def chain_oracle(algo):
    """(decoded bytes uint8 [96, 144] of oracle.decode, residual bit errors per frame, expected payload, status, tally)."""
    K, M, z, rows, cols = chain_graph()
    payload, src, bits, y = chain_sent()
    og = oracle.Graph(rows, cols, M, N, K)
    out = np.asarray(oracle.decode(og, y, algo, max_iter=BUDGET[algo], layer_rows=z)["out"], np.uint8).reshape(FRAMES, K // 8)
    residual = np.unpackbits(out ^ src, axis=1).sum(axis=1)
    want_payload, want_status = chain_code().decode(out)
    for a in (out, residual, want_payload, want_status):
        a.setflags(write=False)
    return out, residual, want_payload, want_status, bch_ref.tally(want_status, want_payload, payload)
