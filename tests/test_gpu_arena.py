"""The device entry points on offset, guarded and partial buffers.

A caller that keeps encode -> rate match -> channel -> recover -> decode -> count in HBM carves one arena into
sub-buffers at whatever offsets its sizes produce, passes frames < max_batch and reuses one handle for calls of different
sizes.  Here every buffer comes from arena_util.Arena: float buffers at 4 modulo 16, byte buffers at odd addresses, each
exactly as large as the call states, with 0xEE all around.  Results are compared exactly with the references the project
already has (oracle.decode, the host channel, ratematch_ref, Gf2Encoder); the guard bands are the overrun check.

What the variants guard, beyond the bytes themselves:
  - "out NULL": a call with out_dev == NULL still writes iters_dev and the summary on every engine.  The streaming
    flooding, streaming layered and layered-host engines write iters_dev in pack_kernel alone, so their tests are the
    ones that notice a pack launch that depends on out_dev;
  - "refusals": out_bytes < 0, a short LDPC_PACK_BITS buffer and frames > max_batch are LDPC_ERR_ARG and enqueue nothing,
    on every engine;
  - test_awgn_device_at_every_phase: awgn_kernel takes its 16-byte store at 16-byte aligned addresses only.

All N hard bits (dump(3)) are compared with the oracle on the streaming engines only.  The LDS-resident and record
engines decode in one launch and keep the hard bits in LDS: dump() reads them only after set_tap(), and a tap stops the
run at a chosen round, which is another run than the one whose out, iters and stats are checked here.  Their K payload
bits and iteration counts are compared in every variant; their messages under a tap are compared in
test_gpu_kernel_matrix.py."""
import ctypes

import numpy as np
import pytest

import oracle
import myldpccppapi_amd as L
from myldpccppapi_amd import _lib

import arena_cases as ac
from arena_util import Arena, FILL

pytestmark = pytest.mark.gpu
f32 = np.float32
ODD = dict(align=2, phase=1)
F4 = dict(align=16, phase=4)


def _torch():
    import torch
    return torch


def _sync():
    _torch().cuda.synchronize()


_graphs = {}


def _graph(code_name):
    if code_name not in _graphs:
        c = ac.code(code_name)
        _graphs[code_name] = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    return _graphs[code_name]


def _decoder(c):
    cd = ac.code(c["code"])
    return L.Decoder(_graph(c["code"]), cd["K"], max_batch=c["max_batch"], algo=c["algo"], max_iter=ac.MAXIT,
                     layer_rows=cd["z"] if c["layer_rows"] else 0, pack_mode=c["pack"], frames_per_lane=c["V"],
                     poll_interval=c["poll"], msg_dtype="f16" if c["f16"] else "f32", tune=c["tune"])


def _streaming(c):
    """engines whose hard bits dump(3) reads without a tap (see the module docstring), and which report frame_rounds"""
    return not c["kernel"].startswith(("fused_", "layered_ldsp", "flood_ldsp"))


class _Buffers:
    """One arena for one decoder: the call's input at 4 modulo 16 with poisoned rows behind it (and once at 0 modulo 16),
    out at an odd address with exactly the bytes of the largest call, iters at 4 modulo 16."""

    def __init__(self, c, frames=None, aligned_copy=True):
        cd = ac.code(c["code"])
        self.N, self.K, self.pack = cd["N"], cd["K"], c["pack"]
        self.rows = c["max_batch"]
        self.cap = frames or c["frames"]                   # frames of the largest call
        self.need = L.out_bytes(self.K, self.cap, self.pack)
        nb_in = self.rows * self.N * 4
        self.ar = Arena(nb_in + (self.cap * self.N * 4 if aligned_copy else 0) + self.need + self.cap * 4 + 4096)
        self.llr = self.ar.carve(nb_in, name="llr", **F4)
        self.llr0 = self.ar.carve(self.cap * self.N * 4, 16, 0, name="llr (16-byte aligned)") if aligned_copy else None
        self.out = self.ar.carve(self.need, name="out", **ODD)
        self.iters = self.ar.carve(self.cap * 4, name="iters", **F4)
        assert self.llr % 16 == 4 and self.out % 2 == 1 and self.iters % 16 == 4

    def load(self, y):
        """y into the input buffers; every row behind it reads NaN"""
        n = y.shape[0]
        self.ar.put_floats(self.llr, y)
        self.ar.poison(self.llr + n * self.N * 4, (self.rows - n) * self.N)
        if self.llr0 is not None:
            self.ar.put_floats(self.llr0, y)

    def refill(self):
        """a stale byte must not pass for a result"""
        self.ar.fill(self.out, self.need)
        self.ar.fill(self.iters, self.cap * 4)

    def got_out(self, nbytes=None):
        return self.ar.get(self.out, self.need if nbytes is None else nbytes)

    def got_iters(self, n):
        return self.ar.get(self.iters, n, np.int32)


def _check_stats(dec, c, w_iters, w_conv, n, what, tail=False):
    st = dec.stats()
    assert st["frames"] == n, what
    assert st["batch_time"] == int(w_iters.max()), (what, st)
    assert st["frames_converged"] == int(w_conv.sum()), (what, st)
    if c["poll"]:
        # dead lanes of the last tile must not keep the batch alive
        assert st["iterations_launched"] == int(w_iters.max()), (what, st)
    if tail:
        F = 64 * c["V"]
        tiles = -(-n // F)
        full = ac.frame_rounds_without_handover(w_iters, F)
        assert full == st["iterations_launched"] * tiles * F, (what, st)      # every tile keeps a frame to the end ...
        assert 0 < st["frame_rounds"] < full, (what, st)                        # ... and still later rounds ran on fewer
    return st


def _run_variants(c):
    """The variants of one row of the table on one decoder."""
    torch = _torch()
    cd = ac.code(c["code"])
    K, N, n = cd["K"], cd["N"], c["frames"]
    w = ac.case_want(c)
    y = ac.case_inputs(c)
    is_tail = c["kind"] == "tail"
    if is_tail:                     # from the oracle alone, before the GPU is touched
        assert ac.handover_round(w["iters"]) is not None and (w["iters"] == ac.MAXIT).sum() >= 10
    dec = _decoder(c)
    b = _Buffers(c)
    b.load(y)
    need = b.need
    assert need == w["out"].size
    name = c["name"]

    # 1. offset and guarded: the input at 4 modulo 16 (init_kernel's scalar branch) and at 0 modulo 16
    for which, llr in (("phase 4", b.llr), ("phase 0", b.llr0)):
        what = (name, "offset and guarded", which)
        b.refill()
        if which == "phase 4":
            dec.set_timing(True)
        dec.decode_device(llr, n, b.out, need, b.iters)
        _sync()
        if which == "phase 4":
            names = {k["name"] for k in dec.kernel_times()}
            dec.set_timing(False)
            assert any(x.startswith(c["kernel"]) for x in names), (what, names)
        assert np.array_equal(b.got_out(), w["out"]), what
        assert np.array_equal(b.got_iters(n), w["iters"]), what
        if _streaming(c):
            assert np.array_equal(dec.dump(3, n).astype(np.uint8), w["hard"]), what
        _check_stats(dec, c, w["iters"], w["converged"], n, what, tail=is_tail)
        b.ar.assert_untouched(str(what))

    # 2. iters_dev = NULL
    what = (name, "iters NULL")
    b.refill()
    dec.decode_device(b.llr, n, b.out, need, None)
    _sync()
    assert np.array_equal(b.got_out(), w["out"]), what
    b.ar.assert_tail_untouched(b.iters, 0, 4 * n, str(what))
    b.ar.assert_untouched(str(what))

    # 3. out_dev = NULL: iteration counts and stats only
    what = (name, "out NULL")
    b.refill()
    dec.decode_device(b.llr, n, None, 0, b.iters)
    _sync()
    assert np.array_equal(b.got_iters(n), w["iters"]), what
    _check_stats(dec, c, w["iters"], w["converged"], n, what, tail=is_tail)
    b.ar.assert_tail_untouched(b.out, 0, need, str(what))
    b.ar.assert_untouched(str(what))
    # ... and neither: stats only
    what = (name, "out and iters NULL")
    b.refill()
    dec.decode_device(b.llr, n, None, 0, None)
    _sync()
    _check_stats(dec, c, w["iters"], w["converged"], n, what, tail=is_tail)
    b.ar.assert_tail_untouched(b.out, 0, need, str(what))
    b.ar.assert_tail_untouched(b.iters, 0, 4 * n, str(what))
    b.ar.assert_untouched(str(what))

    if c["pack"] == ac.PACK_BYTES:
        # 4. out_bytes cut in the middle of a frame
        cut = need - K // 16 - 1
        what = (name, "out_bytes cut", cut)
        assert 0 < cut < need and cut > ac.frame_byte_index(K, n)[-1, 0]
        b.refill()
        dec.decode_device(b.llr, n, b.out, cut, b.iters)
        _sync()
        assert np.array_equal(b.got_out(cut), w["out"][:cut]), what
        b.ar.assert_tail_untouched(b.out, cut, need, str(what))
        assert np.array_equal(b.got_iters(n), w["iters"]), what
        b.ar.assert_untouched(str(what))
        # 5. K % 8 != 0: the bits between frames read 0 although the buffer held 0xEE
        if K % 8:
            gaps = np.setdiff1d(np.arange(need), ac.frame_byte_index(K, n).reshape(-1))
            assert gaps.size > 0
            b.refill()
            dec.decode_device(b.llr, n, b.out, need, b.iters)
            _sync()
            got = b.got_out()
            assert not got[gaps].any(), (name, "gap bytes")
            assert np.array_equal(got, w["out"]), (name, "gap bytes")

    # 6. refusals enqueue nothing: out and iters of their own, all 0xEE afterwards
    r = Arena(need + 4 * n + 1024)
    r_out = r.carve(need, name="out", **ODD)
    r_iters = r.carve(4 * n, name="iters", **F4)
    refused = [(n, -1), (c["max_batch"] + 1, need)]
    if c["pack"] == ac.PACK_BITS:
        refused.append((n, need - 1))
    for frames, nbytes in refused:
        with pytest.raises(L.LdpcError) as e:
            dec.decode_device(b.llr, frames, r_out, nbytes, r_iters)
        assert e.value.code == 1, (name, "refusal", frames, nbytes)
    _sync()
    r.assert_all_untouched(str((name, "refusals")))
    b.ar.assert_untouched(str((name, "refusals")))
    dec.close()


@pytest.mark.parametrize("tag", ["w576", "w648", "w648b"])
@pytest.mark.parametrize("V", [1, 2, 4])
@pytest.mark.parametrize("algo", ["sp", "ms", "ms16"])
def test_decode_device_streaming_flooding(built, algo, V, tag):
    """sp, ms and ms with fp16 messages through the streaming kernels, 64 V + 5 frames; w648: K % 8 = 4 in
    LDPC_PACK_BYTES, w648b: the same in LDPC_PACK_BITS."""
    _run_variants(ac.CASES["flood_%s_v%d_%s" % (algo, V, tag)])


@pytest.mark.parametrize("V", [1, 4])
def test_decode_device_column_fused_check_launch(built, V):
    _run_variants(ac.CASES["link_ms_v%d" % V])


@pytest.mark.parametrize("code_name", ["w576", "w648"])
@pytest.mark.parametrize("algo", ["layered", "ms", "sp", "ms_fused"])
def test_decode_device_lds_resident(built, algo, code_name):
    _run_variants(ac.CASES["lds_%s_%s" % (algo, code_name)])


@pytest.mark.parametrize("code_name", ["w576", "w648"])
@pytest.mark.parametrize("form", ["packed", "unpacked"])
@pytest.mark.parametrize("algo", ["layered", "ms", "ms_fused"])
def test_decode_device_record_kernels(built, algo, form, code_name):
    """several frames per wave (z <= 32) and one frame per workgroup (ldsp_pack off), a grid of 4 workgroups for 13 frames"""
    _run_variants(ac.CASES["record_%s_%s_%s" % (algo, form, code_name)])


@pytest.mark.parametrize("tag", ["w576", "w648", "w648b"])
@pytest.mark.parametrize("V", [1, 4])
def test_decode_device_streaming_layered(built, V, tag):
    _run_variants(ac.CASES["layered_stream_v%d_%s" % (V, tag)])


def test_decode_device_layered_host(built):
    _run_variants(ac.CASES["layered_host"])


@pytest.mark.parametrize("algo", ["ms", "sp"])
def test_decode_device_polled_tail_compaction(built, algo):
    """300 frames in 5 tiles, polled every round: the child decoder finishes the stragglers"""
    _run_variants(ac.CASES["polled_tail_%s" % algo])


@pytest.mark.parametrize("V", [1, 4])
@pytest.mark.parametrize("algo", ["ms", "sp"])
def test_decode_device_device_side_tail(built, algo, V):
    """2100 frames without polling: the stragglers move to the overflow tiles on the device"""
    _run_variants(ac.CASES["device_tail_%s_v%d" % (algo, V)])


def test_ms_fused_refuses_bit_packing_of_ragged_frames(built):
    cd = ac.code("w648")
    for choice in ("1", "ldsp"):
        with pytest.raises(L.LdpcError) as e:
            L.Decoder(_graph("w648"), cd["K"], max_batch=13, algo="ms_fused", max_iter=ac.MAXIT, layer_rows=cd["z"],
                      pack_mode=ac.PACK_BITS, tune=ac.kernel_choice(choice))
        assert e.value.code == 4


def test_creation_that_fails_late_frees_what_it_took(built):
    """A config that is refused only after the handle has allocated its common arrays: LDPC_ALGO_MS_FUSED on the
    (648, 324) code with one circulant no longer cyclic (two of its rows trade their columns).  32 such creations must
    not cost device memory: the free memory falls by less than one handle's common arrays (S, worked out from the
    shapes below), where a leak would cost 32 S.  The device then still decodes: a valid decoder of the same graph
    against the oracle."""
    torch = _torch()
    cd = ac.code("w648")
    rows, cols, M, N, K, z = np.array(cd["rows"]), np.array(cd["cols"]), cd["M"], cd["N"], cd["K"], cd["z"]
    e0 = int(np.nonzero(rows == 0)[0][0])
    e1 = int([e for e in np.nonzero(rows == 1)[0] if cols[e] // z == cols[e0] // z][0])
    cols[e0], cols[e1] = cols[e1], cols[e0]
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    g = L.Graph(rows, cols, M, N)
    B, max_iter, V = 262144, 100, 4
    F = 64 * V
    T = (B + F - 1) // F
    # hard [T][N][V] words, failw [max_iter + 2][T][V] words, done [T][V] words, iters [T * F] int32
    S = 8 * T * N * V + 8 * (max_iter + 2) * T * V + 8 * T * V + 4 * T * F
    assert 20 * 2 ** 20 < S < 64 * 2 ** 20

    def refused():
        with pytest.raises(L.LdpcError) as e:
            L.Decoder(g, K, max_batch=B, algo="ms_fused", max_iter=max_iter, layer_rows=z, frames_per_lane=V)
        assert e.value.code == 4 and "quasi-cyclic" in str(e.value)

    refused()                               # what the runtime sets up once per process is not counted
    _sync()
    before, _ = torch.cuda.mem_get_info()
    for _ in range(32):
        refused()
    _sync()
    after, _ = torch.cuda.mem_get_info()
    print("free device memory: %d -> %d bytes (S = %d)" % (before, after, S))
    assert before - after < S, (before, after, S)

    y = ac.mix_channel(N, 64, 0.55, 0.95, seed=648)
    ref = oracle.decode(oracle.Graph(rows, cols, M, N, K), y, "ms", max_iter=ac.MAXIT)
    dec = L.Decoder(g, K, max_batch=64, algo="ms", max_iter=ac.MAXIT)
    out, iters = dec.decode(y)
    dec.close()
    assert np.array_equal(out, ref["out"]) and np.array_equal(iters, ref["iters"])


# --------------------------------------------------------------------------- call sequences on one handle

def _sequence(c, calls):
    """calls: (kind, frames, variant) in order; every call takes the last `frames` frames of its input set (so that a
    call of one frame is not always frame 0) and is compared with the oracle's slice."""
    cd = ac.code(c["code"])
    K, N = cd["K"], cd["N"]
    assert K % 8 == 0 and c["pack"] == ac.PACK_BYTES
    kb = K // 8
    cap = max(n for _, n, _ in calls)
    dec = _decoder(c)
    b = _Buffers(c, frames=cap, aligned_copy=False)
    for i, (kind, n, variant) in enumerate(calls):
        what = (c["name"], "call %d" % i, kind, n)
        b.refill()
        if n == 0:
            dec.decode_device(b.llr, 0, b.out, 0, b.iters)
            _sync()
            b.ar.assert_tail_untouched(b.out, 0, b.need, str(what))
            b.ar.assert_tail_untouched(b.iters, 0, 4 * cap, str(what))
            b.ar.assert_untouched(str(what))
            continue
        total = cap if n == cap else max(cap // 2, n)           # the input set the slice comes from
        w = ac.case_want(c, kind=kind, frames=total, variant=variant)
        y = ac.case_inputs(c, kind=kind, frames=total, variant=variant)[total - n:]
        w_out = w["out"].reshape(total, kb)[total - n:].reshape(-1)
        w_iters, w_conv = w["iters"][total - n:], w["converged"][total - n:]
        b.load(y)
        nb = L.out_bytes(K, n)
        dec.decode_device(b.llr, n, b.out, nb, b.iters)
        _sync()
        assert np.array_equal(b.got_out(nb), w_out), what
        assert np.array_equal(b.got_iters(n), w_iters), what
        b.ar.assert_tail_untouched(b.out, nb, b.need, str(what))
        b.ar.assert_tail_untouched(b.iters, 4 * n, 4 * cap, str(what))
        _check_stats(dec, c, w_iters, w_conv, n, what, tail=kind == "tail" and n == cap)
        b.ar.assert_untouched(str(what))
    dec.close()


@pytest.mark.parametrize("name", ["flood_ms_v4_w576", "record_layered_packed_w576", "lds_sp_w576", "layered_stream_v4_w576",
                                  "polled_tail_ms"])
def test_call_sequence_on_one_handle(built, name):
    """max_batch (hard mix), 1, 64 V, 64 V + 1, 0, max_batch (all easy), max_batch (hard mix), 1 on one handle: state a
    larger call leaves (the compaction child, finished tiles, the idle hint) must not reach a smaller next call."""
    c = dict(ac.CASES[name])
    V = max(c["V"], 1)
    mb = c["max_batch"]
    hard = c["kind"]                       # "mix", or "tail" for the polled decoder: other hard frames on every call
    poll = 1 if c["poll"] else 0
    calls = [(hard, mb, 0), (hard, 1, 1 * poll), (hard, 64 * V, 2 * poll), (hard, 64 * V + 1, 3 * poll), (hard, 0, 0),
             ("easy", mb, 0), (hard, mb, 1 * poll), (hard, 1, 2 * poll)]
    _sequence(c, calls)


def test_call_sequence_on_the_device_side_tail(built):
    """2100 (hard mix), 300 (too few tiles for the tail), 2100 (all easy), 2100 (hard mix), 1"""
    c = dict(ac.CASES["device_tail_ms_v4"])
    calls = [("tail", 2100, 0), ("tail", 300, 0), ("easy", 2100, 0), ("tail", 2100, 0), ("tail", 1, 0)]
    _sequence(c, calls)


# --------------------------------------------------------------------------- ldpc_awgn_device

@pytest.mark.parametrize("N,frames", [(576, 5), (67, 33), (2304, 3)])
def test_awgn_device_at_every_phase(built, tmp_path, N, frames):
    """llr_dev at 0, 4, 8 and 12 modulo 16, bits_dev at an odd address: every float the host generator's, bit for bit,
    nothing outside the buffer (N = 67: the last group of four is partial)."""
    from util import host_channel_lib
    lib = host_channel_lib(tmp_path)
    lb = _lib.load()
    stream = _torch().cuda.current_stream().cuda_stream
    bits = np.random.default_rng(N).integers(0, 2, (frames, N)).astype(np.uint8)
    sd, seed = 0.8, 99
    ar = Arena(4 * (frames * N * 4 + 256) + frames * N + 1024)
    pb = ar.carve(frames * N, name="bits", **ODD)
    ar.put(pb, bits)
    for phase in (0, 4, 8, 12):
        p = ar.carve(frames * N * 4, 16, phase, name="llr at %d mod 16" % phase)
        assert p % 16 == phase
        for first in (0, (1 << 33) + 5):
            for with_bits in (False, True):
                what = (N, frames, phase, first, with_bits)
                want = np.empty((frames, N), f32)
                lib.awgn(want.ctypes.data_as(ctypes.c_void_p), frames, N,
                         bits.ctypes.data_as(ctypes.c_void_p) if with_bits else None, sd, seed, first)
                ar.fill(p, frames * N * 4)
                _lib.check(lb.ldpc_awgn_device(p, frames, N, pb if with_bits else None, sd, seed, first, 0, stream))
                _sync()
                got = ar.get(p, frames * N, np.uint32)
                assert np.array_equal(got, want.reshape(-1).view(np.uint32)), what
                ar.assert_untouched(str(what))
    assert np.array_equal(ar.get(pb, frames * N), bits.reshape(-1))


# --------------------------------------------------------------------------- ldpc_count_errors_device

def _count(out_ptr, ref_ptr, frames, per, stream=None):
    res = (ctypes.c_int64 * 3)()
    if stream is None:
        stream = _torch().cuda.current_stream().cuda_stream
    _lib.check(_lib.load().ldpc_count_errors_device(out_ptr, ref_ptr, frames, per, res, 0, stream))
    return int(res[0]), int(res[1]), int(res[2])


def _numpy_count(x):
    """x = out ^ ref, uint8 [frames, per]: (bits, bytes, frames) as test_device_error_count counts them"""
    return int(np.unpackbits(x).sum()), int((x != 0).sum()), int((x != 0).any(axis=1).sum())


@pytest.mark.parametrize("frames", [1, 37])
@pytest.mark.parametrize("per", [1, 63, 255, 256, 257, 1025])
def test_count_errors_device_on_odd_buffers(built, per, frames):
    rng = np.random.default_rng(per * 100 + frames)
    n = frames * per
    ar = Arena(2 * n + 1024)
    po = ar.carve(n, 16, 3, name="out")
    pr = ar.carve(n, 16, 9, name="ref")
    assert po % 2 == 1 and pr % 2 == 1 and po % 16 != pr % 16
    # every byte differs
    ar.put(po, np.full(n, 0xFF, np.uint8))
    ar.put(pr, np.zeros(n, np.uint8))
    assert _count(po, pr, frames, per) == (8 * n, n, frames)
    # a sparse random set of differing bytes, one frame without any where there are several
    a = rng.integers(0, 256, (frames, per)).astype(np.uint8)
    bb = a.copy()
    hit = rng.choice(n, max(1, n // 20), replace=False)
    bb.reshape(-1)[hit] ^= rng.integers(1, 256, hit.size).astype(np.uint8)
    if frames > 5:
        bb[5] = a[5]
    ar.put(po, bb)
    ar.put(pr, a)
    assert _count(po, pr, frames, per) == _numpy_count(a ^ bb)
    # ref = NULL: the all-zero payload
    assert _count(po, None, frames, per) == _numpy_count(bb)
    ar.assert_untouched(str((per, frames)))
    assert np.array_equal(ar.get(po, n), bb.reshape(-1)) and np.array_equal(ar.get(pr, n), a.reshape(-1))


def test_count_errors_follows_a_decode_on_its_stream(built):
    """count enqueued on a non-default stream straight behind a decode_device on that stream, no synchronise between"""
    torch = _torch()
    c = ac.CASES["flood_ms_v1_w576"]
    cd = ac.code(c["code"])
    n, kb = c["frames"], cd["K"] // 8
    w = ac.case_want(c)
    dec = _decoder(c)
    b = _Buffers(c, aligned_copy=False)
    b.load(ac.case_inputs(c))
    b.refill()
    _sync()
    stream = torch.cuda.Stream()
    dec.decode_device(b.llr, n, b.out, b.need, b.iters, stream.cuda_stream)
    got = _count(b.out, None, n, kb, stream.cuda_stream)
    want = _numpy_count(w["out"].reshape(n, kb))
    assert want[2] > 0
    assert got == want
    _sync()
    b.ar.assert_untouched("count behind decode")
    dec.close()


# --------------------------------------------------------------------------- the whole chain in one arena

def test_whole_chain_in_one_arena(built):
    """encode -> match -> channel -> recover (two transmissions, soft-combined) -> layered decode -> count, 70 frames of
    the BG1-profile code at Z = 16 on one non-default stream, every buffer carved from one arena: byte buffers at odd
    addresses, float buffers at 4 modulo 16.  Every stage against its host reference."""
    import ratematch_ref as ref
    import ratematch_util as U
    import encoder_util as EU
    from oracle.gf2_encoder import Gf2Encoder
    torch = _torch()
    frames, N, K, Z = 70, U.N, U.K, U.Z
    kb = K // 8
    rows, cols, og = U.bg1()
    rng = np.random.default_rng(70)
    info = rng.integers(0, 2, (frames, K), dtype=np.uint8)
    info[:, U.FILLER[0]:U.FILLER[1]] = 0
    src = np.packbits(info, axis=1, bitorder="little").reshape(-1)
    ge = Gf2Encoder(rows, cols, U.M, N)
    code_want = np.unpackbits(EU.reference_packed(ge, src, frames), axis=1, bitorder="little")
    spec = U.scenario_spec(1e-6)
    snr, txs = U.SCENARIOS["S4"]
    assert len(txs) == 2 and txs[0] != txs[1]
    sd = 10.0 ** (-snr / 20.0)
    # host references of every stage
    tx_want, rx_want, soft_w, y_w = [], [], None, None
    for t, (k0, E) in enumerate(txs):
        tx_want.append(ref.match(U.scenario_spec(0.0), code_want, k0, E))
        rx_want.append(oracle.awgn(E, 0, frames, sd, seed=100 + t, codewords=tx_want[t]))
        soft_w, y_w = ref.recover(spec, rx_want[t], k0, E, soft_w)
    dw = oracle.decode(og, y_w, "layered", max_iter=U.MAX_ITER, llr_scale=U.LLR_SCALE, layer_rows=Z)
    assert not dw["undefined"].any() and np.unique(dw["iters"]).size >= 2

    g = L.Graph(rows, cols, U.M, N)
    enc = L.Encoder(g, K, Z, max_frames=frames + 7)
    rm = L.RateMatcher(**spec.kwargs())
    dec = L.Decoder(g, K, max_batch=frames + 64, algo="layered", max_iter=U.MAX_ITER, llr_scale=U.LLR_SCALE, layer_rows=Z)
    need = L.out_bytes(K, frames)
    sizes = src.size + frames * N + sum(frames * E * 5 for _, E in txs) + 2 * frames * N * 4 + need + frames * 4
    ar = Arena(sizes + 4096)
    p_src = ar.carve(src.size, name="src", **ODD)
    p_code = ar.carve(frames * N, name="code", **ODD)
    p_tx = [ar.carve(frames * E, name="tx%d" % t, **ODD) for t, (_, E) in enumerate(txs)]
    p_rx = [ar.carve(frames * E * 4, name="rx%d" % t, **F4) for t, (_, E) in enumerate(txs)]
    p_soft = ar.carve(frames * N * 4, name="soft", **F4)
    p_y = ar.carve(frames * N * 4, name="y", **F4)
    p_out = ar.carve(need, name="out", **ODD)
    p_iters = ar.carve(frames * 4, name="iters", **F4)
    ar.put(p_src, src)
    _sync()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    lb = _lib.load()
    enc.encode_device(p_src, src.size, frames, p_code, frames * N, "bits", s)
    for t, (k0, E) in enumerate(txs):
        rm.match_device(p_code, frames, k0, E, p_tx[t], frames * E, "bits", "bits", s)
        _lib.check(lb.ldpc_awgn_device(p_rx[t], frames, E, p_tx[t], sd, 100 + t, 0, 0, s))
        rm.recover_device(p_rx[t], frames, k0, E, p_soft, t > 0, p_y, s)
    dec.decode_device(p_y, frames, p_out, need, p_iters, s)
    errors = _count(p_out, p_src, frames, kb, s)                # blocks on the stream
    _sync()
    assert np.array_equal(ar.get(p_code, frames * N).reshape(frames, N), code_want)
    for t, (k0, E) in enumerate(txs):
        assert np.array_equal(ar.get(p_tx[t], frames * E).reshape(frames, E), tx_want[t]), t
        assert np.array_equal(ar.get(p_rx[t], frames * E, np.uint32), rx_want[t].reshape(-1).view(np.uint32)), t
    assert np.array_equal(ar.get(p_soft, frames * N, np.uint32), soft_w.reshape(-1).view(np.uint32))
    assert np.array_equal(ar.get(p_y, frames * N, np.uint32), y_w.reshape(-1).view(np.uint32))
    assert np.array_equal(ar.get(p_out, need), dw["out"])
    assert np.array_equal(ar.get(p_iters, frames, np.int32), dw["iters"])
    assert errors == _numpy_count(dw["out"].reshape(frames, kb) ^ src.reshape(frames, kb))
    assert np.array_equal(ar.get(p_src, src.size), src)
    ar.assert_untouched("chain")
    dec.close()
    enc.close()
