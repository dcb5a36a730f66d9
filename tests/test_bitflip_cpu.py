"""Hard-decision bit flipping (algo = bitflip) without a GPU: the numpy reference (tests/bitflip_ref.py) against cases worked
out by hand, the threshold formula written out, the comparison of schedules that chose the default (printed), and what the
library decides in front of any device: the struct layout, the threshold entries and the other refusals.

A soft-output request needs a handle and a handle needs a device, so that refusal is tested in tests/test_gpu_bitflip.py."""
import ctypes

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, codes

import bitflip_ref as B
from osd_cases import HAMMING, edges_of

LDPC_OK, LDPC_ERR_ARG, LDPC_ERR_HIP, LDPC_ERR_UNSUPPORTED = 0, 1, 2, 4


def _wimax(N, rate=codes.RATE_1_2):
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    return B.Code(rows, cols, M, N)


def _hamming():
    return B.Code(*edges_of(HAMMING))


# ---- the rule by hand -------------------------------------------------------------------------------------------------

def test_threshold_formula_written_out():
    """T(d, i) = max(floor((d + 1) / 2) + 1, d + 1 - (i - 1)) for d = 2, 3, 6 over rounds 1 .. 8."""
    assert [B.threshold(2, i) for i in range(1, 9)] == [3, 2, 2, 2, 2, 2, 2, 2]
    assert [B.threshold(3, i) for i in range(1, 9)] == [4, 3, 3, 3, 3, 3, 3, 3]
    assert [B.threshold(6, i) for i in range(1, 9)] == [7, 6, 5, 4, 4, 4, 4, 4]


def test_threshold_table_indexing():
    """Entry j is the offset of round j + 1; the last entry serves every later round; all zero is the default; 62 from the
    start is strict majority from round 1."""
    t = [5, 0, 1, 2] + [3] * 11 + [4]
    assert [B.offset(i, t) for i in (1, 2, 3, 4, 5, 15, 16, 17, 40)] == [5, 0, 1, 2, 3, 3, 4, 4, 4]
    assert [B.threshold(6, i, t) for i in (1, 2, 3, 4, 5, 16, 17)] == [4, 7, 6, 5, 4, 4, 4]
    assert [B.offset(i, [0] * 16) for i in (1, 2, 17, 30)] == [0, 1, 16, 29]
    assert [B.threshold(d, 1, [62] * 16) for d in (0, 1, 2, 3, 6, 7)] == [1, 2, 2, 3, 4, 5]


def test_hamming_one_flipped_bit_corrects_in_round_one():
    """H's columns are the numbers 1 .. 7 in binary; the all-zero codeword with bit 6 (column 111, degree 3) flipped.
    Round 1: s = (1, 1, 1), u = the column degrees (1, 1, 2, 1, 2, 2, 3), x = r so E = u.  T(d, 1) = d + 1: no column has
    a hit, so the frame flips the columns of its largest E = 3: bit 6 alone.  Round 2 finds s = 0: done, iters = 1."""
    code = _hamming()
    assert code.col_deg.tolist() == [1, 1, 2, 1, 2, 2, 3]
    y = np.ones((1, 7), np.float32)
    y[0, 6] = -1
    for max_iter in (2, 5):
        w = B.decode(code, y, max_iter)
        assert w["hard"].tolist() == [[0] * 7] and w["iters"].tolist() == [1] and w["done"].tolist() == [True]
    one = B.decode(code, y, 1)                    # the flip is made in round 1, but nothing looks at the result any more
    assert one["hard"].tolist() == [[0] * 7] and one["iters"].tolist() == [1] and one["done"].tolist() == [False]
    assert one["syndrome"].tolist() == [[1, 1, 1]]
    # without the fall-back round 1 flips nothing (E = d < T = d + 1) and round 2, T(3, 2) = 3 and T(2, 2) = 2, flips the
    # three columns of degree 2 along with bit 6
    thr = B.decode(code, y, 2, schedule="threshold")
    assert thr["hard"].tolist() == [[0, 0, 1, 0, 1, 1, 0]] and thr["done"].tolist() == [False]


def test_hamming_degree_one_column_is_out_of_reach():
    """Bit 0 (column 001, degree 1) flipped: s = (1, 0, 0), every column of that row has u = 1, the largest E is 1 < 2 and
    T >= 2: nothing ever flips."""
    y = np.ones((1, 7), np.float32)
    y[0, 0] = -1
    w = B.decode(_hamming(), y, 6)
    assert w["hard"].tolist() == [[1, 0, 0, 0, 0, 0, 0]] and w["iters"].tolist() == [6] and not w["done"][0]


def test_codeword_returns_untouched_with_zero_iterations():
    code = _wimax(576)
    y = np.ones((3, 576), np.float32)
    y[1] = [np.nan, -0.0, 0.0] * 192              # none of them is below zero
    w = B.decode(code, y, 9)
    assert not w["hard"].any() and w["iters"].tolist() == [0, 0, 0] and w["done"].all() and not w["syndrome"].any()
    cw = np.array([1, 1, 1, 0, 0, 0, 0], np.uint8)                # columns 1 ^ 2 ^ 3 = 0
    w = B.decode(_hamming(), (1.0 - 2.0 * cw)[None, :], 4)
    assert w["hard"].tolist() == [cw.tolist()] and w["iters"].tolist() == [0]


def test_done_frames_keep_their_bits_and_counts():
    """Running more rounds changes nothing about a frame that was done earlier."""
    code = _wimax(576)
    y = B.bsc(64, 576, 0.01, seed=3)
    a, b = B.decode(code, y, 6), B.decode(code, y, 20)
    early = a["done"]
    assert early.sum() >= 20 and (~early).sum() >= 1
    assert np.array_equal(a["hard"][early], b["hard"][early]) and np.array_equal(a["iters"][early], b["iters"][early])
    assert (b["iters"][~early] >= 6).all()


# ---- the schedule --------------------------------------------------------------------------------------------------------

def test_schedule_comparison_and_the_default_decodes(capsys):
    """802.16e rate 1/2 at N = 576 and 2304, a binary symmetric channel at crossover 0.01, 0.02 and 0.03, 512 frames of the
    all-zero codeword, 30 rounds: frames left in error by the default rule (thresholds, and the largest E where no column
    reaches its threshold), by the thresholds alone, by strict majority from round 1 and by flipping only the largest E in
    every round.  A record, printed; the one assertion: at N = 576 and 0.01 the default leaves fewer frames in error than
    arrive dirty.  Measured when the default was chosen: (576, 0.01) 511 dirty -> 29 / 86 / 85 / 28, (576, 0.02) 512 ->
    124 / 252 / 249 / 148, (576, 0.03) 512 -> 273 / 402 / 397 / 307, (2304, 0.01) 512 -> 93 / 234 / 234 / 103,
    (2304, 0.02) 512 -> 324 / 475 / 473 / 378, (2304, 0.03) 512 -> 466 / 511 / 510 / 499."""
    table = B.schedule_table(_wimax)
    with capsys.disabled():
        print("\n   N     K     p  dirty  " + "  ".join("%9s" % s for s in B.SCHEDULES))
        for N, K, p, dirty, *left in table:
            print("%4d  %4d  %.2f  %5d  " % (N, K, p, dirty) + "  ".join("%9d" % v for v in left))
    N, K, p, dirty, default = table[0][:5]
    assert (N, p) == (576, 0.01) and dirty > 400
    assert default < dirty


# ---- what the library decides in front of any device -----------------------------------------------------------------------

def _cfg(**kw):
    K, M, z = codes.wimax_dims(codes.RATE_1_2, 576)
    cfg = _lib.DecoderConfigBf()
    assert _lib.load().ldpc_decoder_config_init_sized(ctypes.byref(cfg), ctypes.sizeof(cfg)) == LDPC_OK
    cfg.K, cfg.max_batch, cfg.algo = K, 64, L.capi.ALGOS["bitflip"]
    tune = kw.pop("tune", None)
    bf = kw.pop("bf_threshold", None)
    for k, v in kw.items():
        setattr(cfg, k, v)
    if bf is not None:
        cfg.bf_threshold[:] = bf
    if tune:
        L.capi.apply_tune(cfg, tune)
    return cfg


def _create(cfg, graph):
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.ldpc_decoder_create(graph._h, ctypes.byref(cfg), ctypes.byref(h))
    if rc == LDPC_OK:
        lib.ldpc_decoder_destroy(h)
    return rc, lib.ldpc_last_error().decode()


@pytest.fixture(scope="module")
def graph(built):
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 576)
    K, M, z = codes.wimax_dims(codes.RATE_1_2, 576)
    return L.Graph(rows, cols, M, 576)


def test_bf_threshold_is_appended(built):
    G, Bf = _lib.DecoderConfigMsg, _lib.DecoderConfigBf
    cfg = _cfg()
    assert list(cfg.bf_threshold) == [0] * 16
    assert Bf.bf_threshold.offset == ctypes.sizeof(G) and cfg.struct_size == ctypes.sizeof(Bf) == ctypes.sizeof(G) + 64
    assert L.capi.ALGOS["bitflip"] == 10 and 7 not in L.capi.ALGOS.values() and _lib.load().ldpc_abi_version() == 3


def test_refusals_in_front_of_the_device(graph):
    A = L.capi.ALGOS
    ok = (LDPC_OK, LDPC_ERR_HIP)
    # the accepted forms get as far as the device
    assert _create(_cfg(), graph)[0] in ok
    assert _create(_cfg(bf_threshold=[62] * 16), graph)[0] in ok
    assert _create(_cfg(bf_threshold=[0, 1, 2, 3] + [4] * 12, early_term=0, pack_mode=1, frames_per_lane=4), graph)[0] in ok
    assert _create(_cfg(crc_kind=16, crc_bits=128), graph)[0] in ok
    # an entry that is no offset
    for j, v in ((0, -1), (3, 63), (15, 1000), (7, -62)):
        t = [1] * 16
        t[j] = v
        rc, msg = _create(_cfg(bf_threshold=t), graph)
        assert rc == LDPC_ERR_ARG and "bf_threshold[%d]" % j in msg, (j, v, msg)
    # the field belongs to this algorithm alone
    for algo in ("ms", "sp", "layered", "bp"):
        rc, msg = _create(_cfg(algo=A[algo], layer_rows=24, bf_threshold=[0] * 15 + [1]), graph)
        assert rc == LDPC_ERR_ARG and "bf_threshold" in msg, (algo, msg)
    # a struct without the field means the default: the bytes behind it are not read
    cfg = _cfg(bf_threshold=[99] * 16)
    cfg.struct_size = ctypes.sizeof(_lib.DecoderConfigMsg)
    assert _create(cfg, graph)[0] in ok
    for size in (ctypes.sizeof(_lib.DecoderConfigMsg) + 4, ctypes.sizeof(_lib.DecoderConfigBf) - 4, ctypes.sizeof(_lib.DecoderConfigBf) + 4):
        cfg.struct_size = size
        rc, msg = _create(cfg, graph)
        assert rc == LDPC_ERR_ARG and "struct_size" in msg, size
    # no messages, no minimum to correct, no soft engines
    for dtype in (L.capi.MSG_F16, L.capi.MSG_F8):
        rc, msg = _create(_cfg(msg_dtype=dtype), graph)
        assert rc == LDPC_ERR_UNSUPPORTED and "BITFLIP" in msg, (dtype, msg)
    assert _create(_cfg(msg_dtype=L.capi.MSG_I8, llr_scale=4.0), graph)[0] == LDPC_ERR_UNSUPPORTED
    for corr in (dict(ms_scale=0.75), dict(ms_offset=0.5)):
        rc, msg = _create(_cfg(**corr), graph)
        assert rc == LDPC_ERR_UNSUPPORTED and "ms_scale" in msg, (corr, msg)
    for tune in ({"fused": True}, {"ldsp": True}):
        rc, msg = _create(_cfg(tune=tune), graph)
        assert rc == LDPC_ERR_UNSUPPORTED and "BITFLIP" in msg, (tune, msg)
    rc, msg = _create(_cfg(tune={"fx_record": True}), graph)
    assert rc == LDPC_ERR_ARG
    # the CRC stop needs early termination, as everywhere
    assert _create(_cfg(crc_kind=16, crc_bits=128, early_term=0), graph)[0] == LDPC_ERR_ARG
    # llr_scale is ignored: values another algorithm refuses pass
    assert _create(_cfg(llr_scale=0.0), graph)[0] in ok


def test_a_column_of_degree_63_is_unsupported(built):
    M, N = 63, 2
    rows = np.repeat(np.arange(M, dtype=np.int32), 2)
    cols = np.tile(np.array([0, 1], np.int32), M)
    g63 = L.Graph(rows, cols, M, N)
    cfg = _cfg(K=1)
    rc, msg = _create(cfg, g63)
    assert rc == LDPC_ERR_UNSUPPORTED and "degree" in msg
    g62 = L.Graph(rows[:-2], cols[:-2], M - 1, N)
    assert _create(cfg, g62)[0] in (LDPC_OK, LDPC_ERR_HIP)


def test_python_layer_reaches_the_struct(graph):
    try:
        dec = L.Decoder(graph, 288, max_batch=64, algo="bitflip", bf_threshold=[1, 2, 3])
        assert dec.cfg.algo == 10 and list(dec.cfg.bf_threshold) == [1, 2] + [3] * 14
        dec.close()
    except L.LdpcError as e:
        assert e.code == LDPC_ERR_HIP
    with pytest.raises(L.LdpcError) as e:
        L.Decoder(graph, 288, max_batch=64, algo="bitflip", bf_threshold=[63])
    assert e.value.code == LDPC_ERR_ARG
    # every other algorithm passes the struct it always passed
    try:
        dec = L.Decoder(graph, 288, max_batch=64, algo="ms")
        assert dec.cfg.struct_size == ctypes.sizeof(_lib.DecoderConfigMsg)
        dec.close()
    except L.LdpcError as e:
        assert e.code == LDPC_ERR_HIP
