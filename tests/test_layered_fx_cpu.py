"""Fixed-point layered min-sum (algo = layered_fx) without a GPU: the numpy reference (tests/layered_fx_ref.py) anchored to
the float layered min-sum where nothing saturates and no message is 0, a row and a two-round decode written out by hand,
the premises of the GPU cases (tests/layered_fx_cases.py) asserted on the reference alone, and everything the library
decides in front of any device: the refusals, the struct layout and the alias of post_bits."""
import ctypes

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, channel, codes

import kernel_matrix as km
import layered_fx_cases as xc
import layered_fx_ref as FX
from fixed_ref import WIDTHS
from ms_correction_ref import Code, layered_ms

f32 = np.float32
I32 = np.int32
LDPC_OK, LDPC_ERR_ARG, LDPC_ERR_HIP, LDPC_ERR_UNSUPPORTED = 0, 1, 2, 4


# ---- the reference against the float decoder --------------------------------------------------------------------------

@pytest.mark.parametrize("setting", [(0.0, 0.0), (0.0, 1.0)])
def test_reference_is_layered_min_sum_where_nothing_saturates(setting):
    """Integer channel values (llr_scale 1), q = 8, p = 16 on WiMAX (576, 288): on the frames in which no t_k is exactly 0
    (the float decoder's sign product dies on a zero, the integer rule counts it as positive) and no |t_k| exceeds 127, the
    reference is ms_correction_ref.layered_ms value for value: R after rounds 1 and 2, P = c + the column's R, bits, bytes
    and iteration counts.  Plain, and with a one-LSB offset (an integer in float too)."""
    c = xc.saturation_code("wimax")
    code = c["code"]
    y = np.rint(channel.awgn_frames(c["N"], 0, 768, 0.5, seed=31) * f32(7)).astype(f32)
    y[y == 0] = 1
    probe = FX.layered_fx(code, y, c["z"], 8, *setting, q=8, p=16, llr_scale=1.0)
    y = y[(probe["zero_t"] == 0) & (probe["peak_t"] <= 127)]
    assert y.shape[0] >= 100
    for tap in (1, 2):
        w = FX.layered_fx(code, y, c["z"], 8, *setting, q=8, p=16, llr_scale=1.0, tap_iter=tap)
        assert w["zero_t"].sum() == 0 and w["peak_t"].max() <= 127 and w["sat"].sum() == 0       # the premise, on these frames
        assert np.array_equal(w["c"], y.astype(I32))
        ms = layered_ms(code, y, c["z"], 8, *setting, tap_iter=tap)
        assert ms["undefined"].sum() == 0
        run = np.nonzero(w["iters"] >= tap)[0]
        assert run.size >= (5 if tap == 2 else 100), run.size
        assert np.array_equal(w["iters"], ms["iters"]) and np.array_equal(w["hard"], ms["hard"]) and np.array_equal(w["out"], ms["out"])
        assert np.array_equal(w["r_tap"][run].astype(f32), ms["r_tap"][run])
        assert np.array_equal(w["hard_tap"][run], ms["hard_tap"][run])
        # the float decoder keeps no P tap; with nothing clamped P is the channel value plus the column's messages
        Rx = np.concatenate([w["r_tap"][run], np.zeros((run.size, 1), I32)], axis=1)
        assert np.array_equal(w["p_tap"][run], w["c"][run] + Rx[:, code.col_edges].sum(axis=2))
        Rm = np.concatenate([ms["r_tap"][run], np.zeros((run.size, 1), f32)], axis=1)
        assert np.array_equal(w["p_tap"][run].astype(f32), y[run] + Rm[:, code.col_edges].sum(axis=2))


def _row(x, scale=0.0, offset=0.0, q=8):
    x = np.asarray(x, I32)
    return FX.row(x[None, None, :], np.ones((1, x.size), bool), scale, offset, q)[0, 0].tolist()


def test_one_row_by_hand():
    # a zero counts as positive and does not kill the row; it is the minimum, so every other edge gets 0
    assert _row([0, -3, 3, 7]) == [-3, 0, 0, 0]
    # a tie of the two minima: the edge that holds the first takes the second, which is the same number
    assert _row([4, -4, 9]) == [-4, 4, -4]
    # a degree-1 row: the start value reads L
    for q in WIDTHS:
        assert _row([-3], q=q) == [FX.limit(q)]
    # truncation: ms_scale = 0.75 is (3m) >> 2, and an offset of one LSB comes first
    for m in range(128):
        assert _row([m, 127], 0.75) == [(3 * 127) >> 2, (3 * m) >> 2]
        assert _row([m, 127], 0.75, 1.0) == [(3 * 126) >> 2, (3 * max(m - 1, 0)) >> 2]
    # the corrected magnitude saturates at L where the inputs were clamped to it
    assert _row([31, -31, 31], 0.0, 0.0, q=6) == [-31, 31, -31]


def test_two_rounds_by_hand():
    """One row over three columns, channel values 7, 7, 7 LSB, q = 4 (L = 7).  With p = 16: round 1 gives R = 7, P = 14;
    round 2 t = 14 - 7 = 7, again R = 7, P = 14.  With p = 4 the memory holds 7 after round 1, and round 2 forms
    t = 7 - 7 = 0 from the saturated P: R = 0, P = 0 -- exactly what a posterior memory of q bits costs."""
    code = Code([0, 0, 0], [0, 1, 2], 1, 3, 3)
    y = np.full((1, 3), 7, f32)
    wide = FX.layered_fx(code, y, 1, 2, q=4, p=16, tap_iter=2, early_term=False)
    assert wide["p_tap"].tolist() == [[14, 14, 14]] and wide["r_tap"].tolist() == [[7, 7, 7]] and wide["sat"][0] == 0
    narrow = FX.layered_fx(code, y, 1, 2, q=4, p=4, tap_iter=2, early_term=False)
    assert narrow["p_tap"].tolist() == [[0, 0, 0]] and narrow["r_tap"].tolist() == [[0, 0, 0]]
    assert narrow["sat"][0] == 3 and narrow["peak_sum"][0] == 14 and narrow["zero_t"][0] == 3
    first = FX.layered_fx(code, y, 1, 1, q=4, p=4, tap_iter=1)
    assert first["p_tap"].tolist() == [[7, 7, 7]] and first["r_tap"].tolist() == [[7, 7, 7]]
    # t is not clamped on its way into P: 7 + 7 = 14 reaches p = 5 (LP = 15) whole although the message was 7 = L
    assert FX.layered_fx(code, y, 1, 1, q=4, p=5, tap_iter=1)["p_tap"].tolist() == [[14, 14, 14]]


# ---- premises of the GPU cases ---------------------------------------------------------------------------------------

def test_premises_of_the_saturation_cases():
    """|t_k| beyond L at every width on both codes; P at +-LP with p = q on both codes and with p = q + 2 on WiMAX; a result
    that differs from the p = 16 result in some frame's bits; and on the star code |t + R| beyond 32767 with both signs, so
    that a wrapping 16-bit store would show."""
    for name in ("wimax", "ira"):
        for q, p in xc.SATURATION_WIDTHS:
            w = xc.saturation_want(name, q, p)
            print(name, q, p, "peak |t| %d, writes at +-LP %d, clamped writes %d" % (w["peak_t"].max(), w["at_limit"].sum(), w["sat"].sum()))
            assert w["peak_t"].max() > FX.limit(q), (name, q, p)
            assert (w["iters"] >= xc.TAP).sum() >= 20 and np.unique(w["iters"]).size >= 2, (name, q, p)
            if p == q or (name == "wimax" and p == q + 2):
                assert w["at_limit"].sum() > 0 and w["sat"].sum() > 0, (name, q, p)
                differ = (w["hard"] != xc.saturation_want(name, q, 16)["hard"]).any(axis=1).sum()
                assert differ >= 1, (name, q, p)
            if p == 16:
                assert w["sat"].sum() == 0
            # NaN reads 0 and the infinities +-L in the stored channel values
            y = xc.saturation_inputs(name, q)
            assert (w["c"][np.isnan(y)] == 0).all() and np.isnan(y).sum() == 5
            assert (w["c"][np.isposinf(y)] == FX.limit(q)).all() and (w["c"][np.isneginf(y)] == -FX.limit(q)).all()
    s = xc.star_want()
    assert s["peak_sum"][0] > 32767 and s["peak_sum"][1] > 32767 and s["sat"][0] > 0 and s["sat"][1] > 0
    assert s["post"][0, 0] == 32767 and s["post"][1, 0] == -32767 and s["p_tap"][0, 0] == 32767
    assert (s["sat"][2:] == 0).all() and (s["iters"] == xc.STAR_TAP).all()


def test_premises_of_the_bg1_and_matrix_cases():
    """The BG1 batch holds frames stopping in rounds 1, 2, 3, 4 and frames that never stop, at both widths, plain and
    corrected, and q = 6 / p = 8 saturates while q = 8 / p = 16 does not; the matrix code has a row of every degree 1 ... 24
    and rows above 24."""
    c = xc.bg1_code()
    for frames in (70, xc.BG1_TWO_TILES):
        for q, p in xc.WIDTHS:
            for corrected in (False, True):
                w = xc.bg1_want(frames, q, p, corrected)
                assert {1, 2, 3, 4} <= set(w["iters"].tolist()), (frames, q, p, corrected)
                assert (~c["code"].syndrome_ok(w["hard"])).sum() >= 1 and (w["iters"] == xc.BG1_MAXIT).any()
                assert (w["sat"].sum() > 0) == (p == 8)
    assert not (xc.bg1_want(70, 6, 8, False)["out"] == xc.bg1_want(70, 6, 8, True)["out"]).all()
    m = xc.matrix()
    rd, _ = km.degree_maps(m["rows"], m["cols"], m["M"], m["N"])
    assert set(range(1, 25)) <= set(rd) and max(rd) > 24
    for q, p in xc.WIDTHS:
        w = xc.matrix_want(q, p, False)
        assert (w["iters"] >= xc.TAP).sum() >= 10 and np.unique(w["iters"]).size >= 3


def test_premises_of_the_crc_and_typed_cases():
    kind, bits, y, w = xc.crc_case()
    assert w["by_stop"].size >= 1                               # frames the CRC stops before the syndrome is clean
    assert np.unique(w["iters"]).size >= 4
    for k in ("i8", "f16"):
        assert np.unique(xc.typed_want(k, 6, 8)["iters"]).size >= 4
    assert not np.array_equal(xc.typed_want("f16", 6, 8)["iters"], xc.bg1_want(70, 6, 8, False)["iters"])   # the rounding shows


# ---- bindings and refusals that precede device use -------------------------------------------------------------------

def _cfg(**kw):
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    cfg = _lib.DecoderConfigMsg()
    assert _lib.load().ldpc_decoder_config_init_sized(ctypes.byref(cfg), ctypes.sizeof(cfg)) == LDPC_OK
    cfg.K, cfg.max_batch, cfg.algo, cfg.layer_rows = K, 64, L.capi.ALGOS["layered_fx"], z
    cfg.msg_dtype, cfg.llr_scale = L.capi.MSG_I8, 8.0
    tune = kw.pop("tune", None)
    for k, v in kw.items():
        setattr(cfg, k, v)
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
    rate, N = codes.RATE_1_2, 576
    rows, cols = codes.wimax_edges(rate, N)
    K, M, z = codes.wimax_dims(rate, N)
    return L.Graph(rows, cols, M, N)


def test_post_bits_takes_the_first_reserved_word(built):
    F, G = _lib.DecoderConfigCrc, _lib.DecoderConfigMsg
    cfg = _cfg()
    assert cfg.post_bits == 0 and list(cfg.msg_reserved) == [0, 0, 0]
    assert G.msg_bits.offset == F.crc_bits.offset + 4 == ctypes.sizeof(F)
    assert cfg.struct_size == ctypes.sizeof(G) == ctypes.sizeof(F) + 16
    assert G.post_bits.offset == G.msg_reserved.offset == G.msg_bits.offset + 4
    cfg.post_bits = 11
    assert list(cfg.msg_reserved) == [11, 0, 0]
    cfg.msg_reserved[0] = 9
    assert cfg.post_bits == 9
    assert L.capi.ALGOS["layered_fx"] == 8 and 7 not in L.capi.ALGOS.values() and _lib.load().ldpc_abi_version() == 3


def test_refusals_in_front_of_the_device(graph):
    """Every refusal of the definition is decided before a device is looked for; the accepted forms get as far as the
    device."""
    A, I8 = L.capi.ALGOS, L.capi.MSG_I8
    rc, msg = _create(_cfg(algo=7), graph)
    assert rc == LDPC_ERR_ARG and "unknown algo" in msg
    for dtype in (L.capi.MSG_F32, L.capi.MSG_F16, L.capi.MSG_F8, 3):
        rc, msg = _create(_cfg(msg_dtype=dtype), graph)
        assert rc == LDPC_ERR_ARG, (dtype, msg)
    for bits in (1, 3, 7, 9, 16, -4):
        rc, msg = _create(_cfg(msg_bits=bits), graph)
        assert rc == LDPC_ERR_ARG and "msg_bits" in msg, bits
    for q, p in ((6, 5), (6, 17), (8, 7), (0, 7), (4, 3), (6, -1), (6, 32), (8, 4)):
        rc, msg = _create(_cfg(msg_bits=q, post_bits=p), graph)
        assert rc == LDPC_ERR_ARG and "post_bits" in msg, (q, p, msg)
    for s in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        rc, msg = _create(_cfg(msg_bits=6, llr_scale=s), graph)
        assert rc == LDPC_ERR_ARG and "llr_scale" in msg, s
    for z in (0, -24, 5, 7):                                     # missing, or not dividing M = 288
        rc, msg = _create(_cfg(layer_rows=z), graph)
        assert rc == LDPC_ERR_ARG and "layer_rows" in msg, z
    for tune in ({"fused": True}, {"ldsp": True}, {"fused": True, "ldsp": True}):
        rc, msg = _create(_cfg(msg_bits=6, post_bits=8, tune=tune), graph)
        assert rc == LDPC_ERR_UNSUPPORTED and "fixed-point" in msg, (tune, msg)
    for k in (1, 2):                                             # the two words that stay reserved
        cfg = _cfg(msg_bits=6)
        cfg.msg_reserved[k] = 1
        assert _create(cfg, graph)[0] == LDPC_ERR_ARG
    # post_bits belongs to this algorithm alone
    for algo, kw in (("ms", {}), ("ms", dict(msg_dtype=L.capi.MSG_F32)), ("layered", dict(msg_dtype=L.capi.MSG_F32)),
                     ("bp", dict(msg_dtype=L.capi.MSG_F32)), ("sp", dict(msg_dtype=L.capi.MSG_F32))):
        rc, msg = _create(_cfg(algo=A[algo], post_bits=8, **kw), graph)
        assert rc == LDPC_ERR_ARG and "post_bits" in msg, (algo, msg)
    # what was refused stays refused: the plain layered algorithm takes no fixed-point messages
    rc, msg = _create(_cfg(algo=A["layered"], msg_bits=6), graph)
    assert rc == LDPC_ERR_UNSUPPORTED and "fixed-point" in msg
    # a struct shorter than the full size means post_bits = 0: the bytes behind it are not read
    cfg = _cfg(algo=A["ms"], msg_dtype=L.capi.MSG_F32, post_bits=77)
    cfg.struct_size = ctypes.sizeof(_lib.DecoderConfigCrc)
    assert _create(cfg, graph)[0] in (LDPC_OK, LDPC_ERR_HIP)
    # the accepted forms
    for q, p in ((0, 0), (4, 4), (4, 16), (5, 7), (6, 8), (6, 6), (8, 8), (8, 16), (8, 0)):
        for corr in ({}, dict(ms_scale=0.75), dict(ms_offset=1.0)):
            rc, msg = _create(_cfg(msg_bits=q, post_bits=p, **corr), graph)
            assert rc in (LDPC_OK, LDPC_ERR_HIP), (q, p, corr, msg)
    assert _create(_cfg(msg_bits=6, post_bits=8, early_term=0, crc_kind=0), graph)[0] in (LDPC_OK, LDPC_ERR_HIP)
    # the Python layer: the name and the keywords reach the struct
    try:
        dec = L.Decoder(graph, 288, max_batch=64, algo="layered_fx", msg_dtype="i8", msg_bits=6, post_bits=8, layer_rows=24,
                        llr_scale=8.0, ms_scale=0.75, ms_offset=1.0)
        assert dec.cfg.algo == 8 and dec.cfg.msg_bits == 6 and dec.cfg.post_bits == 8
        dec.close()
    except L.LdpcError as e:
        assert e.code == LDPC_ERR_HIP
    with pytest.raises(L.LdpcError) as e:
        L.Decoder(graph, 288, max_batch=64, algo="layered_fx", msg_dtype="i8", msg_bits=6, post_bits=5, layer_rows=24)
    assert e.value.code == LDPC_ERR_ARG
