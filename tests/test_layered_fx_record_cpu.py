"""LDPC_TUNE_FX_RECORD (algo = layered_fx on the fixed-point record kernel) without a GPU: the 8-byte check record as the only
row state (tests/layered_fx_record_ref.py) gives what tests/layered_fx_ref.py gives -- layout, ties and the degree-1 row --,
the two words survive their field limits, and everything the library decides about the field in front of any device."""
import ctypes

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, codes

import layered_fx_cases as xc
import layered_fx_record_ref as REC
import layered_fx_ref as FX
from ms_correction_ref import Code

LDPC_OK, LDPC_ERR_ARG, LDPC_ERR_HIP, LDPC_ERR_UNSUPPORTED = 0, 1, 2, 4
FX_RECORD = 1 << 30
KEYS = ("out", "iters", "hard", "r_tap", "p_tap", "hard_tap", "c", "post")


def _same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (k,) + what


# ---- the record is enough state ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("q,p,corrected", [(6, 8, True), (8, 16, False)])
def test_records_on_the_bg1_profile_code(q, p, corrected):
    """z = 16, 70 frames, row degrees 3 ... 19, 42 external columns; also with every column in P"""
    c = xc.bg1_code()
    assert REC.external_rows(c["code"]).sum() > 0
    want = xc.bg1_want(70, q, p, corrected)
    for ext in (True, False):
        got = REC.layered_fx_record(c["code"], xc.bg1_inputs(70), c["z"], xc.BG1_MAXIT, *xc.setting(corrected), q=q, p=p,
                                    llr_scale=xc.LLR_SCALE[q], tap_iter=xc.TAP, ext=ext)
        _same(got, want, (q, p, corrected, ext))


@pytest.mark.parametrize("q,p", xc.SATURATION_WIDTHS)
def test_records_on_the_saturation_overlay(q, p):
    """WiMAX (576, 288): zeros (a zero message's sign is immaterial), +-L, NaN, the infinities; P at +-LP"""
    c = xc.saturation_code("wimax")
    for corrected in (False, True):
        got = REC.layered_fx_record(c["code"], xc.saturation_inputs("wimax", q), c["z"], xc.SATURATION_MAXIT["wimax"],
                                    *xc.setting(corrected), q=q, p=p, llr_scale=xc.LLR_SCALE[q], tap_iter=xc.TAP)
        _same(got, xc.saturation_want("wimax", q, p, corrected), (q, p, corrected))


def test_records_on_the_star_code():
    """300 rows of degree 2, each a layer: one entry in P, one in the record; the centre column passes 32767"""
    c = xc.star_code()
    assert REC.external_rows(c["code"]).sum() == xc.STAR_ROWS - (c["K"] - 1)
    got = REC.layered_fx_record(c["code"], xc.star_inputs(), 1, 2, q=8, p=16, llr_scale=xc.LLR_SCALE[8], tap_iter=xc.STAR_TAP)
    _same(got, xc.star_want(), ("star",))
    assert got["p_tap"][0, 0] == 32767 and got["p_tap"][1, 0] == -32767


def test_records_of_degree_one_rows_and_ties():
    """A row of degree 1 keeps the start value as its second candidate (corrected, it is not the corrected L), once with its
    column in P and once in the record; a row whose entries all tie."""
    code = Code([0, 1, 1, 1, 2], [0, 0, 1, 2, 3], 3, 4, 1)
    assert REC.external_rows(code).tolist() == [False, True, True]
    y = np.array([[3, 3, 3, -5], [-2, 2, 2, 2], [0, 0, 0, 0]], np.float32)
    for scale, offset in ((0.0, 0.0), (0.75, 1.0), (0.01, 0.0)):
        for q, p in ((4, 4), (6, 8), (8, 16)):
            kw = dict(q=q, p=p, tap_iter=2, early_term=False)
            want = FX.layered_fx(code, y, 1, 3, scale, offset, **kw)
            for ext in (True, False):
                _same(REC.layered_fx_record(code, y, 1, 3, scale, offset, ext=ext, **kw), want, (scale, offset, q, p, ext))


def test_the_two_words_at_their_field_limits():
    for signs, argmin, m1, m2, ext in ((0xffffff, 23, 127, 127, 32767), (0xffffff, 23, 127, 127, -32767), (0, 0, 0, 0, 0),
                                       (1 << 23, 23, 0, 127, -32768), (0x555555, 17, 127, 0, -1), (1, 0, 1, 2, 1)):
        w0, w1 = REC.pack(signs, argmin, m1, m2, ext)
        assert w0.dtype == np.uint32 and w1.dtype == np.uint32
        assert [int(v) for v in REC.unpack(w0, w1)] == [signs, argmin, m1, m2, ext]
    w0, w1 = REC.pack(0xffffff, 23, 127, 127, -32767)
    assert int(w0) == 0x17ffffff and int(w1) == 0x80017f7f
    # message k: the sign bit k, the second minimum at the argmin
    w0, w1 = REC.pack(0b101, 1, 3, 9, 0)
    assert REC.messages(w0, w1, 4).tolist() == [-3, 9, -3, 3]
    for bad in ((1 << 24, 0, 0, 0, 0), (0, 24, 0, 0, 0), (0, 0, 128, 0, 0), (0, 0, 0, 128, 0), (0, 0, 0, 0, 32768)):
        with pytest.raises(AssertionError):
            REC.pack(*bad)


# ---- the field, in front of the device ---------------------------------------------------------------------------------

def _cfg(algo="layered_fx", **kw):
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    cfg = _lib.DecoderConfigMsg()
    assert _lib.load().ldpc_decoder_config_init_sized(ctypes.byref(cfg), ctypes.sizeof(cfg)) == LDPC_OK
    cfg.K, cfg.max_batch, cfg.algo, cfg.layer_rows = K, 64, L.capi.ALGOS[algo], z
    cfg.msg_dtype, cfg.llr_scale = L.capi.MSG_I8, 8.0
    cfg.msg_bits, cfg.post_bits = 6, 8
    for k, v in kw.items():
        setattr(cfg, k, v)
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


def test_apply_tune_sets_bit_30():
    cfg = _cfg()
    L.capi.apply_tune(cfg, {"fx_record": True})
    assert cfg.tune_flags == FX_RECORD
    L.capi.apply_tune(cfg, {"fx_record": True, "ldsp_ext": False, "ldsp_per_cu": 3})
    assert cfg.tune_flags == FX_RECORD | (2 << 4) and cfg.tune_ldsp_shape == 3
    for off in (False, None):
        L.capi.apply_tune(cfg, {"fx_record": off})
        assert cfg.tune_flags == 0
    assert L.capi.tune_from_env({"LDPC_TUNE_FX_RECORD": "1"}) == {"fx_record": True}
    assert L.capi.tune_from_env({"LDPC_TUNE_FX_RECORD": "0"}) == {"fx_record": False}


def test_the_accepted_form_reaches_the_device(graph):
    """layered_fx with the field on is no argument error: it gets as far as the device (LDPC_ERR_HIP where there is none)"""
    for kw in ({}, dict(ms_scale=0.75, ms_offset=1.0), dict(early_term=0), dict(pack_mode=L.capi.PACK_BITS),
               dict(tune_ldsp_grid=3, tune_ldsp_shape=(3 << 8) | 1), dict(msg_bits=8, post_bits=16)):
        rc, msg = _create(_cfg(tune_flags=FX_RECORD, **kw), graph)
        assert rc in (LDPC_OK, LDPC_ERR_HIP), (kw, rc, msg)
    rc, msg = _create(_cfg(tune_flags=FX_RECORD | (2 << 4)), graph)         # with LDPC_TUNE_OFF(LDPC_TUNE_LDSP_EXT)
    assert rc in (LDPC_OK, LDPC_ERR_HIP), (rc, msg)


def test_refusals_in_front_of_the_device(graph):
    # a box-plus row has D independent messages
    rc, msg = _create(_cfg("layered_bp_fx", tune_flags=FX_RECORD), graph)
    assert rc == LDPC_ERR_UNSUPPORTED and "box-plus" in msg and "record" in msg, msg
    # no CRC rule in a record kernel
    for kind in (16, 24, 25):                                    # LDPC_CRC16, LDPC_CRC24A, LDPC_CRC24B
        rc, msg = _create(_cfg(tune_flags=FX_RECORD, crc_kind=kind, crc_bits=288), graph)
        assert rc == LDPC_ERR_UNSUPPORTED and "crc_kind" in msg and "record" in msg, (kind, msg)
    assert _create(_cfg(tune_flags=FX_RECORD, crc_kind=1, crc_bits=288), graph)[0] == LDPC_ERR_ARG     # no such CRC
    # what was refused stays refused, with the field on as well
    for more in (1 << 0, 1 << 2, (1 << 0) | (1 << 2)):
        rc, msg = _create(_cfg(tune_flags=FX_RECORD | more), graph)
        assert rc == LDPC_ERR_UNSUPPORTED and "fixed-point" in msg, (more, msg)
    # the field belongs to the fixed-point layered algorithms: with any other the bit is out of range
    F32 = L.capi.MSG_F32
    for algo, kw in (("sp", dict(msg_dtype=F32)), ("ms", dict(msg_dtype=F32)), ("ms", dict(post_bits=0)), ("layered", dict(msg_dtype=F32)),
                     ("ms_fused", dict(msg_dtype=F32)), ("bp", dict(msg_dtype=F32)), ("layered_bp", dict(msg_dtype=F32))):
        kw = dict(dict(msg_bits=0, post_bits=0), **kw)
        rc, msg = _create(_cfg(algo, tune_flags=FX_RECORD, **kw), graph)
        assert rc == LDPC_ERR_ARG, (algo, rc, msg)
    # no "off" value: bit 31 makes the word negative, both bits likewise
    for flags in (-(1 << 31), -(1 << 31) | FX_RECORD, -1):
        assert _create(_cfg(tune_flags=flags), graph)[0] == LDPC_ERR_ARG, flags
    # the last reserved words of the config stay reserved
    for k in (1, 2):
        cfg = _cfg(tune_flags=FX_RECORD)
        cfg.msg_reserved[k] = 1
        assert _create(cfg, graph)[0] == LDPC_ERR_ARG
    # the argument errors of layered_fx come first
    assert _create(_cfg(tune_flags=FX_RECORD, post_bits=5), graph)[0] == LDPC_ERR_ARG
    assert _create(_cfg(tune_flags=FX_RECORD, layer_rows=7), graph)[0] == LDPC_ERR_ARG


def test_the_python_layer(graph):
    try:
        dec = L.Decoder(graph, 288, max_batch=64, algo="layered_fx", msg_dtype="i8", msg_bits=6, post_bits=8, layer_rows=24,
                        llr_scale=8.0, tune={"fx_record": True})
        assert dec.cfg.tune_flags == FX_RECORD
        dec.close()
    except L.LdpcError as e:
        assert e.code == LDPC_ERR_HIP
    with pytest.raises(L.LdpcError) as e:
        L.Decoder(graph, 288, max_batch=64, algo="layered_bp_fx", msg_dtype="i8", msg_bits=6, post_bits=8, layer_rows=24,
                  llr_scale=8.0, tune={"fx_record": True})
    assert e.value.code == LDPC_ERR_UNSUPPORTED
