"""Normalized / offset min-sum without a GPU: the numpy restatement (ms_correction_ref.py) against the CPU
oracle with the correction off, a hand-computed row with it on, and the config checks of the C ABI
(ms_scale / ms_offset in ldpc_decoder_config), which all happen before a device is touched."""
import ctypes
import math

import numpy as np
import pytest

import oracle
import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, channel, codes
import fp16_cases as fc
from ms_correction_ref import Code, flood_ms, layered_ms
from util import golden_files, load_golden, wimax_oracle_graph

LDPC_OK, LDPC_ERR_ARG, LDPC_ERR_HIP, LDPC_ERR_UNSUPPORTED = 0, 1, 2, 4


def _same(ref, want, what):
    assert np.array_equal(ref["out"], want["out"]), what + ": bytes"
    assert np.array_equal(ref["iters"], want["iters"]), what + ": iterations"
    assert np.array_equal(ref["hard"], want["hard"]), what + ": hard bits"


def _random_qc(seed, z, mb, nb, dmax):
    rng = np.random.default_rng(seed)
    base = -np.ones((mb, nb), np.int64)
    for i in range(mb):
        d = int(rng.integers(1, min(dmax, nb) + 1))
        base[i, rng.choice(nb, d, replace=False)] = rng.integers(0, z, d)
    for j in range(nb):
        if (base[:, j] < 0).all():
            base[int(rng.integers(0, mb)), j] = rng.integers(0, z)
    rows, cols = codes.qc_edges(base, z)
    M, N = mb * z, nb * z
    K = max(8, (N - M) // 8 * 8)
    return rows, cols, M, N, K


@pytest.mark.parametrize("path", golden_files("flood"), ids=lambda p: p.split("flood_")[-1][:-4])
def test_restatement_equals_oracle_flooding_ms(path):
    gd = load_golden(path)
    g, rows, cols, K, M, z = wimax_oracle_graph(int(gd["rate"]), int(gd["N"]))
    code = Code(rows, cols, M, int(gd["N"]), K)
    y, it = gd["y"], int(gd["times"])
    for f16 in (False, True):
        want = oracle.decode(g, y, "ms", max_iter=it, tap_iter=2, msg_f16=f16)
        ref = flood_ms(code, y, it, f16=f16, tap_iter=2)
        _same(ref, want, "ms f16=%s" % f16)
        run = want["iters"] >= 2
        assert np.array_equal(ref["r_tap"][run], want["taps"]["r"][run])


@pytest.mark.parametrize("path", golden_files("layered"), ids=lambda p: p.split("layered_")[-1][:-4])
def test_restatement_equals_oracle_layered(path):
    gd = load_golden(path)
    g, rows, cols, K, M, z = wimax_oracle_graph(int(gd["rate"]), int(gd["N"]))
    code = Code(rows, cols, M, int(gd["N"]), K)
    y, it = gd["y"], int(gd["times"])
    want = oracle.decode(g, y, "layered", max_iter=it, layer_rows=z, tap_iter=2)
    ref = layered_ms(code, y, z, it, tap_iter=2)
    _same(ref, want, "layered")
    assert np.array_equal(ref["undefined"], want["undefined"])
    run = want["iters"] >= 2
    assert np.array_equal(ref["r_tap"][run], want["taps"]["r"][run])


@pytest.mark.parametrize("case", [(1, 5, 3, 9, 5), (2, 17, 6, 14, 6), (3, 24, 10, 16, 2), (4, 33, 7, 40, 20)])
def test_restatement_equals_oracle_on_random_qc_codes(case):
    seed, z, mb, nb, dmax = case
    rows, cols, M, N, K = _random_qc(seed, z, mb, nb, dmax)
    g = oracle.Graph(rows, cols, M, N, K)
    code = Code(rows, cols, M, N, K)
    y = channel.awgn_frames(N, 0, 13, 0.8, seed=seed)
    y[3, ::3] = 0.0
    y[5, :] = 2000.0                 # |q| > 1000 everywhere: the layered oracle's undefined frame
    for f16 in (False, True):
        _same(flood_ms(code, y, 12, f16=f16), oracle.decode(g, y, "ms", max_iter=12, msg_f16=f16), "ms %s" % (case,))
    want = oracle.decode(g, y, "layered", max_iter=12, layer_rows=z)
    ref = layered_ms(code, y, z, 12)
    _same(ref, want, "layered %s" % (case,))
    assert np.array_equal(ref["undefined"], want["undefined"]) and want["undefined"][5]


def _same_taps(ref, want, what):
    """R on the frames that reached the tapped round, Q on those that went on: bit patterns, NaN where the oracle has NaN
    (a frame that had stopped, or a NaN message)"""
    run_r, run_q = fc.tap_frames(want["iters"])
    assert run_q.size > 0, what
    assert fc.same_floats(ref["r_tap"][run_r], want["taps"]["r"][run_r]), what + ": R tap"
    assert fc.same_floats(ref["q_tap"][run_q], want["taps"]["q"][run_q]), what + ": Q tap"
    stopped = np.nonzero(want["iters"] <= fc.TAP)[0]
    assert np.isnan(ref["q_tap"][stopped]).all() and np.isnan(want["taps"]["q"][stopped]).all(), what


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("name", ["wimax", "ira3", "ira7", "ira16"])
def test_restatement_equals_oracle_on_degenerate_frames_and_q_tap(name, f16):
    """scale = offset = 0: the overlay of fp16_cases.py (zeros, values around binary16's largest number, infinities, NaN,
    binary16 subnormals and ties, -0) and the variable->check tap.  The NaN frame is where a restatement that takes argmin
    over |q| differs from the oracle's fminf chain, which skips a NaN."""
    c = fc.wimax() if name == "wimax" else fc.staircase(int(name[3:]), "ride")
    y = fc.overlay(channel.awgn_frames(c["N"], 0, fc.DEGENERATE_FRAMES, 0.7, seed=21))
    assert np.isnan(y[7]).sum() == 5
    want = oracle.decode(c["og"], y, "ms", max_iter=fc.DEGENERATE_MAXIT, tap_iter=fc.TAP, msg_f16=f16)
    ref = flood_ms(c["code"], y, fc.DEGENERATE_MAXIT, f16=f16, tap_iter=fc.TAP)
    _same(ref, want, "%s f16=%s" % (name, f16))
    _same_taps(ref, want, "%s f16=%s" % (name, f16))
    assert want["iters"][7] > fc.TAP                        # the NaN frame runs on: its Q tap is compared


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("d", fc.DEGREES)
def test_restatement_q_tap_equals_oracle_on_staircase_codes(d, f16):
    c = fc.staircase(d, "ride")
    want = oracle.decode(c["og"], c["y"], "ms", max_iter=fc.MAXIT, tap_iter=fc.TAP, msg_f16=f16)
    ref = flood_ms(c["code"], c["y"], fc.MAXIT, f16=f16, tap_iter=fc.TAP)
    _same(ref, want, "d=%d f16=%s" % (d, f16))
    _same_taps(ref, want, "d=%d f16=%s" % (d, f16))


def test_hand_computed_row():
    """One check row of weight 4, q = (0.5, -2, 1.25, -3): min1 = 0.5 at edge 0, min2 = 1.25, sign parity even.
    alpha = 0.75, beta = 0.25: min1' = (0.5 - 0.25) * 0.75 = 0.1875, min2' = (1.25 - 0.25) * 0.75 = 0.75."""
    code = Code([0, 0, 0, 0], [0, 1, 2, 3], 1, 4, 0)
    y = np.array([[0.5, -2.0, 1.25, -3.0]], np.float32)
    r = flood_ms(code, y, 1, scale=0.75, offset=0.25, tap_iter=1)["r_tap"][0]
    assert r.tolist() == [0.75, -0.1875, 0.1875, -0.1875]
    r = flood_ms(code, y, 1, scale=0.75, tap_iter=1)["r_tap"][0]
    assert r.tolist() == [0.9375, -0.375, 0.375, -0.375]
    r = flood_ms(code, y, 1, offset=0.75, tap_iter=1)["r_tap"][0]
    assert r.tolist() == [0.5, -0.0, 0.0, -0.0]          # fmaxf(0.5 - 0.75, 0) = 0; the sign still applies
    # fp16 messages: 0.7f * 0.5 = 0.349999994 is no binary16 value; R is rounded to 0.35009765625 where produced
    r = flood_ms(code, y, 1, scale=0.7, f16=True, tap_iter=1)["r_tap"][0]
    assert r[1] == np.float32(-0.35009765625) and r[0] == np.float32(np.float16(np.float32(1.25) * np.float32(0.7)))
    # layered, one row: q = P - 0 = y; b = 0.5 (edge 0), c = 1.25, product sign +
    r = layered_ms(code, y, 1, 1, scale=0.75, offset=0.25, tap_iter=1)["r_tap"][0]
    assert r.tolist() == [0.75, -0.1875, 0.1875, -0.1875]


def _create(cfg, g):
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.ldpc_decoder_create(g._h, ctypes.byref(cfg), ctypes.byref(h))
    if rc == LDPC_OK:
        lib.ldpc_decoder_destroy(h)
    return rc


def _cfg(algo, **kw):
    cfg = _lib.DecoderConfig()
    _lib.load().ldpc_decoder_config_init(ctypes.byref(cfg))
    cfg.K, cfg.max_batch, cfg.algo, cfg.layer_rows = 480, 4, algo, 24
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_config_fields_default_to_off(built):
    cfg = _cfg(L.capi.ALGOS["ms"])
    assert cfg.ms_scale == 0.0 and cfg.ms_offset == 0.0
    assert _lib.DecoderConfig.ms_scale.offset == _lib.DecoderConfig.tune_q_order.offset + 4
    assert ctypes.sizeof(_lib.DecoderConfig) == _lib.DecoderConfig.ms_offset.offset + 4


def test_config_validation_without_a_device(built):
    rate, N = codes.RATE_5_6, 576             # every row of one weight: LAYERED_HOST is otherwise allowed
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    g = L.Graph(rows, cols, M, N)
    ms, lay = L.capi.ALGOS["ms"], L.capi.ALGOS["layered"]
    for algo in (ms, lay):
        for scale, offset in ((math.nan, 0.0), (0.0, math.nan), (-0.5, 0.0), (0.0, -0.25), (1.5, 0.0),
                              (0.75, 1000.0), (0.0, 5000.0), (math.inf, 0.0), (0.0, math.inf)):
            cfg = _cfg(algo, K=K, layer_rows=z, ms_scale=scale, ms_offset=offset)
            assert _create(cfg, g) == LDPC_ERR_ARG, (algo, scale, offset)
            assert "ms_" in _lib.load().ldpc_last_error().decode()
    for name in ("sp", "ms_fused", "layered_host"):
        for scale, offset in ((0.75, 0.0), (0.0, 0.25), (1.0, 0.0)):
            cfg = _cfg(L.capi.ALGOS[name], K=K, layer_rows=z, ms_scale=scale, ms_offset=offset)
            assert _create(cfg, g) == LDPC_ERR_UNSUPPORTED, (name, scale, offset)
    # valid settings get as far as the device check (no device here: LDPC_ERR_HIP)
    for algo in (ms, lay):
        for scale, offset in ((0.75, 0.0), (0.0, 0.5), (1.0, 999.0), (0.8, 0.1)):
            cfg = _cfg(algo, K=K, layer_rows=z, ms_scale=scale, ms_offset=offset)
            assert _create(cfg, g) in (LDPC_OK, LDPC_ERR_HIP), (algo, scale, offset)


def test_config_of_the_previous_size_is_accepted(built):
    """A caller built against the header before ms_scale / ms_offset passes struct_size = offsetof(ms_scale):
    accepted, and the bytes behind it are not read (here they hold values that would be refused)."""
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    g = L.Graph(rows, cols, M, N)
    old = _lib.DecoderConfig.ms_scale.offset
    for name in ("ms", "layered", "sp", "ms_fused"):
        cfg = _cfg(L.capi.ALGOS[name], K=K, layer_rows=z, ms_scale=math.nan, ms_offset=-1.0)
        cfg.struct_size = old
        assert _create(cfg, g) in (LDPC_OK, LDPC_ERR_HIP), name
        cfg.struct_size = old + 4
        assert _create(cfg, g) == LDPC_ERR_ARG
    lib = _lib.load()
    h = ctypes.c_void_p()
    devs = (ctypes.c_int32 * 1)(0)
    cfg = _cfg(L.capi.ALGOS["ms"], K=K, layer_rows=z, ms_scale=math.nan)
    cfg.struct_size = old
    rc = lib.ldpc_decoder_create_multi(g._h, ctypes.byref(cfg), devs, 1, ctypes.byref(h))
    assert rc in (LDPC_OK, LDPC_ERR_HIP)
    if rc == LDPC_OK:
        lib.ldpc_decoder_destroy(h)
    cfg.struct_size = ctypes.sizeof(cfg)
    assert lib.ldpc_decoder_create_multi(g._h, ctypes.byref(cfg), devs, 1, ctypes.byref(h)) == LDPC_ERR_ARG


def test_coder_refuses_a_correction_for_reference_kernels(built, tmp_path):
    """Coder::setMinSumCorrection: DecodeMSCL, and DecodeTDMP on a code of uniform row weight (the reference's
    host-layered path), fail in addDecodeType with a reason -- before any device is touched."""
    import subprocess
    from coder_harness import coder_ms_correction_exe
    exe = coder_ms_correction_exe(tmp_path)
    for rate, mode, word in ((codes.RATE_1_2, "MSCL", "DecodeMSCL"), (codes.RATE_5_6, "TDMP", "DecodeTDMP")):
        p = subprocess.run([exe, str(rate), "576", "8", mode, "0.75", "0", "/nonexistent", "/nonexistent"],
                           capture_output=True, text=True)
        assert p.returncode == 3, p.stdout + p.stderr
        assert word in p.stdout and "setMinSumCorrection" in p.stdout, p.stdout
