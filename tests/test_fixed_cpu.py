"""CPU side of fixed-point messages (msg_dtype = i8): the integer restatement (tests/fixed_ref.py) against the oracle
where no message saturates, a check row by hand, every edge of the store rule sq, the premises of the GPU cases
(tests/test_gpu_fixed.py), and the bindings and refusals that precede any use of a device.  Every test prints the counts
it found (pytest -s shows them)."""
import ctypes

import numpy as np
import pytest

import oracle
from oracle import refkernels
import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, channel, codes

import fp16_cases as fc
import fixed_cases as fxc
import fixed_ref as RI
from ms_correction_ref import Code

f32 = np.float32
LDPC_OK, LDPC_ERR_ARG, LDPC_ERR_HIP, LDPC_ERR_UNSUPPORTED = 0, 1, 2, 4


# ---- the anchor -----------------------------------------------------------------------------------------------------

def _anchor_case():
    """WiMAX (576, 288), no row of degree 1; 48 frames of integer channel values around +2 (BPSK 1 plus noise of 0.7,
    times 2, rounded): small enough that nothing reaches 127 within 10 rounds"""
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    y = np.rint(channel.awgn_frames(N, 0, 48, 0.7, seed=5) * f32(2)).astype(f32)
    return rows, cols, M, N, K, y


def test_anchor_where_nothing_saturates_it_is_the_oracles_min_sum():
    """Integer channel values, q = 8, llr_scale 1: no channel value and no P - R of any frame in any round reaches 127 (no
    frame is excluded), so the store rule never acts and the integer reference must equal float min-sum: the reference's
    own kernels (oracle.refkernels, where the reference is present) and the C oracle, in bytes, iteration counts, hard
    bits and the R and Q values after round 2."""
    rows, cols, M, N, K, y = _anchor_case()
    assert np.bincount(rows, minlength=M).min() >= 2
    maxit = 10
    got = RI.flood(Code(rows, cols, M, N, K), y, maxit, q=8, llr_scale=1.0, tap_iter=fc.TAP)
    print("anchor: largest |c| %d, largest |P - R| %d, rounds %s" % (np.abs(y).max(), got["peak"].max(), np.bincount(got["iters"])))
    assert np.abs(y).max() < 127 and got["peak"].max() < 127 and got["peak"].min() > 0
    assert np.array_equal(got["c"], y.astype(np.int32))
    run_r, run_q = fc.tap_frames(got["iters"])
    assert run_q.size >= 10 and np.unique(got["iters"]).size >= 3
    want = fc.as_ref(oracle.decode(oracle.Graph(rows, cols, M, N, K), y, "ms", max_iter=maxit, tap_iter=fc.TAP))
    for key in ("out", "iters", "hard"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(fxc.as_float(got["r_tap"][run_r]), want["r_tap"][run_r])
    assert np.array_equal(fxc.as_float(got["q_tap"][run_q]), want["q_tap"][run_q])
    if refkernels.available():
        ref = refkernels.decode(refkernels.RefGraph(rows, cols, M, N, K), y, "ms", times=maxit, tap_iter=fc.TAP)
        assert np.array_equal(got["out"], ref["out"]) and np.array_equal(got["hard"], ref["hard"])
        assert ref["time"] == got["iters"].max()
        assert np.array_equal(fxc.as_float(got["r_tap"][run_r]), ref["taps"]["r"][run_r])
        assert np.array_equal(fxc.as_float(got["q_tap"][run_q]), ref["taps"]["q"][run_q])
        print("anchor: equal to the reference's kernels as well")


def test_a_check_row_by_hand():
    """One row of degree 3 and one of degree 1.  Plain: R = sign * min of the others, the degree-1 row gives L.  Corrected
    with ms_scale 0.75: exactly (3 m) >> 2 for every m = 0 .. 127; with an offset of 0.15 LSB: m - 1 (0 stays 0)."""
    code = Code(np.array([0, 0, 0, 1]), np.array([0, 1, 2, 3]), 2, 4, 1)
    Q = np.array([[5, -3, 9, -2]], np.int32)
    for q in RI.WIDTHS:
        Lq = RI.limit(q)
        Qq = np.clip(Q, -Lq, Lq)
        a = np.abs(Qq[0])
        assert RI._check(code, Qq, 0.0, 0.0, q).tolist() == [[-3, min(5, Lq), -3, Lq]], q
        r = RI._check(code, Qq, 0.75, 0.0, q)
        assert r.tolist() == [[-((3 * 3) >> 2), (3 * a[0]) >> 2, -((3 * 3) >> 2), min((3 * 1000) >> 2, Lq)]], q
    m = np.arange(128)
    assert np.array_equal(RI.corrected(m, 0.75, 0.0, 8), (3 * m) >> 2)
    assert np.array_equal(RI.corrected(m, 0.0, 0.15, 8), np.maximum(m - 1, 0))
    assert np.array_equal(RI.corrected(m, 0.8, 0.05, 8), np.trunc((np.maximum(m.astype(f32) - f32(0.05), 0) * f32(0.8)).astype(f32)))
    for q in RI.WIDTHS:
        assert RI.corrected(np.array([1000]), 0.75, 0.0, q)[0] == RI.limit(q)


@pytest.mark.parametrize("q", RI.WIDTHS)
def test_every_edge_of_sq(q):
    """Ties at +-0.5, +-1.5, +-2.5 go to even; L and L + 0.49 give L, L + 0.5 and 1000 and +inf give L (their negatives -L);
    NaN gives 0; -0 and an fp32 denormal give 0; the result is an int32 in [-L, L] whatever comes in."""
    Lq = RI.limit(q)
    want = {0.5: 0, -0.5: 0, 1.5: 2, -1.5: -2, 2.5: 2, -2.5: -2, 3.5: 4, Lq: Lq, Lq + 0.49: Lq, Lq + 0.5: Lq, 1000: Lq,
            np.inf: Lq, -np.inf: -Lq, -1000: -Lq, -(Lq + 0.5): -Lq, -Lq: -Lq, np.nan: 0, -0.0: 0, 1e-41: 0, -1e-41: 0, Lq - 0.5: Lq - 1 + (Lq - 1) % 2,
            128: Lq, 255: Lq, 256: Lq, -128: -Lq, 3.4e38: Lq}
    for k, v in want.items():
        got = RI.sq(f32(k), q)
        assert got.dtype == np.int32 and got == v, (q, k, int(got), v)
    x = RI.edge_inputs(q)
    s = RI.sq(x, q)
    assert s.min() == -Lq and s.max() == Lq
    fin = np.isfinite(x)
    # nearest integer, of two equally near ones the even one, then the clamp: in exact rational arithmetic (float64 holds them)
    xd = x[fin].astype(np.float64)
    fl = np.floor(xd)
    near = np.where(xd - fl < 0.5, fl, np.where(xd - fl > 0.5, fl + 1, np.where(fl % 2 == 0, fl, fl + 1)))
    assert np.array_equal(s[fin], np.clip(near, -Lq, Lq).astype(np.int32))
    assert np.array_equal(RI.sq(np.arange(-300, 301), q), np.clip(np.arange(-300, 301), -Lq, Lq))
    assert np.array_equal(RI.channel_values(np.array([1.0, -0.3, 0.31], f32), 8.0, q), np.clip([8, -2, 2], -Lq, Lq))


# ---- the premises of the GPU cases ----------------------------------------------------------------------------------

@pytest.mark.parametrize("d,q", fxc.FUSED_CASES)
def test_premises_of_the_column_fused_cases(d, q):
    """On staircase(d), 133 frames, 25 rounds, under the fixed-point rule at q bits, plain and with each correction: frames
    stop at several distinct rounds, at least one frame compares its Q tap, messages saturate (some |P - R| exceeds L), the
    result differs from the fp16 expectation (a kernel that silently ran another type would fail), and -- corrected
    min-sum -- the model of a kernel that forgets MsgRound in the column-fused registers changes the Q tap of at least one
    compared frame.  Plain min-sum has no such model on these codes: without a row of degree 1 every R is +-|q| of a stored
    message, and the start value is never read."""
    c = fc.staircase(d, "ride")
    assert np.bincount(c["rows"], minlength=c["M"]).min() >= 2
    for setting in (None,) + fc.SETTINGS:
        w = fxc.want(d, q, "ride", setting)
        it = w["iters"]
        run_r, run_q = fc.tap_frames(it)
        differ16 = int((it != fc.want(d, "ride", setting)["iters"]).sum())
        sat = int((w["peak"] > RI.limit(q)).sum())
        print("d=%d q=%d %s: %d distinct rounds, %d frames compare Q, %d frames saturate, iterations differ from fp16 in %d frames"
              % (d, q, setting, np.unique(it).size, run_q.size, sat, differ16))
        assert np.unique(it).size >= 2 and run_q.size >= 1 and sat >= 1 and differ16 >= 1, (d, q, setting)
        assert np.abs(w["q_tap"][run_q]).max() == RI.limit(q) and np.abs(w["r_tap"][run_r]).max() <= RI.limit(q)
        if setting is None:
            continue
        bad = fxc.want_registers_raw(d, q, setting)
        q_frames = [f for f in run_q if not np.array_equal(bad["q_tap"][f], w["q_tap"][f])]
        print("    MsgRound forgotten in registers: Q tap differs in %d of %d compared frames" % (len(q_frames), run_q.size))
        assert len(q_frames) >= 1, (d, q, setting)


@pytest.mark.parametrize("q", (6, 8))
def test_premises_of_the_degenerate_cases(q):
    """The overlay reaches every edge of sq in the stored channel values; the frame of +-(L - 1) makes |P - R| > L in
    columns of degree 3 and more, and at q = 8 beyond 255, where a store that wrapped instead of clamping would show even
    if it clamped at the byte's own range."""
    Lq = RI.limit(q)
    for name in ("wimax", "ira"):
        y = fxc.degenerate_inputs(name, q)
        c = RI.channel_values(y, fxc.LLR_SCALE[q], q)
        assert (c[2] == Lq).sum() >= 40 and (c[3] == -Lq).sum() >= 40 and (c[4] == Lq).sum() >= 40 and (c[5] == Lq).sum() >= 40
        assert (c[6] == Lq).sum() >= 20 and (c[7] == -Lq).sum() >= 20 and (c[1] == 0).all()
        assert np.isnan(y[8]).sum() == 5 and (c[8][np.isnan(y[8])] == 0).all()
        assert set(np.unique(c[9])) >= {-2, 0, 2} and (c[13] == Lq - 1).sum() > (c[13] == -(Lq - 1)).sum() > 0
        for corrected in (False, True):
            w = fxc.degenerate_want(name, q, corrected)
            f = fxc.SATURATING_FRAME
            print(name, q, corrected, "the +-(L - 1) frame: rounds %d, largest |P - R| in columns of degree >= 3: %d" % (w["iters"][f], w["peak_deg3"][f]))
            assert w["iters"][f] > fc.TAP and w["peak_deg3"][f] > Lq
            assert (np.abs(w["q_tap"][f]) == Lq).sum() >= 1
            if q == 8:
                assert w["peak_deg3"][f] > 255


def test_premises_of_the_handover_case():
    """The hand-over batch leaves frames running: between 20 and 100 of the 700 run all rounds."""
    w = fxc.handover_want(fc.HANDOVER_BATCHES[0])
    full = int((w["iters"] == fc.HANDOVER_MAXIT).sum())
    print("hand-over: %d of %d frames run all rounds, %d converge" % (full, w["iters"].size, w["n_conv"]))
    assert 20 <= full <= fc.HANDOVER_STRAGGLERS + 10


# ---- bindings and refusals that precede device use -------------------------------------------------------------------

def _cfg(**kw):
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    cfg = _lib.DecoderConfigMsg()
    assert _lib.load().ldpc_decoder_config_init_sized(ctypes.byref(cfg), ctypes.sizeof(cfg)) == LDPC_OK
    cfg.K, cfg.max_batch, cfg.algo, cfg.layer_rows = K, 64, L.capi.ALGOS["ms"], z
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
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    return L.Graph(rows, cols, M, N)


def test_msg_bits_is_appended_and_defaults_to_zero(built):
    F, G = _lib.DecoderConfigCrc, _lib.DecoderConfigMsg
    cfg = _cfg()
    assert cfg.msg_bits == 0 and list(cfg.msg_reserved) == [0, 0, 0]
    assert G.msg_bits.offset == F.crc_bits.offset + 4 == ctypes.sizeof(F)
    assert cfg.struct_size == ctypes.sizeof(G) == ctypes.sizeof(F) + 16
    assert L.capi.MSG_I8 == 4 and _lib.load().ldpc_abi_version() == 3


def test_the_four_struct_sizes(graph):
    """offsetof(ms_scale), offsetof(crc_kind), offsetof(msg_bits) -- the full size before this feature: the bytes behind it
    are not read -- and the full size; the sizes in between stay an ABI mismatch."""
    before_ms, before_crc = _lib.DecoderConfig.ms_scale.offset, ctypes.sizeof(_lib.DecoderConfig)
    before_bits, full = ctypes.sizeof(_lib.DecoderConfigCrc), ctypes.sizeof(_lib.DecoderConfigMsg)
    cfg = _cfg(msg_bits=77)                                      # would be refused if it were read
    for size in (before_ms, before_crc, before_bits):
        cfg.struct_size = size
        assert _create(cfg, graph)[0] in (LDPC_OK, LDPC_ERR_HIP), size
    for size in (before_bits + 4, before_bits + 8, before_bits + 12, full + 4, 0):
        cfg.struct_size = size
        rc, msg = _create(cfg, graph)
        assert rc == LDPC_ERR_ARG and "struct_size" in msg, size
    cfg.struct_size = full
    rc, msg = _create(cfg, graph)
    assert rc == LDPC_ERR_ARG and "msg_bits" in msg
    lib = _lib.load()
    buf = (ctypes.c_uint8 * (full + 16))(*([0xA5] * (full + 16)))
    ptr = ctypes.cast(buf, ctypes.POINTER(_lib.DecoderConfigMsg))
    for size in (before_bits, full):
        assert lib.ldpc_decoder_config_init_sized(ptr, size) == LDPC_OK
        assert ptr.contents.struct_size == size and bytes(buf[size:]) == b"\xa5" * (len(buf) - size)
        assert bytes(buf[before_crc:size]) == b"\0" * (size - before_crc)
        for i in range(len(buf)):
            buf[i] = 0xA5


def test_refusals_in_front_of_the_device(graph):
    """An unknown width, a width with another message type, a reserved word set, i8 with every other algorithm, and an
    llr_scale that is no positive finite number: all refused before a device is looked for; the accepted forms get as far
    as the device."""
    I8 = L.capi.MSG_I8
    for bits in (1, 2, 3, 7, 9, 16, -4):
        rc, msg = _create(_cfg(msg_dtype=I8, msg_bits=bits), graph)
        assert rc == LDPC_ERR_ARG and "msg_bits" in msg, bits
    for dtype in (L.capi.MSG_F32, L.capi.MSG_F16, L.capi.MSG_F8):
        rc, msg = _create(_cfg(msg_dtype=dtype, msg_bits=6), graph)
        assert rc == LDPC_ERR_ARG and "msg_bits" in msg, dtype
    cfg = _cfg(msg_dtype=I8, msg_bits=6)
    cfg.msg_reserved[1] = 1
    assert _create(cfg, graph)[0] == LDPC_ERR_ARG
    for algo in ("sp", "layered", "ms_fused", "layered_host", "bp", "layered_bp"):
        rc, msg = _create(_cfg(msg_dtype=I8, msg_bits=6, algo=L.capi.ALGOS[algo]), graph)
        # LAYERED_HOST on this code is refused even earlier, for its unequal row weights, with the same code
        assert rc == LDPC_ERR_UNSUPPORTED and ("fixed-point" in msg or algo == "layered_host"), (algo, msg)
    for s in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        rc, msg = _create(_cfg(msg_dtype=I8, msg_bits=6, llr_scale=s), graph)
        assert rc == LDPC_ERR_ARG and "llr_scale" in msg, s
    for unknown in (3, 5, -1):                                   # 3 is not assigned: it stays the unknown value it always was
        rc, msg = _create(_cfg(msg_dtype=unknown), graph)
        assert rc == LDPC_ERR_ARG and "msg_dtype" in msg, unknown
    for bits in (0, 4, 5, 6, 8):
        assert _create(_cfg(msg_dtype=I8, msg_bits=bits, llr_scale=4.0), graph)[0] in (LDPC_OK, LDPC_ERR_HIP), bits
    # the Python layer: the name and the keyword reach the struct
    try:
        dec = L.Decoder(graph, 288, max_batch=64, algo="ms", msg_dtype="i8", msg_bits=5, llr_scale=4.0)
        assert dec.cfg.msg_dtype == I8 and dec.cfg.msg_bits == 5
        dec.close()
    except L.LdpcError as e:
        assert e.code == LDPC_ERR_HIP
    with pytest.raises(L.LdpcError) as e:
        L.Decoder(graph, 288, max_batch=64, algo="ms", msg_dtype="i8", msg_bits=7)
    assert e.value.code == LDPC_ERR_ARG
