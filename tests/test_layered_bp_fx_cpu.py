"""Fixed-point layered box-plus (algo = layered_bp_fx, LDPC_ALGO_LAYERED_BP_FX) without a device: the correction table the
library hands out, the properties of the integer box-plus, the rule by hand, the premises of the GPU cases shown on the
reference (tests/layered_bp_fx_ref.py), the config field, every refusal that is decided in front of the device, and the
premise of the feature: what the table is worth at a hardware width."""
import ctypes

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, codes

import bp_cases as bc
import kernel_matrix as km
import layered_bp_fx_cases as bx
import layered_bp_fx_ref as BX
import layered_bp_ref as LB
import layered_fx_cases as xc
import layered_fx_ref as FX
from ms_correction_ref import Code

f32 = np.float32
I32 = np.int32
LDPC_OK, LDPC_ERR_ARG, LDPC_ERR_HIP, LDPC_ERR_UNSUPPORTED = 0, 1, 2, 4
WIDTHS = (4, 5, 6, 8)


# ---- the table -------------------------------------------------------------------------------------------------------

def test_table_is_the_rounded_double_formula_and_far_from_every_tie(built):
    """T_f[d] = floor(2^f log(1 + exp(-d / 2^f)) + 0.5) for f = 0 ... 4, cut at its first 0; no value in front of the floor
    lies within 1e-6 of an integer, so no libm can round an entry the other way; the table does not increase."""
    sizes = {}
    for f in range(5):
        t = L.bp_fx_table(f)
        d = np.arange(t.size + 8, dtype=np.float64)
        raw = 2.0 ** f * np.log(1.0 + np.exp(-d / 2.0 ** f)) + 0.5
        want = np.floor(raw).astype(I32)
        assert np.array_equal(t, want[:t.size]), (f, t.tolist())
        assert t[-1] == 0 and (t[:-1] > 0).all() and (want[t.size:] == 0).all(), f
        assert (np.diff(t) <= 0).all(), f
        dist = np.abs(raw - np.rint(raw)).min()
        print("f = %d: %d entries, T[0] = %d, nearest tie %.3g away" % (f, t.size, t[0], dist))
        assert dist > 1e-6, (f, dist)
        sizes[f] = t.size
    assert L.bp_fx_table(0).tolist() == [1, 0]
    assert sizes[4] == 57 and L.bp_fx_table(4)[0] == 11
    assert L.bp_fx_table(2).tolist() == [3, 2, 2, 2, 1, 1, 1, 1, 1, 0]           # the table of the cases by hand below


def test_table_entry_point_arguments(built):
    lib = _lib.load()
    n = ctypes.c_int32(-1)
    i32p = ctypes.POINTER(ctypes.c_int32)
    for f in (-1, 5, 100):
        assert lib.ldpc_bp_fx_table(f, None, 0, ctypes.byref(n)) == LDPC_ERR_ARG and n.value == 0, f
    assert lib.ldpc_bp_fx_table(2, None, 0, None) == LDPC_ERR_ARG
    assert lib.ldpc_bp_fx_table(2, None, 0, ctypes.byref(n)) == LDPC_OK and n.value == 10      # the count alone
    buf = np.full(12, -7, I32)
    assert lib.ldpc_bp_fx_table(2, buf.ctypes.data_as(i32p), 9, ctypes.byref(n)) == LDPC_ERR_ARG and n.value == 10
    assert (buf == -7).all()                                                                    # too short: nothing written
    assert lib.ldpc_bp_fx_table(2, buf.ctypes.data_as(i32p), 10, ctypes.byref(n)) == LDPC_OK
    assert buf[:10].tolist() == L.bp_fx_table(2).tolist() and (buf[10:] == -7).all()


# ---- box-plus --------------------------------------------------------------------------------------------------------

def test_boxplus_properties_on_every_pair(built):
    """Over all pairs (a, b) of every width and every f: commutative, |a [+] b| <= min(|a|, |b|), a zero counts as positive
    (and a [+] 0 = 0), the sign of a non-zero result is the XOR of the signs -- and the value in front of the max with 0 is
    never negative, so the max only ever holds a 0 that the subtraction produced."""
    for f in range(5):
        for q in WIDTHS:
            Lq = FX.limit(q)
            v = np.arange(-Lq, Lq + 1, dtype=I32)
            a, b = np.meshgrid(v, v, indexing="ij")
            T = BX.padded(bx.table(f), q)
            st = {}
            r = BX.boxplus(a, b, T, st)
            assert np.array_equal(r, BX.boxplus(b, a, T)), (f, q)
            assert (np.abs(r) <= np.minimum(np.abs(a), np.abs(b))).all(), (f, q)
            assert (r[(a == 0) | (b == 0)] == 0).all(), (f, q)
            nz = r != 0
            assert ((r < 0) == ((a < 0) ^ (b < 0)))[nz].all(), (f, q)
            assert st["clipped"] == 0 and st["zero_g"] > 0, (f, q, st)
    T = BX.padded(bx.table(2), 6)
    assert BX.boxplus(0, -3, T) == 0 and BX.boxplus(-3, 0, T) == 0          # (0 < 0) is false: s = 1, g = 0
    assert BX.boxplus(1, 1, T) == 0 and BX.boxplus(-1, 1, T) == 0           # 1 + T[2] - T[0] = 1 + 2 - 3
    assert BX.boxplus(5, -3, T) == -2 and BX.boxplus(31, 31, T) == 28       # 3 + T[8] - T[2]; 31 + T[62] - T[0]


def test_row_with_an_all_zero_table_is_the_min_sum_row_of_layered_fx():
    """The anchor to the old rule: T = 0 makes a [+] b = sign * min, and the forward / backward association then gives
    layered_fx's plain row value for value -- rows of degree 1 (L), 2 and up to 30, zeros and ties among the inputs."""
    rng = np.random.default_rng(3)
    for q in WIDTHS:
        Lq = FX.limit(q)
        deg = np.concatenate([np.arange(1, 31), rng.integers(1, 31, 34)])
        valid = np.arange(30)[None, :] < deg[:, None]
        x = rng.integers(-Lq, Lq + 1, (50,) + valid.shape).astype(I32)
        x[rng.random(x.shape) < 0.1] = 0
        x = np.where(valid[None], x, 0).astype(I32)
        zero = BX.padded(np.zeros(1, I32), q)
        got = BX.row(x, valid, zero, q)
        want = np.where(valid[None], FX.row(x, valid, 0.0, 0.0, q), 0)
        assert np.array_equal(got, want), q
    # and the table changes it
    x = np.clip(x, -31, 31)
    assert not np.array_equal(BX.row(x, valid, BX.padded(bx.table(2), 6), 6), BX.row(x, valid, BX.padded(np.zeros(1, I32), 6), 6))


# ---- by hand, f = 2 (T = 3 2 2 2 1 1 1 1 1 0), q = 6 -----------------------------------------------------------------

def _row(x, f=2, q=6):
    x = np.asarray(x, I32)[None, None, :]
    return BX.row(x, np.ones((1, x.shape[2]), bool), BX.padded(bx.table(f), q), q)[0, 0].tolist()


def test_one_row_by_hand(built):
    """x = (5, -3, 12):  F_1 = 5 [+] -3 = -(3 + T[8] - T[2]) = -2;  B_1 = -3 [+] 12 = -(3 + T[15] - T[9]) = -3;
    R_0 = B_1 = -3,  R_1 = F_0 [+] B_2 = 5 [+] 12 = 5 + T[17] - T[7] = 4,  R_2 = F_1 = -2.  Min-sum gives (-3, 5, -3)."""
    assert _row([5, -3, 12]) == [-3, 4, -2]
    # a zero counts as positive, stays a zero through every box-plus, and does not kill the row:
    # R_0 = -3 [+] 3 = -(3 + T[6] - T[0]) = -1
    assert _row([0, -3, 3]) == [-1, 0, 0]
    assert _row([7, -9]) == [-9, 7]                             # degree 2: each edge gets the other
    for q in WIDTHS:
        assert _row([-3], q=q) == [FX.limit(q)]                 # degree 1: +L
    assert _row([31, -31, 31]) == [-28, 28, -28]                # 31 + T[62] - T[0]


def test_two_rounds_by_hand(built):
    """Rows (0, 1, 2) and (0, 1, 3), every row a layer, channel values 5, -3, 12, 6 LSB, q = 6, p = 8, f = 2.
    Round 1: row 0 on t = (5, -3, 12) gives R = (-3, 4, -2) and P = (2, 1, 10, 6); row 1 on t = (2, 1, 6) gives
    R = (1, 2, 1) and P = (3, 3, 10, 7).  Round 2: row 0 on t = (6, -1, 12) gives R = (-1, 5, -1) and P = (5, 4, 11, 7);
    row 1 on t = (4, 2, 6) gives R = (2, 2, 1) and P = (6, 4, 11, 7)."""
    code = Code([0, 0, 0, 1, 1, 1], [0, 1, 2, 0, 1, 3], 2, 4, 2)
    y = np.array([[5, -3, 12, 6]], f32)
    one = BX.layered_bp_fx(code, y, 1, 1, bx.table(2), q=6, p=8, tap_iter=1, early_term=False)
    assert one["c"].tolist() == [[5, -3, 12, 6]]
    assert one["r_tap"].tolist() == [[-3, 4, -2, 1, 2, 1]] and one["p_tap"].tolist() == [[3, 3, 10, 7]]
    two = BX.layered_bp_fx(code, y, 1, 2, bx.table(2), q=6, p=8, tap_iter=2, early_term=False)
    assert two["r_tap"].tolist() == [[-1, 5, -1, 2, 2, 1]] and two["p_tap"].tolist() == [[6, 4, 11, 7]]
    assert two["iters"].tolist() == [2] and two["hard"].tolist() == [[0, 0, 0, 0]]
    # with early termination the frame stops in round 1: its bits are a codeword
    assert BX.layered_bp_fx(code, y, 1, 2, bx.table(2), q=6, p=8)["iters"].tolist() == [1]
    # the posterior memory saturates as in layered_fx: channel values at L, p = q
    y = np.full((1, 4), 31, f32)
    w = BX.layered_bp_fx(code, y, 1, 1, bx.table(2), q=6, p=6, tap_iter=1)
    assert w["p_tap"].tolist() == [[31, 31, 31, 31]] and w["sat"][0] == 6 and w["peak_sum"][0] == 31 + 28


# ---- premises of the GPU cases ---------------------------------------------------------------------------------------

def test_premises_of_the_saturation_cases(built):
    """On the overlay over WiMAX (576, 288): |t_k| beyond L at every width; P at +-LP and clamped writes with p = q and with
    p = q + 2, none with p = 16; box-plus results that are 0 although neither input is."""
    for q, p, f in bx.SATURATION_WIDTHS:
        w = bx.saturation_want(q, p, f)
        print(q, p, f, "peak |t| %d, writes at +-LP %d, clamped writes %d, g = 0 from non-zero inputs %d"
              % (w["peak_t"].max(), w["at_limit"].sum(), w["sat"].sum(), w["zero_g"]))
        assert w["peak_t"].max() > FX.limit(q), (q, p, f)
        assert (w["iters"] >= bx.TAP).sum() >= 20 and np.unique(w["iters"]).size >= 2, (q, p, f)
        assert w["zero_g"] > 0 and w["clipped"] == 0, (q, p, f)
        if p <= q + 2:
            assert w["at_limit"].sum() > 0 and w["sat"].sum() > 0, (q, p, f)
        if p == 16:
            assert w["sat"].sum() == 0
        y = bx.saturation_inputs(q)
        assert (w["c"][np.isnan(y)] == 0).all() and np.isnan(y).sum() == 5
        assert (w["c"][np.isposinf(y)] == FX.limit(q)).all() and (w["c"][np.isneginf(y)] == -FX.limit(q)).all()


def test_premises_of_the_bg1_and_matrix_cases(built):
    """The BG1 batch holds frames stopping in each of the rounds 1, 2, 3, 4 and frames that never stop, at both widths; the
    result differs from layered_fx at the same q and p; q = 6 / p = 8 saturates and q = 8 / p = 16 does not; the matrix code
    has a row of every degree 1 ... 24 and rows above 24."""
    c = bx.bg1_code()
    for frames in (70, bx.BG1_TWO_TILES):
        for q, p, f in bx.WIDTHS:
            w = bx.bg1_want(frames, q, p, f)
            assert {1, 2, 3, 4} <= set(w["iters"].tolist()), (frames, q, p, f)
            assert (~c["code"].syndrome_ok(w["hard"])).sum() >= 1 and (w["iters"] == bx.BG1_MAXIT).any()
            assert (w["sat"].sum() > 0) == (p == 8)
            assert w["zero_g"] > 0
            ms = xc.bg1_want(frames, q, p, False)
            assert not np.array_equal(w["r_tap"], ms["r_tap"]) and not np.array_equal(w["iters"], ms["iters"]), (frames, q, p, f)
            assert not np.array_equal(w["out"], ms["out"]), (frames, q, p, f)
    m = bx.matrix()
    rd, _ = km.degree_maps(m["rows"], m["cols"], m["M"], m["N"])
    assert set(range(1, 25)) <= set(rd) and max(rd) > 24
    for q, p, f in bx.WIDTHS:
        w = bx.matrix_want(q, p, f)
        assert (w["iters"] >= bx.TAP).sum() >= 10 and (w["iters"] < bx.TAP).sum() >= 10      # frames on both sides of the tap


def test_premises_of_the_crc_and_typed_cases(built):
    kind, bits, y, w = bx.crc_case()
    assert w["by_stop"].size >= 1                               # frames the CRC stops before the syndrome is clean
    assert np.unique(w["iters"]).size >= 4
    for k in ("i8", "f16"):
        assert np.unique(bx.typed_want(k, 6, 8, 2)["iters"]).size >= 4
    assert not np.array_equal(bx.typed_want("f16", 6, 8, 2)["post"], bx.bg1_want(70, 6, 8, 2)["post"])   # the rounding shows


# ---- bindings and refusals that precede device use -------------------------------------------------------------------

def _cfg(**kw):
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    cfg = _lib.DecoderConfigMsg()
    assert _lib.load().ldpc_decoder_config_init_sized(ctypes.byref(cfg), ctypes.sizeof(cfg)) == LDPC_OK
    cfg.K, cfg.max_batch, cfg.algo, cfg.layer_rows = K, 64, L.capi.ALGOS["layered_bp_fx"], z
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


def test_bp_frac_bits_takes_the_second_reserved_word(built):
    F, G = _lib.DecoderConfigCrc, _lib.DecoderConfigMsg
    cfg = _cfg()
    assert cfg.bp_frac_bits == 0 and cfg.post_bits == 0 and list(cfg.msg_reserved) == [0, 0, 0]
    assert cfg.struct_size == ctypes.sizeof(G) == ctypes.sizeof(F) + 16
    assert G.post_bits.offset == G.msg_reserved.offset == G.msg_bits.offset + 4
    assert G.bp_frac_bits.offset == G.msg_reserved.offset + 4 and G.msg_reserved3.offset == G.msg_reserved.offset + 8
    cfg.bp_frac_bits, cfg.post_bits = 3, 11
    assert list(cfg.msg_reserved) == [11, 3, 0]
    cfg.msg_reserved[1] = 2
    assert cfg.bp_frac_bits == 2 and cfg.post_bits == 11
    A = L.capi.ALGOS
    assert A["layered_bp_fx"] == 9 and 9 in A.values() and 7 not in A.values() and A["layered_fx"] == 8
    assert _lib.load().ldpc_abi_version() == 3


def test_refusals_in_front_of_the_device(graph):
    """Every refusal of the definition is decided before a device is looked for; the accepted forms get as far as the
    device."""
    A = L.capi.ALGOS
    rc, msg = _create(_cfg(algo=7), graph)
    assert rc == LDPC_ERR_ARG and "unknown algo" in msg
    for f in (-1, 5, 8, 1 << 20):
        rc, msg = _create(_cfg(msg_bits=6, post_bits=8, bp_frac_bits=f), graph)
        assert rc == LDPC_ERR_ARG and "bp_frac_bits" in msg, (f, msg)
    # bp_frac_bits belongs to this algorithm alone
    for algo, kw in (("layered_fx", {}), ("ms", {}), ("ms", dict(msg_dtype=L.capi.MSG_F32)), ("layered", dict(msg_dtype=L.capi.MSG_F32)),
                     ("bp", dict(msg_dtype=L.capi.MSG_F32)), ("layered_bp", dict(msg_dtype=L.capi.MSG_F32)),
                     ("sp", dict(msg_dtype=L.capi.MSG_F32))):
        rc, msg = _create(_cfg(algo=A[algo], bp_frac_bits=2, **kw), graph)
        assert rc == LDPC_ERR_ARG and "bp_frac_bits" in msg, (algo, msg)
    cfg = _cfg(msg_bits=6, bp_frac_bits=2)                      # the last word stays reserved
    cfg.msg_reserved[2] = 1
    assert _create(cfg, graph)[0] == LDPC_ERR_ARG
    # a non-zero correction: there is no minimum to correct
    for corr in (dict(ms_scale=0.75), dict(ms_offset=1.0), dict(ms_scale=0.75, ms_offset=1.0)):
        rc, msg = _create(_cfg(msg_bits=6, post_bits=8, bp_frac_bits=2, **corr), graph)
        assert rc == LDPC_ERR_UNSUPPORTED and "ms_scale" in msg, (corr, msg)
    for tune in ({"fused": True}, {"ldsp": True}, {"fused": True, "ldsp": True}):
        rc, msg = _create(_cfg(msg_bits=6, post_bits=8, bp_frac_bits=2, tune=tune), graph)
        assert rc == LDPC_ERR_UNSUPPORTED and "fixed-point" in msg, (tune, msg)
    # the LDPC_ERR_ARG cases of layered_fx, unchanged
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
    # a struct shorter than the full size means bp_frac_bits = 0: the bytes behind it are not read
    cfg = _cfg(algo=A["ms"], msg_dtype=L.capi.MSG_F32, bp_frac_bits=77)
    cfg.struct_size = ctypes.sizeof(_lib.DecoderConfigCrc)
    assert _create(cfg, graph)[0] in (LDPC_OK, LDPC_ERR_HIP)
    # the accepted forms
    for q, p in ((0, 0), (4, 4), (4, 16), (5, 7), (6, 8), (6, 6), (8, 8), (8, 16), (8, 0)):
        for f in range(5):
            rc, msg = _create(_cfg(msg_bits=q, post_bits=p, bp_frac_bits=f), graph)
            assert rc in (LDPC_OK, LDPC_ERR_HIP), (q, p, f, msg)
    assert _create(_cfg(msg_bits=6, post_bits=8, bp_frac_bits=2, early_term=0), graph)[0] in (LDPC_OK, LDPC_ERR_HIP)
    # the Python layer: the name and the keywords reach the struct
    try:
        dec = L.Decoder(graph, 288, max_batch=64, algo="layered_bp_fx", msg_dtype="i8", msg_bits=6, post_bits=8, bp_frac_bits=2,
                        layer_rows=24, llr_scale=8.0)
        assert dec.cfg.algo == 9 and dec.cfg.msg_bits == 6 and dec.cfg.post_bits == 8 and dec.cfg.bp_frac_bits == 2
        dec.close()
    except L.LdpcError as e:
        assert e.code == LDPC_ERR_HIP
    with pytest.raises(L.LdpcError) as e:
        L.Decoder(graph, 288, max_batch=64, algo="layered_bp_fx", msg_dtype="i8", msg_bits=6, post_bits=8, bp_frac_bits=5,
                  layer_rows=24)
    assert e.value.code == LDPC_ERR_ARG


# ---- the premise of the feature --------------------------------------------------------------------------------------

def test_the_table_recovers_most_of_what_min_sum_loses_at_six_bits(built):
    """WiMAX (576, 288), 2000 frames at 2.0 dB on the same noise, 20 rounds, the reference alone: layered_bp_fx at q = 6, p = 8,
    f = 2 (llr_scale = 4 * 2 / sd^2: the LLR in quarter units) against plain layered_fx at the same widths and scale, and
    against the float layered_bp (llr_scale = 2 / sd^2).  Measured: 41, 212 and 34 frame errors."""
    rate, N = codes.RATE_1_2, 576
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    code = Code(rows, cols, M, N, K)
    y, sd = bc.wimax_frames(N, 2000, 2.0, 5)
    llr = 2.0 / sd ** 2

    def errors(w):
        return int(w["hard"].any(axis=1).sum())                 # the all-zero codeword was sent

    bpfx = errors(BX.layered_bp_fx(code, y, z, 20, bx.table(2), q=6, p=8, llr_scale=4.0 * llr))
    fx = errors(FX.layered_fx(code, y, z, 20, q=6, p=8, llr_scale=4.0 * llr))
    bp = errors(LB.layered_bp(code, y, z, 20, llr_scale=llr))
    counts = "frame errors of 2000: layered_bp_fx %d, layered_fx %d, layered_bp (fp32) %d" % (bpfx, fx, bp)
    print(counts)
    assert bp <= bpfx < fx, counts
