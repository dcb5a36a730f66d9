"""Typed channel values -- int8 and fp16 input for every decode entry point -- on the GPU.

One scheme throughout: tests/typed_input_ref.py dequantises the caller's buffer in numpy, y = x.astype(float32) *
float32(unit), and the expectation is the CPU reference of the algorithm on that y (oracle.decode, fp8_ref, bp_ref,
layered_bp_ref, soft_ref) -- never the GPU's own float path.  That the handle's float entry point gives the same on the
same y is asserted in addition.  Everything is compared on bit patterns.  Every test needs the new entry points and fails
without them."""
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, codes

import arena_cases as ac
import bp_ref as RB
import fp16_cases as fc
import handover_cases as hc
import layered_bp_ref as LB
import oracle
import soft_ref as SR
import typed_input_ref as T
from util import kernel_choice, host_channel_lib

pytestmark = pytest.mark.gpu

F32 = np.float32
LDPC_ERR_ARG = 1
OFFSETS = (0, 1, 3)                 # element offsets of the caller's buffer inside a larger device allocation


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _place(x, offset, fill=0x7F):
    """The array's bytes at element offset `offset` of a larger device allocation whose other bytes are `fill`;
    returns (tensor that owns the memory, device address of the first element)"""
    import torch
    raw = np.ascontiguousarray(x).view(np.uint8).ravel()
    lead = offset * x.itemsize
    host = np.full(lead + raw.size + 64, fill, np.uint8)
    host[lead:lead + raw.size] = raw
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + lead


def _typed(dec, ptr, kind, frames, K, soft=None):
    """one ldpc_decode_typed_device (or its soft form) call: (bytes, iters[, soft values])"""
    import torch
    nb = L.out_bytes(K, frames)
    out = torch.full((nb + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    it = torch.full((frames + 4,), -7, dtype=torch.int32, device="cuda")
    kw = {}
    if soft is not None:
        sv = torch.full((frames * dec.N + 8,), float("nan"), dtype=torch.float32, device="cuda")
        kw = dict(soft_ptr=sv.data_ptr(), soft_floats=frames * dec.N, soft=soft)
    if kind != "f32":               # "f32": the plain entry point, ldpc_decode_device / ldpc_decode_soft_device
        kw.update(llr_type=kind, llr_unit=T.UNITS[kind])
    dec.decode_device(ptr, frames, out.data_ptr(), nb, it.data_ptr(), _stream(), **kw)
    torch.cuda.synchronize()
    o, i = out.cpu().numpy(), it.cpu().numpy()
    assert (o[nb:] == 0xEE).all() and (i[frames:] == -7).all()
    if soft is None:
        return o[:nb], i[:frames]
    s = sv.cpu().numpy()
    assert np.isnan(s[frames * dec.N:]).all()
    return o[:nb], i[:frames], s[:frames * dec.N].reshape(frames, dec.N)


# ---- the streaming flooding engine ----------------------------------------------------------------------------------

@pytest.mark.parametrize("cname", T.FLOOD_CODES)
@pytest.mark.parametrize("algo,storage", T.FLOOD_ARITH, ids=["%s-%s" % a for a in T.FLOOD_ARITH])
def test_flooding_streaming_reads_typed_rows(built, algo, storage, cname):
    """sp, ms (f32 / f16 / f8 messages) and bp (f32 / f16) at 1, 2 and 4 frames per lane, 64 V + 5 frames (a full tile and
    a ragged one), int8 and fp16 input at element offsets 0, 1 and 3 of a larger allocation.  (576, 288): the row stride
    allows 16-byte loads for both types (at offset 0); (648, 324): int8 rows are no 16-byte multiples; the matrix code:
    N = 583, every path per element and a ragged last patch.  Bytes, iteration counts, the stored channel term (tap 2) and
    all N hard bits after round TAP (tap 3) against the CPU reference; and the float entry point on the same y."""
    import torch
    c = T.code(cname)
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    scale = T.llr_scale(algo, cname)
    for V in (1, 2, 4):
        frames = 64 * V + 5
        dec = L.Decoder(g, c["K"], max_batch=frames, algo=algo, msg_dtype=storage, max_iter=T.MAXIT, frames_per_lane=V,
                        llr_scale=scale)
        for kind in ("i8", "f16"):
            w = T.head(T.flood_want(cname, kind, algo, storage), frames, c["K"])
            x = T.inputs(cname, kind)[:frames]
            for off in OFFSETS:
                what = (algo, storage, cname, V, kind, off)
                keep, ptr = _place(x, off)
                out, iters = _typed(dec, ptr, kind, frames, c["K"])
                assert np.array_equal(iters, w["iters"]), ("iterations",) + what
                assert np.array_equal(out, w["out"]), ("bytes",) + what
                dec.set_tap(T.TAP)
                _typed(dec, ptr, kind, frames, c["K"])
                assert fc.same_floats(dec.dump(2, frames), w["chan"]), ("tap 2: channel term",) + what
                assert np.array_equal(dec.dump(3, frames).astype(np.uint8), w["hard_tap"]), ("tap 3: bits",) + what
                dec.set_tap(0)
            y = torch.from_numpy(T.values(cname, kind)[:frames].copy()).cuda()
            out, iters = _typed(dec, y.data_ptr(), "f32", frames, c["K"])
            assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), ("float entry point", V, kind)
        dec.close()


# ---- the streaming layered engine -----------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ["layered", "layered_host", "layered_bp"])
def test_layered_streaming_reads_typed_rows(built, algo):
    """layered and layered_bp on the BG1-profile test code (N = 1088, z = 16), layered_host on WiMAX N = 576 at rate 5/6
    (uniform row weight, where it is defined); 64 * 4 + 6 frames at 4 frames per lane, both input types, offsets 0 and 1.
    Bytes, iteration counts, P after round TAP and the bits."""
    import torch
    c = T.layered_code(algo)
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    frames = T.LAYERED_FRAMES
    dec = L.Decoder(g, c["K"], max_batch=frames, algo=algo, max_iter=T.MAXIT, frames_per_lane=4, layer_rows=c["z"],
                    llr_scale=T.llr_scale("bp", c["name"]), tune=kernel_choice("0"))
    for kind in ("i8", "f16"):
        w = T.layered_want(algo, kind)
        ok = ~w["undefined"]
        run = np.nonzero((w["iters"] >= T.TAP) & ok)[0]
        early = np.nonzero((w["iters"] < T.TAP) & ok)[0]
        assert run.size > 0
        x = T.inputs(c["name"], kind, frames)
        for off in (0, 1):
            what = (algo, kind, off)
            keep, ptr = _place(x, off)
            dec.set_timing(True)
            out, iters = _typed(dec, ptr, kind, frames, c["K"])
            names = {k["name"] for k in dec.kernel_times()}
            dec.set_timing(False)
            assert any(n.startswith("layer_kernel") for n in names) and "llr_widen_kernel" not in names, (what, names)
            assert np.array_equal(iters[ok], w["iters"][ok]), ("iterations",) + what
            assert np.array_equal(out, w["out"]), ("bytes",) + what
            dec.set_tap(T.TAP)
            _typed(dec, ptr, kind, frames, c["K"])
            assert fc.same_floats(dec.dump(2, frames)[run], w["p_tap"][run]), ("P tap",) + what
            bits = dec.dump(3, frames).astype(np.uint8)
            assert np.array_equal(bits[run], w["hard_tap"][run]), ("bit tap",) + what
            assert np.array_equal(bits[early], w["hard"][early]), ("bits of the frames that had stopped",) + what
            dec.set_tap(0)
        y = torch.from_numpy(T.values(c["name"], kind, frames).copy()).cuda()
        out, iters = _typed(dec, y.data_ptr(), "f32", frames, c["K"])
        assert np.array_equal(iters[ok], w["iters"][ok]) and np.array_equal(out, w["out"]), ("float entry point", kind)
    dec.close()


# ---- one-launch and record kernels: the widen pass ------------------------------------------------------------------

ONE_LAUNCH = (("ms_fused", "w576", "1"), ("ms_fused", "w576", "ldsp"), ("ms", "w576", "1"), ("ms", "w576", "ldsp"),
              ("sp", "w576", "1"), ("layered", "w576", "1"), ("layered", "w576", "ldsp"), ("layered", "bg1", None))


@pytest.mark.parametrize("algo,cname,choice", ONE_LAUNCH, ids=["%s-%s-%s" % a for a in ONE_LAUNCH])
def test_one_launch_kernels_get_a_widen_pass(built, algo, cname, choice):
    """ms_fused and the LDS-resident / record kernels on (576, 288) with layer_rows = 24, and the default layered decoder
    -- the record kernel -- on the BG1 test code: a typed call equals the oracle on the dequantised values and shows one
    llr_widen_kernel launch; a plain call on the same handle, before and after it, gives what it gave and shows none."""
    import torch
    c = T.code(cname)
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    frames = 70
    maxit = 120 if algo == "ms_fused" else T.MAXIT
    dec = L.Decoder(g, c["K"], max_batch=frames, algo=algo, max_iter=maxit, layer_rows=c["z"],
                    tune=kernel_choice(choice) if choice else None)
    yf = fc.noisy_frames(c["N"], frames, *T.NOISE[cname], seed=77)
    wf = oracle.decode(c["og"], yf, algo, max_iter=maxit, layer_rows=c["z"])
    okf = ~np.asarray(wf.get("undefined", np.zeros(frames, np.uint8))).astype(bool)
    yd = torch.from_numpy(yf.copy()).cuda()

    def plain(when):
        dec.set_timing(True)
        out, iters = _typed(dec, yd.data_ptr(), "f32", frames, c["K"])
        names = [k["name"] for k in dec.kernel_times()]
        dec.set_timing(False)
        assert "llr_widen_kernel" not in names and names, (when, names)
        assert np.array_equal(iters[okf], wf["iters"][okf]) and np.array_equal(out, wf["out"]), when
        return sorted(names)

    before = plain("before")
    for kind in ("i8", "f16"):
        x = T.inputs(cname, kind, T.LAYERED_FRAMES if cname == "bg1" else T.FLOOD_FRAMES)[:frames]
        y = T.dequantize(x, T.UNITS[kind])
        w = oracle.decode(c["og"], y, algo, max_iter=maxit, layer_rows=c["z"])
        ok = ~np.asarray(w.get("undefined", np.zeros(frames, np.uint8))).astype(bool)
        for off in (0, 1):
            keep, ptr = _place(x, off)
            dec.set_timing(True)
            out, iters = _typed(dec, ptr, kind, frames, c["K"])
            kt = {k["name"]: k["launches"] for k in dec.kernel_times()}
            dec.set_timing(False)
            assert kt.get("llr_widen_kernel") == 1 and len(kt) == len(before) + 1, (kind, off, kt)
            assert np.array_equal(iters[ok], w["iters"][ok]), (algo, cname, choice, kind, off)
            assert np.array_equal(out, w["out"]), (algo, cname, choice, kind, off)
    assert plain("after") == before
    dec.close()


# ---- soft output ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind_of_soft", ["posterior", "extrinsic"])
def test_soft_output_from_int8_input(built, kind_of_soft):
    """Flooding ms (f32 and f16 storage) and layered_bp with int8 input: the stop-round posterior, and that minus y_n where
    y_n is the product x * unit as the decoder read it (ms, rounded to fp16 with fp16 storage) or llr_scale * (x * unit)
    (layered_bp) -- 0 ulp against soft_ref / layered_bp_ref on the dequantised values."""
    c = T.code("w648")
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    frames = 64 + 5
    x = T.inputs("w648", "i8")[:frames]
    y = T.values("w648", "i8")[:frames]
    for storage in ("f32", "f16"):
        w = SR.expected(c["og"], y, "ms", T.MAXIT, f16=storage == "f16")
        want = w["post"] if kind_of_soft == "posterior" else w["ext"]
        for V in (1, 4):
            dec = L.Decoder(g, c["K"], max_batch=frames, algo="ms", msg_dtype=storage, max_iter=T.MAXIT, frames_per_lane=V)
            for off in (0, 1):
                keep, ptr = _place(x, off)
                out, iters, soft = _typed(dec, ptr, "i8", frames, c["K"], soft=kind_of_soft)
                assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), (storage, V, off)
                SR.assert_same_bits(soft, want, None, str(("ms", storage, V, off, kind_of_soft)))
            dec.close()
    c = T.layered_code("layered_bp")
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    frames = T.LAYERED_FRAMES
    w = T.layered_want("layered_bp", "i8")
    x = T.inputs("bg1", "i8", frames)
    dec = L.Decoder(g, c["K"], max_batch=frames, algo="layered_bp", max_iter=T.MAXIT, frames_per_lane=4, layer_rows=c["z"],
                    llr_scale=T.llr_scale("bp", "bg1"))
    for off in (0, 1):
        keep, ptr = _place(x, off)
        out, iters, soft = _typed(dec, ptr, "i8", frames, c["K"], soft=kind_of_soft)
        assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), off
        SR.assert_same_bits(soft, RB.soft_of(w, kind_of_soft), None, str(("layered_bp", off, kind_of_soft)))
    dec.close()


# ---- the host path --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["i8", "f16"])
def test_host_path_in_launch_groups(built, kind):
    """ldpc_decode_typed with max_batch = 64 and 200 frames: four launch groups, the last ragged, sized in bytes of the
    element type.  host_input staged and lock_pages (which is treated as staged for narrow values: the same bytes), and a
    device list [0, 0]; the guard bytes around out / iters stay; no page-locked range is left behind."""
    c = T.code("w648")
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    frames, guard = 200, 32
    x = np.ascontiguousarray(T.inputs("w648", kind)[:frames])
    w = T.head(T.flood_want("w648", kind, "ms", "f32"), frames, c["K"])
    lib = _lib.load()
    nb = L.out_bytes(c["K"], frames)
    for kw in (dict(host_input="staged"), dict(host_input="lock_pages"), dict(devices=[0, 0])):
        dec = L.Decoder(g, c["K"], max_batch=64, algo="ms", max_iter=T.MAXIT, frames_per_lane=1, **kw)
        out = np.full(nb + guard, 0xEE, np.uint8)
        out[:nb] = 0        # K % 8 = 4: the byte between two launch groups is nobody's (ldpc_decode leaves it alone as well)
        iters = np.full(frames + guard, -7, np.int32)
        _lib.check(lib.ldpc_decode_typed(dec._h, x.ctypes.data, T.TYPE_IDS[kind], T.UNITS[kind], frames, out.ctypes.data, nb,
                                         iters.ctypes.data))
        assert np.array_equal(iters[:frames], w["iters"]) and np.array_equal(out[:nb], w["out"]), (kind, kw)
        assert (out[nb:] == 0xEE).all() and (iters[frames:] == -7).all(), (kind, kw)
        if "devices" not in kw:
            assert dec.stats()["frames"] == frames
        out2, iters2 = dec.decode(x, llr_unit=T.UNITS[kind])                  # the Python binding, dtype from the array
        assert np.array_equal(iters2, w["iters"]) and np.array_equal(out2, w["out"]), (kind, kw)
        out3, iters3 = dec.decode(T.values("w648", kind)[:frames])            # and the plain call on the same handle
        assert np.array_equal(iters3, w["iters"]) and np.array_equal(out3, w["out"]), (kind, kw)
        dec.close()
        assert L.capi.host_locked_ranges() == (0, 0), kw
    # soft output through the host path
    sw = SR.expected(c["og"], T.values("w648", kind)[:frames], "ms", T.MAXIT)
    dec = L.Decoder(g, c["K"], max_batch=64, algo="ms", max_iter=T.MAXIT, frames_per_lane=1)
    out, iters, soft = dec.decode(x, soft="extrinsic", llr_unit=T.UNITS[kind])
    assert np.array_equal(iters, sw["iters"]) and np.array_equal(out, sw["out"])
    SR.assert_same_bits(soft, sw["ext"], None, "host path, extrinsic, " + kind)
    dec.close()


# ---- hand-over ------------------------------------------------------------------------------------------------------

def test_polled_hand_over_with_int8_input(built):
    """4500 frames of the (648, 324) code in the three noise populations of handover_cases' case A, as int8: a polled decode
    whose stragglers move to the 1024-frame child decoder (and on).  The children take their state from the parent's
    arrays and never read the input; the result is the oracle's on the dequantised values."""
    from myldpccppapi_amd import channel
    cs = hc.CASES["A"]
    cd = ac.code("w648")
    N, B = cd["N"], cs["frames"]
    y = channel.awgn_frames(N, 0, B, cs["base"], seed=1)
    order = np.random.default_rng(cs["perm"]).permutation(B)
    med, hard = order[:cs["n_med"]], order[cs["n_med"]:cs["n_med"] + cs["n_hard"]]
    y[med] = channel.awgn_frames(N, 20000, med.size, cs["med"], seed=2)
    y[hard] = channel.awgn_frames(N, 40000, hard.size, cs["hard"], seed=3)
    unit = T.UNITS["i8"]
    x = T.quantize(y, unit, "i8")
    w = oracle.decode(cd["og"], T.dequantize(x, unit), "ms", max_iter=hc.MAXIT)
    ev = hc.model(w["iters"], B, 4)
    assert ev and ev[0][2] == 1024, ev                       # the premise: the model says a hand-over happens
    dec = L.Decoder(L.Graph(cd["rows"], cd["cols"], cd["M"], N), cd["K"], max_batch=B, algo="ms", max_iter=hc.MAXIT,
                    poll_interval=1, frames_per_lane=4)
    for call in range(2):
        out, iters = dec.decode(x, llr_unit=unit)
        assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"]), call
        st = dec.stats()
        assert st["frame_rounds"] < ac.frame_rounds_without_handover(w["iters"], 256, hc.MAXIT), st
    dec.close()


# ---- the quantiser --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["i8", "f16"])
def test_quantiser_against_the_numpy_rule(built, kind):
    """ldpc_llr_quantize_device on 10^5 values -- the hand cases of the CPU test, normal values of every magnitude the
    formats hold, ties -- against typed_input_ref.quantize, bit for bit, with unit 1 (the hand cases as they are meant)
    and with the cases' unit; the bytes behind the output stay."""
    import torch
    rng = np.random.default_rng(5)
    n = 100000
    v = (rng.standard_normal(n) * np.exp(rng.uniform(-12, 12, n))).astype(F32)
    hand = T.hand_values()
    v[:hand.size] = hand
    v[hand.size:hand.size + 600] = (np.arange(600, dtype=F32) - 300) / 2          # ties of the int8 grid at unit 1
    for unit in (1.0, T.UNITS[kind]):
        yd = torch.from_numpy(v.copy()).cuda()
        esz = np.dtype(T.DTYPES[kind]).itemsize
        out = torch.full((n * esz + 32,), 0x5A, dtype=torch.uint8, device="cuda")
        L.quantize_device(yd.data_ptr(), n, kind, unit, out.data_ptr(), 0, _stream())
        torch.cuda.synchronize()
        raw = out.cpu().numpy()
        assert (raw[n * esz:] == 0x5A).all()
        got = raw[:n * esz].view(T.DTYPES[kind])
        want = T.quantize(v, unit, kind)
        if kind == "f16":
            nan = np.isnan(want)
            assert np.isnan(got[nan]).all() and np.array_equal(got[~nan].view(np.uint16), want[~nan].view(np.uint16)), unit
        else:
            assert np.array_equal(got, want), (unit, np.nonzero(got != want)[0][:5])
            assert got.min() >= -127
    with pytest.raises(L.LdpcError) as e:
        L.quantize_device(yd.data_ptr(), n, "f32", 1.0, out.data_ptr(), 0, _stream())
    assert e.value.code == LDPC_ERR_ARG
    with pytest.raises(L.LdpcError) as e:
        L.quantize_device(yd.data_ptr(), n, kind, 1.0, yd.data_ptr() + 8, 0, _stream())        # overlap
    assert e.value.code == LDPC_ERR_ARG


@pytest.mark.parametrize("kind", ["i8", "f16"])
def test_channel_quantise_decode_chain_in_hbm(built, kind, tmp_path):
    """ldpc_awgn_device -> ldpc_llr_quantize_device -> ldpc_decode_typed_device on (648, 324), nothing leaves HBM; the CPU
    side runs the same channel (csrc/ldpc_channel.h compiled for the host), the numpy quantiser and the oracle on the
    dequantised values, and the quantised values themselves are compared too."""
    import torch
    c = T.code("w648")
    N, frames, sd, seed = c["N"], 133, 0.8, 99
    lib = _lib.load()
    yd = torch.zeros(frames * N, dtype=torch.float32, device="cuda")
    _lib.check(lib.ldpc_awgn_device(yd.data_ptr(), frames, N, None, sd, seed, 0, 0, _stream()))
    esz = np.dtype(T.DTYPES[kind]).itemsize
    xd = torch.zeros(frames * N * esz, dtype=torch.uint8, device="cuda")
    L.quantize_device(yd.data_ptr(), frames * N, kind, T.UNITS[kind], xd.data_ptr(), 0, _stream())
    dec = L.Decoder(L.Graph(c["rows"], c["cols"], c["M"], N), c["K"], max_batch=frames, algo="ms", max_iter=T.MAXIT,
                    frames_per_lane=2)
    out, iters = _typed(dec, xd.data_ptr(), kind, frames, c["K"])
    dec.close()
    ch = host_channel_lib(tmp_path)
    y = np.zeros((frames, N), F32)
    ch.awgn(y.ctypes.data, frames, N, None, sd, seed, 0)
    x = T.quantize(y, T.UNITS[kind], kind)
    assert np.array_equal(xd.cpu().numpy().view(T.DTYPES[kind]).view(np.uint8), x.ravel().view(np.uint8))
    w = oracle.decode(c["og"], T.dequantize(x, T.UNITS[kind]), "ms", max_iter=T.MAXIT)
    assert np.array_equal(iters, w["iters"]) and np.array_equal(out, w["out"])


# ---- refusals -------------------------------------------------------------------------------------------------------

def test_refusals_enqueue_nothing(built):
    """An unknown type; llr_unit 0, negative, NaN and inf; F32 with a unit other than 1; an fp16 pointer at an odd address;
    a soft buffer that overlaps the bytes of the typed buffer: LDPC_ERR_ARG each, with the output untouched, and a plain
    decode right after is what it was."""
    import torch
    c = T.code("w648")
    frames = 64 + 5
    dec = L.Decoder(L.Graph(c["rows"], c["cols"], c["M"], c["N"]), c["K"], max_batch=frames, algo="ms", max_iter=T.MAXIT,
                    frames_per_lane=1)
    w = T.head(T.flood_want("w648", "i8", "ms", "f32"), frames, c["K"])
    x = T.inputs("w648", "i8")[:frames]
    keep, ptr = _place(x, 0)
    yd = torch.from_numpy(T.values("w648", "i8")[:frames].copy()).cuda()
    nb = L.out_bytes(c["K"], frames)
    out = torch.full((nb,), 0xEE, dtype=torch.uint8, device="cuda")
    it = torch.full((frames,), -7, dtype=torch.int32, device="cuda")
    lib = _lib.load()

    def refused(rc, what):
        assert rc == LDPC_ERR_ARG, (what, rc, lib.ldpc_last_error())
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0xEE).all() and (it.cpu().numpy() == -7).all(), what
        o, i = _typed(dec, yd.data_ptr(), "f32", frames, c["K"])
        assert np.array_equal(i, w["iters"]) and np.array_equal(o, w["out"]), what

    def call(p, ty, unit):
        return lib.ldpc_decode_typed_device(dec._h, p, ty, unit, frames, out.data_ptr(), nb, it.data_ptr(), _stream())

    refused(call(ptr, 3, 1.0), "unknown type")
    refused(call(ptr, -1, 1.0), "unknown type")
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        refused(call(ptr, T.LLR_I8, bad), ("unit", bad))
    refused(call(yd.data_ptr(), T.LLR_F32, 0.5), "F32 with a unit other than 1")
    refused(call(ptr + 1, T.LLR_F16, 1.0), "odd fp16 address")
    # the soft buffer starts inside the int8 buffer's bytes -- far behind where frames * N FLOATS before it would end
    soft = torch.zeros(frames * c["N"] + 64, dtype=torch.float32, device="cuda")
    inside = soft.data_ptr() + 4 * (frames * c["N"] // 4 - 8)          # 4-byte aligned, 32 bytes before the int8 rows end
    host = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).ravel().copy())
    soft.view(torch.uint8)[:host.numel()] = host.cuda()
    rc = lib.ldpc_decode_soft_typed_device(dec._h, soft.data_ptr(), T.LLR_I8, T.UNITS["i8"], frames, out.data_ptr(), nb,
                                           it.data_ptr(), inside, frames * c["N"], 1, _stream())
    refused(rc, "soft overlaps the typed buffer")
    # a typed call still works afterwards
    o, i = _typed(dec, ptr, "i8", frames, c["K"])
    assert np.array_equal(i, w["iters"]) and np.array_equal(o, w["out"])
    dec.close()


# ---- Coder ----------------------------------------------------------------------------------------------------------

def test_coder_decode_typed_equals_the_c_abi(built, tmp_path):
    """Coder::decodeTyped / decodeSoftTyped (tests/cpp/coder_typed_input.cpp) give the bytes and soft values of the C ABI's
    typed host call -- and of the oracle on the dequantised values."""
    from coder_typed_input_harness import coder_typed_input_exe
    exe = coder_typed_input_exe(tmp_path)
    N, frames = 576, 40
    c = T.code("w576")
    g = L.Graph(c["rows"], c["cols"], c["M"], N)
    for kind in ("i8", "f16"):
        x = np.ascontiguousarray(T.inputs("w576", kind)[:frames])
        x.tofile(str(tmp_path / "in"))
        y = T.values("w576", kind)[:frames]
        sw = SR.expected(c["og"], y, "ms", 20)
        for soft_kind, name in ((0, None), (1, "posterior"), (2, "extrinsic")):
            p = subprocess.run([exe, str(int(codes.RATE_1_2)), str(N), str(frames), str(T.TYPE_IDS[kind]), repr(T.UNITS[kind]),
                                str(soft_kind), str(tmp_path / "in"), str(tmp_path / "out"), str(tmp_path / "soft")],
                               capture_output=True, text=True)
            assert p.returncode == 0, p.stdout + p.stderr
            got = np.fromfile(str(tmp_path / "out"), np.uint8)
            dec = L.Decoder(g, c["K"], max_batch=frames, algo="ms", max_iter=20, layer_rows=c["z"], poll_interval=4)
            res = dec.decode(x, soft=name, llr_unit=T.UNITS[kind])
            dec.close()
            assert np.array_equal(got, res[0][:got.size]) and np.array_equal(got, sw["out"][:got.size]), (kind, soft_kind)
            if soft_kind:
                soft = np.fromfile(str(tmp_path / "soft"), np.float32).reshape(frames, N)
                SR.assert_same_bits(soft, res[2], None, str(("coder against the C ABI", kind, name)))
                SR.assert_same_bits(soft, sw["post"] if soft_kind == 1 else sw["ext"], None, str(("coder against the oracle", kind, name)))
