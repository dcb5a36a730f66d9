"""Hard-decision bit flipping (algo = bitflip) on the GPU against tests/bitflip_ref.py: 802.16e (576, 288) rate 1/2 and
(672, 448) rate 2/3A and the Hamming (7, 4) code, at 1, 63, 64, 65 and 130 frames -- a partial word, exactly one word, a word
plus one bit, a third partial word --, one round and twelve, early termination on and off, both pack modes, float, fp16
and int8 input, degenerate channel values, a codeword beside a frame that never converges in one word, a custom
bf_threshold, the CRC stop, the host path over several launch groups, a device list, the refusals that need a handle and
Coder's DecodeBitFlip.

bitflip is this repository's own definition (include/ldpc_hip.h: LDPC_ALGO_BITFLIP); the expectation is the numpy
restatement in integers.  Every comparison is exact: bytes, iteration counts (a frame is done iff its count is below
max_iter), the number of done frames, all N bits and the syndrome words of the tapped round."""
import functools
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import codes

import bitflip_ref as B
import crc_term_ref
import tb_ref
from osd_cases import HAMMING, edges_of

pytestmark = pytest.mark.gpu

LDPC_ERR_ARG, LDPC_ERR_UNSUPPORTED = 1, 4
FRAMES = (1, 63, 64, 65, 130)
CROSSOVER = 0.02


@functools.lru_cache(maxsize=None)
def _code(name):
    """dict(rows, cols, M, N, K, z, code = the reference's Code, word = one codeword that is not all zero)"""
    if name == "hamming":
        rows, cols, M, N = edges_of(HAMMING)
        c = dict(rows=rows, cols=cols, M=M, N=N, K=4, z=0, word=np.array([1, 1, 1, 0, 0, 0, 0], np.uint8))
    else:
        rate, N = {"half": (codes.RATE_1_2, 576), "two_thirds": (codes.RATE_2_3_A, 672)}[name]
        K, M, z = codes.wimax_dims(rate, N)
        rows, cols = codes.wimax_edges(rate, N)
        g = L.Graph(rows, cols, M, N)
        enc = L.Encoder(g, K, block_rows=z, max_frames=1)
        payload = np.random.default_rng(5).integers(0, 256, K // 8, dtype=np.uint8)
        word = np.unpackbits(enc.encode(payload), bitorder="little")[:N]
        enc.close()
        c = dict(rows=rows, cols=cols, M=M, N=N, K=K, z=z, word=word)
    c["code"] = B.Code(c["rows"], c["cols"], c["M"], c["N"])
    assert c["word"].any() and not c["code"].syndrome(c["word"][:, None]).any()       # a codeword, by the reference's own H
    return c


@functools.lru_cache(maxsize=None)
def _inputs(name, frames, crossover=CROSSOVER, seed=17):
    """Even frames carry the all-zero codeword, odd frames the encoded payload, through a binary symmetric channel."""
    c = _code(name)
    bits = np.zeros((frames, c["N"]), np.uint8)
    bits[1::2] = c["word"]
    y = B.bsc(frames, c["N"], crossover, seed + frames, bits)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def _want(name, frames, max_iter, bf=None, crossover=CROSSOVER):
    return B.decode(_code(name)["code"], _inputs(name, frames, crossover), max_iter, bf)


def _decoder(name, B_, max_iter, **kw):
    c = _code(name)
    return L.Decoder(L.Graph(c["rows"], c["cols"], c["M"], c["N"]), c["K"], max_batch=B_, algo="bitflip", max_iter=max_iter, **kw)


def _check(dec, y, want, c, what, pack_bits=False, **decode_kw):
    out, iters = dec.decode(y, **decode_kw)
    frames = want["hard"].shape[0]
    assert np.array_equal(iters, want["iters"]), ("iterations",) + what
    packed = B.pack_bits(want["hard"], c["K"]) if pack_bits else B.pack_bytes(want["hard"], c["K"])
    assert np.array_equal(out, packed), ("bytes",) + what
    assert np.array_equal(dec.dump(3, frames).astype(np.uint8), want["hard"]), ("bits",) + what
    st = dec.stats()
    assert st["frames_converged"] == int(want["done"].sum()) and st["frames"] == frames, ("done frames",) + what
    assert np.array_equal(iters < dec.cfg.max_iter, want["done"]), ("done flags",) + what


@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("name", ["half", "two_thirds", "hamming"])
def test_bitflip_codes_and_frame_counts(built, name, frames):
    """Twelve rounds and one, early termination on; the syndrome words and the bits of the tapped round 2."""
    c = _code(name)
    y = _inputs(name, frames)
    for max_iter in (12, 1):
        dec = _decoder(name, frames, max_iter)
        _check(dec, y, _want(name, frames, max_iter), c, (name, frames, max_iter))
        if max_iter == 12:
            tap = _want(name, frames, 2)
            dec.set_tap(2)
            dec.decode(y)
            assert np.array_equal(dec.dump(0, frames).astype(np.uint8), tap["syndrome"]), ("syndrome tap", name, frames)
            assert np.array_equal(dec.dump(3, frames).astype(np.uint8), tap["hard"]), ("bit tap", name, frames)
            dec.set_tap(0)
        dec.close()
    if name != "hamming" and frames == 130:     # the premise: frames that stop at once, early, late and not at all
        it = _want(name, frames, 12)["iters"]
        assert (it == 12).any() and ((it > 0) & (it < 12)).any(), np.bincount(it)


@pytest.mark.parametrize("early_term", [1, 0])
@pytest.mark.parametrize("pack", ["bytes", "bits"])
def test_bitflip_early_termination_and_pack_modes(built, early_term, pack):
    """early_term = 0 launches every round on every tile and changes nothing; LDPC_PACK_BITS on the Hamming code packs
    K = 4 bits per frame across byte boundaries."""
    for name, frames in (("half", 130), ("hamming", 65)):
        c = _code(name)
        if pack == "bytes" and c["K"] % 8:
            continue
        dec = _decoder(name, frames, 12, early_term=bool(early_term), pack_mode=L.capi.PACK_BITS if pack == "bits" else L.capi.PACK_BYTES)
        _check(dec, _inputs(name, frames), _want(name, frames, 12), c, (name, early_term, pack), pack_bits=pack == "bits")
        assert dec.stats()["iterations_launched"] == 12
        dec.close()


def test_bitflip_kernels_by_name(built):
    dec = _decoder("half", 130, 12)
    dec.set_timing(True)
    dec.decode(_inputs("half", 130))
    names = {k["name"]: k["launches"] for k in dec.kernel_times() if k["phase"] in (0, 1)}
    assert names == {"bitflip_check_kernel": 12, "bitflip_vote_kernel": 12, "bitflip_flip_kernel": 12}, names
    dec.close()


@pytest.mark.parametrize("kind", ["f16", "i8"])
def test_bitflip_typed_input(built, kind):
    """The sign of the stored value decides: fp16 and int8 rows with a unit, zeros among them, give the bits of their floats."""
    c = _code("two_thirds")
    y = _inputs("two_thirds", 130)
    if kind == "f16":
        x, unit = (y * np.float32(3.5)).astype(np.float16), 0.25
        x[::7, ::5] = np.float16(0.0)
        x[3::7, 1::5] = np.float16(-0.0)
    else:
        x, unit = (y * 9).astype(np.int8), 0.125
        x[::7, ::5] = 0
    want = B.decode(c["code"], x.astype(np.float32) * np.float32(unit), 12)
    dec = _decoder("two_thirds", 130, 12)
    _check(dec, x, want, c, (kind,), llr_unit=unit)
    dec.close()


def test_bitflip_degenerate_channel_values(built):
    """NaN, -0.0 and +0.0 read bit 0; infinities and denormals read their sign."""
    c = _code("half")
    y = _inputs("half", 65).copy()
    y[:, 0::13] = np.nan
    y[:, 1::13] = -0.0
    y[:, 2::13] = 0.0
    y[:, 3::13] = -np.inf
    y[:, 4::13] = np.inf
    y[:, 5::13] = -1e-45
    r = B.received(y)
    assert not r[:, 0::13].any() and not r[:, 1::13].any() and not r[:, 2::13].any() and r[:, 3::13].all() and r[:, 5::13].all()
    dec = _decoder("half", 65, 1)
    dec.set_tap(1)
    dec.decode(y)
    want = B.decode(c["code"], y, 1)
    assert np.array_equal(dec.dump(0, 65).astype(np.uint8), want["syndrome"])        # s of round 1 is H r
    dec.set_tap(0)
    _check(dec, y, want, c, ("degenerate", 1))
    dec.close()
    dec = _decoder("half", 65, 12)
    _check(dec, y, B.decode(c["code"], y, 12), c, ("degenerate", 12))
    dec.close()


def test_bitflip_freezes_per_bit(built):
    """A codeword (iters 0) beside frames that never converge, in one 64-frame word: the codeword's bits stay as they are
    through all rounds, with early termination on and off."""
    c = _code("half")
    y = _inputs("half", 64, crossover=0.2).copy()
    y[5] = 1.0 - 2.0 * c["word"]
    y[6] = 1.0
    want = B.decode(c["code"], y, 12)
    assert want["iters"][5] == 0 and want["iters"][6] == 0 and (np.delete(want["iters"], [5, 6]) == 12).all()
    assert np.array_equal(want["hard"][5], c["word"])
    for early_term in (True, False):
        dec = _decoder("half", 64, 12, early_term=early_term)
        _check(dec, y, want, c, ("freeze", early_term))
        dec.close()


def test_bitflip_custom_thresholds(built):
    """A table of the caller's: other bits than the default's, the last entry serving rounds 17 .. 20; strict majority from
    round 1 as [62] * 16; a short Python list repeats its last entry."""
    c = _code("half")
    y = _inputs("half", 130)
    table = (3, 0, 1, 2, 2, 3, 3, 1, 0, 2, 3, 3, 1, 2, 3, 2)
    want = _want("half", 130, 20, table)
    assert not np.array_equal(want["hard"], _want("half", 130, 20)["hard"])
    dec = _decoder("half", 130, 20, bf_threshold=table)
    _check(dec, y, want, c, ("table",))
    dec.close()
    dec = _decoder("half", 130, 12, bf_threshold=[62])
    _check(dec, y, _want("half", 130, 12, (62,) * 16), c, ("majority",))
    dec.close()


def test_bitflip_crc_stop(built):
    """(576, 288), CRC16 over the first 128 bits (112 payload bits and their parity), 130 frames, 12 rounds: the CRC rule of
    tests/crc_term_ref.py over the reference -- in round i the bits after i - 1 rounds are tested, a frame stops at the
    first i where its syndrome is clean or its CRC passes, iters = i - 1."""
    c = _code("half")
    K, N, frames, max_iter = c["K"], c["N"], 130, 12
    rng = np.random.default_rng(23)
    info = rng.integers(0, 2, (frames, K), dtype=np.uint8)
    info[:, 112:128] = tb_ref.parity(16, info[:, :112])
    g = L.Graph(c["rows"], c["cols"], c["M"], N)
    enc = L.Encoder(g, K, block_rows=c["z"], max_frames=frames)
    words = np.unpackbits(enc.encode(np.packbits(info, axis=1, bitorder="little")).reshape(frames, N // 8), axis=1, bitorder="little")
    enc.close()
    assert np.array_equal(words[:, :K], info)
    y = B.bsc(frames, N, 0.025, 29, words)

    def after(ys, i):               # the bits round i tests: those after i - 1 rounds
        return B.decode(c["code"], ys, i - 1)["hard"]

    w = crc_term_ref.crc_rule(after, y, c["rows"], c["cols"], c["M"], N, K, 16, 128, max_iter)
    # crc_rule numbers a stop by the round that tested the bits, i; the frame then has run i - 1 rounds.  The bits of round
    # max_iter itself are never tested: the frames no rule stopped have run max_iter rounds
    stopped = np.ones(frames, bool)
    stopped[w["never"]] = False
    iters = np.where(stopped, w["iters"] - 1, max_iter).astype(np.int32)
    hard = w["hard"].copy()
    hard[~stopped] = B.decode(c["code"], y[~stopped], max_iter)["hard"]
    assert w["by_crc"].size >= 3 and (~stopped).any(), (w["by_crc"].size, int((~stopped).sum()))
    dec = _decoder("half", frames, max_iter, crc_kind=16, crc_bits=128)
    out, got = dec.decode(y)
    assert np.array_equal(got, iters)
    assert np.array_equal(out, B.pack_bytes(hard, K))
    assert np.array_equal(dec.dump(3, frames).astype(np.uint8), hard)
    assert dec.crc_stops() == w["by_crc"].size and dec.stats()["frames_converged"] == int(stopped.sum())
    dec.close()


def test_bitflip_host_path_in_groups_and_device_list(built):
    """130 frames through a handle of max_batch 64 (three launch groups) and through a device list of two entries."""
    c = _code("two_thirds")
    y = _inputs("two_thirds", 130)
    want = _want("two_thirds", 130, 12)
    for kw in (dict(), dict(devices=[0, 0])):
        dec = _decoder("two_thirds", 64, 12, **kw)
        out, iters = dec.decode(y)
        assert np.array_equal(iters, want["iters"]) and np.array_equal(out, B.pack_bytes(want["hard"], c["K"])), kw
        assert dec.stats()["frames_converged"] == int(want["done"].sum())
        dec.close()


def test_bitflip_device_entry_point(built):
    import torch
    c = _code("half")
    y = _inputs("half", 65)
    want = _want("half", 65, 12)
    dec = _decoder("half", 130, 12)
    yd = torch.from_numpy(np.array(y)).cuda()
    nb = L.capi.out_bytes(c["K"], 65)
    out = torch.full((nb + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    it = torch.zeros(65, dtype=torch.int32, device="cuda")
    dec.decode_device(yd.data_ptr(), 65, out.data_ptr(), nb, it.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(it.cpu().numpy(), want["iters"])
    assert np.array_equal(out.cpu().numpy()[:nb], B.pack_bytes(want["hard"], c["K"])) and (out.cpu().numpy()[nb:] == 0xA5).all()
    dec.close()


def test_bitflip_refusals_that_need_a_handle(built):
    c = _code("half")
    dec = _decoder("half", 64, 4)
    y = _inputs("half", 64)
    for soft in ("posterior", "extrinsic"):
        with pytest.raises(L.LdpcError) as e:
            dec.decode(y, soft=soft)
        assert e.value.code == LDPC_ERR_UNSUPPORTED and "hard-decision" in str(e.value)
    with pytest.raises(L.LdpcError) as e:
        dec.decode(y.astype(np.float16), soft="posterior", llr_unit=1.0)
    assert e.value.code == LDPC_ERR_UNSUPPORTED
    dec.decode(y)
    for which in (1, 2):
        with pytest.raises(L.LdpcError) as e:
            dec.dump(which, 64)
        assert e.value.code == LDPC_ERR_ARG
    dec.close()
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    for kw, code in ((dict(msg_dtype="f16"), LDPC_ERR_UNSUPPORTED), (dict(ms_scale=0.75), LDPC_ERR_UNSUPPORTED),
                     (dict(tune={"fused": True}), LDPC_ERR_UNSUPPORTED), (dict(tune={"ldsp": True}), LDPC_ERR_UNSUPPORTED),
                     (dict(tune={"fx_record": True}), LDPC_ERR_ARG), (dict(bf_threshold=[63]), LDPC_ERR_ARG)):
        with pytest.raises(L.LdpcError) as e:
            L.Decoder(g, c["K"], max_batch=64, algo="bitflip", **kw)
        assert e.value.code == code, kw
    with pytest.raises(L.LdpcError) as e:
        L.Decoder(g, c["K"], max_batch=64, algo="ms", bf_threshold=[1])
    assert e.value.code == LDPC_ERR_ARG


def test_coder_decode_bitflip(built, tmp_path):
    """Coder::addDecodeType(DecodeBitFlip) + decode / decodeTyped give the bytes of the C ABI decoder; setBitFlipThresholds
    reaches the table; decodeSoft is refused."""
    from coder_bitflip_harness import coder_bitflip_exe
    exe = coder_bitflip_exe(tmp_path)
    c = _code("half")
    frames = 130
    y = _inputs("half", frames)
    fin, fin8, fout = tmp_path / "in.f32", tmp_path / "in.i8", tmp_path / "out.bin"
    np.array(y).tofile(fin)
    (np.array(y) * 5).astype(np.int8).tofile(fin8)
    table = (3, 0, 1, 2)
    for offsets, unit, bf, max_iter in (("-", 0, None, 12), ("3,0,1,2", 0, table + (2,) * 12, 12), ("-", 0.5, None, 7)):
        dec = _decoder("half", frames, max_iter, bf_threshold=bf)
        want, _ = dec.decode(y)
        dec.close()
        assert np.array_equal(want, B.pack_bytes(B.decode(c["code"], y, max_iter, bf)["hard"], c["K"]))
        r = subprocess.run([exe, "0", str(c["N"]), str(frames), str(max_iter), offsets, str(unit), "0",
                            str(fin8 if unit else fin), str(fout)], capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert np.array_equal(np.fromfile(fout, np.uint8), want), (offsets, unit)
    r = subprocess.run([exe, "0", str(c["N"]), str(frames), "12", "-", "0", "1", str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 4 and "hard-decision" in r.stdout, (r.returncode, r.stdout)
    r = subprocess.run([exe, "0", str(c["N"]), str(frames), "12", "63", "0", "0", str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 3 and "bf_threshold" in r.stdout, (r.returncode, r.stdout)
