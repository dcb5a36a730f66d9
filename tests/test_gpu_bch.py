"""The outer code on the GPU (ldpc_bch_encode_device / ldpc_bch_decode_device / ldpc_bch_tally_device and the host-buffer
forms) against bch_ref, bit for bit: on shifted pointers with guard regions around every output, rows with and without
filler bytes, clean, damaged and hopeless frames side by side and alone, each nullable output alone, the tally, refused
calls, and the chain BCH encode -> LDPC encoder -> channel -> decoder -> BCH decode -> tally in HBM."""
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import channel

import bch_ref
import bch_util as BU

pytestmark = pytest.mark.gpu

GUARD, MARK, EXTRA = 64, 0xEE, 3
FRAME_COUNTS = (1, 63, 65, 130)
SHIFTS = ((0, 0), (1, 3), (3, 1))


def _torch():
    import torch
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _code(shape, extra=0):
    m, t, n = shape
    return L.BchCode(n, t, row_bytes=n // 8 + extra, m=m, prim=BU.PRIM[m])


def _up(host, shift):
    torch = _torch()
    host = np.ascontiguousarray(host, np.uint8).reshape(-1)
    t = torch.zeros(shift + host.size, dtype=torch.uint8, device="cuda")
    t[shift:] = torch.from_numpy(np.array(host)).cuda()
    return t, t.data_ptr() + shift


def _out(n, shift):
    """A marker-filled output of n bytes, GUARD + shift marker bytes in front of it and GUARD behind."""
    t = _torch().full((GUARD + shift + n + GUARD,), MARK, dtype=_torch().uint8, device="cuda")
    return t, t.data_ptr() + GUARD + shift


def _down(t, n, shift, what):
    host = t.cpu().numpy()
    lo = GUARD + shift
    assert (host[:lo] == MARK).all() and (host[lo + n:] == MARK).all(), "wrote outside the %s buffer" % what
    return host[lo:lo + n]


def _status_out(frames):
    """int32 status buffer with 16 guard words on either side, filled with a value no frame can have."""
    t = _torch().full((16 + frames + 16,), -77, dtype=_torch().int32, device="cuda")
    return t, t.data_ptr() + 64


def _status_down(t, frames):
    host = t.cpu().numpy()
    assert (host[:16] == -77).all() and (host[16 + frames:] == -77).all(), "wrote outside the status buffer"
    return host[16:16 + frames]


def _encode_device(code, payload, in_shift=0, out_shift=0):
    payload = np.ascontiguousarray(payload, np.uint8).reshape(-1, code.k // 8)
    frames = payload.shape[0]
    keep, pay_ptr = _up(payload, in_shift)
    n = frames * code.row_bytes
    src, src_ptr = _out(n, out_shift)
    code.encode_device(pay_ptr, frames, src_ptr, n, _stream())
    _torch().cuda.synchronize()
    return _down(src, n, out_shift, "src").reshape(frames, code.row_bytes)


def _decode_device(code, rows, want=("payload", "status"), in_shift=0, out_shift=0):
    rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, code.row_bytes)
    frames = rows.shape[0]
    keep, dec_ptr = _up(rows, in_shift)
    pay = _out(frames * (code.k // 8), out_shift) if "payload" in want else (None, None)
    st = _status_out(frames) if "status" in want else (None, None)
    code.decode_device(dec_ptr, frames, pay[1], st[1], _stream())
    _torch().cuda.synchronize()
    assert np.array_equal(keep.cpu().numpy()[in_shift:], rows.reshape(-1)), "the input was changed"
    got = {}
    if "payload" in want:
        got["payload"] = _down(pay[0], frames * (code.k // 8), out_shift, "payload").reshape(frames, code.k // 8)
    if "status" in want:
        got["status"] = _status_down(st[0], frames)
    return got


@pytest.mark.parametrize("shape", BU.SHAPES, ids=BU.shape_id)
def test_encode_equals_the_reference(built, shape):
    rng = np.random.default_rng(700 + BU.SHAPES.index(shape))
    ref = BU.ref_code(shape)
    payload = rng.integers(0, 256, (130, ref.k // 8), dtype=np.uint8)
    payload[1] = 0
    payload[2] = 0xFF
    want = ref.encode(payload)
    assert not ref.syndromes(bch_ref.bits_of(want)).any()
    for extra in (0, EXTRA):
        code = _code(shape, extra)
        wide = np.zeros((130, code.row_bytes), np.uint8)             # filler bytes come out zero over the marker
        wide[:, :ref.n // 8] = want
        for frames in FRAME_COUNTS:
            for in_shift, out_shift in SHIFTS:
                got = _encode_device(code, payload[:frames], in_shift, out_shift)
                assert np.array_equal(got, wide[:frames]), (shape, extra, frames, in_shift, out_shift)


@pytest.mark.parametrize("shape", BU.SHAPES, ids=BU.shape_id)
def test_decode_equals_the_reference(built, shape):
    """Frame f carries an error of weight (0, 1, t, t + 1, 3t)[f % 5] at the places bch_util.damaged lists; rows with
    garbage behind bit n and rows that end at bit n; all frame counts; both outputs, then each alone."""
    payload, rows, bad, want_payload, want_status = BU.decode_case(shape, EXTRA, 130, 710 + BU.SHAPES.index(shape))
    ref = BU.ref_code(shape)
    t = ref.t
    # what the restatement says about this batch: clean stay, up to t are repaired, beyond t nothing is reported clean
    weights = np.array([(0, 1, t, t + 1, 3 * t)[f % 5] for f in range(130)])
    few = weights <= t
    assert np.array_equal(want_status[few], weights[few]) and np.array_equal(want_payload[few], payload[few])
    assert (want_status[~few] != 0).all() and (want_status == -1).sum() >= 26
    failed = want_status == -1
    assert np.array_equal(want_payload[failed], np.asarray(bad)[failed, :ref.k // 8])
    for extra in (EXTRA, 0):
        code = _code(shape, extra)
        given = np.asarray(bad)[:, :code.row_bytes]
        for frames in FRAME_COUNTS:
            for in_shift, out_shift in SHIFTS:
                got = _decode_device(code, given[:frames], in_shift=in_shift, out_shift=out_shift)
                assert np.array_equal(got["status"], want_status[:frames]), (shape, extra, frames, in_shift, out_shift)
                assert np.array_equal(got["payload"], want_payload[:frames]), (shape, extra, frames, in_shift, out_shift)
        for names in (("payload",), ("status",)):
            got = _decode_device(code, given, names, 1, 3)
            for k in names:
                assert np.array_equal(got[k], {"payload": want_payload, "status": want_status}[k]), (shape, extra, names)


@pytest.mark.parametrize("shape", BU.SHAPES, ids=BU.shape_id)
def test_all_clean_and_all_dirty_batches(built, shape):
    ref = BU.ref_code(shape)
    code = _code(shape)
    payload, rows, bad, want_payload, want_status = BU.decode_case(shape, 0, 65, 730 + BU.SHAPES.index(shape), True)
    assert (want_status >= 1).all() and want_status.max() == ref.t and np.array_equal(want_payload, payload)
    got = _decode_device(code, bad, in_shift=3, out_shift=1)
    assert np.array_equal(got["status"], want_status) and np.array_equal(got["payload"], payload), shape
    got = _decode_device(code, rows, in_shift=1, out_shift=3)
    assert not got["status"].any() and np.array_equal(got["payload"], payload), shape
    # decode(encode(x)) = x through the library alone, and the host forms equal the device forms
    assert np.array_equal(code.encode(payload), rows)
    host_payload, host_status = code.decode(bad)
    assert np.array_equal(host_payload, payload) and np.array_equal(host_status, want_status)


def test_tally_equals_numpy(built):
    torch = _torch()
    rng = np.random.default_rng(740)
    code = _code(BU.SHAPES[0])
    frames, per = 300, code.k // 8
    ref = rng.integers(0, 256, (frames, per), dtype=np.uint8)
    payload = ref.copy()
    status = rng.integers(-1, 4, frames).astype(np.int32)
    status[:6] = (0, 0, 1, 3, -1, -1)
    wrong = rng.integers(0, 2, frames).astype(bool)
    wrong[:6] = (False, True, False, True, False, True)
    for f in np.nonzero(wrong)[0]:
        payload[f, (f * 7) % per] ^= 1 << (f % 8)
    payload[7], wrong[7] = ref[7], True
    payload[7, per - 1] ^= 0x80                                      # the last bit of a row
    want = bch_ref.tally(status, payload, ref)
    assert want[1] == int(wrong.sum()) and min(want) > 0
    sd, pd, rd = (torch.from_numpy(a).cuda() for a in (status, payload, ref))
    assert code.tally_device(sd.data_ptr(), pd.data_ptr(), rd.data_ptr(), frames, _stream()) == want
    keep, p1 = _up(payload, 3)
    assert code.tally_device(sd.data_ptr(), p1, None, frames, _stream()) == bch_ref.tally(status, payload, None)
    zero = np.zeros_like(payload)
    zero[9, 3] = 1
    keep2, z1 = _up(zero, 1)
    assert code.tally_device(sd.data_ptr(), z1, None, frames, _stream()) == bch_ref.tally(status, zero, None)
    assert code.tally_device(sd.data_ptr(), z1, None, 0, _stream()) == (0,) * 6


def test_host_forms_over_two_chunks(built):
    """Rows of 7290 bytes: the 64 MiB scratch holds 9205 of them, so 9206 frames take two chunks in both calls."""
    shape = (16, 8, 58320)
    ref, code = BU.ref_code(shape), _code(shape)
    frames = 9206
    assert (64 << 20) // code.row_bytes == frames - 1
    payload = np.random.default_rng(750).integers(0, 256, (frames, code.k // 8), dtype=np.uint8)
    rows = code.encode(payload)
    for f in (0, frames - 2, frames - 1):
        assert np.array_equal(rows[f], ref.encode(payload[f:f + 1])[0]), f
    BU.flip(rows, frames - 1, 17)                   # in the second chunk
    BU.flip(rows, 5, code.n - 1)
    BU.flip(rows, 5, 0)
    got, status = code.decode(rows)
    want = np.zeros(frames, np.int32)
    want[frames - 1], want[5] = 1, 2
    assert np.array_equal(status, want) and np.array_equal(got, payload)


def test_refused_calls_enqueue_nothing(built):
    torch = _torch()
    code = _code(BU.SHAPES[0])                       # 28 payload bytes, rows of 31 bytes
    buf = torch.full((4096,), MARK, dtype=torch.uint8, device="cuda")
    src = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p, s = buf.data_ptr(), src.data_ptr()
    bad = _code(BU.SHAPES[0])
    bad.spec.prim = 0x11B
    for call in (lambda: code.encode_device(s, 4, p, 4 * 31 - 1, _stream()),
                 lambda: code.encode_device(p, 4, p + 111, 4 * 31, _stream()),
                 lambda: bad.encode_device(s, 4, p, 4096, _stream()),
                 lambda: code.decode_device(s, 4, None, None, _stream()),
                 lambda: code.decode_device(p, 4, p + 123, None, _stream()),
                 lambda: code.decode_device(p, 4, None, p + 120, _stream()),
                 lambda: code.decode_device(s, 4, p, p + 108, _stream()),
                 lambda: code.decode_device(s, 4, p, p + 1026, _stream()),
                 lambda: bad.decode_device(s, 4, p, None, _stream()),
                 lambda: code.decode_device(s, -1, p, None, _stream())):
        with pytest.raises(L.LdpcError) as e:
            call()
        assert e.value.code == 1
    code.encode_device(s, 0, p, 0, _stream())          # frames == 0: nothing
    code.decode_device(s, 0, p, p + 1024, _stream())
    assert code.tally_device(s, s, None, 0, _stream()) == (0,) * 6
    torch.cuda.synchronize()
    assert bool((buf == MARK).all())


# ---- the chain in device memory ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", sorted(BU.BUDGET))
def test_chain_equals_the_oracle(built, algo):
    """BchCode.encode_device -> Encoder -> ldpc_awgn_device -> Decoder -> BchCode.decode_device -> tally_device, all in HBM,
    on the scenario whose premises test_bch_cpu pins.  The decoder's bytes are the oracle's; the outer code's outputs
    equal the restatement applied to the decoder's own output bytes; the tally equals numpy's."""
    torch = _torch()
    K, M, z, rows, cols = BU.chain_graph()
    payload, want_src, want_bits, want_y = BU.chain_sent()
    want_out, residual, want_payload, want_status, want_counts = BU.chain_oracle(algo)
    t, frames, N = BU.T, BU.FRAMES, BU.N
    kinds = (int((residual == 0).sum()), int(((residual > 0) & (residual <= t)).sum()), int((residual > t).sum()))
    print("%s max_iter %d: clean %d, 1..t %d, > t %d; tally %s" % ((algo, BU.BUDGET[algo]) + kinds + (want_counts,)))
    assert min(kinds) >= 3
    code = L.BchCode(K, t)
    assert (code.k, code.row_bytes) == (BU.chain_code().k, K // 8)
    g = L.Graph(rows, cols, M, N)
    enc = L.Encoder(g, K, z, max_frames=frames)
    dec = L.Decoder(g, K, max_batch=frames, algo=algo, max_iter=BU.BUDGET[algo], layer_rows=z)
    pay = torch.from_numpy(np.array(payload)).cuda()
    src = torch.full((frames, K // 8), MARK, dtype=torch.uint8, device="cuda")
    bits = torch.empty((frames, N), dtype=torch.uint8, device="cuda")
    out = torch.zeros(L.out_bytes(K, frames), dtype=torch.uint8, device="cuda")
    back = torch.full((frames, code.k // 8), MARK, dtype=torch.uint8, device="cuda")
    status = torch.full((frames,), -77, dtype=torch.int32, device="cuda")
    code.encode_device(pay.data_ptr(), frames, src.data_ptr(), src.numel(), _stream())
    enc.encode_device(src.data_ptr(), src.numel(), frames, bits.data_ptr(), bits.numel(), "bits", _stream())
    y = channel.awgn_device(N, 0, frames, BU.SD, seed=BU.NOISE_SEED, codewords=bits, stream=_stream())
    dec.decode_device(y.data_ptr(), frames, out.data_ptr(), out.numel(), None, _stream())
    code.decode_device(out.data_ptr(), frames, back.data_ptr(), status.data_ptr(), _stream())
    counts = code.tally_device(status.data_ptr(), back.data_ptr(), pay.data_ptr(), frames, _stream())
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), want_src)
    assert np.array_equal(bits.cpu().numpy(), want_bits)
    assert np.array_equal(y.cpu().numpy().view(np.uint32), want_y.view(np.uint32))
    got_out = out.cpu().numpy().reshape(frames, K // 8)
    assert np.array_equal(got_out, want_out)
    own_payload, own_status = BU.chain_code().decode(got_out)        # the restatement on the decoder's own bytes
    assert np.array_equal(status.cpu().numpy(), own_status) and np.array_equal(back.cpu().numpy(), own_payload)
    assert counts == bch_ref.tally(own_status, own_payload, payload) == want_counts
    dec.close()
    enc.close()


def test_coder_with_outer_bch(built, tmp_path):
    """tests/cpp/coder_outer_bch.cpp: Coder(1152, 2304, rate_1_2) with setOuterBch(8): encode -> test(0.4) -> decode returns
    the payload with every frame clean; with 3, 8 and 9 wrong bits planted in the source rows of three frames the outer code
    repairs the first two and reports the third as not decodable, its payload as the inner decoder left it."""
    out = subprocess.run([BU.coder_outer_bch_exe(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "refused=ok lengths=ok ErrNum=0 clean=ok repaired=ok" in out.stdout, out.stdout
