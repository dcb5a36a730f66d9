"""The transport-block stage on the GPU (ldpc_tb_attach_device / ldpc_tb_check_device / ldpc_tb_tally_device and the
host-buffer forms) against tb_ref: byte for byte on shifted pointers with guard regions behind every output, detection of
single flips and bursts, the tally, the host forms over two chunks, refused calls, the chain attach -> encoder -> match ->
channel -> recover -> decoder -> check -> tally in HBM against the oracle, and Coder::setTransportBlock."""
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import channel

import ratematch_util as U
import tb_ref
import tb_util as TU

pytestmark = pytest.mark.gpu

GUARD, MARK = 64, 0xA5


def _torch():
    import torch
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _tb(shape):
    A, tb_crc, C, cb_crc, K = shape
    return L.TransportBlock(A, K, C=C, tb_crc=tb_crc, cb_crc=cb_crc)


def _up(host, shift):
    """uint8 array -> (cuda tensor that holds it `shift` bytes in, device pointer of its first byte)."""
    torch = _torch()
    host = np.ascontiguousarray(host, np.uint8).reshape(-1)
    t = torch.zeros(shift + host.size, dtype=torch.uint8, device="cuda")
    t[shift:] = torch.from_numpy(host).cuda()
    return t, t.data_ptr() + shift


def _out(n, shift):
    """A marker-filled output of n bytes, `shift` bytes into its buffer, 64 guard bytes behind it."""
    t = _torch().full((shift + n + GUARD,), MARK, dtype=_torch().uint8, device="cuda")
    return t, t.data_ptr() + shift


def _down(t, n, shift, what):
    host = t.cpu().numpy()
    assert (host[:shift] == MARK).all() and (host[shift + n:] == MARK).all(), "wrote outside the %s buffer" % what
    return host[shift:shift + n]


def _attach_device(tb, payload, in_shift=0, out_shift=0):
    payload = np.ascontiguousarray(payload, np.uint8).reshape(-1, tb.A // 8)
    tbs = payload.shape[0]
    keep, pay_ptr = _up(payload, in_shift)
    n = tbs * tb.C * (tb.K // 8)
    src, src_ptr = _out(n, out_shift)
    tb.attach_device(pay_ptr, tbs, src_ptr, n, _stream())
    _torch().cuda.synchronize()
    return _down(src, n, out_shift, "src").reshape(tbs * tb.C, tb.K // 8)


def _check_device(tb, dec, want=("payload", "cb_ok", "tb_ok"), in_shift=0, out_shift=0):
    """-> {name: array} for the outputs in `want`; the others are passed as NULL."""
    dec = np.ascontiguousarray(dec, np.uint8).reshape(-1, tb.K // 8)
    tbs = dec.shape[0] // tb.C
    keep, dec_ptr = _up(dec, in_shift)
    sizes = {"payload": tbs * (tb.A // 8), "cb_ok": tbs * tb.C, "tb_ok": tbs}
    bufs = {k: _out(sizes[k], out_shift) for k in want}
    ptr = {k: (bufs[k][1] if k in bufs else None) for k in sizes}
    tb.check_device(dec_ptr, tbs, ptr["payload"], ptr["cb_ok"], ptr["tb_ok"], _stream())
    _torch().cuda.synchronize()
    got = {k: _down(bufs[k][0], sizes[k], out_shift, k) for k in want}
    if "payload" in got:
        got["payload"] = got["payload"].reshape(tbs, tb.A // 8)
    return got


def _damage(frames, spec, rng):
    """A copy of attach output [tbs * C, K/8] in which every second transport block has one random bit flipped --
    anywhere in its C frames, fillers included -- and every fifth a random byte replaced."""
    bad = np.array(frames).reshape(-1, spec.C * (spec.K // 8))
    for t in range(bad.shape[0]):
        if t % 2:
            bit = int(rng.integers(0, spec.C * spec.K))
            bad[t, bit >> 3] ^= 1 << (bit & 7)
        if t % 5 == 4:
            bad[t, int(rng.integers(0, bad.shape[1]))] = int(rng.integers(0, 256))
    return bad.reshape(-1, spec.K // 8)


@pytest.mark.parametrize("shape", TU.SHAPES, ids=lambda s: "A%d_tb%d_C%d_cb%d_K%d" % s)
def test_attach_and_check_equal_the_reference(built, shape):
    rng = np.random.default_rng(80 + TU.SHAPES.index(shape))
    spec, tb = TU.ref_spec(shape), _tb(shape)
    payload = rng.integers(0, 256, (65, spec.A // 8), dtype=np.uint8)
    want_frames = tb_ref.attach(spec, payload)
    bad = _damage(want_frames, spec, rng)
    want = dict(zip(("payload", "cb_ok", "tb_ok"), tb_ref.check(spec, bad)))
    assert 0 < int(want["tb_ok"].sum()) < 65
    for tbs in (1, 65):
        rows = tbs * spec.C
        for in_shift, out_shift in ((1, 3), (3, 1)):
            got = _attach_device(tb, payload[:tbs], in_shift, out_shift)
            assert np.array_equal(got, want_frames[:rows]), (shape, tbs, in_shift, out_shift)
            # check(attach(x)) = x with every flag set
            back = _check_device(tb, got, in_shift=in_shift, out_shift=out_shift)
            assert np.array_equal(back["payload"], payload[:tbs]) and back["cb_ok"].all() and back["tb_ok"].all(), (shape, tbs)
            # damaged blocks: all three outputs together, then each alone
            for names in (("payload", "cb_ok", "tb_ok"), ("payload",), ("cb_ok",), ("tb_ok",)):
                res = _check_device(tb, bad[:rows], names, in_shift, out_shift)
                for k in names:
                    n = {"payload": tbs, "cb_ok": rows, "tb_ok": tbs}[k]
                    assert np.array_equal(res[k], want[k][:n]), (shape, tbs, names, k, in_shift, out_shift)


@pytest.mark.parametrize("shape", [TU.SHAPES[2], TU.SHAPES[8]], ids=["A312", "C4"])
def test_every_flip_and_burst_is_judged_as_the_reference_does(built, shape):
    """Transport block t of the first batch is one valid block with bit t of its C frames flipped; the second batch has
    bursts of up to L bits (L = the length of the CRC that covers the place).  One launch each."""
    rng = np.random.default_rng(90)
    spec, tb = TU.ref_spec(shape), _tb(shape)
    row = spec.C * spec.K
    valid = tb_ref.bits_of(tb_ref.attach(spec, rng.integers(0, 256, (1, spec.A // 8), dtype=np.uint8))).reshape(-1)
    flips = np.tile(valid, (row, 1))
    flips[np.arange(row), np.arange(row)] ^= 1
    L_cover = 24 if spec.cb_crc else spec.tb_crc
    bursts = np.tile(valid, (256, 1))
    inside = np.zeros(256, bool)
    frame_of = np.zeros(256, int)
    for t in range(256):
        n = int(rng.integers(1, L_cover + 1))
        at = int(rng.integers(0, row - n + 1))
        pattern = rng.integers(0, 2, n, dtype=np.uint8)
        pattern[0] = pattern[-1] = 1
        bursts[t, at:at + n] ^= pattern
        frame_of[t] = at // spec.K
        inside[t] = (at + n - 1) // spec.K == frame_of[t] and (at + n - 1) % spec.K < spec.Kp
    for batch in (flips, bursts):
        dec = tb_ref.bytes_of(batch.reshape(-1, spec.K))
        got = _check_device(tb, dec)
        want = tb_ref.check(spec, dec)
        for k, w in zip(("payload", "cb_ok", "tb_ok"), want):
            assert np.array_equal(got[k], w), (shape, k)
    # beyond the reference: every flip in front of the fillers is detected, every flip inside them changes nothing
    got = _check_device(tb, tb_ref.bytes_of(flips.reshape(-1, spec.K)))
    cb_ok = got["cb_ok"].reshape(row, spec.C)
    for t in range(row):
        c, i = divmod(t, spec.K)
        if i < spec.Kp:
            assert got["tb_ok"][t] == 0, (shape, t)
            if spec.cb_crc:
                assert cb_ok[t, c] == 0 and cb_ok[t].sum() == spec.C - 1, (shape, t)
        else:
            assert got["tb_ok"][t] == 1 and cb_ok[t].all(), (shape, t)
    # a burst no longer than the CRC, inside one frame's first Kp bits, is always detected
    got = _check_device(tb, tb_ref.bytes_of(bursts.reshape(-1, spec.K)))
    assert inside.sum() > 100
    assert not got["tb_ok"][inside].any()
    if spec.cb_crc:
        assert not got["cb_ok"].reshape(256, spec.C)[np.nonzero(inside)[0], frame_of[inside]].any()


def test_tally_equals_numpy(built):
    torch = _torch()
    rng = np.random.default_rng(91)
    tb = _tb(TU.SHAPES[2])
    tbs, per = 300, tb.A // 8
    ref = rng.integers(0, 256, (tbs, per), dtype=np.uint8)
    payload = ref.copy()
    ok = np.ones(tbs, np.uint8)
    kind = np.arange(tbs) % 4                     # 0 good, 1 undetected, 2 detected, 3 parity only
    kind[:4] = (0, 1, 2, 3)
    kind[4:] = rng.integers(0, 4, tbs - 4)
    for t in range(tbs):
        if kind[t] in (1, 2):
            payload[t, (t * 7) % per] ^= 1 << (t % 8)          # the last byte and the first among them
        if kind[t] in (2, 3):
            ok[t] = 0
    payload[5] = ref[5]
    payload[5, per - 1] ^= 0x80
    kind[5], ok[5] = 1, 1
    want = tb_ref.tally(ok, payload, ref)
    assert want == (int((kind >= 2).sum()), int(((kind == 1) | (kind == 2)).sum()), int((kind == 1).sum()), int((kind == 3).sum()))
    assert min(want) > 0
    okd, pd, rd = (torch.from_numpy(a).cuda() for a in (ok, payload, ref))
    assert tb.tally_device(okd.data_ptr(), pd.data_ptr(), rd.data_ptr(), tbs, _stream()) == want
    # ref NULL = all zero; shifted pointers
    keep1, p1 = _up(payload, 3)
    keep2, o1 = _up(ok, 1)
    assert tb.tally_device(o1, p1, None, tbs, _stream()) == tb_ref.tally(ok, payload, None)
    zero = np.zeros_like(payload)
    zero[7, 3] = 1
    keep3, z1 = _up(zero, 1)
    assert tb.tally_device(o1, z1, None, tbs, _stream()) == tb_ref.tally(ok, zero, None)
    assert tb.tally_device(o1, z1, None, 0, _stream()) == (0, 0, 0, 0)


def test_host_forms_equal_the_device_forms(built):
    rng = np.random.default_rng(92)
    for shape in (TU.SHAPES[2], TU.SHAPES[7], TU.SHAPES[12]):
        spec, tb = TU.ref_spec(shape), _tb(shape)
        payload = rng.integers(0, 256, (9, spec.A // 8), dtype=np.uint8)
        frames = tb.attach(payload)
        assert np.array_equal(frames, _attach_device(tb, payload)) and np.array_equal(frames, tb_ref.attach(spec, payload))
        bad = _damage(frames, spec, rng)
        got = tb.check(bad)
        dev = _check_device(tb, bad)
        for k, g, w in zip(("payload", "cb_ok", "tb_ok"), got, tb_ref.check(spec, bad)):
            assert np.array_equal(g, dev[k]) and np.array_equal(g, w), (shape, k)


def test_host_forms_over_two_chunks(built):
    """K = 8448, C = 8: a transport block is 8448 bytes of frames, so the 64 MiB scratch holds 7943 of them and 7944 take
    two chunks in both calls."""
    torch = _torch()
    shape = (8 * 8424 - 24, 24, 8, 24, 8448)
    spec, tb = TU.ref_spec(shape), _tb(shape)
    tbs = 7944
    assert (64 << 20) // (spec.C * spec.K // 8) == tbs - 1
    payload = np.random.default_rng(93).integers(0, 256, (tbs, spec.A // 8), dtype=np.uint8)
    frames = tb.attach(payload)
    pd = torch.from_numpy(payload).cuda()
    fd = torch.empty(frames.size, dtype=torch.uint8, device="cuda")
    tb.attach_device(pd.data_ptr(), tbs, fd.data_ptr(), fd.numel(), _stream())
    torch.cuda.synchronize()
    assert np.array_equal(frames.reshape(-1), fd.cpu().numpy())
    for t in (0, tbs - 2, tbs - 1):
        assert np.array_equal(frames[t * spec.C:(t + 1) * spec.C], tb_ref.attach(spec, payload[t:t + 1])), t
    frames[(tbs - 1) * spec.C + 3, 17] ^= 4             # in the second chunk
    frames[5 * spec.C, spec.K // 8 - 1] ^= 0x80         # the last CRC24B bit of a code block in the first chunk (Kp = K here)
    got, cb_ok, tb_ok = tb.check(frames)
    want_payload = payload.copy()
    s = 3 * spec.S + 17 * 8 + 2                         # the stream bit behind bit 2 of byte 17 of code block 3
    want_payload[tbs - 1, s >> 3] ^= 1 << (s & 7)
    want_cb = np.ones(tbs * spec.C, np.uint8)
    want_cb[(tbs - 1) * spec.C + 3] = want_cb[5 * spec.C] = 0
    want_tb = np.ones(tbs, np.uint8)
    want_tb[tbs - 1] = want_tb[5] = 0
    assert np.array_equal(got, want_payload) and np.array_equal(cb_ok, want_cb) and np.array_equal(tb_ok, want_tb)


def test_refused_calls_enqueue_nothing(built):
    torch = _torch()
    tb = _tb(TU.SHAPES[8])                               # A/8 = 126, 4 frames of 36 bytes
    buf = torch.full((4096,), MARK, dtype=torch.uint8, device="cuda")
    src = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p, s = buf.data_ptr(), src.data_ptr()
    bad = _tb(TU.SHAPES[8])
    bad.spec.C = 5
    for call in (lambda: tb.attach_device(s, 4, p, 4 * 144 - 1, _stream()),
                 lambda: tb.attach_device(p, 4, p + 503, 4 * 144, _stream()),
                 lambda: bad.attach_device(s, 4, p, 4096, _stream()),
                 lambda: tb.check_device(s, 4, None, None, None, _stream()),
                 lambda: tb.check_device(p, 4, p + 575, None, None, _stream()),
                 lambda: tb.check_device(s, 4, p, p + 503, None, _stream()),
                 lambda: bad.check_device(s, 4, p, None, None, _stream()),
                 lambda: tb.check_device(s, -1, p, None, None, _stream())):
        with pytest.raises(L.LdpcError) as e:
            call()
        assert e.value.code == 1
    tb.attach_device(s, 0, p, 0, _stream())              # tbs == 0: nothing
    tb.check_device(s, 0, p, p + 1024, p + 2048, _stream())
    assert tb.tally_device(s, s, None, 0, _stream()) == (0, 0, 0, 0)
    torch.cuda.synchronize()
    assert bool((buf == MARK).all())


# ---- the chain in device memory against the oracle ---------------------------------------------------------------

@pytest.mark.parametrize("point", ["clean", "hard"])
@pytest.mark.parametrize("algo", ["layered", "ms", "sp"])
def test_chain_equals_the_oracle(built, algo, point):
    """TransportBlock.attach_device -> Encoder -> RateMatcher.match_device -> ldpc_awgn_device -> recover_device -> Decoder
    -> check_device -> tally_device, all in HBM, at the clean and the hard point of tb_util; decoded bytes and iteration
    counts against the oracle, flags, payload and counts against tb_ref applied to the oracle's output."""
    torch = _torch()
    snr = TU.chain_points(algo)[point == "hard"]
    payload, want_src, want_code = TU.chain_payload()
    want_tx, want_rx, want_y, sd = TU.chain_received(snr)
    want_out, want_iters, want_payload, want_cb, want_tb, want_counts = TU.chain_oracle(algo, snr)
    print("%s %.1f dB: oracle leaves failed %d wrong %d undetected %d parity-only %d of %d" % ((algo, snr) + want_counts + (U.FRAMES,)))
    if point == "hard":
        assert TU.WINDOW[0] <= want_counts[0] <= TU.WINDOW[1]        # the comparison below is not vacuous
    else:
        assert want_counts == (0, 0, 0, 0)
    rows, cols, _ = U.bg1()
    tb = L.TransportBlock(TU.A, U.K)
    assert (tb.filler_lo, tb.filler_hi) == U.FILLER
    g = L.Graph(rows, cols, U.M, U.N)
    enc = L.Encoder(g, U.K, U.Z, max_frames=U.FRAMES)
    rm = L.RateMatcher(U.N, punctured=U.P, filler=(tb.filler_lo, tb.filler_hi), fill_llr=10.0, erasure_llr=TU.ERASURE)
    dec = L.Decoder(g, U.K, max_batch=U.FRAMES, algo=algo, max_iter=U.MAX_ITER, llr_scale=TU.HARD[algo][1], layer_rows=U.Z)
    pay = torch.from_numpy(np.array(payload)).cuda()
    src = torch.full((U.FRAMES, U.K // 8), MARK, dtype=torch.uint8, device="cuda")
    code = torch.empty((U.FRAMES, U.N), dtype=torch.uint8, device="cuda")
    tx = torch.empty((U.FRAMES, TU.E), dtype=torch.uint8, device="cuda")
    y = torch.full((U.FRAMES, U.N), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.zeros(L.out_bytes(U.K, U.FRAMES), dtype=torch.uint8, device="cuda")
    iters = torch.zeros(U.FRAMES, dtype=torch.int32, device="cuda")
    back = torch.full((U.FRAMES, TU.A // 8), MARK, dtype=torch.uint8, device="cuda")
    cb_ok = torch.full((U.FRAMES,), MARK, dtype=torch.uint8, device="cuda")
    tb_ok = torch.full((U.FRAMES,), MARK, dtype=torch.uint8, device="cuda")
    tb.attach_device(pay.data_ptr(), U.FRAMES, src.data_ptr(), src.numel(), _stream())
    enc.encode_device(src.data_ptr(), src.numel(), U.FRAMES, code.data_ptr(), code.numel(), "bits", _stream())
    rm.match_device(code.data_ptr(), U.FRAMES, TU.K0, TU.E, tx.data_ptr(), tx.numel(), "bits", "bits", _stream())
    rx = channel.awgn_device(TU.E, 0, U.FRAMES, sd, seed=TU.SEED, codewords=tx, stream=_stream())
    rm.recover_device(rx.data_ptr(), U.FRAMES, TU.K0, TU.E, None, False, y.data_ptr(), _stream())
    dec.decode_device(y.data_ptr(), U.FRAMES, out.data_ptr(), out.numel(), iters.data_ptr(), _stream())
    tb.check_device(out.data_ptr(), U.FRAMES, back.data_ptr(), cb_ok.data_ptr(), tb_ok.data_ptr(), _stream())
    counts = tb.tally_device(tb_ok.data_ptr(), back.data_ptr(), pay.data_ptr(), U.FRAMES, _stream())
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), want_src)
    assert np.array_equal(code.cpu().numpy(), want_code)
    assert np.array_equal(tx.cpu().numpy(), want_tx)
    assert np.array_equal(rx.cpu().numpy().view(np.uint32), want_rx.view(np.uint32))
    assert np.array_equal(y.cpu().numpy().view(np.uint32), want_y.view(np.uint32))
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(iters.cpu().numpy(), want_iters)
    assert np.array_equal(cb_ok.cpu().numpy(), want_cb) and np.array_equal(tb_ok.cpu().numpy(), want_tb)
    assert np.array_equal(back.cpu().numpy(), want_payload)
    assert counts == want_counts
    dec.close()
    enc.close()


def test_coder_with_transport_block(built, tmp_path):
    """tests/cpp/coder_transport_block.cpp: Coder(1152, 2304, rate_1_2) with setTransportBlock(1128), srand(1), encode ->
    test(0.4) -> decode returns the payload bytes and every CRC passes; with frame 7 of the received values replaced by
    noise exactly that frame fails; setTransportBlock(1160) is refused."""
    out = subprocess.run([TU.coder_transport_block_exe(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "refused=ok lengths=ok ErrNum=0 CrcFailures=0 noisy=ok" in out.stdout, out.stdout
