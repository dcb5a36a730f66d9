"""The modem stage on the GPU (ldpc_modem_transmit_device / ldpc_modem_demap_device and their host-buffer forms) against
modem_ref: symbols and demapped values as uint32 bit patterns, shifted pointers, guard regions around every output, the
Qm = 1 case against ldpc_awgn_device and the oracle's channel, and the closed chain encoder -> match -> transmit -> demap
-> recover -> decoder against the oracle."""
import subprocess

import numpy as np
import pytest

import oracle
import myldpccppapi_amd as L
from myldpccppapi_amd import channel

import modem_ref as mref
import modem_util as MU
import ratematch_util as U

pytestmark = pytest.mark.gpu

GUARD = 64
QMS = (1, 2, 4, 6, 8)


def _torch():
    import torch
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _transmit_device(md, bits, sd, seed, first_frame, fmt="bits", tx_shift=0, sym_shift=0):
    """bits uint8 [frames, E] -> symbols as the device writes them, float32 [frames, symbol_floats]; the output is
    pre-filled with NaN, starts `sym_shift` floats into its buffer and has 64 guard floats behind it."""
    torch = _torch()
    frames, E = bits.shape
    src = np.ascontiguousarray(bits if fmt == "bits" else np.packbits(bits, axis=1, bitorder="little")).reshape(-1)
    td = torch.zeros(tx_shift + src.size, dtype=torch.uint8, device="cuda")
    td[tx_shift:] = torch.from_numpy(src).cuda()
    n = frames * md.symbol_floats(E)
    sym = torch.full((sym_shift + n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    md.transmit_device(td.data_ptr() + tx_shift, frames, E, sd, seed, sym.data_ptr() + 4 * sym_shift, n, first_frame, fmt, _stream())
    torch.cuda.synchronize()
    host = sym.cpu().numpy()
    assert np.isnan(host[:sym_shift]).all() and np.isnan(host[sym_shift + n:]).all(), "wrote outside the sym buffer"
    return host[sym_shift:sym_shift + n].reshape(frames, -1)


def _demap_device(md, sym, E, rx_shift=0, sym_shift=0):
    """sym float32 [frames, symbol_floats] -> rx float32 [frames, E] as the device writes it (NaN-prefilled, guards)."""
    torch = _torch()
    frames = sym.shape[0]
    sd = torch.zeros(sym_shift + sym.size, dtype=torch.float32, device="cuda")
    sd[sym_shift:] = torch.from_numpy(np.ascontiguousarray(sym).reshape(-1)).cuda()
    rx = torch.full((rx_shift + frames * E + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    md.demap_device(sd.data_ptr() + 4 * sym_shift, frames, E, rx.data_ptr() + 4 * rx_shift, _stream())
    torch.cuda.synchronize()
    host = rx.cpu().numpy()
    assert np.isnan(host[:rx_shift]).all() and np.isnan(host[rx_shift + frames * E:]).all(), "wrote outside the rx buffer"
    out = host[rx_shift:rx_shift + frames * E].reshape(frames, E)
    assert not np.isnan(out).any(), "left a position of rx unwritten"
    return out


def _special_symbols(Qm, shape, rng):
    """Axis values on the levels, exactly midway between neighbouring levels (0 among them: D1 = D0), on and beyond the
    outermost levels up to |r| = 3."""
    if Qm == 1:
        pool = np.array([0.0, -0.0, 1.0, -1.0, 3.0, -3.0, 0.5], np.float32)
    else:
        lev = np.sort(mref.axis_levels(Qm)[1])
        mid = ((lev[1:] + lev[:-1]) * np.float32(0.5)).astype(np.float32)
        pool = np.concatenate([lev, mid, -mid, [np.float32(-0.0)], [lev[-1] * np.float32(1.5), lev[0] * np.float32(1.5)],
                               np.array([3.0, -3.0, 2.999, -2.5], np.float32)]).astype(np.float32)
    return pool[rng.integers(0, pool.size, shape)]


@pytest.mark.parametrize("Qm", QMS)
def test_transmit_and_demap_equal_the_reference_bit_for_bit(built, Qm):
    rng = np.random.default_rng(60 + Qm)
    case = 0
    for frames in (1, 65):
        for S in MU.S_GRID:
            E = S * Qm
            bits = rng.integers(0, 2, (frames, E), dtype=np.uint8)
            for il in (False, True):
                md = L.Modem(Qm, interleave=il)
                assert md.symbol_floats(E) == mref.symbol_floats(Qm, E)
                for first_frame in (0, 2 ** 32 + 5):
                    for sd in (0.0, 0.3):
                        want = mref.transmit(Qm, il, bits, sd, 77, first_frame, MU.chlib())
                        for fmt in ("bits", "packed") if E % 8 == 0 else ("bits",):
                            case += 1
                            got = _transmit_device(md, bits, sd, 77, first_frame, fmt, tx_shift=case % 4, sym_shift=case % 2)
                            assert _same(got, want), (Qm, il, S, frames, first_frame, sd, fmt, case % 4, case % 2)
                    # demap: what was received at sd = 0.3, then the special values
                    for sym in (want, _special_symbols(Qm, want.shape, rng)):
                        case += 1
                        got = _demap_device(md, sym, E, rx_shift=case % 2, sym_shift=(case // 2) % 2)
                        assert _same(got, mref.demap(Qm, il, sym, E)), (Qm, il, S, frames, case)


def test_midway_symbols_demap_to_zero(built):
    """r = 0 lies exactly between the two innermost levels of every axis: D1 = D0 for the axis' first bit, y = +0."""
    for Qm in (2, 4, 6, 8):
        md = L.Modem(Qm, interleave=False)
        y = _demap_device(md, np.zeros((1, 2 * 3), np.float32), 3 * Qm).reshape(3, Qm)
        assert _same(y[:, :2], np.zeros((3, 2), np.float32))
        assert (y[:, 2:] != 0).all()


def test_bpsk_reproduces_ldpc_awgn_device(built):
    torch = _torch()
    rng = np.random.default_rng(66)
    md = L.Modem(1, interleave=False)
    for frames, E in ((1, 37), (65, 1032), (65, 1031)):
        bits = rng.integers(0, 2, (frames, E), dtype=np.uint8)
        for first_frame in (0, 2 ** 32 + 5):
            got = _transmit_device(md, bits, 0.7, 9, first_frame, "bits", tx_shift=1, sym_shift=1)
            dev = channel.awgn_device(E, first_frame, frames, 0.7, seed=9, codewords=torch.from_numpy(bits).cuda())
            assert _same(got, dev.cpu().numpy()), (frames, E, first_frame)
            assert _same(got, oracle.awgn(E, first_frame, frames, 0.7, seed=9, codewords=bits)), (frames, E, first_frame)
            assert _same(_demap_device(md, got, E, rx_shift=1), got)


def test_host_forms_equal_the_device_forms(built):
    rng = np.random.default_rng(67)
    for Qm, il, frames, E in ((6, True, 65, 6 * 257), (4, False, 3, 4 * 65), (1, False, 5, 37)):
        md = L.Modem(Qm, interleave=il)
        bits = rng.integers(0, 2, (frames, E), dtype=np.uint8)
        sym = md.transmit(bits, 0.3, 5, first_frame=11)
        assert _same(sym, _transmit_device(md, bits, 0.3, 5, 11))
        assert _same(sym, mref.transmit(Qm, il, bits, 0.3, 5, 11, MU.chlib()))
        if E % 8 == 0:
            assert _same(sym, md.transmit(np.packbits(bits, axis=1, bitorder="little"), 0.3, 5, first_frame=11, tx_fmt="packed"))
        assert _same(md.demap(sym, E), _demap_device(md, sym, E))


def test_host_forms_over_two_chunks(built):
    """QPSK, E = 48576: a frame is 194304 bytes of symbols and of rx, so the 64 MiB scratch holds 345 frames and 346
    frames take two chunks in both calls; the second chunk's noise must continue at first_frame + 345."""
    torch = _torch()
    frames, E = 346, 48576
    assert (64 << 20) // (4 * E) == 345
    md = L.Modem(2)
    bits = np.random.default_rng(68).integers(0, 2, (frames, E), dtype=np.uint8)
    sym = md.transmit(bits, 0.5, 21, first_frame=3)
    td = torch.from_numpy(bits).cuda()
    sd = torch.empty(frames * E, dtype=torch.float32, device="cuda")
    rd = torch.empty(frames * E, dtype=torch.float32, device="cuda")
    md.transmit_device(td.data_ptr(), frames, E, 0.5, 21, sd.data_ptr(), sd.numel(), 3, "bits", _stream())
    md.demap_device(sd.data_ptr(), frames, E, rd.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _same(sym.reshape(-1), sd.cpu().numpy())
    assert _same(md.demap(sym, E).reshape(-1), rd.cpu().numpy())
    for f in (0, 344, 345):
        assert _same(sym[f:f + 1], mref.transmit(2, True, bits[f:f + 1], 0.5, 21, 3 + f, MU.chlib())), f


def test_refused_calls_enqueue_nothing(built):
    torch = _torch()
    md = L.Modem(4)
    buf = torch.full((4 * 64,), 5.0, dtype=torch.float32, device="cuda")
    tx = torch.zeros(4 * 64, dtype=torch.uint8, device="cuda")
    for call in (lambda: md.demap_device(buf.data_ptr(), 2, 64, buf.data_ptr() + 4 * 63, _stream()),
                 lambda: md.transmit_device(tx.data_ptr(), 4, 64, 0.3, 1, buf.data_ptr(), 4 * 32 - 1, 0, "bits", _stream()),
                 lambda: md.transmit_device(tx.data_ptr(), 4, 62, 0.3, 1, buf.data_ptr(), 4 * 64, 0, "bits", _stream()),
                 lambda: md.transmit_device(tx.data_ptr(), 4, 64, -1.0, 1, buf.data_ptr(), 4 * 64, 0, "bits", _stream())):
        with pytest.raises(L.LdpcError) as e:
            call()
        assert e.value.code == 1
    md.transmit_device(tx.data_ptr(), 0, 64, 0.3, 1, buf.data_ptr(), 0, 0, "bits", _stream())      # frames == 0: nothing
    torch.cuda.synchronize()
    assert bool((buf == 5.0).all())


# ---- the chain in device memory against the oracle ---------------------------------------------------------------

@pytest.mark.parametrize("algo", ["layered", "ms", "sp"])
@pytest.mark.parametrize("Qm", [4, 6])
def test_chain_equals_the_oracle(built, Qm, algo):
    """Encoder -> RateMatcher.match_device -> Modem.transmit_device -> demap_device -> recover_device -> Decoder, all in
    HBM, at the scenario of DESIGN.md section 8f with the interleaver; every stage against its reference."""
    torch = _torch()
    rows, cols, _ = U.bg1()
    info, src_bytes, code_want = U.payload()
    scale, fill = MU.decoder_settings(Qm, algo)
    sd_noise = MU.POINTS[Qm]
    g = L.Graph(rows, cols, U.M, U.N)
    enc = L.Encoder(g, U.K, U.Z, max_frames=U.FRAMES)
    src = torch.from_numpy(np.array(src_bytes)).cuda()
    code = torch.empty((U.FRAMES, U.N), dtype=torch.uint8, device="cuda")
    enc.encode_device(src.data_ptr(), src.numel(), U.FRAMES, code.data_ptr(), code.numel(), "bits", _stream())
    rm = L.RateMatcher(U.N, punctured=U.P, filler=U.FILLER, fill_llr=fill, erasure_llr=MU.ERASURE)
    md = L.Modem(Qm)
    E = MU.E
    tx = torch.empty((U.FRAMES, E), dtype=torch.uint8, device="cuda")
    sym = torch.full((U.FRAMES, md.symbol_floats(E)), float("nan"), dtype=torch.float32, device="cuda")
    rx = torch.full((U.FRAMES, E), float("nan"), dtype=torch.float32, device="cuda")
    y = torch.full((U.FRAMES, U.N), float("nan"), dtype=torch.float32, device="cuda")
    rm.match_device(code.data_ptr(), U.FRAMES, MU.K0, E, tx.data_ptr(), tx.numel(), "bits", "bits", _stream())
    md.transmit_device(tx.data_ptr(), U.FRAMES, E, sd_noise, MU.SEED, sym.data_ptr(), sym.numel(), 0, "bits", _stream())
    md.demap_device(sym.data_ptr(), U.FRAMES, E, rx.data_ptr(), _stream())
    rm.recover_device(rx.data_ptr(), U.FRAMES, MU.K0, E, None, False, y.data_ptr(), _stream())
    dec = L.Decoder(g, U.K, max_batch=U.FRAMES, algo=algo, max_iter=U.MAX_ITER, llr_scale=scale, layer_rows=U.Z)
    out = torch.zeros(L.out_bytes(U.K, U.FRAMES), dtype=torch.uint8, device="cuda")
    iters = torch.zeros(U.FRAMES, dtype=torch.int32, device="cuda")
    dec.decode_device(y.data_ptr(), U.FRAMES, out.data_ptr(), out.numel(), iters.data_ptr(), _stream())
    torch.cuda.synchronize()
    want_sym, want_rx = MU.received(Qm, True)
    assert np.array_equal(code.cpu().numpy(), code_want)
    assert np.array_equal(tx.cpu().numpy(), MU.tx_bits())
    assert _same(sym.cpu().numpy(), want_sym)
    assert _same(rx.cpu().numpy(), want_rx)
    assert _same(y.cpu().numpy(), MU.recovered(Qm, True, fill))
    want_out, want_iters, wrong = MU.oracle_decode(Qm, True, algo)
    print("Qm %d %s: oracle frames wrong %d / %d, mean iterations %.2f" % (Qm, algo, wrong, U.FRAMES, float(np.mean(want_iters))))
    assert wrong == 0                      # the equality below is not vacuous: the oracle decodes every frame
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(iters.cpu().numpy(), want_iters)
    dec.close()
    enc.close()


def test_coder_with_modulation(built, tmp_path):
    """tests/cpp/coder_modulation.cpp: Coder(1152, 2304, rate_1_2) with setModulation(4), srand(1), encode -> test(0.3) ->
    decode returns the source bytes; without the setter test() writes the reference's samples; setModulation(3) is refused."""
    out = subprocess.run([MU.coder_modulation_exe(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "refused=ok plain=ok ErrNum=0" in out.stdout, out.stdout
