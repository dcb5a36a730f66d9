"""The batched encoder on the GPU (ldpc_encode_device / ldpc_encode / Coder::setEncodeOnDevice).

Expected bytes never come from the code under test.  Small codes: oracle.gf2_encoder.Gf2Encoder (plain Gaussian
elimination).  Large codes: a systematic codeword with H c = 0 is unique once the parity part is nonsingular (it is
for the recognised structures), so "information part equals the source bits and the syndrome is zero" pins every
parity bit; where codes.py has a numpy encoder it is compared too."""
import subprocess

import numpy as np
import pytest

import oracle
import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes
from oracle.gf2_encoder import Gf2Encoder

from encoder_util import (coder_device_encode_exe, info_bits, reference_packed, stream_length, syndrome_weight)

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _encode_device(enc, src, frames, fmt, src_nbytes=None):
    """src: numpy uint8 stream -> numpy uint8 [frames, N/8] (packed) or [frames, N] (bits) through device buffers."""
    torch = _torch()
    sd = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    per = enc.N // 8 if fmt == "packed" else enc.N
    code = torch.full((frames * per + 64,), 0xEE, dtype=torch.uint8, device="cuda")       # 64 guard bytes behind
    enc.encode_device(sd.data_ptr(), src.size if src_nbytes is None else src_nbytes, frames, code.data_ptr(), frames * per, fmt,
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = code.cpu().numpy()
    assert (host[frames * per:] == 0xEE).all(), "wrote behind the end of the code buffer"
    return host[:frames * per].reshape(frames, per)


def _check_against_gf2(rows, cols, M, N, K, z, frames=70, cut=5, seed=0):
    rng = np.random.default_rng(seed)
    g = L.Graph(rows, cols, M, N)
    ge = Gf2Encoder(rows, cols, M, N)
    src = rng.integers(0, 256, stream_length(K, frames, cut), dtype=np.uint8)
    want = reference_packed(ge, src, frames)
    enc = L.Encoder(g, K, z, max_frames=128)
    packed = _encode_device(enc, src, frames, "packed")
    assert np.array_equal(packed, want)
    bits = _encode_device(enc, src, frames, "bits")
    assert np.array_equal(bits, np.unpackbits(want, axis=1, bitorder="little"))
    # host buffers: one chunk, chunks of 32 frames, a single frame
    assert np.array_equal(enc.encode(src).reshape(frames, -1), want)
    enc.close()
    small = L.Encoder(g, K, z, max_frames=32)
    assert np.array_equal(small.encode(src).reshape(frames, -1), want)
    one = small.encode(src[:K // 8 - 3])
    assert np.array_equal(one, ge.encode_bytes(src[:K // 8 - 3].tobytes()))
    small.close()
    return want


@pytest.mark.parametrize("N", [576, 648, 2304])
@pytest.mark.parametrize("rate", range(6))
def test_wimax_seeds_equal_gaussian_elimination(built, rate, N):
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    _check_against_gf2(rows, cols, M, N, K, z, seed=100 * rate + N)


def test_bg1_profile_small_equals_gaussian_elimination_and_the_numpy_encoder(built):
    Z = 16
    rows, cols = codes.nr_bg1_profile_edges(Z)
    want = _check_against_gf2(rows, cols, 46 * Z, 68 * Z, 22 * Z, Z, seed=5)
    base = codes.nr_bg1_profile_base(Z=Z)
    bits = np.unpackbits(want, axis=1, bitorder="little")
    for f in (0, 33, 69):
        assert np.array_equal(bits[f], codes.nr_bg1_profile_encode(base, Z, bits[f, :22 * Z]))


def test_bg1_profile_z384(built):
    Z, frames = 384, 130
    M, N, K = 46 * Z, 68 * Z, 22 * Z
    rows, cols = codes.nr_bg1_profile_edges(Z)
    rng = np.random.default_rng(6)
    src = rng.integers(0, 256, stream_length(K, frames), dtype=np.uint8)
    enc = L.Encoder(L.Graph(rows, cols, M, N), K, Z, max_frames=256)
    bits = _encode_device(enc, src, frames, "bits")
    assert np.array_equal(bits[:, :K], info_bits(K, src, frames))
    assert syndrome_weight(rows, cols, M, bits) == 0
    base = codes.nr_bg1_profile_base(Z=Z)
    for f in (0, 63, 64, 129):
        assert np.array_equal(bits[f], codes.nr_bg1_profile_encode(base, Z, bits[f, :K]))
    assert np.array_equal(np.packbits(bits, axis=1, bitorder="little"), _encode_device(enc, src, frames, "packed"))
    enc.close()


def test_dvbs2_profile_small_equals_gaussian_elimination(built):
    rows, cols = codes.dvbs2_profile_edges(12960, 6480)
    _check_against_gf2(rows, cols, 6480, 12960, 6480, 0, seed=7)


def test_dvbs2_profile_64800(built):
    N, K, frames = 64800, 32400, 260
    M = N - K
    rows, cols = codes.dvbs2_profile_edges(N, K)
    rng = np.random.default_rng(8)
    src = rng.integers(0, 256, stream_length(K, frames, cut=9), dtype=np.uint8)
    enc = L.Encoder(L.Graph(rows, cols, M, N), K, 0, max_frames=512)
    bits = _encode_device(enc, src, frames, "bits")
    info = info_bits(K, src, frames)
    assert np.array_equal(bits[:, :K], info)
    assert syndrome_weight(rows, cols, M, bits) == 0
    sel = cols < K
    for f in (0, 64, 191, 259):
        lam = np.zeros(M, np.int64)
        np.add.at(lam, rows[sel], info[f][cols[sel]])
        assert np.array_equal(bits[f, K:], (np.cumsum(lam & 1) & 1).astype(np.uint8))
    assert np.array_equal(np.packbits(bits, axis=1, bitorder="little"), _encode_device(enc, src, frames, "packed"))
    enc.close()


def test_rate_3_4_b_at_64800(built):
    """The seed whose weight-3 parity column has a non-zero middle shift, at a size no host encoder of the project serves."""
    rate, N, frames = codes.RATE_3_4_B, 64800, 64
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    rng = np.random.default_rng(9)
    src = rng.integers(0, 256, stream_length(K, frames), dtype=np.uint8)
    enc = L.Encoder(L.Graph(rows, cols, M, N), K, z, max_frames=64)
    assert enc.structure()["b"] == 80 * z // 96
    bits = _encode_device(enc, src, frames, "bits")
    assert np.array_equal(bits[:, :K], info_bits(K, src, frames))
    assert syndrome_weight(rows, cols, M, bits) == 0
    enc.close()


def test_frames_do_not_depend_on_their_neighbours(built):
    rate, N, frames = codes.RATE_2_3_A, 2304, 2100
    K, M, z = codes.wimax_dims(rate, N)
    assert K % 8 == 0
    rows, cols = codes.wimax_edges(rate, N)
    rng = np.random.default_rng(10)
    src = rng.integers(0, 256, frames * K // 8, dtype=np.uint8)
    enc = L.Encoder(L.Graph(rows, cols, M, N), K, z, max_frames=2112)
    whole = _encode_device(enc, src, frames, "packed")
    first = _encode_device(enc, src[:2048 * K // 8], 2048, "packed")
    rest = _encode_device(enc, src[2048 * K // 8:], frames - 2048, "packed")
    assert np.array_equal(whole, np.concatenate([first, rest]))
    assert syndrome_weight(rows, cols, M, np.unpackbits(whole[::37], axis=1, bitorder="little")) == 0
    ge = Gf2Encoder(rows, cols, M, N)
    for f in (0, 2047, 2048, 2099):
        assert np.array_equal(whole[f], ge.encode_bytes(src[f * K // 8:(f + 1) * K // 8].tobytes()))
    enc.close()


def test_closed_loop_in_device_memory(built):
    """encode -> channel -> decode -> count on buffers that never leave HBM, against the oracle at every stage."""
    torch = _torch()
    rate, N, frames, sd, seed = codes.RATE_1_2, 2304, 64, 0.8, 4242
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    g = L.Graph(rows, cols, M, N)
    og = oracle.Graph(rows, cols, M, N, K)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    src = torch.randint(0, 256, (frames * K // 8,), dtype=torch.uint8, device="cuda", generator=gen)
    src_host = src.cpu().numpy()
    enc = L.Encoder(g, K, z, max_frames=frames)
    code = torch.empty((frames, N), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    enc.encode_device(src.data_ptr(), src.numel(), frames, code.data_ptr(), code.numel(), "bits", stream)
    y = channel.awgn_device(N, 0, frames, sd, seed=seed, codewords=code)
    want_bits = np.unpackbits(reference_packed(Gf2Encoder(rows, cols, M, N), src_host, frames), axis=1, bitorder="little")
    assert np.array_equal(code.cpu().numpy(), want_bits)
    want_y = oracle.awgn(N, 0, frames, sd, seed=seed, codewords=want_bits)
    assert np.array_equal(y.cpu().numpy().view(np.uint32), want_y.view(np.uint32))
    for algo in ("ms", "layered"):
        dec = L.Decoder(g, K, max_batch=frames, algo=algo, max_iter=20, layer_rows=z)
        out = torch.zeros(L.out_bytes(K, frames), dtype=torch.uint8, device="cuda")
        dec.decode_device(y.data_ptr(), frames, out.data_ptr(), out.numel(), None, stream)
        got = channel.count_errors_device(out, src, frames)
        ref = oracle.decode(og, want_y, algo, max_iter=20, layer_rows=z)["out"]
        assert np.array_equal(out.cpu().numpy(), ref), algo
        x = (ref ^ src_host).reshape(frames, K // 8)
        want = (int(np.unpackbits(x).sum()), int((x != 0).sum()), int((x != 0).any(axis=1).sum()))
        print("closed loop %s: (bit, byte, frame) errors device %s oracle %s" % (algo, got, want))
        assert got == want, algo
        dec.close()
    enc.close()


def test_argument_errors_enqueue_nothing(built):
    torch = _torch()
    rate, N = codes.RATE_1_2, 648
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    enc = L.Encoder(L.Graph(rows, cols, M, N), K, z, max_frames=8)
    src = torch.zeros(8 * 41, dtype=torch.uint8, device="cuda")
    code = torch.full((8 * N,), 0xEE, dtype=torch.uint8, device="cuda")
    s, c = src.data_ptr(), code.data_ptr()
    for args in ((s, src.numel(), 9, c, code.numel(), "bits"),          # frames > max_frames
                 (s, 80, 4, c, code.numel(), "bits"),                   # frame 3 starts at byte 121
                 (s, src.numel(), 8, c, 8 * N - 1, "bits"),             # code buffer too small
                 (s, src.numel(), 8, c, 8 * N // 8 - 1, "packed"),
                 (None, src.numel(), 8, c, code.numel(), "bits"),
                 (s, src.numel(), 8, None, code.numel(), "bits"),
                 (s, src.numel(), 8, c, code.numel(), 7)):              # unknown format
        with pytest.raises(L.LdpcError) as e:
            enc.encode_device(*args)
        assert e.value.code == 1, args
    torch.cuda.synchronize()
    assert bool((code == 0xEE).all())
    # N % 8 != 0: bits only
    Z = 3
    r2, c2 = codes.nr_bg1_profile_edges(Z)
    odd = L.Encoder(L.Graph(r2, c2, 46 * Z, 68 * Z), 22 * Z, Z, max_frames=8)
    with pytest.raises(L.LdpcError) as e:
        odd.encode_device(s, src.numel(), 2, c, code.numel(), "packed")
    assert e.value.code == 1
    rng = np.random.default_rng(12)
    stream_bytes = rng.integers(0, 256, stream_length(22 * Z, 5), dtype=np.uint8)
    bits = _encode_device(odd, stream_bytes, 5, "bits")
    ge = Gf2Encoder(r2, c2, 46 * Z, 68 * Z)
    info = info_bits(22 * Z, stream_bytes, 5)
    for f in range(5):
        assert np.array_equal(bits[f], np.concatenate([info[f], ge.parity(info[f])]))
    odd.close()
    enc.close()


def test_buffers_of_any_alignment(built):
    """Code buffers that start at an odd address take the byte-wise stores: same bytes."""
    torch = _torch()
    rate, N, frames = codes.RATE_5_6, 576, 70
    K, M, z = codes.wimax_dims(rate, N)
    rows, cols = codes.wimax_edges(rate, N)
    rng = np.random.default_rng(13)
    src = rng.integers(0, 256, stream_length(K, frames), dtype=np.uint8)
    want = reference_packed(Gf2Encoder(rows, cols, M, N), src, frames)
    enc = L.Encoder(L.Graph(rows, cols, M, N), K, z, max_frames=128)
    sd = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), src])).cuda()
    for fmt, per, ref in (("packed", N // 8, want), ("bits", N, np.unpackbits(want, axis=1, bitorder="little"))):
        for shift in (1, 4, 8):
            code = torch.full((frames * per + 64,), 0xEE, dtype=torch.uint8, device="cuda")
            enc.encode_device(sd.data_ptr() + 3, src.size, frames, code.data_ptr() + shift, frames * per, fmt,
                              torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            host = code.cpu().numpy()
            assert (host[:shift] == 0xEE).all() and (host[shift + frames * per:] == 0xEE).all(), (fmt, shift)
            assert np.array_equal(host[shift:shift + frames * per].reshape(frames, per), ref), (fmt, shift)
    enc.close()


@pytest.mark.parametrize("rate,N", [(0, 648), (0, 2304), (1, 2304), (2, 2304), (3, 2304), (5, 2304), (4, 2304)])
def test_coder_device_path_equals_host_path(built, tmp_path, rate, N):
    """Coder::encode with setEncodeOnDevice(true) against the host path, byte for byte: a multi-frame payload with a
    short tail; (0, 648) has K % 8 = 4; rate 4 (3/4B) is the seed the host solves by dense elimination."""
    exe = coder_device_encode_exe(tmp_path)
    K = codes.wimax_dims(rate, N)[0]
    out = subprocess.run([exe, "compare", str(rate), str(N), str(stream_length(K, 70, cut=7))], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host=0 device=0 " in out.stdout and " differ=0" in out.stdout, out.stdout


def test_coder_rate_3_4_b_at_64800_round_trip(built, tmp_path):
    """Coder(48600, 64800, rate_3_4_b): the host path answers LDPC_ERR_UNSUPPORTED (4), the device path encodes, and
    encode -> test -> decode(DecodeMS) of 8 frames at sd = 0.3 (10.5 dB) returns the payload."""
    exe = coder_device_encode_exe(tmp_path)
    out = subprocess.run([exe, "roundtrip", "4", "64800", "8", "0.3"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    assert "hostForEncoder=4 ParityFail=0 ErrNum=0" in out.stdout, out.stdout
