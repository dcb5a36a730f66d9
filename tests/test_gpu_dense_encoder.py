"""The dense encoder on the GPU (ldpc_encoder_create_dense + ldpc_encode_device / ldpc_encode).

Everything is GF(2): every comparison is exact.  A codeword is pinned by two facts, because the parity bits are the
unique solution of H_p p = H_s u: H' c = 0 for every frame (numpy, from the dense H') and c[0..K) = the source bits under
the data rule of ldpc_encode_device.  Where K = N - M the bytes are also those of oracle/gf2_encoder.py or of the
structured encoder, two solvers that share nothing with the dense one.  Shapes are the smallest that reach each guard of
enc_dense_kernel: W = 1, 2 and 65 words (the last crosses the 64-word tile of grid.y), rho = 100 < one row block, rho <
M, M = 324 = 5 * 64 + 4 (last stage and last word of T ragged), rho = 1152 = 18 row blocks."""
import numpy as np
import pytest

import oracle
import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes
from oracle.gf2_encoder import Gf2Encoder

import dense_encoder_util as U
from encoder_util import frame_starts, info_bits, reference_packed, stream_length

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def mats(built):
    """name -> dict(rows, cols, M, N, K, H): R and G re-ordered by the numpy elimination's systematic order."""
    out = {}
    for name, make in (("R", U.matrix_r), ("G", U.matrix_g)):
        rows, cols, M, N = make()
        perm, rank = U.systematic_order(U.dense(rows, cols, M, N))
        rows2, cols2 = codes.permute_columns(rows, cols, perm)
        out[name] = dict(rows=rows2, cols=cols2, M=M, N=N, K=N - rank, H=U.dense(rows2, cols2, M, N))
    assert out["R"]["K"] == 100 and out["G"]["K"] == 104
    return out


def _encode_device(enc, src, frames, fmt):
    """numpy uint8 stream -> numpy uint8 [frames, N/8] (packed) or [frames, N] (bits); 64 guard bytes on either side."""
    torch = _torch()
    sd = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    per = enc.N // 8 if fmt == "packed" else enc.N
    code = torch.full((frames * per + 128,), 0xEE, dtype=torch.uint8, device="cuda")
    enc.encode_device(sd.data_ptr(), src.size, frames, code.data_ptr() + 64, frames * per, fmt, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = code.cpu().numpy()
    assert (host[:64] == 0xEE).all() and (host[64 + frames * per:] == 0xEE).all(), "wrote outside the code buffer"
    return host[64:64 + frames * per].reshape(frames, per)


def _check_codewords(m, bits, src, frames):
    assert np.array_equal(bits[:, :m["K"]], info_bits(m["K"], src, frames))
    assert U.syndrome_weight_dense(m["H"], bits) == 0
    assert bits[:, m["K"]:].any(), "all parity bits zero: the payload was not random"


@pytest.mark.parametrize("frames", [1, 70, 4097])
def test_random_matrix_bits_and_packed(mats, frames):
    m = mats["R"]
    K, N = m["K"], m["N"]
    assert K % 8 == 4 and N % 8 == 0
    src = np.random.default_rng(frames).integers(0, 256, stream_length(K, frames), dtype=np.uint8)
    enc = L.DenseEncoder(L.Graph(m["rows"], m["cols"], m["M"], N), K, max_frames=frames)
    assert enc.structure() == dict(kind="dense", rho=100, rank_hp=100, M=100, t_words=2)
    bits = _encode_device(enc, src, frames, "bits")
    assert not bits[:, K - K % 8:K].any()          # information bits 96 .. 99 read zero
    _check_codewords(m, bits, src, frames)
    packed = _encode_device(enc, src, frames, "packed")
    assert np.array_equal(packed, np.packbits(bits, axis=1, bitorder="little"))
    enc.close()


def test_gallager_matrix_with_redundant_rows(mats):
    torch = _torch()
    m, frames = mats["G"], 70
    K, N = m["K"], m["N"]
    assert N - K < m["M"] and N % 8 == 4
    src = np.random.default_rng(2).integers(0, 256, stream_length(K, frames), dtype=np.uint8)
    enc = L.DenseEncoder(L.Graph(m["rows"], m["cols"], m["M"], N), K, max_frames=128)
    _check_codewords(m, _encode_device(enc, src, frames, "bits"), src, frames)
    sd = torch.from_numpy(src).cuda()
    code = torch.full((frames * N,), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(L.LdpcError) as e:
        enc.encode_device(sd.data_ptr(), src.size, frames, code.data_ptr(), code.numel(), "packed")
    assert e.value.code == 1
    with pytest.raises(L.LdpcError) as e:
        enc.encode(src)
    assert e.value.code == 1
    torch.cuda.synchronize()
    assert bool((code == 0xEE).all())
    enc.close()


def test_swapped_wimax_equals_gaussian_elimination(built):
    rows, cols, M, N = U.matrix_w648s()
    K, frames = N - M, 130
    src = np.random.default_rng(3).integers(0, 256, stream_length(K, frames, cut=5), dtype=np.uint8)
    want = reference_packed(Gf2Encoder(rows, cols, M, N), src, frames)
    g = L.Graph(rows, cols, M, N)
    with pytest.raises(L.LdpcError) as e:
        L.Encoder(g, K, 27)
    assert e.value.code == 4
    enc = L.DenseEncoder(g, K, max_frames=256)
    assert np.array_equal(_encode_device(enc, src, frames, "packed"), want)
    assert np.array_equal(_encode_device(enc, src, frames, "bits"), np.unpackbits(want, axis=1, bitorder="little"))
    assert np.array_equal(enc.encode(src).reshape(frames, -1), want)
    enc.close()


def test_wimax_2304_dense_equals_structured(built):
    """The same H through two independent solvers: T of the elimination against the dual-diagonal substitution."""
    K, M, z = codes.wimax_dims(codes.RATE_1_2, 2304)
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 2304)
    g, frames = L.Graph(rows, cols, M, 2304), 130
    src = np.random.default_rng(4).integers(0, 256, stream_length(K, frames), dtype=np.uint8)
    dense, structured = L.DenseEncoder(g, K, max_frames=192), L.Encoder(g, K, z, max_frames=192)
    assert dense.structure()["t_words"] == 18
    for fmt in ("bits", "packed"):
        a, b = _encode_device(dense, src, frames, fmt), _encode_device(structured, src, frames, fmt)
        assert a[:, -8:].any()
        assert np.array_equal(a, b), fmt
    dense.close()
    structured.close()


def test_host_buffers_in_chunks(mats):
    m, frames = mats["R"], 150
    src = np.random.default_rng(5).integers(0, 256, stream_length(m["K"], frames), dtype=np.uint8)
    g = L.Graph(m["rows"], m["cols"], m["M"], m["N"])
    whole = L.DenseEncoder(g, m["K"], max_frames=256)
    one_call = _encode_device(whole, src, frames, "packed")
    whole.close()
    small = L.DenseEncoder(g, m["K"], max_frames=64)        # three chunks, the last one of 22 frames
    got = small.encode(src)
    small.close()
    assert np.array_equal(got.reshape(frames, -1), one_call)
    _check_codewords(m, np.unpackbits(one_call, axis=1, bitorder="little"), src, frames)


def test_offset_buffers_and_frame_limit(mats):
    torch = _torch()
    m, frames = mats["R"], 128
    K, N = m["K"], m["N"]
    src = np.random.default_rng(6).integers(0, 256, stream_length(K, frames + 1), dtype=np.uint8)
    enc = L.DenseEncoder(L.Graph(m["rows"], m["cols"], m["M"], N), K, max_frames=frames)
    want = _encode_device(enc, src[:stream_length(K, frames)], frames, "bits")
    sd = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), src])).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for fmt, per, ref in (("bits", N, want), ("packed", N // 8, np.packbits(want, axis=1, bitorder="little"))):
        code = torch.full((64 + 1 + frames * per + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        enc.encode_device(sd.data_ptr() + 3, stream_length(K, frames), frames, code.data_ptr() + 65, frames * per, fmt, stream)
        torch.cuda.synchronize()
        host = code.cpu().numpy()
        assert (host[:65] == 0xEE).all() and (host[65 + frames * per:] == 0xEE).all(), fmt
        assert np.array_equal(host[65:65 + frames * per].reshape(frames, per), ref), fmt
    code = torch.full(((frames + 1) * N,), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(L.LdpcError) as e:
        enc.encode_device(sd.data_ptr() + 3, src.size, frames + 1, code.data_ptr(), code.numel(), "bits", stream)
    assert e.value.code == 1
    torch.cuda.synchronize()
    assert bool((code == 0xEE).all())
    enc.close()


def test_closed_loop_in_device_memory(mats):
    """DenseEncoder -> ldpc_awgn_device -> min-sum -> count, all in HBM: no bit error at sd = 0.3 (10.5 dB), the noise and
    seed at which the oracle's min-sum alone returns the payload (checked below, on the same channel values)."""
    torch = _torch()
    m, frames, sd, seed = mats["R"], 64, 0.3, 4242
    K, N, M = m["K"], m["N"], m["M"]
    rng = np.random.default_rng(21)
    src_host = np.zeros(stream_length(K, frames), np.uint8)         # the bytes between frames (K % 8 = 4) stay zero
    for at in frame_starts(K, frames):
        src_host[at:at + K // 8] = rng.integers(0, 256, K // 8, dtype=np.uint8)
    assert src_host.any()
    src = torch.from_numpy(src_host).cuda()
    g = L.Graph(m["rows"], m["cols"], M, N)
    enc = L.DenseEncoder(g, K, max_frames=frames)
    code = torch.empty((frames, N), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    enc.encode_device(src.data_ptr(), src.numel(), frames, code.data_ptr(), code.numel(), "bits", stream)
    y = channel.awgn_device(N, 0, frames, sd, seed=seed, codewords=code)
    dec = L.Decoder(g, K, max_batch=frames, algo="ms", max_iter=20, layer_rows=0)
    out = torch.zeros(L.out_bytes(K, frames), dtype=torch.uint8, device="cuda")
    assert out.numel() == src.numel()
    dec.decode_device(y.data_ptr(), frames, out.data_ptr(), out.numel(), None, stream)
    got = channel.count_errors_device(out, src, 1)
    bits = code.cpu().numpy()
    _check_codewords(m, bits, src_host, frames)
    ref = oracle.decode(oracle.Graph(m["rows"], m["cols"], M, N, K), oracle.awgn(N, 0, frames, sd, seed=seed, codewords=bits), "ms",
                        max_iter=20, layer_rows=0)["out"]
    assert np.array_equal(ref, src_host), "the oracle's min-sum does not return the payload at this sd and seed"
    print("closed loop on R': (bit, byte, frame) errors", got)
    assert got[0] == 0
    assert np.array_equal(out.cpu().numpy(), src_host)
    dec.close()
    enc.close()
