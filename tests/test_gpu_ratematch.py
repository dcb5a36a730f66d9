"""Rate matching on the GPU (ldpc_rate_match_device / ldpc_rate_recover_device and their host-buffer forms) against
ratematch_ref: bits and packed formats byte for byte, recovered sums and decoder inputs as uint32 bit patterns, guard
regions behind every output, the closed chain encoder -> match -> channel -> recover -> decoder against the oracle, and
element offsets beyond 2^31."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes

import ratematch_ref as ref
import ratematch_util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def _torch():
    import torch
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _match_device(rm, code_bits, k0, E, code_fmt, tx_fmt, shift=0):
    """code_bits uint8 [frames, N] -> tx as the device writes it, uint8 [frames, E or E/8]; 64 guard bytes behind (and
    `shift` in front of) the output must survive."""
    torch = _torch()
    frames = code_bits.shape[0]
    src = code_bits if code_fmt == "bits" else np.packbits(code_bits, axis=1, bitorder="little")
    cd = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    per = E if tx_fmt == "bits" else E // 8
    tx = torch.full((shift + frames * per + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    rm.match_device(cd.data_ptr(), frames, k0, E, tx.data_ptr() + shift, frames * per, code_fmt, tx_fmt, _stream())
    torch.cuda.synchronize()
    host = tx.cpu().numpy()
    assert (host[:shift] == 0xEE).all() and (host[shift + frames * per:] == 0xEE).all(), "wrote outside the tx buffer"
    return host[shift:shift + frames * per].reshape(frames, per)


@pytest.mark.parametrize("frames", [1, 65])
def test_match_equals_the_reference_over_the_grid(built, frames):
    rng = np.random.default_rng(20 + frames)
    code = rng.integers(0, 2, (frames, U.N_GRID), dtype=np.uint8)
    for spec, k0, E in U.grid_cases():
        rm = L.RateMatcher(**spec.kwargs())
        want = ref.match(spec, code, k0, E)
        for code_fmt in ("bits", "packed"):
            got = _match_device(rm, code, k0, E, code_fmt, "bits")
            assert np.array_equal(got, want), (spec.P, spec.lo, spec.hi, k0, E, code_fmt)
            if E % 8 == 0:
                got = _match_device(rm, code, k0, E, code_fmt, "packed")
                assert np.array_equal(got, np.packbits(want, axis=1, bitorder="little")), (spec.P, spec.lo, spec.hi, k0, E, code_fmt)


def test_match_packed_output_and_odd_sizes(built):
    """Packed tx needs E % 8 == 0, which the grid rarely has: E in {8, 616, 1032, 2072} here; then N = 1001 with
    E = 37 (bits only: neither is a multiple of 8), rows of tx that start at every byte alignment."""
    rng = np.random.default_rng(31)
    code = rng.integers(0, 2, (65, U.N_GRID), dtype=np.uint8)
    spec = ref.Spec(U.N_GRID, 32, (328, 352))
    rm = L.RateMatcher(**spec.kwargs())
    for k0, E in ((0, 8), (0, 616), (300, 1032), (1055, 2072)):
        want = np.packbits(ref.match(spec, code, k0, E), axis=1, bitorder="little")
        for code_fmt in ("bits", "packed"):
            assert np.array_equal(_match_device(rm, code, k0, E, code_fmt, "packed"), want), (k0, E, code_fmt)
        assert np.array_equal(rm.match(code, k0, E, "bits", "packed"), want)                   # host buffers
    odd = ref.Spec(1001, 5, (100, 117))
    rmo = L.RateMatcher(**odd.kwargs())
    code = rng.integers(0, 2, (65, 1001), dtype=np.uint8)
    for k0, E in ((0, 37), (990, 37), (96, 2000)):
        want = ref.match(odd, code, k0, E)
        for shift in (0, 1, 2, 3):
            assert np.array_equal(_match_device(rmo, code, k0, E, "bits", "bits", shift), want), (k0, E, shift)
        assert np.array_equal(rmo.match(code, k0, E), want)
    with pytest.raises(L.LdpcError) as e:
        rmo.match_device(1 << 20, 1, 0, 40, 1 << 21, 1 << 20, "packed", "bits")               # N % 8 != 0
    assert e.value.code == 1


def _recover_device(rm, rx, k0, E, soft=None, want_soft=True, want_y=True):
    """rx float32 [frames, E] -> (soft, y) as the device writes them; outputs pre-filled with NaN, guard floats behind."""
    torch = _torch()
    frames, N = rx.shape[0], rm.N
    rd = torch.from_numpy(np.ascontiguousarray(rx)).cuda()
    bufs = []
    for want, init in ((want_soft, soft), (want_y, None)):
        if not want:
            bufs.append(None)
            continue
        b = torch.full((frames * N + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        if init is not None:
            b[:frames * N] = torch.from_numpy(np.ascontiguousarray(init).reshape(-1)).cuda()
        bufs.append(b)
    sb, yb = bufs
    rm.recover_device(rd.data_ptr(), frames, k0, E, None if sb is None else sb.data_ptr(), soft is not None,
                      None if yb is None else yb.data_ptr(), _stream())
    torch.cuda.synchronize()
    out = []
    for b in bufs:
        if b is None:
            out.append(None)
            continue
        h = b.cpu().numpy()
        assert np.isnan(h[frames * N:]).all(), "wrote behind the end of an output"
        out.append(h[:frames * N].reshape(frames, N))
    return out


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


RECOVER_CASES = [  # (P, filler, k0, E): E % 4 in {1, 2, 3}, wrap-around, E = 3L + 7, E < 64
    (32, (328, 352), 0, 1032), (32, (328, 352), 0, 617), (32, (328, 352), 100, 1030), (32, (328, 352), 1000, 1031),
    (32, (328, 352), 300, 3 * 1032 + 7), (32, (328, 352), 1055, 37), (0, (0, 0), 5, 63), (0, (0, 8), 0, 1080 * 2 + 5),
    (32, (32, 40), 3, 1), (0, (0, 0), 1087, 1088)]


@pytest.mark.parametrize("eps", [0.0, 1e-6])
def test_recover_equals_the_reference_bit_for_bit(built, eps):
    rng = np.random.default_rng(41)
    for frames in (1, 65):
        for P, filler, k0, E in RECOVER_CASES:
            spec = ref.Spec(U.N_GRID, P, filler, 10.0, eps)
            rm = L.RateMatcher(**spec.kwargs())
            rx = rng.standard_normal((frames, E)).astype(np.float32)
            rx[:, ::7] = 0.0                     # received zeros are erasures too
            rx[0, 1::11] = -0.0
            ws, wy = ref.recover(spec, rx, k0, E)
            s, y = _recover_device(rm, rx, k0, E)
            assert _same(s, ws) and _same(y, wy), (P, filler, k0, E, frames)
            if frames == 65:
                s, y = _recover_device(rm, rx, k0, E, want_y=False)
                assert y is None and _same(s, ws)
                s, y = _recover_device(rm, rx, k0, E, want_soft=False)
                assert s is None and _same(y, wy)
                hs, hy = rm.recover(rx, k0, E)                                             # host buffers
                assert _same(hs, ws) and _same(hy, wy)


def test_recover_with_an_odd_code_length(built):
    rng = np.random.default_rng(42)
    spec = ref.Spec(1001, 5, (100, 117), 7.5, 1e-6)
    rm = L.RateMatcher(**spec.kwargs())
    for k0, E in ((0, 37), (990, 37), (96, 2000)):
        rx = rng.standard_normal((65, E)).astype(np.float32)
        ws, wy = ref.recover(spec, rx, k0, E)
        s, y = _recover_device(rm, rx, k0, E)
        assert _same(s, ws) and _same(y, wy), (k0, E)


def test_three_accumulated_transmissions(built):
    rng = np.random.default_rng(43)
    spec = ref.Spec(U.N_GRID, 32, (328, 352), 10.0, 1e-6)
    rm = L.RateMatcher(**spec.kwargs())
    frames = 65
    soft = want = None
    hsoft = None
    for k0, E in ((0, 464), (488, 470), (900, 1301)):
        rx = rng.standard_normal((frames, E)).astype(np.float32)
        want, wy = ref.recover(spec, rx, k0, E, want)
        soft, y = _recover_device(rm, rx, k0, E, soft=soft if soft is not None else np.zeros((frames, U.N_GRID), np.float32))
        assert _same(soft, want) and _same(y, wy), (k0, E)
        if hsoft is None:
            hsoft, hy = rm.recover(rx, k0, E)
        else:
            _, hy = rm.recover(rx, k0, E, soft=hsoft)
        assert _same(hsoft, want) and _same(hy, wy), (k0, E)


def test_accumulate_off_ignores_what_soft_held(built):
    torch = _torch()
    spec = ref.Spec(U.N_GRID, 32, (328, 352), 10.0, 0.0)
    rm = L.RateMatcher(**spec.kwargs())
    rx = np.random.default_rng(44).standard_normal((3, 500)).astype(np.float32)
    ws, _ = ref.recover(spec, rx, 7, 500)
    rd = torch.from_numpy(rx).cuda()
    soft = torch.full((3 * U.N_GRID,), 123.0, dtype=torch.float32, device="cuda")
    rm.recover_device(rd.data_ptr(), 3, 7, 500, soft.data_ptr(), False, None, _stream())
    torch.cuda.synchronize()
    assert _same(soft.cpu().numpy().reshape(3, -1), ws)


def test_aliased_soft_and_y_are_refused(built):
    torch = _torch()
    rm = L.RateMatcher(U.N_GRID, punctured=32)
    rx = torch.zeros(4 * 100, dtype=torch.float32, device="cuda")
    buf = torch.full((8 * U.N_GRID,), 5.0, dtype=torch.float32, device="cuda")
    for off in (0, 4, 4 * (4 * U.N_GRID - 1)):
        with pytest.raises(L.LdpcError) as e:
            rm.recover_device(rx.data_ptr(), 4, 0, 100, buf.data_ptr(), False, buf.data_ptr() + off, _stream())
        assert e.value.code == 1 and "alias" in str(e.value)
    torch.cuda.synchronize()
    assert bool((buf == 5.0).all())
    rm.recover_device(rx.data_ptr(), 4, 0, 100, buf.data_ptr(), False, buf.data_ptr() + 4 * 4 * U.N_GRID, _stream())   # adjacent: fine
    torch.cuda.synchronize()


# ---- the chain in device memory against the oracle ---------------------------------------------------------------

def _chain(name, eps, transmissions, algo):
    """Encoder -> match -> ldpc_awgn_device(N = E) -> recover (through `soft`) -> Decoder on device buffers.
    Returns (decoded bytes, iterations, y) as numpy arrays."""
    torch = _torch()
    rows, cols, _ = U.bg1()
    info, src_bytes, code_want = U.payload()
    g = L.Graph(rows, cols, U.M, U.N)
    enc = L.Encoder(g, U.K, U.Z, max_frames=U.FRAMES)
    src = torch.from_numpy(np.array(src_bytes)).cuda()
    code = torch.empty((U.FRAMES, U.N), dtype=torch.uint8, device="cuda")
    enc.encode_device(src.data_ptr(), src.numel(), U.FRAMES, code.data_ptr(), code.numel(), "bits", _stream())
    rm = L.RateMatcher(**U.scenario_spec(eps).kwargs())
    soft = torch.full((U.FRAMES, U.N), float("nan"), dtype=torch.float32, device="cuda")
    y = torch.full((U.FRAMES, U.N), float("nan"), dtype=torch.float32, device="cuda")
    (txs, sd) = U.received(name)
    for t, (k0, E, tx_want, rx_want) in enumerate(txs[:transmissions]):
        tx = torch.empty((U.FRAMES, E), dtype=torch.uint8, device="cuda")
        rm.match_device(code.data_ptr(), U.FRAMES, k0, E, tx.data_ptr(), tx.numel(), "bits", "bits", _stream())
        rx = channel.awgn_device(E, 0, U.FRAMES, sd, seed=100 + t, codewords=tx)
        rm.recover_device(rx.data_ptr(), U.FRAMES, k0, E, soft.data_ptr(), t > 0, y.data_ptr(), _stream())
        assert np.array_equal(tx.cpu().numpy(), tx_want)
        assert _same(rx.cpu().numpy(), rx_want)
    assert np.array_equal(code.cpu().numpy(), code_want)
    dec = L.Decoder(g, U.K, max_batch=U.FRAMES, algo=algo, max_iter=U.MAX_ITER, llr_scale=U.LLR_SCALE, layer_rows=U.Z)
    out = torch.zeros(L.out_bytes(U.K, U.FRAMES), dtype=torch.uint8, device="cuda")
    iters = torch.zeros(U.FRAMES, dtype=torch.int32, device="cuda")
    dec.decode_device(y.data_ptr(), U.FRAMES, out.data_ptr(), out.numel(), iters.data_ptr(), _stream())
    torch.cuda.synchronize()
    res = out.cpu().numpy(), iters.cpu().numpy(), y.cpu().numpy()
    dec.close()
    enc.close()
    return res


@pytest.mark.parametrize("algo", ["layered", "ms", "sp"])
@pytest.mark.parametrize("name,transmissions", [("S1", 1), ("S4", 1), ("S4", 2)])
def test_chain_equals_the_oracle(built, name, transmissions, algo):
    eps = 1e-6
    out, iters, y = _chain(name, eps, transmissions, algo)
    assert _same(y, U.recovered(name, eps, transmissions))
    want_out, want_iters, wrong = U.oracle_decode(name, eps, transmissions, algo)
    print("%s x%d %s: oracle frames wrong %d / %d, mean iterations %.2f" % (name, transmissions, algo, wrong, U.FRAMES,
                                                                             float(np.mean(want_iters))))
    if algo in ("layered", "ms"):           # the equality below is not vacuous: the oracle decodes (or, tx1 alone, cannot)
        assert wrong == (U.FRAMES if (name, transmissions) == ("S4", 1) else 0)
    assert np.array_equal(out, want_out) and np.array_equal(iters, want_iters)


def test_chain_layered_with_exact_erasures_fails_as_the_oracle_does(built):
    """erasure_llr = 0: the documented behaviour -- layered fails every frame, and it fails exactly as the oracle."""
    out, iters, y = _chain("S1", 0.0, 1, "layered")
    assert _same(y, U.recovered("S1", 0.0, 1))
    want_out, want_iters, wrong = U.oracle_decode("S1", 0.0, 1, "layered")
    assert wrong == U.FRAMES
    assert np.array_equal(out, want_out) and np.array_equal(iters, want_iters)


def test_element_offsets_beyond_2_31(built):
    """frames x N = 33200 x 64800 > 2^31 floats; E = 64808 wraps once (eight code bits are received twice)."""
    torch = _torch()
    N, frames, E, k0, sd = 64800, 33200, 64808, 0, 0.5
    assert frames * N > 2 ** 31 and frames * E > 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of free device memory, %.1f GB are free" % (free / 2 ** 30))
    spec = ref.Spec(N, 0, (0, 0), 10.0, 1e-6)
    rm = L.RateMatcher(**spec.kwargs())
    rx = channel.awgn_device(E, 0, frames, sd, seed=77)
    y = torch.full((frames * N + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    rm.recover_device(rx.data_ptr(), frames, k0, E, None, False, y.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[frames * N:]).all())
    for f in (0, 16600, 33199):
        want = ref.recover(spec, oracle.awgn(E, f, 1, sd, seed=77), k0, E)[1]
        assert _same(y[f * N:(f + 1) * N].cpu().numpy().reshape(1, N), want), f
    del rx, y
    torch.cuda.empty_cache()


def test_coder_with_rate_matching(built, tmp_path):
    """tests/cpp/coder_ratematch.cpp: Coder(1152, 2304, rate_1_2) with setRateMatch(E = 1920, k0 = 0): lengths, and
    encode -> test(sd = 0.3) -> decode(DecodeMS) returns the source bytes; a second Coder without the setter reports
    the lengths of the mother code."""
    exe = str(tmp_path / "coder_ratematch")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "coder_ratematch.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "myldpccppapi_amd"), "-lmyldpc", "-lldpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myldpccppapi_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "lengths=ok plain=ok ErrNum=0" in out.stdout, out.stdout
