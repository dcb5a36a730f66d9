"""Host logic and the C ABI surface without a GPU: the library loads, exports every
symbol include/ldpc_hip.h declares, validates its arguments, and -- on a box
without a HIP device -- refuses to decode instead of falling back to a CPU path."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, channel, codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(built):
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    declared = set(re.findall(r"\b(ldpc_[a-z_]+)\s*\(", header))
    declared -= {"ldpc_graph", "ldpc_decoder"}
    assert declared == set(_lib.EXPORTS)
    for s in declared:
        assert hasattr(lib, s), s
    assert lib.ldpc_abi_version() == 3


def test_c_abi_header_compiles_and_links_as_plain_c(built, tmp_path):
    """include/ldpc_hip.h is a C header: a C99 program includes it, links libldpc_hip.so and uses the
    host-only entry points (graph, config defaults, shard arithmetic, error text)."""
    exe = str(tmp_path / "cabi_smoke")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "cabi_smoke.c"), "-o", exe,
                           "-L" + os.path.join(ROOT, "myldpccppapi_amd"), "-lldpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myldpccppapi_amd")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "cabi ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


def test_cpp_class_library_exports_the_reference_api(built):
    """include/MyLdpc.h: every public method of the reference's `Coder` (MyLdpc.h:107-126) and the
    free function gaussian() are defined in libmyldpc.so."""
    so = os.path.join(ROOT, "myldpccppapi_amd", "libmyldpc.so")
    syms = subprocess.run("nm -D --defined-only %s | c++filt" % so, shell=True, capture_output=True, text=True).stdout
    for want in ("Coder::Coder(int, int, rate_type)", "Coder::~Coder()", "Coder::forEncoder()", "Coder::forDecoder(int)",
                 "Coder::addDecodeType(decodeType)", "Coder::encode(char*, char*, int)",
                 "Coder::decode(float*, char*, int, decodeType)", "Coder::test(char*, float*, int, float)",
                 "Coder::getPriorCodeLength(int)", "Coder::getPostCodeLength(int)", "Coder::getCodeSize(int)",
                 "gaussian(float, float)"):
        assert want in syms, want


def test_out_bytes_follows_tochar_and_decodecpu(built):
    assert L.out_bytes(432, 8) == 8 * 54
    # K % 8 != 0: frame b starts at (b*K)/8, each frame writes K/8 whole bytes (decodeCL.c:191-192)
    assert L.out_bytes(324, 9) == (8 * 324) // 8 + 40
    assert L.out_bytes(324, 9, L.PACK_BITS) == (9 * 324 + 7) // 8
    assert L.out_bytes(324, 0) == 0


def test_graph_validation(built):
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 648)
    g = L.Graph(rows, cols, 324, 648)
    info = g.info()
    assert info == dict(M=324, N=648, E=2052, max_row_deg=7, max_col_deg=6)
    with pytest.raises(L.LdpcError) as e:
        L.Graph(rows[::-1].copy(), cols[::-1].copy(), 324, 648)      # not row-major
    assert e.value.code == 1 and "row-major" in str(e.value)
    with pytest.raises(L.LdpcError):
        L.Graph(rows, cols, 100, 648)                                  # row out of range
    with pytest.raises(L.LdpcError):
        L.Graph(np.r_[rows, rows[-1]], np.r_[cols, cols[-1]], 324, 648)  # duplicate edge


def test_config_defaults_are_the_references(built):
    cfg = _lib.DecoderConfig()
    _lib.load().ldpc_decoder_config_init(ctypes.byref(cfg))
    assert cfg.struct_size == ctypes.sizeof(_lib.DecoderConfig)
    assert cfg.max_iter == 40            # MyLdpc.cpp:24
    assert cfg.llr_scale == 8.0          # decodeCL.c:9
    assert cfg.early_term == 1 and cfg.algo == L.ALGO_SP and cfg.pack_mode == L.PACK_BYTES


def test_no_cpu_fallback_without_a_device(built):
    if L.device_count() > 0:
        pytest.skip("a HIP device is present")
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 648)
    g = L.Graph(rows, cols, 324, 648)
    with pytest.raises(L.LdpcError) as e:
        L.Decoder(g, 324, 8, algo="ms")
    assert e.value.code == 2             # LDPC_ERR_HIP: no silent CPU path


def test_bad_config_is_rejected_before_touching_the_device(built):
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 648)
    g = L.Graph(rows, cols, 324, 648)
    for kw in (dict(K=0), dict(max_batch=0), dict(max_iter=0), dict(algo=7), dict(frames_per_lane=3),
               dict(pack_mode=5)):
        args = dict(K=324, max_batch=4, algo="ms", max_iter=40)
        args.update(kw)
        with pytest.raises(L.LdpcError) as e:
            L.Decoder(g, args.pop("K"), args.pop("max_batch"), **args)
        assert e.value.code == 1, kw


def test_host_layered_algo_is_refused_where_the_reference_is_wrong(built):
    """LDPC_ALGO_LAYERED_HOST exists only for H whose rows all have one weight: elsewhere the
    reference's host-layered path mis-sizes its layers (MyLdpc.cpp:907,958).  Refused with
    LDPC_ERR_UNSUPPORTED before the device is touched."""
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 576)
    g = L.Graph(rows, cols, 288, 576)
    with pytest.raises(L.LdpcError) as e:
        L.Decoder(g, 288, 4, algo="layered_host", layer_rows=24)
    assert e.value.code == 4 and "same weight" in str(e.value)


def test_tuning_fields_are_validated_and_no_environment_is_read(built):
    """The tuning knobs live in the config (two-bit fields + integers); out-of-range values are
    argument errors before the device is touched, and the library never calls getenv."""
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 648)
    g = L.Graph(rows, cols, 324, 648)
    lib = _lib.load()
    for field, value in (("tune_flags", 3), ("tune_flags", 1 << 30), ("tune_rows_per_wave", -1), ("tune_link_rows", -2),
                         ("tune_compact", -2), ("tune_ldsp_shape", 1 << 16), ("host_input", 3), ("host_input", -1),
                         ("host_copy_threads", 17), ("host_copy_threads", -1),
                         ("tune_q_order", 2), ("tune_q_order", -2)):
        cfg = _lib.DecoderConfig()
        lib.ldpc_decoder_config_init(ctypes.byref(cfg))
        cfg.K, cfg.max_batch = 324, 4
        setattr(cfg, field, value)
        h = ctypes.c_void_p()
        assert lib.ldpc_decoder_create(g._h, ctypes.byref(cfg), ctypes.byref(h)) == 1, field
    cfg = _lib.DecoderConfig()
    L.capi.apply_tune(cfg, {"fused": True, "ldsp": False, "link_rows": -1, "compact": 64, "ldsp_per_cu": 2, "ldsp_waves": 3})
    assert cfg.tune_flags == (1 << 0) | (2 << 2) and cfg.tune_link_rows == -1 and cfg.tune_compact == 64
    assert cfg.tune_ldsp_shape == 2 | (3 << 8)
    with pytest.raises(KeyError):
        L.capi.apply_tune(cfg, {"no_such_knob": 1})
    assert L.capi.tune_from_env({"LDPC_TUNE_FUSED": "0", "LDPC_TUNE_LINK_RPW": "0", "LDPC_TUNE_COMPACT": "9"}) == \
        {"fused": False, "link_rows": -1, "compact": 9}
    out = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "getenv" not in out


def test_shard_ranges_of_the_c_abi(built):
    """ldpc_shard_range: contiguous, balanced, boundaries on multiples of the unit; unit 1 is the
    arithmetic the benchmark's rank sharding uses (sharding.shard_range)."""
    from myldpccppapi_amd import sharding
    for total in (0, 1, 5, 8, 700, 4096, 4099):
        for parts in (1, 2, 3, 8):
            r = [L.shard_range(total, k, parts) for k in range(parts)]
            assert r == [sharding.shard_range(total, k, parts) for k in range(parts)]
            for unit in (2, 8, 64):
                r = [L.shard_range(total, k, parts, unit) for k in range(parts)]
                assert r[0][0] == 0 and r[-1][1] == total
                assert all(r[i][1] == r[i + 1][0] for i in range(parts - 1))
                assert all(lo % unit == 0 or lo == total for lo, _ in r)
                assert max(b - a for a, b in r) - min(b - a for a, b in r) < 2 * unit       # balanced in units
    with pytest.raises(L.LdpcError):
        L.shard_range(10, 2, 2)


def test_multi_device_handle_validates_its_list(built):
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 648)
    g = L.Graph(rows, cols, 324, 648)
    with pytest.raises(L.LdpcError) as e:
        L.Decoder(g, 324, 8, algo="ms", devices=[])
    assert e.value.code == 1
    if L.device_count() == 0:
        with pytest.raises(L.LdpcError) as e:
            L.Decoder(g, 324, 8, algo="ms", devices=[0, 0])
        assert e.value.code == 2         # LDPC_ERR_HIP: no device, no CPU path


def test_bench_multi_gpu_form_starts_its_own_ranks(built):
    """`python bench.py --gpus 2` invoked plainly launches torch.distributed.run itself (round 1: it
    exited 1 asking for a launcher).  Without a GPU the ranks fail -- loudly and with the children's
    status -- but they must have been started, and the parent must not touch the GPU itself."""
    if L.device_count() > 0:
        pytest.skip("GPU box: the positive form of this test is in test_gpu_multi.py")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([os.sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--backend", "gloo", "--no-cpu-baseline", "--no-extras"], capture_output=True, text=True,
                       env=env, timeout=600)
    assert p.returncode != 0
    assert "must be launched with" not in p.stderr + p.stdout
    assert "torch.distributed" in p.stderr or "ChildFailedError" in p.stderr or "local_rank" in p.stderr


def test_bench_dump_outputs_is_a_fixed_sample_within_64_mb(tmp_path):
    """bench.py --dump-outputs: the headline batch (4096 frames of K/8 = 4050 bytes) is cut to the same seeded
    sample of whole frames in every run, float32 / float64 files of at most 64 MB in all; a small batch is
    written whole."""
    import torch
    import bench
    out = torch.randint(0, 256, (4096 * 4050,), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, 4096)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["decoded_bytes.npy", "frame_index.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10 ** 6
    got, idx = np.load(tmp_path / "a" / "decoded_bytes.npy"), np.load(tmp_path / "a" / "frame_index.npy")
    assert got.dtype == np.float32 and idx.dtype == np.float64 and len(idx) > 2048
    assert np.array_equal(idx, np.unique(idx)) and idx[-1] < 4096
    assert np.array_equal(got, out.numpy().reshape(4096, 4050)[idx.astype(np.int64)].astype(np.float32))
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    bench.dump_outputs(str(tmp_path / "c"), out[:256 * 4050], 256)
    assert np.array_equal(np.load(tmp_path / "c" / "frame_index.npy"), np.arange(256))
    assert np.array_equal(np.load(tmp_path / "c" / "decoded_bytes.npy"), out[:256 * 4050].numpy().reshape(256, 4050))


# ---------------------------------------------------------------- host-side data

@pytest.mark.parametrize("rate", range(6))
def test_wimax_edges_three_ways(rate):
    """numpy builder == oracle C builder (== the C++ Coder, checked in test_cpp_coder)."""
    for N in (576, 960, 2304):
        r, c = codes.wimax_edges(rate, N)
        ro, co = oracle.wimax_edges(rate, N)
        assert np.array_equal(r, ro) and np.array_equal(c, co)
        K, M, z = codes.wimax_dims(rate, N)
        assert r.max() == M - 1 and c.max() == N - 1


def test_dvbs2_profile_structure():
    r, c = codes.dvbs2_profile_edges(64800, 32400)
    assert len(r) == 226799                       # E of the rate-1/2 code
    rd, cd = np.bincount(r), np.bincount(c)
    assert rd[0] == 6 and np.all(rd[1:] == 7)     # check degree 7, first row 6
    assert np.all(cd[:12960] == 8) and np.all(cd[12960:32400] == 3)
    assert np.all(cd[32400:-1] == 2) and cd[-1] == 1
    r2, c2 = codes.dvbs2_profile_edges(64800, 32400)
    assert np.array_equal(r, r2) and np.array_equal(c, c2)   # seeded: reproducible
    r9, c9 = codes.dvbs2_profile_edges(64800, 58320)
    assert len(r9) == 194399 and np.bincount(r9)[1:].max() == 30


def test_bg1_profile_layers_are_column_disjoint():
    Z = 48
    r, c = codes.nr_bg1_profile_edges(Z)
    assert len(r) == 316 * Z
    for layer in range(46):
        cs = c[(r >= layer * Z) & (r < (layer + 1) * Z)]
        assert len(np.unique(cs)) == len(cs)


def test_alist_round_trip(tmp_path):
    rows, cols = codes.wimax_edges(codes.RATE_2_3_A, 672)
    K, M, z = codes.wimax_dims(codes.RATE_2_3_A, 672)
    p = str(tmp_path / "h.alist")
    codes.save_alist(p, rows, cols, M, 672)
    r2, c2, M2, N2 = codes.load_alist(p)
    assert (M2, N2) == (M, 672) and np.array_equal(r2, rows) and np.array_equal(c2, cols)


def test_channel_is_counter_based():
    a = channel.awgn_frames(648, 0, 6, 0.8, seed=5)
    b = channel.awgn_frames(648, 4, 2, 0.8, seed=5)
    assert np.array_equal(a[4:], b)
    assert abs(channel.snr_db_to_sd(3.0) - 0.7079458) < 1e-6        # Test.cpp:56


def test_shared_expf_matches_libm_on_a_sample(tmp_path):
    """ldpc_expf (used by the SP init kernel) against the host libm the oracle uses.
    tools/check_expf.c does all 2^32 inputs; here 4M samples + edge cases."""
    src = tmp_path / "e.c"
    src.write_text('#include "%s/myldpccppapi_amd/csrc/ldpc_expf.h"\n'
                   'void run(const float*x,float*y,long n){for(long i=0;i<n;++i)y[i]=ldpc_expf(x[i]);}\n' % ROOT)
    so = tmp_path / "e.so"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so), "-lm"])
    lib = ctypes.CDLL(str(so))
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-110, 95, 2_000_000), 8 * (1 + rng.standard_normal(2_000_000)),
                        [0.0, -0.0, 88.72, 88.73, -103.9, -104.0, np.inf, -np.inf, 1e-30,
                         float.fromhex("0x1.04845ep+5"), float.fromhex("-0x1.f8cbb2p+5")]]).astype(np.float32)
    y = np.empty_like(x)
    lib.run(x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(x.size))
    libm = ctypes.CDLL("libm.so.6")
    libm.expf.restype = ctypes.c_float
    libm.expf.argtypes = [ctypes.c_float]
    idx = np.r_[rng.integers(0, x.size, 200_000), np.arange(x.size - 11, x.size)]
    want = np.array([libm.expf(float(v)) for v in x[idx]], np.float32)
    assert np.array_equal(y[idx].view(np.uint32), want.view(np.uint32))


def test_shared_expf_equals_libm_on_every_float(tmp_path):
    """tools/check_expf.c: ldpc_expf (csrc/ldpc_expf.h, the exp of the sum-product kernels, identical
    on host and device) against the host libm's expf -- the oracle's exp -- on all 2^32 float bit
    patterns.  0 mismatches (NaN results compared as NaN)."""
    exe = str(tmp_path / "check_expf")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-pthread", os.path.join(ROOT, "tools", "check_expf.c"),
                           "-lm", "-o", exe])
    out = subprocess.run([exe, str(min(8, os.cpu_count() or 1))], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "mismatches=0" in out.stdout, out.stdout


def test_counter_based_channel_generator(tmp_path):
    """csrc/ldpc_channel.h on the host: Philox4x32-10 against the Random123 known-answer vectors,
    and the normals it feeds (own log / sqrt / sin / cos in IEEE double) against N(0, 1)."""
    from scipy import stats
    from util import host_channel_lib
    lib = host_channel_lib(tmp_path)
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        c = (ctypes.c_uint32 * 4)(*ctr)
        lib.philox(c, ctypes.c_uint32(key[0]), ctypes.c_uint32(key[1]))
        assert tuple(c) == want
    n = 1 << 19
    z = np.empty(4 * n)
    lib.normals(20260101, 3, n, z.ctypes.data_as(ctypes.c_void_p))
    assert abs(z.mean()) < 4 / np.sqrt(z.size) and abs(z.var() - 1) < 6 * np.sqrt(2 / z.size)
    assert abs(stats.skew(z)) < 0.01 and abs(stats.kurtosis(z)) < 0.02
    assert stats.kstest(z[:300000], "norm").pvalue > 1e-3
    assert abs((np.abs(z) > 3).mean() / (2 * stats.norm.sf(3)) - 1) < 0.1
    assert abs(np.corrcoef(z[0::4], z[1::4])[0, 1]) < 0.01 and abs(np.corrcoef(z[:-1], z[1:])[0, 1]) < 0.01
    # frames are independent streams, reproducible from (seed, frame) alone
    a, b = np.empty(64), np.empty(64)
    lib.normals(20260101, 3, 16, a.ctypes.data_as(ctypes.c_void_p))
    lib.normals(20260101, 4, 16, b.ctypes.data_as(ctypes.c_void_p))
    assert np.array_equal(a, z[:64]) and not np.array_equal(a, b)
    # the oracle's host evaluation (bench.py's CPU-baseline inputs) is the same function
    import oracle
    bits = np.random.default_rng(3).integers(0, 2, (3, 67)).astype(np.uint8)
    want = np.empty((3, 67), np.float32)
    lib.awgn(want.ctypes.data_as(ctypes.c_void_p), 3, 67, bits.ctypes.data_as(ctypes.c_void_p), 0.7, 9, 5)
    assert np.array_equal(oracle.awgn(67, 5, 3, 0.7, seed=9, codewords=bits).view(np.uint32), want.view(np.uint32))
    assert abs(float(oracle.awgn(64800, 0, 2, 0.95).mean()) - 1.0) < 0.01


# ------------------------------------------------------------- oracle vs reference

def test_oracle_against_reference_kernels_on_fresh_seeds():
    """The reference kernels' results on frames of a generator no other fixture uses
    (tests/golden/fresh_seeds.npz, made by oracle/make_golden.py's fresh_seeds)."""
    from util import GOLDEN, load_golden
    gd = load_golden(os.path.join(GOLDEN, "fresh_seeds.npz"))
    assert len(gd["cases"]) == 4
    for i, (rate, N) in enumerate(gd["cases"].tolist()):
        K, M, z = codes.wimax_dims(rate, N)
        rows, cols = codes.wimax_edges(rate, N)
        g = oracle.Graph(rows, cols, M, N, K)
        y = gd["y%d" % i]
        for algo in ("ms", "sp"):
            o = oracle.decode(g, y, algo)
            assert np.array_equal(o["out"], gd["%s_out%d" % (algo, i)]) and np.array_equal(o["hard"], gd["%s_hard%d" % (algo, i)])
            assert int(o["iters"].max()) == int(gd["%s_time%d" % (algo, i)])
        if rate != 1:
            o = oracle.decode(g, y, "layered", layer_rows=z)
            assert np.array_equal(o["out"], gd["layered_out%d" % i])


# ------------------------------------------------------------------- C++ Coder

def _build_roundtrip(tmp_path):
    exe = str(tmp_path / "coder_roundtrip")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "coder_roundtrip.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "myldpccppapi_amd"), "-lmyldpc", "-lldpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myldpccppapi_amd")])
    return exe


def test_cpp_coder_encoder_satisfies_h(built, tmp_path):
    """Coder::encode (structured solve) produces systematic codewords with H c = 0 for
    all six rates, short last frames included.  CPU only."""
    exe = _build_roundtrip(tmp_path)
    for rate in range(6):
        for N, src in ((576, 1000), (2304, 777)):
            out = subprocess.run([exe, str(rate), str(N), str(src), "4", "3", "ENC"],
                                 capture_output=True, text=True)
            assert out.returncode == 0 and "ParityFail=0" in out.stdout, (rate, N, out.stdout)
    # a payload large enough for encode() to spread its frames over several host threads (>= 2 Mbit of code bits per
    # thread): 8000 frames of (2304, 1152) and a short last one, and (648, 324) where frames start inside a byte
    for rate, N, src in ((0, 2304, 8000 * 144 + 77), (0, 648, 20000 * 81 // 2 + 5)):
        out = subprocess.run([exe, str(rate), str(N), str(src), "4", "3", "ENC"], capture_output=True, text=True)
        assert out.returncode == 0 and "ParityFail=0" in out.stdout, (rate, N, out.stdout)


def test_cpp_coder_encoder_equals_independent_gf2_solve(built, tmp_path):
    """Coder::encode (structured O(E) solve) against oracle/gf2_encoder.py -- plain Gaussian
    elimination on H, no structure assumed -- byte for byte, for all six seed matrices, several frames
    and a short last frame; and for (648, 324), where K % 8 != 0 makes frame f start at source byte
    (f*K)/8 as in the reference (MyLdpc.cpp:556-564): 0, 40, 81, 121, ...  CPU only."""
    from oracle.gf2_encoder import Gf2Encoder
    exe = _build_roundtrip(tmp_path)
    mbs = [12, 8, 8, 6, 6, 4]
    for rate, N, src_len in [(r, 576, 3 * (576 - mbs[r] * 24) // 8 + 11) for r in range(6)] + \
                            [(0, 2304, 300), (5, 2304, 500), (0, 648, 4 * 40 + 7), (0, 648, 120)]:
        K = N - mbs[rate] * (N // 24)
        pre = str(tmp_path / ("enc_%d_%d_%d" % (rate, N, src_len)))
        out = subprocess.run([exe, str(rate), str(N), str(src_len), "4", "3", "ENC", "1", "--dump", pre],
                             capture_output=True, text=True)
        assert out.returncode == 0 and "ParityFail=0" in out.stdout, (rate, N, out.stdout)
        prior = np.fromfile(pre + ".prior", np.uint8)
        rows, cols = codes.wimax_edges(rate, N)
        enc = Gf2Encoder(rows, cols, N - K, N)
        src = bytes((ord("a") + i % 26) for i in range(src_len))          # the harness's payload (Test.cpp:43-45)
        kb, nb = K // 8, N // 8
        f = 0
        while True:                                                        # the reference's loop, :556-567
            at = f * K // 8
            last = not ((f + 1) * K // 8 < src_len)
            want = enc.encode_bytes(src[at:at + kb], kb if not last else src_len - at)
            assert np.array_equal(prior[f * N // 8:f * N // 8 + nb], want), (rate, N, src_len, f)
            f += 1
            if last:
                break
        assert f >= 2


def test_lock_mode_blocks_stay_inside_the_call_and_are_page_disjoint(built):
    """LDPC_HOST_INPUT_LOCK_PAGES page arithmetic (ldpc_host_block_plan): for every launch
    group the page-locked block consists of whole pages, lies inside the call's own byte range
    [base, base + frames*N*4) -- also when a tiny last group shares the previous group's last page,
    the case that used to round a block UP past the caller's buffer -- blocks of different groups are
    page-disjoint, and head + body + tail tile the group's bytes exactly."""
    rng = np.random.default_rng(5)
    cases = [(0x7f0000001000 + 12, 2049, 648, 2048),          # ADVICE's example: 2592-byte last group
             (0x7f0000000ff8, 2049, 648, 2048), (0x7f0000000000, 4097, 648, 2048),
             (0x7f0000000004, 3 * 4096 + 1, 64800, 4096), (0x7f0000000800, 5000, 2304, 1024),
             (0x7f0000000000, 3, 1, 1), (0x7f0000000ffc, 2, 1024, 1), (0x7f0000000010, 4096, 64800, 4096)]
    for _ in range(200):
        cases.append((0x7f0000000000 + int(rng.integers(0, 8192)) * 4, int(rng.integers(1, 6000)),
                      int(rng.integers(1, 3000)), int(rng.integers(1, 2500))))
    for base, frames, N, B in cases:
        end = base + frames * N * 4
        groups = (frames + B - 1) // B
        prev_b1, prev_s1 = 0, base
        for k in range(groups):
            s0, s1, b0, b1, body_end, whole = L.capi.host_block_plan(base, frames, N, B, k)
            assert s0 == prev_s1 and s1 == base + min(frames, (k + 1) * B) * N * 4
            prev_s1 = s1
            if whole:
                assert b0 == b1 == 0
                continue
            assert b0 % 4096 == 0 and b1 % 4096 == 0 and b0 < b1
            assert base <= b0 and b1 <= end, (base, frames, N, B, k)          # never past the call's bytes
            assert s0 <= b0 < s0 + 4096 and b0 <= body_end <= min(b1, s1)
            assert body_end == min(b1, s1) and s1 - body_end < 4096           # tail shorter than a page
            assert b0 >= prev_b1                                               # page-disjoint from the group before
            prev_b1 = b1
        assert prev_s1 == end
    with pytest.raises(L.LdpcError):
        L.capi.host_block_plan(0x1000, 10, 8, 4, 3)                           # group 3 of 3 groups (0..2)
    assert L.capi.host_locked_ranges() == (0, 0)


def test_worker_threads_and_lock_registry_unit(built, tmp_path):
    """csrc/host_stage.hpp compiled for the host: the persistent worker behind every handle's threads (FIFO
    order, return codes and the worker thread's error text, exceptions caught inside the job, queued jobs run
    at stop), the lock-pages page arithmetic on ADVICE r2's example, and the page-lock registry's paths that
    need no device (a failed registration leaves no record; releasing an unknown block is refused)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "host_stage_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(root, "tests", "cpp", "host_stage_test.cpp"), "-o", exe,
                           "-L/opt/rocm/lib", "-lamdhip64", "-lpthread", "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout + p.stderr


def test_resource_owners_unit_under_host_sanitizers(built, tmp_path):
    """csrc/hip_host.hpp: the owners of pinned memory, events and streams (and DevBuf's make-if-absent) in a
    stand-alone program whose host code is built with the address and undefined-behaviour sanitizers: moves,
    release twice, make-if-absent twice, destruction of a never-created owner.  The program runs with every device
    hidden, so each create fails and must leave its owner empty."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "hip_holders_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(root, "tests", "cpp", "hip_holders_test.cpp"), "-o", exe])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
    assert "5 refused" in p.stdout, p.stdout
