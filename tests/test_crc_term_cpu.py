"""CRC-aided early termination without a GPU: the expectation helper (crc_term_ref.py) on the chain scenario, the host
arithmetic (ldpc_crc_weights, ldpc_tb_frame_crc) against tb_ref, the config checks of the C ABI -- which all happen before a
device is touched --, Coder::setCrcEarlyStop's refusals, and csrc/crc_term_host.hpp under the host sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib, codes

import crc_term_cases as CC
import crc_term_ref as CR
import ratematch_util as U
import tb_ref
import tb_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDPC_OK, LDPC_ERR_ARG, LDPC_ERR_HIP, LDPC_ERR_UNSUPPORTED = 0, 1, 2, 4
CRC16, CRC24A, CRC24B = 16, 24, 25


@pytest.mark.parametrize("algo,snr,earlier,never", [("ms", 0.0, 32, 8), ("sp", 1.5, 32, 8), ("layered", 3.0, 16, 0)])
def test_scenario_is_not_vacuous(algo, snr, earlier, never):
    """Conditions on the inputs, met by the oracle alone: enough frames the CRC stops before the syndrome would, and at
    the hard points enough frames neither rule stops."""
    r = CR.chain(algo, snr)
    print("%s %.1f dB: earlier %d, crc only %d, never %d, mean stop %.2f vs %.2f" %
          (algo, snr, r["earlier"].size, r["crc_only"].size, r["never"].size, r["iters"].mean(), r["syn_iters"].mean()))
    assert r["earlier"].size >= earlier and r["never"].size >= never
    assert np.array_equal(r["earlier"], r["by_crc"])
    # the rule never stops a frame later than the syndrome does, and where neither stops both say max_iter
    assert (r["iters"] <= r["syn_iters"]).all() and (r["iters"][r["never"]] == U.MAX_ITER).all()
    # a frame stopped by either rule has bits that pass the CRC or a clean syndrome; here no CRC stop has a wrong payload
    sent = tb_ref.bits_of(TU.chain_payload()[1])[:, :CR.CHAIN_BITS]
    assert np.array_equal(r["hard"][r["by_crc"], :CR.CHAIN_BITS], sent[r["by_crc"]])


@pytest.mark.parametrize("name,threshold", [("POLLED", 64), ("TAIL", 512)])
def test_hand_over_mixtures_are_not_vacuous(name, threshold):
    """The mixtures of the GPU hand-over tests, from the helper alone: a hand-over happens within a few rounds (at most
    `threshold` frames and at most a quarter of the batch still run) and at least 4 frames stop by the CRC alone later."""
    case = getattr(CC, name)
    rnd, late = CC.crc_stops_after_handover(case, threshold)
    print(name, "hand-over after round", rnd, "frames that stop by the CRC alone afterwards:", late.size)
    assert rnd <= 4 and late.size >= 4
    assert CC.want(*case)["never"].size >= 1          # and some frame runs all rounds wherever it sits


def test_syndrome_rule_of_the_helper_is_the_oracles():
    """The helper's by-product, the syndrome rule alone, equals one oracle.decode over all rounds."""
    for algo in ("ms", "layered"):
        snr = TU.HARD[algo][0]
        r = CR.chain(algo, snr)
        want = TU.chain_oracle(algo, snr)[1]
        assert np.array_equal(r["syn_iters"], want)


@pytest.mark.parametrize("kind", [CRC16, CRC24A, CRC24B])
def test_weights_equal_the_reference(built, kind):
    rng = np.random.default_rng(kind)
    for n in (17, 18, 25, 26, 63, 64, 65, 327, 328, 329, 8447, 8448, 8449):
        w = L.TransportBlock.crc_weights(kind, n)
        assert w.shape == (n,) and w.dtype == np.uint32
        ks = np.arange(n) if n < 400 else np.unique(np.r_[0, 1, n - 2, n - 1, rng.integers(0, n, 24)])
        unit = np.zeros((ks.size, n), np.uint8)
        unit[np.arange(ks.size), ks] = 1
        par = tb_ref.parity(kind, unit)
        Lb = par.shape[1]
        want = (par.astype(np.uint64) << np.arange(Lb - 1, -1, -1, dtype=np.uint64)).sum(axis=1)
        assert np.array_equal(w[ks].astype(np.uint64), want), (kind, n)
        assert int(w[ks[0]]) == tb_ref.crc(kind, unit[0])
        for _ in range(3):
            row = rng.integers(0, 2, n, dtype=np.uint8)
            assert int(np.bitwise_xor.reduce(w[row.astype(bool)])) == tb_ref.crc(kind, row), (kind, n)
    assert L.TransportBlock.crc_weights(kind, 0).size == 0
    lib = _lib.load()
    assert lib.ldpc_crc_weights(kind, -1, None) == LDPC_ERR_ARG and lib.ldpc_crc_weights(kind, 8, None) == LDPC_ERR_ARG
    assert lib.ldpc_crc_weights(17, 8, np.zeros(8, np.uint32).ctypes.data) == LDPC_ERR_ARG


def test_frame_crc_over_the_shapes(built):
    refused = []
    for shape in TU.SHAPES:
        A, tb_crc, C, cb_crc, K = shape
        ref = TU.ref_spec(shape)
        tb = L.TransportBlock(A, K, C=C, tb_crc=tb_crc, cb_crc=cb_crc)
        if cb_crc == 24:
            assert tb.frame_crc() == (CRC24B, ref.Kp), shape
        elif C == 1 and tb_crc:
            assert tb.frame_crc() == ({16: CRC16, 24: CRC24A}[tb_crc], ref.Kp), shape
        else:
            with pytest.raises(L.LdpcError) as e:
                tb.frame_crc()
            assert e.value.code == LDPC_ERR_ARG and "no CRC" in str(e.value)
            refused.append(shape)
    assert refused == [(1000, 24, 2, 0, 512)]
    tb = L.TransportBlock(1000, 1024, C=1, tb_crc=0, cb_crc=0)              # no CRC at all
    with pytest.raises(L.LdpcError):
        tb.frame_crc()
    # the multi-block frames of the GPU tests: CRC24A on the block gives S = 328 and Kp = K, the rule's CRC16 Kp = 348
    assert L.TransportBlock(632, 352, C=2, tb_crc=24).frame_crc() == (CRC24B, 352)
    assert L.TransportBlock(632, 352, C=2).frame_crc() == (CRC24B, 348)


def _create(cfg, g):
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.ldpc_decoder_create(g._h, ctypes.byref(cfg), ctypes.byref(h))
    if rc == LDPC_OK:
        lib.ldpc_decoder_destroy(h)
    return rc, lib.ldpc_last_error().decode()


def _cfg(algo, **kw):
    cfg = _lib.DecoderConfigCrc()
    assert _lib.load().ldpc_decoder_config_init_sized(ctypes.byref(cfg), ctypes.sizeof(cfg)) == LDPC_OK
    cfg.K, cfg.max_batch, cfg.algo, cfg.layer_rows = U.K, 64, L.capi.ALGOS[algo], U.Z
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


@pytest.fixture(scope="module")
def graph(built):
    rows, cols, _ = U.bg1()
    return L.Graph(rows, cols, U.M, U.N)


def test_config_fields_are_appended_and_default_to_off(built):
    """_lib.DecoderConfig stays the struct as it was before the two fields (what a caller built against that header
    passes); _lib.DecoderConfigCrc is all of ldpc_decoder_config."""
    C, F = _lib.DecoderConfig, _lib.DecoderConfigCrc
    cfg = _cfg("ms")
    assert cfg.crc_kind == 0 and cfg.crc_bits == 0
    assert F.crc_kind.offset == C.ms_offset.offset + 4 == ctypes.sizeof(C)
    assert ctypes.sizeof(F) == F.crc_bits.offset + 4 == cfg.struct_size
    assert _lib.load().ldpc_abi_version() == 3


def test_config_init_never_writes_behind_the_callers_struct(built):
    """ldpc_decoder_config_init_sized fills exactly the size it is told, one of the three accepted ones, with the same
    defaults; the exported ldpc_decoder_config_init -- what a caller built against the header before crc_kind / crc_bits
    calls with its shorter struct -- fills offsetof(crc_kind) bytes and says so in struct_size."""
    lib = _lib.load()
    C, F = _lib.DecoderConfig, _lib.DecoderConfigCrc
    sizes = (C.ms_scale.offset, ctypes.sizeof(C), ctypes.sizeof(F))

    def fresh():
        buf = (ctypes.c_uint8 * (ctypes.sizeof(F) + 16))(*([0xA5] * (ctypes.sizeof(F) + 16)))
        return buf, ctypes.cast(buf, ctypes.POINTER(C))

    for size in sizes:
        buf, ptr = fresh()
        assert lib.ldpc_decoder_config_init_sized(ptr, size) == LDPC_OK
        cfg = ptr.contents
        assert (cfg.struct_size, cfg.max_iter, cfg.llr_scale, cfg.early_term, cfg.max_batch) == (size, 40, 8.0, 1, 1)
        assert bytes(buf[size:]) == b"\xa5" * (len(buf) - size), size
        assert bytes(buf[C.poll_interval.offset + 4:size]) == b"\0" * (size - C.poll_interval.offset - 4), size
    for size in (0, 4, sizes[0] + 4, sizes[1] + 4, sizes[2] + 8):
        buf, ptr = fresh()
        assert lib.ldpc_decoder_config_init_sized(ptr, size) == LDPC_ERR_ARG and "struct_size" in lib.ldpc_last_error().decode()
        assert bytes(buf) == b"\xa5" * len(buf), size
    assert lib.ldpc_decoder_config_init_sized(None, sizes[2]) == LDPC_ERR_ARG
    buf, ptr = fresh()
    lib.ldpc_decoder_config_init(ptr)
    assert ptr.contents.struct_size == ctypes.sizeof(C) and bytes(buf[ctypes.sizeof(C):]) == b"\xa5" * (len(buf) - ctypes.sizeof(C))


def test_the_three_struct_sizes(graph):
    """offsetof(ms_scale), offsetof(crc_kind) -- the full size before this feature, CRC off: the bytes behind it are not
    read -- and the full size; anything else is an ABI mismatch."""
    before_ms, before_crc, full = (_lib.DecoderConfig.ms_scale.offset, ctypes.sizeof(_lib.DecoderConfig),
                                   ctypes.sizeof(_lib.DecoderConfigCrc))
    for algo in ("ms", "sp", "layered", "ms_fused"):
        cfg = _cfg(algo, crc_kind=99, crc_bits=-7)                # would be refused if they were read
        for size in (before_ms, before_crc):
            cfg.struct_size = size
            assert _create(cfg, graph)[0] in (LDPC_OK, LDPC_ERR_HIP), (algo, size)
        for size in (before_ms + 4, before_crc + 4, full + 4, full + 8, 0):
            cfg.struct_size = size
            rc, msg = _create(cfg, graph)
            assert rc == LDPC_ERR_ARG and "struct_size" in msg, (algo, size)
        cfg.struct_size = full
        rc, msg = _create(cfg, graph)
        assert rc == LDPC_ERR_ARG and "crc_kind" in msg
    lib = _lib.load()
    h = ctypes.c_void_p()
    devs = (ctypes.c_int32 * 1)(0)
    cfg = _cfg("ms", crc_kind=99)
    cfg.struct_size = before_crc
    rc = lib.ldpc_decoder_create_multi(graph._h, ctypes.byref(cfg), devs, 1, ctypes.byref(h))
    assert rc in (LDPC_OK, LDPC_ERR_HIP)
    if rc == LDPC_OK:
        lib.ldpc_decoder_destroy(h)
    cfg.struct_size = full
    assert lib.ldpc_decoder_create_multi(graph._h, ctypes.byref(cfg), devs, 1, ctypes.byref(h)) == LDPC_ERR_ARG


def test_config_refusals_name_the_field(graph):
    for algo in ("sp", "ms", "layered"):
        for kind in (1, 17, 23, 26, -16, 1 << 20):
            rc, msg = _create(_cfg(algo, crc_kind=kind, crc_bits=328), graph)
            assert rc == LDPC_ERR_ARG and "crc_kind" in msg, (algo, kind)
        for kind, bits in ((CRC16, 16), (CRC16, 0), (CRC16, -1), (CRC16, U.K + 1), (CRC24A, 24), (CRC24B, 24), (CRC24B, U.K + 1),
                           (CRC24A, 1 << 30)):
            rc, msg = _create(_cfg(algo, crc_kind=kind, crc_bits=bits), graph)
            assert rc == LDPC_ERR_ARG and "crc_bits" in msg, (algo, kind, bits)
        rc, msg = _create(_cfg(algo, crc_kind=CRC16, crc_bits=328, early_term=0), graph)
        assert rc == LDPC_ERR_ARG and "early_term" in msg, algo
        # the LDS-resident and the record kernels do not carry the rule: forcing them is refused
        for field in ("fused", "ldsp"):
            cfg = _cfg(algo, crc_kind=CRC16, crc_bits=328)
            L.capi.apply_tune(cfg, {field: True})
            rc, msg = _create(cfg, graph)
            assert rc == LDPC_ERR_UNSUPPORTED and "crc_kind" in msg, (algo, field)
    # the two that reproduce reference kernels, on a code LAYERED_HOST is otherwise allowed on (every row of one weight)
    rate, N = codes.RATE_5_6, 576
    K, M, z = codes.wimax_dims(rate, N)
    wg = L.Graph(*codes.wimax_edges(rate, N), M, N)
    for algo in ("ms_fused", "layered_host"):
        assert _create(_cfg(algo, K=K, layer_rows=z), wg)[0] in (LDPC_OK, LDPC_ERR_HIP), algo
        rc, msg = _create(_cfg(algo, K=K, layer_rows=z, crc_kind=CRC16, crc_bits=328), wg)
        assert rc == LDPC_ERR_UNSUPPORTED and "crc_kind" in msg, algo
    # crc_kind = 0: crc_bits is not read
    assert _create(_cfg("ms", crc_kind=0, crc_bits=-5), graph)[0] in (LDPC_OK, LDPC_ERR_HIP)


def test_valid_configs_reach_the_device_check(graph):
    for algo, kw in (("sp", {}), ("ms", {}), ("layered", {}), ("ms", dict(msg_dtype=L.capi.MSG_F16)), ("ms", dict(ms_scale=0.75)),
                     ("layered", dict(ms_offset=0.1)), ("ms", dict(frames_per_lane=4, poll_interval=1))):
        for kind, bits in ((CRC16, 328), (CRC16, 17), (CRC24A, 25), (CRC24B, U.K), (CRC24A, 331)):
            assert _create(_cfg(algo, crc_kind=kind, crc_bits=bits, **kw), graph)[0] in (LDPC_OK, LDPC_ERR_HIP), (algo, kw, kind, bits)
    # forcing the one-launch kernels OFF is no conflict
    cfg = _cfg("ms", crc_kind=CRC16, crc_bits=328)
    L.capi.apply_tune(cfg, {"fused": False, "ldsp": False})
    assert _create(cfg, graph)[0] in (LDPC_OK, LDPC_ERR_HIP)


def test_crc_stops_needs_a_call_and_a_handle(built):
    lib = _lib.load()
    n = ctypes.c_int64(5)
    assert lib.ldpc_decoder_crc_stops(None, ctypes.byref(n)) == LDPC_ERR_ARG


def test_coder_exports_and_refusals(built, tmp_path):
    so = os.path.join(ROOT, "myldpccppapi_amd", "libmyldpc.so")
    syms = subprocess.run("nm -D --defined-only %s | c++filt" % so, shell=True, capture_output=True, text=True).stdout
    assert "Coder::setCrcEarlyStop(bool)" in syms
    exe = CC.coder_crc_early_stop_exe(tmp_path)
    p = subprocess.run([exe, "refusals"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("refused=ok"), p.stdout + p.stderr


def test_host_header_under_host_sanitizers(tmp_path):
    """csrc/crc_term_host.hpp in a stand-alone program built with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "crc_term_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "crc_term_host_test.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
