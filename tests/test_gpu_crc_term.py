"""CRC-aided early termination on the GPU (ldpc_decoder_config::crc_kind / crc_bits) against crc_term_ref.py -- the CPU
oracle run round by round with tb_ref's CRC on its hard bits: all output bytes, all iteration counts and the number of
frames stopped by the CRC alone, bit for bit.  Inputs beyond the chain scenario, and what makes them reach the paths they
are there for: crc_term_cases.py."""
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L

import arena_cases as ac
import crc_term_cases as CC
import crc_term_ref as CR
import ratematch_util as U
import tb_util as TU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def graph(built):
    rows, cols, _ = U.bg1()
    return L.Graph(rows, cols, U.M, U.N)


def _assert_rule(dec, out, iters, w, what):
    assert np.array_equal(iters, w["iters"]), what
    assert np.array_equal(out, w["out"]), what
    assert dec.crc_stops() == w["by_crc"].size, (what, dec.crc_stops(), w["by_crc"].size)
    st = dec.stats()
    assert st["frames_converged"] == w["iters"].size - w["never"].size, (what, st)
    return st


# (algo, variant of crc_term_ref.chain, Decoder keywords)
CHAIN = [("sp", "", {}), ("ms", "", {}), ("layered", "", {}), ("ms", "f16", dict(msg_dtype="f16")), ("ms", "scale", dict(ms_scale=0.75))]


@pytest.mark.parametrize("point", [0, 1], ids=["clean", "hard"])
@pytest.mark.parametrize("algo,variant,kw", CHAIN, ids=["sp", "ms", "layered", "ms16", "ms_scale"])
def test_chain_scenario_equals_the_rule(graph, algo, variant, kw, point):
    """64 frames of the chain scenario at both of its points, tiles of 64, 128 and 256 frames."""
    snr = TU.chain_points(algo)[point]
    w = CR.chain(algo, snr, variant)
    y = TU.chain_received(snr)[2]
    print(algo, variant, snr, "stopped by the CRC alone:", w["by_crc"].size, "never:", w["never"].size)
    assert w["by_crc"].size >= 4
    for fpl in (1, 2, 4):
        dec = L.Decoder(graph, U.K, max_batch=64, algo=algo, max_iter=U.MAX_ITER, llr_scale=TU.HARD[algo][1], layer_rows=U.Z,
                        frames_per_lane=fpl, crc_kind=CR.CHAIN_KIND, crc_bits=CR.CHAIN_BITS, **kw)
        for call in range(2):
            out, iters = dec.decode(y)
            st = _assert_rule(dec, out, iters, w, (algo, variant, snr, fpl, call))
            assert st["batch_time"] == int(w["iters"].max())
        dec.close()


@pytest.mark.parametrize("algo", ["sp", "ms", "layered"])
def test_crc_off_is_the_syndrome_rule(graph, algo):
    """crc_kind = 0 on the same inputs: bytes and iteration counts of the oracle's syndrome rule alone, no CRC stops --
    on the kernels the library picks and on the streaming ones."""
    for snr in TU.chain_points(algo):
        want = TU.chain_oracle(algo, snr)
        y = TU.chain_received(snr)[2]
        for tune in (None, {"fused": False, "ldsp": False}):
            dec = L.Decoder(graph, U.K, max_batch=64, algo=algo, max_iter=U.MAX_ITER, llr_scale=TU.HARD[algo][1], layer_rows=U.Z,
                            frames_per_lane=0 if tune is None else 1, crc_kind=0, crc_bits=CR.CHAIN_BITS, tune=tune)
            out, iters = dec.decode(y)
            assert np.array_equal(out, want[0]) and np.array_equal(iters, want[1]), (algo, snr, tune)
            assert dec.crc_stops() == 0
            dec.close()


@pytest.mark.parametrize("algo", ["ms", "layered", "sp"])
@pytest.mark.parametrize("block", ["cb", "cb348", "a24"])
def test_multi_block_frames_and_the_other_polynomials(graph, block, algo):
    """Frames of a two-block transport block: CRC24B over all K = 352 information bits (no fillers), and over 348 bits, no
    multiple of 8 or 64; a one-block transport block with CRC24A.  Random payloads, every third frame at the hard noise."""
    kind, bits, spec = CC.frame_crc(block)
    assert (kind, bits) == {"cb": (25, 352), "cb348": (25, 348), "a24": (24, 328)}[block]
    assert L.TransportBlock(spec.A, U.K, C=spec.C, tb_crc=spec.tb_crc).frame_crc() == (kind, bits)
    case = (block, algo, 64, 0.75, 0.98, 3)
    w = CC.want(*case)
    assert w["by_crc"].size >= 16
    y = CC.received(*case[:1], *case[2:])
    for fpl in (1, 2):
        dec = L.Decoder(graph, U.K, max_batch=64, algo=algo, max_iter=CC.MAXIT, llr_scale=U.LLR_SCALE, layer_rows=U.Z,
                        frames_per_lane=fpl, crc_kind=kind, crc_bits=bits)
        out, iters = dec.decode(y)
        _assert_rule(dec, out, iters, w, (block, algo, fpl))
        dec.close()


@pytest.mark.parametrize("max_batch", [64, 70])
def test_ragged_and_chunked_host_call(graph, max_batch):
    """150 frames through ldpc_decode in launch groups of 64 and of 70 (ragged tiles); crc_stops covers all groups."""
    case = ("chain", "ms", 150, 0.75, 0.98, 3)
    w = CC.want(*case)
    y = CC.received(case[0], *case[2:])
    for kw in (dict(), dict(poll_interval=1), dict(frames_per_lane=2)):
        dec = L.Decoder(graph, U.K, max_batch=max_batch, algo="ms", max_iter=CC.MAXIT, crc_kind=16, crc_bits=328, **kw)
        out, iters = dec.decode(y)
        st = _assert_rule(dec, out, iters, w, (max_batch, kw))
        assert st["frames"] == 150
        dec.close()


def test_polled_hand_over_stops_by_crc_inside_the_child(graph):
    """256 frames in 4 tiles of 64, polled every round: after round 2 fewer than 64 frames run and go to the child
    decoder, where dozens of them later stop by the CRC alone.  The child inherits the two config fields and runs the
    kernel in its own rounds; its count joins the parent's."""
    case = CC.POLLED
    rnd, late = CC.crc_stops_after_handover(case, 64)
    assert late.size >= 4
    w = CC.want(*case)
    y = CC.received(case[0], *case[2:])
    B = case[2]
    dec = L.Decoder(graph, U.K, max_batch=B, algo="ms", max_iter=CC.MAXIT, frames_per_lane=1, poll_interval=1, crc_kind=16, crc_bits=328)
    for call in range(2):
        out, iters = dec.decode(y)
        st = _assert_rule(dec, out, iters, w, ("polled", call))
        full = ac.frame_rounds_without_handover(w["iters"], 64, CC.MAXIT)
        print("polled: hand-over after round", rnd, "late CRC stops", late.size, "frame_rounds", st["frame_rounds"], "of", full)
        assert st["frame_rounds"] < full            # the stragglers left their tiles
    dec.close()
    # the same without a child
    ref = L.Decoder(graph, U.K, max_batch=B, algo="ms", max_iter=CC.MAXIT, frames_per_lane=1, poll_interval=1, crc_kind=16, crc_bits=328,
                    tune={"compact": -1})
    out, iters = ref.decode(y)
    _assert_rule(ref, out, iters, w, "polled, no hand-over")
    ref.close()


def test_device_side_tail_stops_by_crc_in_the_overflow_tiles(graph):
    """2048 frames in 32 tiles of 64 without host polling: after round 2 about a hundred frames run and move to the
    overflow tiles, where they stop by the CRC alone in later rounds (tile_select with the tail, fail slot stride TA * V)."""
    import torch
    case = CC.TAIL
    rnd, late = CC.crc_stops_after_handover(case, 512)
    assert late.size >= 4
    w = CC.want(*case)
    B = case[2]
    yd = torch.tensor(CC.received(case[0], *case[2:])).cuda()
    nb = L.out_bytes(U.K, B)
    for tune in ({}, {"device_tail": False}):
        dec = L.Decoder(graph, U.K, max_batch=B, algo="ms", max_iter=CC.MAXIT, frames_per_lane=1, poll_interval=0, crc_kind=16, crc_bits=328,
                        tune=tune)
        for call in range(2):
            out = torch.full((nb,), 0xEE, dtype=torch.uint8, device="cuda")
            it = torch.zeros(B, dtype=torch.int32, device="cuda")
            dec.decode_device(yd.data_ptr(), B, out.data_ptr(), nb, it.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            st = _assert_rule(dec, out.cpu().numpy(), it.cpu().numpy(), w, ("tail", tune, call))
            full = ac.frame_rounds_without_handover(w["iters"], 64, CC.MAXIT)
            print("tail", tune, "hand-over after round", rnd, "late CRC stops", late.size, "frame_rounds", st["frame_rounds"], "of", full)
            assert (st["frame_rounds"] < full) == tune.get("device_tail", True)
        dec.close()


@pytest.mark.parametrize("algo", ["ms", "layered"])
def test_device_entry_point_contract(graph, algo):
    """out_dev == NULL with iters_dev, and an llr_dev that is 4-byte aligned only: the same iteration counts and count."""
    import torch
    case = ("chain", algo, 64, 0.75, 0.98, 3)
    w = CC.want(*case)
    y = CC.received(case[0], *case[2:])
    B, nb = 64, L.out_bytes(U.K, 64)
    dec = L.Decoder(graph, U.K, max_batch=B, algo=algo, max_iter=CC.MAXIT, layer_rows=U.Z, frames_per_lane=1, crc_kind=16, crc_bits=328)
    buf = torch.zeros(B * U.N + 8, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for off in (0, 1):                                  # 16-byte aligned; 4 modulo 16
        buf[off:off + B * U.N] = torch.tensor(y).reshape(-1).cuda()
        out = torch.full((nb,), 0xEE, dtype=torch.uint8, device="cuda")
        it = torch.zeros(B, dtype=torch.int32, device="cuda")
        dec.decode_device(buf.data_ptr() + 4 * off, B, out.data_ptr(), nb, it.data_ptr(), stream)
        torch.cuda.synchronize()
        _assert_rule(dec, out.cpu().numpy(), it.cpu().numpy(), w, (algo, "offset", off))
        it.fill_(-1)
        dec.decode_device(buf.data_ptr() + 4 * off, B, None, 0, it.data_ptr(), stream)
        torch.cuda.synchronize()
        assert np.array_equal(it.cpu().numpy(), w["iters"]) and dec.crc_stops() == w["by_crc"].size, (algo, "out NULL", off)
    dec.close()


def test_coder_end_to_end(built, tmp_path):
    """Coder::setTransportBlock + setCrcEarlyStop(true) against the same Coder without it, on the same received values:
    equal payload bytes wherever the CRC passed, no more iterations, and frames stopped by the CRC alone."""
    p = subprocess.run([CC.coder_crc_early_stop_exe(tmp_path)], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    f = dict(kv.split("=") for kv in p.stdout.split())
    assert f["refused"] == "ok" and f["same"] == "ok", p.stdout
    assert int(f["TimeCrc"]) <= int(f["Time"]) and int(f["CrcStops"]) > 0 and int(f["CrcStopsPlain"]) == 0, p.stdout
    plain, early = (int(v) for v in f["CrcFailures"].split("/"))
    assert early <= plain, p.stdout
