#!/usr/bin/env python3
"""Times ldpc_encode_device at 4096 frames for the three large codes, next to what it replaces.

Per code (802.16e-shaped (64800, 32400), DVB-S2-profile (64800, 32400), BG1-profile Z = 384) and per output format:
HIP-event time of one call, median of 20 after 3 warm-up calls, the bytes the call reads and writes, and the rate
that makes next to the same run's ldpc_hbm_probe_device.  Beside it (b), the path a device-resident simulation had
before: encode on the host + unpack to one byte per code bit + upload.  The host encode is Coder::encode (CoderBench,
its own 16 threads) for the 802.16e code; for the two profile codes it is the numpy encoder timed on a few frames and
scaled to the batch as if 16 threads shared it perfectly (which flatters the host).  Unpack and upload are timed on
the whole batch.  One JSON line per measurement; exit status 1 if a device call is not faster than (b).

    python tools/encoder_measure.py [--frames 4096] [--skip-host] [--codes wimax,dvbs2,bg1]
--skip-host: device calls only (for a run under a profiler).

    python tools/encoder_measure.py --dense [--frames 4096] [--skip-host] [--cap]
The dense encoder (ldpc_encoder_create_dense) instead: 802.16e rate 1/2 at N = 2304 and N = 16128 through the dense and the
structured handle (the same H, so the difference of the two calls is enc_rows over all rows + enc_dense_kernel against
enc_rows + enc_dd_core_kernel), creation time of the dense handle and of its host analysis alone, the work of
enc_dense_kernel (word-XORs = rho * M * W, LDS reads = rho * ceil(M / 4) * W of 8 bytes), and -- unless --skip-host -- the
path it replaces for an unstructured code: numpy Gf2Encoder + unpack + upload for the swapped (648, 324) matrix and the
(2304, 1152) one.  --cap adds the creation time at the limit M = 16384 (a permuted triangular parity part with random
fill; host only, tens of seconds).  With LDPC_HIP_LIB naming a build with other LDPC_ENC_DENSE_ROWS / LDPC_ENC_DENSE_GROUPS
the same lines compare table shapes; a per-kernel split needs one rocprofv3 --kernel-trace run of `--dense --skip-host`."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
import myldpccppapi_amd as L
from myldpccppapi_amd import capi, codes

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--skip-host", action="store_true")
ap.add_argument("--codes", default="wimax,dvbs2,bg1")
ap.add_argument("--dense", action="store_true")
ap.add_argument("--cap", action="store_true")
args = ap.parse_args()
B = args.frames
HOST_THREADS = 16


def device_ms(enc, src, code, fmt):
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda: enc.encode_device(src.data_ptr(), src.numel(), B, code.data_ptr(), code.numel(), fmt, stream)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times))


def host_encode_s(name, rows, cols, M, N, K):
    """Seconds the host needs to encode B frames; how it was obtained."""
    if name == "wimax":
        exe = os.path.join(ROOT, "myldpccppapi_amd", "CoderBench")
        out = subprocess.run([exe, "0", str(N), str(B), str(B), "10", "MS", "--iters", "1"], capture_output=True, text=True,
                             timeout=900).stdout
        return float([l for l in out.split() if l.startswith("encode_s=")][0].split("=")[1]), "Coder::encode, its own threads"
    rng = np.random.default_rng(0)
    sample = 4
    info = rng.integers(0, 2, (sample, K)).astype(np.uint8)
    if name == "bg1":
        base = codes.nr_bg1_profile_base(Z=N // 68)
        t0 = time.perf_counter()
        for f in range(sample):
            codes.nr_bg1_profile_encode(base, N // 68, info[f])
        per = (time.perf_counter() - t0) / sample
    else:
        sel = cols < K
        r, c = rows[sel], cols[sel]
        ptr = np.searchsorted(r, np.arange(M))
        t0 = time.perf_counter()
        for f in range(sample):
            lam = np.bitwise_xor.reduceat(info[f][c], ptr)
            np.bitwise_xor.accumulate(lam)
        per = (time.perf_counter() - t0) / sample
    return per * B / HOST_THREADS, "numpy encoder, %.2f ms per frame on one thread, scaled to %d threads" % (per * 1e3, HOST_THREADS)


def cap_matrix(M=16384, seed=1):
    """M x 2M, unstructured and encodable as it stands: the parity part is a unit lower triangular matrix with two more
    ones per column below the diagonal, its rows and columns shuffled; the information part has three ones per column."""
    rng = np.random.default_rng(seed)
    d = np.arange(M)
    lo = np.minimum(d + 1 + rng.integers(0, M, (2, M)) % np.maximum(M - 1 - d, 1), M - 1)
    pr = np.concatenate([d, lo[0], lo[1]])
    pc = np.concatenate([d, d, d])
    pr, pc = rng.permutation(M)[pr], rng.permutation(M)[pc]
    ir = rng.integers(0, M, 3 * M)
    ic = np.repeat(np.arange(M), 3)
    edges = np.unique(np.stack([np.concatenate([ir, pr]), np.concatenate([ic, M + pc])]), axis=1)
    rows, cols = codes.row_major(edges[0], edges[1])
    return rows, cols, M, 2 * M


def dense_mode():
    from oracle.gf2_encoder import Gf2Encoder
    probe = capi.hbm_probe(0)
    print(json.dumps({"hbm_probe_copy_gbs": round(probe, 1), "frames": B, "lib": os.path.basename(capi._lib.LIB_PATH)}), flush=True)
    W = (B + 63) // 64
    for N in (2304, 16128):
        K, M, z = codes.wimax_dims(0, N)
        rows, cols = codes.wimax_edges(0, N)
        g = L.Graph(rows, cols, M, N)
        t0 = time.perf_counter()
        L.dense_parity(g, K)
        t1 = time.perf_counter()
        dense = L.DenseEncoder(g, K, max_frames=B)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        print(json.dumps({"code": "wimax", "N": N, "M": M, "host_analysis_s": round(t1 - t0, 4), "create_dense_s": round(t2 - t1, 4),
                          "T_bytes": (N - K) * ((M + 63) // 64) * 8}), flush=True)
        structured = L.Encoder(g, K, z, max_frames=B)
        src = torch.randint(0, 256, (B * K // 8,), dtype=torch.uint8, device="cuda")
        for fmt in ("bits", "packed"):
            code = torch.empty(capi.code_bytes(N, B, fmt), dtype=torch.uint8, device="cuda")
            ref = torch.empty_like(code)
            ms_s, best_s = device_ms(structured, src, ref, fmt)
            ms_d, best_d = device_ms(dense, src, code, fmt)
            assert torch.equal(code, ref), "dense and structured encoders differ"
            xors = (N - K) * M * W
            reads = (N - K) * ((M + 3) // 4) * W * 8
            print(json.dumps({"code": "wimax", "N": N, "K": K, "format": fmt, "dense_ms_median": round(ms_d, 4), "dense_ms_min": round(best_d, 4),
                              "structured_ms_median": round(ms_s, 4), "structured_ms_min": round(best_s, 4),
                              "dense_minus_structured_ms": round(ms_d - ms_s, 4), "word_xors": xors, "lds_read_bytes": reads,
                              "word_xors_per_s_if_all_of_the_difference": "%.3g" % (xors / max(ms_d - ms_s, 1e-6) * 1e3),
                              "lds_read_tb_s_if_all_of_the_difference": round(reads / max(ms_d - ms_s, 1e-6) / 1e9, 2)}), flush=True)
        dense.close()
        structured.close()
    if not args.skip_host:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import dense_encoder_util as U
        from encoder_util import reference_packed
        for name, (rows, cols, M, N) in (("W648s", U.matrix_w648s()), ("W2304", (*codes.wimax_edges(0, 2304), 1152, 2304))):
            K = N - M
            src = np.random.default_rng(0).integers(0, 256, B * K // 8 + K // 8 + 1, dtype=np.uint8)
            t0 = time.perf_counter()
            ge = Gf2Encoder(rows, cols, M, N)
            t1 = time.perf_counter()
            sample = 64
            reference_packed(ge, src, sample)
            per = (time.perf_counter() - t1) / sample
            packed = np.random.default_rng(1).integers(0, 256, (B, N // 8), dtype=np.uint8)
            t0u = time.perf_counter()
            bits = np.unpackbits(packed, axis=1, bitorder="little")
            unpack_s = time.perf_counter() - t0u
            torch.cuda.synchronize()
            t0u = time.perf_counter()
            up = torch.from_numpy(bits).cuda()
            torch.cuda.synchronize()
            upload_s = time.perf_counter() - t0u
            del up
            print(json.dumps({"code": name, "replaced_path_ms": round((per * B + unpack_s + upload_s) * 1e3, 2),
                              "gf2_encode_ms": round(per * B * 1e3, 2), "gf2_encode": "numpy Gf2Encoder, %.3f ms per frame on one thread, %d frames timed" % (per * 1e3, sample),
                              "gf2_setup_ms": round((t1 - t0) * 1e3, 1), "unpack_ms": round(unpack_s * 1e3, 2), "upload_ms": round(upload_s * 1e3, 2)}), flush=True)
    if args.cap:
        rows, cols, M, N = cap_matrix()
        g = L.Graph(rows, cols, M, N)
        t0 = time.perf_counter()
        info = L.dense_parity(g, N - M)
        print(json.dumps({"code": "cap", "M": M, "N": N, "edges": int(rows.size), "host_analysis_s": round(time.perf_counter() - t0, 2), **info}), flush=True)
    return 0


if args.dense:
    sys.exit(dense_mode())
probe = capi.hbm_probe(0)
print(json.dumps({"hbm_probe_copy_gbs": round(probe, 1), "frames": B}), flush=True)
slower = False
for name in args.codes.split(","):
    if name == "wimax":
        N, z = 64800, 2700
        K, M, _ = codes.wimax_dims(0, N)
        rows, cols = codes.wimax_edges(0, N)
    elif name == "dvbs2":
        N, K, z = 64800, 32400, 0
        M = N - K
        rows, cols = codes.dvbs2_profile_edges(N, K)
    else:
        z = 384
        N, K, M = 68 * z, 22 * z, 46 * z
        rows, cols = codes.nr_bg1_profile_edges(z)
    enc = L.Encoder(L.Graph(rows, cols, M, N), K, z, max_frames=B)
    src = torch.randint(0, 256, (B * K // 8,), dtype=torch.uint8, device="cuda")
    replaced = None
    if not args.skip_host:
        enc_s, how = host_encode_s(name, rows, cols, M, N, K)
        packed = np.random.default_rng(1).integers(0, 256, (B, N // 8), dtype=np.uint8)
        t0 = time.perf_counter()
        bits = np.unpackbits(packed, axis=1, bitorder="little")
        unpack_s = time.perf_counter() - t0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        up = torch.from_numpy(bits).cuda()
        torch.cuda.synchronize()
        upload_s = time.perf_counter() - t0
        del up, bits
        replaced = enc_s + unpack_s + upload_s
        print(json.dumps({"code": name, "replaced_path_ms": round(replaced * 1e3, 2), "host_encode_ms": round(enc_s * 1e3, 2),
                          "host_encode": how, "unpack_ms": round(unpack_s * 1e3, 2), "upload_ms": round(upload_s * 1e3, 2),
                          "upload_bytes": B * N}), flush=True)
    for fmt in ("bits", "packed"):
        code = torch.empty(capi.code_bytes(N, B, fmt), dtype=torch.uint8, device="cuda")
        med, best = device_ms(enc, src, code, fmt)
        moved = src.numel() + code.numel()
        rec = {"code": name, "N": N, "K": K, "format": fmt, "structure": enc.structure()["kind"], "device_ms_median": round(med, 4),
               "device_ms_min": round(best, 4), "bytes_read": src.numel(), "bytes_written": code.numel(),
               "gbs": round(moved / med / 1e6, 1), "fraction_of_probe": round(moved / med / 1e6 / probe, 3),
               "info_gbit_s": round(B * K / med / 1e6, 1)}
        if replaced is not None:
            rec["speedup_over_replaced_path"] = round(replaced * 1e3 / med, 1)
            slower = slower or not (med < replaced * 1e3)
        print(json.dumps(rec), flush=True)
        del code
    enc.close()
sys.exit(1 if slower else 0)
