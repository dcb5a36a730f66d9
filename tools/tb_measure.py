#!/usr/bin/env python3
"""Times the transport-block kernels (ldpc_tb_attach_device, ldpc_tb_check_device) at sizes a simulation runs, next to the
same process's ldpc_hbm_probe_device and to ldpc_encode_device (packed output) on the same frames.

Shapes: dvbs2 -- K = 32400, A = 32376, C = 1 (CRC24A, no code-block CRC), 4096 transport blocks, the DVB-S2-profile
(64800, 32400) encoder; bg1 -- K = 8448, C = 8, CRC24A + CRC24B, A = 8 * 8424 - 24, 1024 transport blocks = 8192 frames,
the BG1-profile Z = 384 encoder.  Per call: HIP-event time, median and minimum of 20 after 3 warm-up calls; the bytes the
call's own loads and stores move (attach: A/8 in + C K/8 out per block; check with all three outputs: C K/8 in + A/8 + C
+ 1 out; check with flags only: C K/8 in + C + 1 out), and that rate over the probe's copy rate.  One JSON line per
measurement.

    python tools/tb_measure.py [--shapes dvbs2,bg1] [--skip-encoder]"""
import argparse, json, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
import myldpccppapi_amd as L
from myldpccppapi_amd import capi, codes

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="dvbs2,bg1")
ap.add_argument("--skip-encoder", action="store_true")
args = ap.parse_args()
SHAPES = {"dvbs2": dict(K=32400, A=32376, C=1, tbs=4096), "bg1": dict(K=8448, A=8 * 8424 - 24, C=8, tbs=1024)}


def event_ms(call):
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


probe = capi.hbm_probe(0)
print(json.dumps({"hbm_probe_copy_gbs": round(probe, 1)}), flush=True)
stream = torch.cuda.current_stream().cuda_stream
for name in args.shapes.split(","):
    K, A, C, tbs = (SHAPES[name][k] for k in ("K", "A", "C", "tbs"))
    tb = L.TransportBlock(A, K)
    assert tb.C == C and tb.tb_crc == 24 and tb.cb_crc == (24 if C > 1 else 0)
    frames = tbs * C
    pay = torch.randint(0, 256, (tbs, A // 8), dtype=torch.uint8, device="cuda")
    src = torch.empty((frames, K // 8), dtype=torch.uint8, device="cuda")
    back = torch.empty_like(pay)
    cb_ok = torch.empty(frames, dtype=torch.uint8, device="cuda")
    tb_ok = torch.empty(tbs, dtype=torch.uint8, device="cuda")

    def report(what, call, moved):
        med, fastest = event_ms(call)
        print(json.dumps({"shape": name, "K": K, "A": A, "C": C, "tbs": tbs, "frames": frames, "call": what, "ms_median": round(med, 4),
                          "ms_min": round(fastest, 4), "bytes_moved": moved, "gbs": round(moved / med / 1e6, 1),
                          "fraction_of_probe": round(moved / med / 1e6 / probe, 3), "payload_gbit_s": round(tbs * A / med / 1e6, 1)}), flush=True)

    report("attach", lambda: tb.attach_device(pay.data_ptr(), tbs, src.data_ptr(), src.numel(), stream), pay.numel() + src.numel())
    report("check payload+cb_ok+tb_ok", lambda: tb.check_device(src.data_ptr(), tbs, back.data_ptr(), cb_ok.data_ptr(), tb_ok.data_ptr(), stream),
           src.numel() + pay.numel() + frames + tbs)
    report("check cb_ok+tb_ok", lambda: tb.check_device(src.data_ptr(), tbs, None, cb_ok.data_ptr(), tb_ok.data_ptr(), stream),
           src.numel() + frames + tbs)
    torch.cuda.synchronize()
    assert bool((back == pay).all()) and bool(cb_ok.all()) and bool(tb_ok.all()), "check(attach(x)) != x"
    if not args.skip_encoder:
        if name == "dvbs2":
            N, z = 64800, 0
            rows, cols = codes.dvbs2_profile_edges(N, K)
        else:
            z = 384
            N = 68 * z
            rows, cols = codes.nr_bg1_profile_edges(z)
        enc = L.Encoder(L.Graph(rows, cols, N - K, N), K, z, max_frames=frames)
        code = torch.empty(capi.code_bytes(N, frames, "packed"), dtype=torch.uint8, device="cuda")
        report("ldpc_encode_device packed", lambda: enc.encode_device(src.data_ptr(), src.numel(), frames, code.data_ptr(), code.numel(), "packed", stream),
               src.numel() + code.numel())
        enc.close()
        del code
    del pay, src, back, cb_ok, tb_ok
    torch.cuda.empty_cache()
