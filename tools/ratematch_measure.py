#!/usr/bin/env python3
"""Times the two rate-matching kernels (ldpc_rate_match_device, ldpc_rate_recover_device) at sizes a simulation runs,
next to the same process's ldpc_hbm_probe_device.

Shapes: BG1-profile Z = 384 (N = 26112, P = 768, E = 20000, 8192 frames) and DVB-S2-sized (N = 64800, E = 48600, 4096
frames).  Per call: HIP-event time, median and minimum of 20 after 3 warm-up calls; the bytes the call's own loads and
stores move (recover: 4 (E + N) per frame for y alone, + 4 N when soft is written, + 4 N more when it is accumulated
into; match: E stored plus the min(E, L) distinct code bytes it loads, per frame, in the bits format), and that rate over the probe's non-temporal copy rate.  The buffers
of a call are far larger than the 256 MiB Infinity Cache.  One JSON line per measurement.

    python tools/ratematch_measure.py [--shapes bg1,dvbs2]"""
import argparse, json, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
import myldpccppapi_amd as L
from myldpccppapi_amd import capi, channel

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="bg1,dvbs2")
args = ap.parse_args()
SHAPES = {"bg1": dict(N=26112, P=768, filler=(0, 0), E=20000, k0=0, frames=8192),
          "dvbs2": dict(N=64800, P=0, filler=(0, 0), E=48600, k0=0, frames=4096)}


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


best, default, nt = capi.hbm_probe(0, by_policy=True)
print(json.dumps({"hbm_probe_copy_gbs": {"default": round(default, 1), "non_temporal": round(nt, 1)}}), flush=True)
stream = torch.cuda.current_stream().cuda_stream
for name in args.shapes.split(","):
    sh = SHAPES[name]
    N, E, k0, B = sh["N"], sh["E"], sh["k0"], sh["frames"]
    rm = L.RateMatcher(N, punctured=sh["P"], filler=sh["filler"], erasure_llr=1e-6)
    code = torch.randint(0, 2, (B, N), dtype=torch.uint8, device="cuda")
    tx = torch.empty((B, E), dtype=torch.uint8, device="cuda")
    txp = torch.empty((B, E // 8), dtype=torch.uint8, device="cuda")
    rx = channel.awgn_device(E, 0, B, 0.7, seed=5, codewords=None)
    y = torch.empty((B, N), dtype=torch.float32, device="cuda")
    soft = torch.zeros((B, N), dtype=torch.float32, device="cuda")
    # the punctured prefix and the part of the buffer a short transmission does not reach are never loaded by match
    calls = (
        ("match bits->bits", lambda: rm.match_device(code.data_ptr(), B, k0, E, tx.data_ptr(), tx.numel(), "bits", "bits", stream),
         B * (E + min(E, rm.lengths()[1]))),
        ("match bits->packed", lambda: rm.match_device(code.data_ptr(), B, k0, E, txp.data_ptr(), txp.numel(), "bits", "packed", stream),
         B * (min(E, rm.lengths()[1]) + E // 8)),
        ("recover y", lambda: rm.recover_device(rx.data_ptr(), B, k0, E, None, False, y.data_ptr(), stream), B * 4 * (E + N)),
        ("recover soft+y", lambda: rm.recover_device(rx.data_ptr(), B, k0, E, soft.data_ptr(), False, y.data_ptr(), stream),
         B * 4 * (E + 2 * N)),
        ("recover soft+=,y", lambda: rm.recover_device(rx.data_ptr(), B, k0, E, soft.data_ptr(), True, y.data_ptr(), stream),
         B * 4 * (E + 3 * N)),
    )
    for what, call, moved in calls:
        med, fastest = event_ms(call)
        print(json.dumps({"shape": name, "N": N, "P": sh["P"], "E": E, "frames": B, "call": what, "ms_median": round(med, 4),
                          "ms_min": round(fastest, 4), "bytes_moved": moved, "gbs": round(moved / med / 1e6, 1),
                          "fraction_of_nt_copy": round(moved / med / 1e6 / nt, 3)}), flush=True)
    del code, tx, txp, rx, y, soft
    torch.cuda.empty_cache()
