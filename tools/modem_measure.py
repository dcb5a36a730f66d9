#!/usr/bin/env python3
"""Times the two modem kernels (ldpc_modem_transmit_device, ldpc_modem_demap_device) at sizes a simulation runs, next to
the same process's ldpc_hbm_probe_device and, for the transmit kernel, next to ldpc_awgn_device at the same number of
real samples (both are bound by the double-precision Box-Muller, not by memory).

Shapes: E = 20000 rounded to a multiple of 24 (19992) with 8192 frames, and E = 48600 -> 48576 with 4096 frames; every Qm
with and without the interleaver.  Per call: HIP-event time, median and minimum of 20 after 3 warm-up calls; the bytes
the call's own loads and stores move (transmit: E bytes of tx in + 4 bytes per real sample out; demap: 4 bytes per real
sample in + 4 E out, per frame), and that rate over the probe's non-temporal copy rate.  The buffers of a call are far
larger than the 256 MiB Infinity Cache.  One JSON line per measurement.

    python tools/modem_measure.py [--shapes bg1,dvbs2] [--qm 1,2,4,6,8]"""
import argparse, json, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
import myldpccppapi_amd as L
from myldpccppapi_amd import capi, channel

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="bg1,dvbs2")
ap.add_argument("--qm", default="1,2,4,6,8")
args = ap.parse_args()
SHAPES = {"bg1": dict(E=20000 // 24 * 24, frames=8192), "dvbs2": dict(E=48600 // 24 * 24, frames=4096)}


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
    E, B = SHAPES[name]["E"], SHAPES[name]["frames"]
    tx = torch.randint(0, 2, (B, E), dtype=torch.uint8, device="cuda")
    txp = torch.randint(0, 256, (B, E // 8), dtype=torch.uint8, device="cuda")
    sym = torch.empty((B, E), dtype=torch.float32, device="cuda")           # E floats hold every Qm's row (2 E / Qm <= E)
    rx = torch.empty((B, E), dtype=torch.float32, device="cuda")

    def report(what, qm, il, samples, call, moved):
        med, fastest = event_ms(call)
        print(json.dumps({"shape": name, "E": E, "frames": B, "Qm": qm, "interleave": il, "call": what, "real_samples_per_frame": samples,
                          "ms_median": round(med, 4), "ms_min": round(fastest, 4), "bytes_moved": moved,
                          "gbs": round(moved / med / 1e6, 1), "fraction_of_nt_copy": round(moved / med / 1e6 / nt, 3),
                          "gsamples_s": round(B * samples / med / 1e6, 2)}), flush=True)

    for n in sorted({E, E // 2, E // 4}):                                   # the sample counts of Qm = 1 / 2, 4, 8
        report("ldpc_awgn_device", 0, 0, n, lambda n=n: channel.awgn_device(n, 0, B, 0.3, seed=5, codewords=None, out=sym), B * 4 * n)
    for qm in [int(x) for x in args.qm.split(",")]:
        for il in ((0,) if qm == 1 else (1, 0)):
            md = L.Modem(qm, interleave=bool(il))
            row = md.symbol_floats(E)
            report("transmit bits", qm, il, row,
                   lambda: md.transmit_device(tx.data_ptr(), B, E, 0.3, 5, sym.data_ptr(), B * row, 0, "bits", stream), B * (E + 4 * row))
            report("transmit packed", qm, il, row,
                   lambda: md.transmit_device(txp.data_ptr(), B, E, 0.3, 5, sym.data_ptr(), B * row, 0, "packed", stream), B * (E // 8 + 4 * row))
            report("transmit bits sd=0", qm, il, row,
                   lambda: md.transmit_device(tx.data_ptr(), B, E, 0.0, 5, sym.data_ptr(), B * row, 0, "bits", stream), B * (E + 4 * row))
            md.transmit_device(tx.data_ptr(), B, E, 0.3, 5, sym.data_ptr(), B * row, 0, "bits", stream)
            report("demap", qm, il, row, lambda: md.demap_device(sym.data_ptr(), B, E, rx.data_ptr(), stream), B * 4 * (row + E))
    del tx, txp, sym, rx
    torch.cuda.empty_cache()
