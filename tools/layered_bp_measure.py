#!/usr/bin/env python3
"""What the box-plus check node costs under the layered schedule, and what the layered schedule buys it (DESIGN.md section
8l, profiles/layered_bp.txt).  The sibling of tools/bp_measure.py for the layered pair.

    python tools/layered_bp_measure.py [--part round|et|all] [--frames 8192] [--reps 5] [--steps 3] [--warmup 2] [--snr 0.0,0.5,1.0]

Code: the BG1-profile QC code at Z = 384 (N = 26112, K = 8448, E = 121344; a PROFILE SURROGATE, codes.py), all-zero codeword.

  round  per round: 20 rounds, early_term = 0, sigma 1.1.  layered_bp against layered on the SAME streaming engine
         (tune ldsp = fused = off), decoders alive in one process, alternating for --reps windows of --steps calls each.
         Both move 16 E bytes per frame-round: per decoder the window times, their median and spread, the TB/s reached;
         the ratio of the medians; per-degree kernel times per launch of one more call timed by HIP events.
  et     against the default layered decoder: early termination, max 20 rounds, polled every 2 rounds, at each --snr
         (sd = 10^(-SNR / 20)): layered_bp (streaming engine, llr_scale = 2 / sd^2), layered with the record kernel the
         library picks by default and offset beta = 0.15 (section 8c), and flooding bp.  Per decoder: ms per batch (median
         and spread of the windows), rounds launched, mean iterations, frame errors."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes

SEED = 20260101
Z = 384
N, K = 68 * Z, 22 * Z

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="all", choices=("round", "et", "all"))
ap.add_argument("--frames", type=int, default=8192)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--snr", default="0.0,0.5,1.0")
args = ap.parse_args()

B = args.frames
rows, cols = codes.nr_bg1_profile_edges(Z)
E = len(rows)
g = L.Graph(rows, cols, N - K, N)
s = torch.cuda.current_stream().cuda_stream
print(json.dumps({"float4_copy_GBs": round(L.capi.hbm_probe(0), 1), "N": N, "K": K, "E": E, "frames": B}), flush=True)


def windows(decs, y):
    """{name: [ms per call of every window]}: the decoders alternate, --reps windows of --steps calls after --warmup"""
    out = {a: torch.empty(L.out_bytes(K, B), dtype=torch.uint8, device="cuda") for a in decs}
    it = {a: torch.empty(B, dtype=torch.int32, device="cuda") for a in decs}
    ms = {a: [] for a in decs}

    def call(a):
        decs[a].decode_device(y.data_ptr(), B, out[a].data_ptr(), out[a].numel(), it[a].data_ptr(), s)

    for _ in range(args.reps):
        for a in decs:
            for _ in range(args.warmup):
                call(a)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call(a)
            torch.cuda.synchronize()
            ms[a].append(round((time.perf_counter() - t0) / args.steps * 1e3, 3))
    return ms, out, it, call


def summary(v):
    return {"ms_windows": v, "ms_median": round(statistics.median(v), 3), "ms_min": min(v), "ms_max": max(v)}


if args.part in ("round", "all"):
    sigma, rounds = 1.1, 20
    y = channel.awgn_device(N, 0, B, sigma, seed=SEED)
    stream = {"ldsp": False, "fused": False}
    decs = {a: L.Decoder(g, K, max_batch=B, algo=a, max_iter=rounds, early_term=False, layer_rows=Z, tune=stream,
                         llr_scale=2.0 / (sigma * sigma)) for a in ("layered", "layered_bp")}
    ms, out, it, call = windows(decs, y)
    res = {"part": "round", "sigma": sigma, "rounds": rounds, "bytes_per_call": 16 * E * B * rounds}
    for a, d in decs.items():
        d.set_timing(True)
        call(a)
        torch.cuda.synchronize()
        kt = d.kernel_times()
        d.set_timing(False)
        r = summary(ms[a])
        r.update(TBs=round(16 * E * B * rounds / (r["ms_median"] * 1e-3) / 1e12, 3),
                 kernels={k["name"]: [k["launches"], round(k["ms_total"] / max(k["launches"], 1), 4),
                                      round(k["bytes_total"] / max(k["ms_total"], 1e-9) / 1e9, 3)] for k in kt if k["phase"] == 2})
        res[a] = r
    res["bp_over_ms_time"] = round(res["layered_bp"]["ms_median"] / res["layered"]["ms_median"], 4)
    print(json.dumps(res), flush=True)
    for d in decs.values():
        d.close()
    del y, out, it
    torch.cuda.empty_cache()

if args.part in ("et", "all"):
    for snr in [float(x) for x in args.snr.split(",")]:
        sd = 10.0 ** (-snr / 20.0)
        scale = 2.0 / (sd * sd)
        y = channel.awgn_device(N, 0, B, sd, seed=SEED)
        common = dict(max_batch=B, max_iter=20, early_term=True, poll_interval=2)
        decs = {"layered_bp": L.Decoder(g, K, algo="layered_bp", layer_rows=Z, llr_scale=scale, **common),
                "layered_offset_default": L.Decoder(g, K, algo="layered", layer_rows=Z, ms_offset=0.15, **common),
                "flooding_bp": L.Decoder(g, K, algo="bp", llr_scale=scale, **common)}
        ms, out, it, call = windows(decs, y)
        res = {"part": "et", "snr_db": snr, "sd": round(sd, 4), "llr_scale": round(scale, 4), "max_iter": 20}
        for a, d in decs.items():
            d.set_timing(True)
            call(a)
            torch.cuda.synchronize()
            st = d.stats()
            names = sorted({k["name"].split("<")[0].split("[")[0] for k in d.kernel_times() if k["name"] != "other"})
            d.set_timing(False)
            r = summary(ms[a])
            r.update(rounds_launched=st["iterations_launched"], mean_iterations=round(float(it[a].float().mean()), 3),
                     frame_errors=int((out[a].view(B, -1) != 0).any(dim=1).sum()), kernels=names)
            res[a] = r
        print(json.dumps(res), flush=True)
        for d in decs.values():
            d.close()
        del y, out, it
        torch.cuda.empty_cache()
