#!/usr/bin/env python3
"""What a round of hard-decision bit flipping (algo bitflip) costs against the streaming flooding
min-sum decoders: the same code, batch and channel decoded by decoders that live in the same process, alternating, best of
two windows of --steps calls each after warm-up.  The result lines are printed and written to --out (profiles/bitflip.txt).

    python tools/bitflip_measure.py [--steps 5] [--warmup 2] [--out PATH]

Per code -- 802.16e (2304, 1152) at 65 536 frames, the DVB-S2-profile (64800, 32400) code (a PROFILE SURROGATE, codes.py) at
4096 frames --, 20 rounds at full work (early_term = 0), sigma 0.8:
  bitflip   algo bitflip, default thresholds
  ms        algo ms, fp32, streaming kernels (layer_rows 0), first allocations (tune place = 1: no placement search)
  msi6      the same with msg_dtype i8, msg_bits 6, llr_scale 8
Per decoder: ms per batch and per round, and from one more call with timing on the per-kernel times and the bytes/s of the
algorithmic bytes (bitflip, per 64 frames and round: check 8 (E + M), vote 8 (E + 2 N), flip 8 (E + 3 N)) next to the float4
copy rate of the same run (ldpc_hbm_probe_device).
Then frame errors of bitflip against fp32 offset min-sum (ms_offset 0.15) on (2304, 1152), 65 536 frames of the all-zero
codeword, 20 rounds with early termination, the same noise, at Eb/N0 = 2, 6 and 8 dB (rate 1/2 BPSK: Eb/N0 = 1 / sd^2):
what soft information buys on this code -- a hard-decision decoder against a soft one, not two of a kind."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes

SEED = 20260101
ROUNDS, SIGMA = 20, 0.8

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bitflip.txt"))
args = ap.parse_args()

copy_gbs = L.capi.hbm_probe(0)
lines = [json.dumps({"float4_copy_GBs": round(copy_gbs, 1), "rounds": ROUNDS, "sigma": SIGMA})]
print(lines[-1], flush=True)
s = torch.cuda.current_stream().cuda_stream

DECODERS = {
    "bitflip": dict(algo="bitflip"),
    "ms": dict(algo="ms", tune={"place": 1}),
    "msi6": dict(algo="ms", msg_dtype="i8", msg_bits=6, llr_scale=8.0, tune={"place": 1}),
}


def measure(name, rows, cols, N, K, B):
    E, M = len(rows), N - K
    g = L.Graph(rows, cols, M, N)
    y = channel.awgn_device(N, 0, B, SIGMA, seed=SEED)
    out = torch.empty(L.out_bytes(K, B), dtype=torch.uint8, device="cuda")
    it = torch.empty(B, dtype=torch.int32, device="cuda")
    dec = {m: L.Decoder(g, K, max_batch=B, max_iter=ROUNDS, early_term=False, **kw) for m, kw in DECODERS.items()}
    res = {"code": name, "N": N, "K": K, "E": E, "frames": B}
    for window in range(2):
        for m, d in dec.items():                # alternating
            def call():
                d.decode_device(y.data_ptr(), B, out.data_ptr(), out.numel(), it.data_ptr(), s)

            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call()
            torch.cuda.synchronize()
            r = res.setdefault(m, {"ms_per_batch": []})
            r["ms_per_batch"].append(round((time.perf_counter() - t0) / args.steps * 1e3, 3))
            if window == 1:
                d.set_timing(True)              # one more, timed per launch (the events are not part of the times above)
                call()
                torch.cuda.synchronize()
                kt = d.kernel_times()
                d.set_timing(False)
                best = min(r["ms_per_batch"])
                r.update(ms_per_round=round(best / ROUNDS, 4), spread_ms=round(max(r["ms_per_batch"]) - best, 3),
                         kernels={k["name"]: [k["launches"], round(k["ms_total"] / max(k["launches"], 1), 4),
                                              round(k["bytes_total"] / (k["ms_total"] * 1e-3) / 1e9, 1) if k["ms_total"] > 0 else None]
                                  for k in kt})
                if m == "bitflip":
                    rounds = [k for k in kt if k["name"].startswith("bitflip_")]
                    ms, by = sum(k["ms_total"] for k in rounds), sum(k["bytes_total"] for k in rounds)
                    r.update(round_kernels_ms=round(ms / ROUNDS, 4), round_GBs=round(by / (ms * 1e-3) / 1e9, 1),
                             round_over_copy=round(by / (ms * 1e-3) / 1e9 / copy_gbs, 4), bytes_per_round=by // ROUNDS)
    for m in ("ms", "msi6"):
        res["%s_over_bitflip_time" % m] = round(min(res[m]["ms_per_batch"]) / min(res["bitflip"]["ms_per_batch"]), 2)
    for d in dec.values():
        d.close()
    return res


K, M, z = codes.wimax_dims(codes.RATE_1_2, 2304)
wrows, wcols = codes.wimax_edges(codes.RATE_1_2, 2304)
lines.append(json.dumps(measure("wimax:0:2304", wrows, wcols, 2304, K, 65536)))
print(lines[-1], flush=True)
drows, dcols = codes.dvbs2_profile_edges(64800, 32400)
lines.append(json.dumps(measure("dvbs2_12 (profile surrogate)", drows, dcols, 64800, 32400, 4096)))
print(lines[-1], flush=True)

# hard decision against soft decision: the same noise through both, early termination on
B, N = 65536, 2304
g = L.Graph(wrows, wcols, M, N)
out = torch.empty(L.out_bytes(K, B), dtype=torch.uint8, device="cuda")
it = torch.empty(B, dtype=torch.int32, device="cuda")
pair = {"bitflip": L.Decoder(g, K, max_batch=B, max_iter=ROUNDS, algo="bitflip"),
        "ms_offset_0.15": L.Decoder(g, K, max_batch=B, max_iter=ROUNDS, algo="ms", ms_offset=0.15, tune={"place": 1})}
gap = {"what": "frame errors, hard-decision bit flipping against fp32 offset min-sum, same noise", "code": "wimax:0:2304",
       "frames": B, "rounds": ROUNDS, "points": []}
for ebn0 in (2.0, 6.0, 8.0):
    sd = 10.0 ** (-ebn0 / 20.0)
    y = channel.awgn_device(N, 0, B, sd, seed=SEED + 1)
    point = {"eb_n0_db": ebn0, "sd": round(sd, 4), "hard_decision_bit_error_rate": round(float((y < 0).float().mean()), 5)}
    for m, d in pair.items():
        d.decode_device(y.data_ptr(), B, out.data_ptr(), out.numel(), it.data_ptr(), s)
        torch.cuda.synchronize()
        point[m] = {"frame_errors": int((out.view(B, -1) != 0).any(dim=1).sum()), "avg_iters": round(float(it.float().mean()), 2)}
    gap["points"].append(point)
for d in pair.values():
    d.close()
lines.append(json.dumps(gap))
print(lines[-1], flush=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
