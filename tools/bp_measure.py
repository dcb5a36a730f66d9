#!/usr/bin/env python3
"""What the box-plus check node costs over min-sum's (profiles/bp_messages.txt): the same code, batch
and channel decoded by a min-sum and a BP decoder that live in the same process, alternating, best of two windows of
--steps calls each after warm-up.

    python tools/bp_measure.py [--steps 5] [--warmup 2] [--only NAME] [--frames N] [--tune JSON]

Codes: the (64800, 32400) rate-1/2 and the (64800, 58320) rate-9/10 DVB-S2-profile codes (PROFILE SURROGATES, codes.py),
4096 frames, fp32 and fp16 messages each:
  full   full work: early_term = 0, 20 rounds
  et     early termination, max 50 rounds, polled every 2 rounds
at 2.0 dB (rate 1/2) and sigma 0.43 (rate 9/10).  Min-sum reads y, BP reads llr_scale * y with llr_scale = 2 / sigma^2.
Per decoder: step time, frames per lane, the check / link forms that ran (kernel names), per-kernel time per launch, mean
iterations and frame errors, and the achieved bytes/s on (4 E + N) * msg_size per frame-round -- ldpc_decoder_stats'
frame_rounds at early termination -- against the float4 copy rate of the same run (ldpc_hbm_probe_device).  The ratio
reported is BP's time over min-sum's in the same run.  --tune applies to the BP decoder only (form experiments)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes

SEED = 20260101
N = 64800
CODES = {"r12": dict(K=32400, sigma=10.0 ** (-2.0 / 20.0)), "r910": dict(K=58320, sigma=0.43)}
MODES = {"full": dict(iters=20, early=False, poll=0), "et": dict(iters=50, early=True, poll=2)}
MSG_SIZE = {"f32": 4, "f16": 2}

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--only", default=None, help="comma-separated parts of a configuration name, e.g. r910,et,f16")
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--tune", default=None, help="JSON tuning fields for the BP decoder")
args = ap.parse_args()

B = args.frames
copy_gbs = L.capi.hbm_probe(0)
print(json.dumps({"float4_copy_GBs": round(copy_gbs, 1), "N": N, "frames": B}), flush=True)
s = torch.cuda.current_stream().cuda_stream

for cname, cc in CODES.items():
    K = cc["K"]
    rows, cols = codes.dvbs2_profile_edges(N, K)
    E = len(rows)
    g = L.Graph(rows, cols, N - K, N)
    y = channel.awgn_device(N, 0, B, cc["sigma"], seed=SEED)
    scale = 2.0 / (cc["sigma"] * cc["sigma"])
    for mname, c in MODES.items():
        for msg in ("f32", "f16"):
            name = "%s_%s_%s" % (cname, mname, msg)
            if args.only and not all(p in name.split("_") for p in args.only.split(",")):
                continue
            out = {a: torch.empty(L.out_bytes(K, B), dtype=torch.uint8, device="cuda") for a in ("ms", "bp")}
            it = {a: torch.empty(B, dtype=torch.int32, device="cuda") for a in ("ms", "bp")}
            dec = {a: L.Decoder(g, K, max_batch=B, algo=a, max_iter=c["iters"], early_term=c["early"], msg_dtype=msg,
                                poll_interval=c["poll"], llr_scale=scale if a == "bp" else 8.0,
                                tune=json.loads(args.tune) if (args.tune and a == "bp") else None) for a in ("ms", "bp")}
            res = {"config": name, "K": K, "E": E, "max_iter": c["iters"], "early_term": c["early"], "sigma": round(cc["sigma"], 4),
                   "llr_scale": round(scale, 4)}
            for window in range(2):
                for a in ("ms", "bp"):                       # alternating: ms, bp, ms, bp
                    d = dec[a]

                    def call():
                        d.decode_device(y.data_ptr(), B, out[a].data_ptr(), out[a].numel(), it[a].data_ptr(), s)

                    for _ in range(args.warmup):
                        call()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        call()
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t0) / args.steps * 1e3
                    r = res.setdefault(a, {"ms_per_call": []})
                    r["ms_per_call"].append(round(ms, 3))
                    if window == 1:
                        # one more, timed per launch (the events are not part of the step times above)
                        d.set_timing(True)
                        call()
                        torch.cuda.synchronize()
                        st, kt = d.stats(), d.kernel_times()
                        d.set_timing(False)
                        frame_rounds = st["frame_rounds"] if c["early"] else B * c["iters"]
                        best = min(r["ms_per_call"])
                        r.update(rounds=st["iterations_launched"], frame_rounds=int(frame_rounds),
                                 link_form=d.link_form(), mean_iterations=round(float(it[a].float().mean()), 3),
                                 frame_errors=int((out[a].view(B, -1) != 0).any(dim=1).sum()),
                                 message_GBs=round((4 * E + N) * MSG_SIZE[msg] * frame_rounds / (best * 1e-3) / 1e9, 1),
                                 info_gbit_s=round(B * K / (best * 1e-3) / 1e9, 2),
                                 kernels={k["name"]: [k["launches"], round(k["ms_total"] / max(k["launches"], 1), 4)] for k in kt})
            res["bp_over_ms_time"] = round(min(res["bp"]["ms_per_call"]) / min(res["ms"]["ms_per_call"]), 4)
            print(json.dumps(res), flush=True)
            for d in dec.values():
                d.close()
            del out, it
            torch.cuda.empty_cache()
    del y
    torch.cuda.empty_cache()
