#!/usr/bin/env python3
"""What fp8 (E4M3) messages buy over fp16 (profiles/fp8_messages.txt): the same code, batch and
channel decoded by an fp16 and an fp8 decoder that live in the same process, alternating, best of two windows of
--steps calls each after warm-up.

    python tools/fp8_measure.py [--steps 5] [--warmup 2] [--only NAME] [--frames N] [--tune JSON]

Configurations, both on the (64800, 58320) rate-9/10 DVB-S2-profile code (a PROFILE SURROGATE, codes.py), 4096 frames:
  full   flooding min-sum at full work: early_term = 0, 20 rounds, sigma 0.43
  et     bench.py's dvbs2_910_f16: early termination, max 50 rounds, sigma 0.43, polled every 2 rounds
Per decoder: step time, frames per lane, the check / link forms that ran (kernel names), per-kernel time per launch, and the
achieved bytes/s on (4 E + N) * msg_size per frame-round -- ldpc_decoder_stats' frame_rounds at early termination -- against
the float4 copy rate of the same run (ldpc_hbm_probe_device).  --tune applies to the fp8 decoder only (form experiments)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes

SEED = 20260101
N, K = 64800, 58320
CONFIGS = {
    "full": dict(iters=20, sigma=0.43, early=False, poll=0),
    "et": dict(iters=50, sigma=0.43, early=True, poll=2),
}
MSG_SIZE = {"f32": 4, "f16": 2, "f8": 1}

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--only", default=None)
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--tune", default=None, help="JSON tuning fields for the fp8 decoder")
ap.add_argument("--fpl", type=int, default=0, help="frames per lane of the fp8 decoder (0: automatic)")
args = ap.parse_args()

rows, cols = codes.dvbs2_profile_edges(N, K)
E, B = len(rows), args.frames
g = L.Graph(rows, cols, N - K, N)
copy_gbs = L.capi.hbm_probe(0)
print(json.dumps({"float4_copy_GBs": round(copy_gbs, 1), "N": N, "K": K, "E": E, "frames": B}), flush=True)
s = torch.cuda.current_stream().cuda_stream

for name, c in CONFIGS.items():
    if args.only and name != args.only:
        continue
    y = channel.awgn_device(N, 0, B, c["sigma"], seed=SEED)
    out = {m: torch.empty(L.out_bytes(K, B), dtype=torch.uint8, device="cuda") for m in ("f16", "f8")}
    it = {m: torch.empty(B, dtype=torch.int32, device="cuda") for m in ("f16", "f8")}
    dec = {m: L.Decoder(g, K, max_batch=B, algo="ms", max_iter=c["iters"], early_term=c["early"], msg_dtype=m,
                        poll_interval=c["poll"], frames_per_lane=args.fpl if m == "f8" else 0,
                        tune=json.loads(args.tune) if (args.tune and m == "f8") else None) for m in ("f16", "f8")}
    res = {"config": name, "max_iter": c["iters"], "early_term": c["early"], "sigma": c["sigma"]}
    for window in range(2):
        for m in ("f16", "f8"):                      # alternating: f16, f8, f16, f8
            d = dec[m]

            def call():
                d.decode_device(y.data_ptr(), B, out[m].data_ptr(), out[m].numel(), it[m].data_ptr(), s)

            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / args.steps * 1e3
            r = res.setdefault(m, {"ms_per_call": []})
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
                         link_form=d.link_form(), mean_iterations=round(float(it[m].float().mean()), 3),
                         frame_errors=int((out[m].view(B, -1) != 0).any(dim=1).sum()),
                         message_GBs=round((4 * E + N) * MSG_SIZE[m] * frame_rounds / (best * 1e-3) / 1e9, 1),
                         info_gbit_s=round(B * K / (best * 1e-3) / 1e9, 2),
                         kernels={k["name"]: [k["launches"], round(k["ms_total"] / max(k["launches"], 1), 4)] for k in kt})
    res["f8_over_f16_time"] = round(min(res["f8"]["ms_per_call"]) / min(res["f16"]["ms_per_call"]), 4)
    print(json.dumps(res), flush=True)
    for d in dec.values():
        d.close()
    del y, out, it
    torch.cuda.empty_cache()
