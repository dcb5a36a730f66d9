#!/usr/bin/env python3
"""What fixed-point messages (msg_dtype i8) cost against fp8 and fp16: the same code, batch and
channel decoded by an fp16, an fp8, a 6-bit and an 8-bit decoder that live in the same process, alternating, best of two
windows of --steps calls each after warm-up.  The result lines are printed and written to --out
(profiles/fixed_messages.txt).

    python tools/fixed_measure.py [--steps 5] [--warmup 2] [--only NAME] [--frames N] [--out PATH]

Configurations, both on the (64800, 58320) rate-9/10 DVB-S2-profile code (a PROFILE SURROGATE, codes.py), 4096 frames:
  full   flooding min-sum at full work: early_term = 0, 20 rounds, sigma 0.43
  et     bench.py's dvbs2_910_f16: early termination, max 50 rounds, sigma 0.43, polled every 2 rounds
Per decoder: step time, frames per lane, the check / link forms that ran (kernel names), per-kernel time per launch, the
achieved bytes/s of the check and of the variable kernels (ldpc_decoder_kernel_times: bytes moved over time) and of the whole
step on (4 E + N) * msg_size per frame-round -- ldpc_decoder_stats' frame_rounds at early termination -- against the float4
copy rate of the same run (ldpc_hbm_probe_device).  i8 reads c = sq(llr_scale * y): llr_scale 8 at 6 bits, 32 at 8 bits
(the clean value 1 at a quarter of the range)."""
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
# name -> (msg_dtype, msg_bits, llr_scale, bytes per message)
DECODERS = {"f16": ("f16", 0, 8.0, 2), "f8": ("f8", 0, 8.0, 1), "i8q6": ("i8", 6, 8.0, 1), "i8q8": ("i8", 8, 32.0, 1)}

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--only", default=None)
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "fixed_messages.txt"))
args = ap.parse_args()

rows, cols = codes.dvbs2_profile_edges(N, K)
E, B = len(rows), args.frames
g = L.Graph(rows, cols, N - K, N)
copy_gbs = L.capi.hbm_probe(0)
lines = [json.dumps({"float4_copy_GBs": round(copy_gbs, 1), "N": N, "K": K, "E": E, "frames": B})]
print(lines[-1], flush=True)
s = torch.cuda.current_stream().cuda_stream

for name, c in CONFIGS.items():
    if args.only and name != args.only:
        continue
    y = channel.awgn_device(N, 0, B, c["sigma"], seed=SEED)
    out = {m: torch.empty(L.out_bytes(K, B), dtype=torch.uint8, device="cuda") for m in DECODERS}
    it = {m: torch.empty(B, dtype=torch.int32, device="cuda") for m in DECODERS}
    dec = {m: L.Decoder(g, K, max_batch=B, algo="ms", max_iter=c["iters"], early_term=c["early"], msg_dtype=t, msg_bits=bits,
                        llr_scale=scale, poll_interval=c["poll"]) for m, (t, bits, scale, _) in DECODERS.items()}
    res = {"config": name, "max_iter": c["iters"], "early_term": c["early"], "sigma": c["sigma"]}
    for window in range(2):
        for m in DECODERS:                      # alternating: f16, f8, i8q6, i8q8, f16, ...
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
                phase_tbs = {}
                for ph, key in ((0, "check_TBs"), (1, "var_TBs")):
                    moved = sum(k["bytes_moved"] for k in kt if k["phase"] == ph)
                    t_ms = sum(k["ms_total"] for k in kt if k["phase"] == ph)
                    phase_tbs[key] = round(moved / (t_ms * 1e-3) / 1e12, 2) if t_ms > 0 else None
                r.update(rounds=st["iterations_launched"], frame_rounds=int(frame_rounds),
                         link_form=d.link_form(), mean_iterations=round(float(it[m].float().mean()), 3),
                         frame_errors=int((out[m].view(B, -1) != 0).any(dim=1).sum()),
                         message_GBs=round((4 * E + N) * DECODERS[m][3] * frame_rounds / (best * 1e-3) / 1e9, 1),
                         info_gbit_s=round(B * K / (best * 1e-3) / 1e9, 2), **phase_tbs,
                         kernels={k["name"]: [k["launches"], round(k["ms_total"] / max(k["launches"], 1), 4)] for k in kt})
    for m in ("i8q6", "i8q8"):
        res["%s_over_f8_time" % m] = round(min(res[m]["ms_per_call"]) / min(res["f8"]["ms_per_call"]), 4)
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)
    for d in dec.values():
        d.close()
    del y, out, it
    torch.cuda.empty_cache()

with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
