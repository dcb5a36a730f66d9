#!/usr/bin/env python3
"""What the correction table of the fixed-point layered box-plus decoder (algo layered_bp_fx) costs over
layered_fx's min-sum row at equal bytes: the same code, batch and channel decoded by decoders that live in the same process,
alternating, best of two windows of --steps calls each after warm-up -- the windows of tools/layered_fixed_measure.py.  The
result lines are printed and written to --out (profiles/layered_bp_fixed.txt).

    python tools/layered_bp_fixed_measure.py [--steps 5] [--warmup 2] [--frames 8192] [--z 384] [--out PATH]

BG1-profile code (a PROFILE SURROGATE, codes.py) at circulant size --z, --frames frames, 20 rounds at full work
(early_term = 0), sigma 0.8:
  bpfx     layered_bp_fx, q = 6 / p = 8 / f = 2, llr_scale = 4 * 2 / sigma^2 (the LLR in quarter units), automatic tile width
  fx       layered_fx, q = 6 / p = 8, the same llr_scale, plain min-sum: the yardstick, the same 6 E bytes per frame-round
  bp       layered_bp, fp32, the streaming engine, llr_scale = 2 / sigma^2: 16 E bytes per frame-round
Per decoder: ms per batch, bytes/s on its bytes per edge, the per-degree kernel times of one more call with timing on, frame
errors; then per row degree the time of the box-plus kernel over the min-sum kernel, and the float4 copy rate of the same
run (ldpc_hbm_probe_device)."""
import argparse, json, os, re, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes

SEED = 20260101
ROUNDS, SIGMA = 20, 0.8

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--frames", type=int, default=8192)
ap.add_argument("--z", type=int, default=384)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "layered_bp_fixed.txt"))
args = ap.parse_args()

Z, B = args.z, args.frames
N, K = 68 * Z, 22 * Z
rows, cols = codes.nr_bg1_profile_edges(Z)
E = len(rows)
g = L.Graph(rows, cols, N - K, N)
copy_gbs = L.capi.hbm_probe(0)
lines = [json.dumps({"float4_copy_GBs": round(copy_gbs, 1), "N": N, "K": K, "E": E, "Z": Z, "frames": B, "rounds": ROUNDS, "sigma": SIGMA})]
print(lines[-1], flush=True)
s = torch.cuda.current_stream().cuda_stream
y = channel.awgn_device(N, 0, B, SIGMA, seed=SEED)

llr = 2.0 / SIGMA ** 2
common = dict(max_batch=B, max_iter=ROUNDS, early_term=False, layer_rows=Z)
widths = dict(msg_dtype="i8", msg_bits=6, post_bits=8, llr_scale=4.0 * llr)
# name -> (decoder keywords, bytes per edge and frame-round that its rule moves)
DECODERS = {
    "bpfx": (dict(widths, algo="layered_bp_fx", bp_frac_bits=2), 6),
    "fx": (dict(widths, algo="layered_fx"), 6),
    "bp": (dict(algo="layered_bp", llr_scale=llr), 16),
}
dec = {m: L.Decoder(g, K, **common, **kw) for m, (kw, _) in DECODERS.items()}
out = torch.empty(L.out_bytes(K, B), dtype=torch.uint8, device="cuda")
it = torch.empty(B, dtype=torch.int32, device="cuda")
res = {}
for window in range(2):
    for m in DECODERS:                          # alternating
        d = dec[m]

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
            d.set_timing(True)                  # one more, timed per launch (the events are not part of the times above)
            call()
            torch.cuda.synchronize()
            kt = d.kernel_times()
            d.set_timing(False)
            best, per_edge = min(r["ms_per_batch"]), DECODERS[m][1]
            r.update(spread_ms=round(max(r["ms_per_batch"]) - min(r["ms_per_batch"]), 3),
                     frame_errors=int((out.view(B, -1) != 0).any(dim=1).sum()),
                     info_gbit_s=round(B * K / (best * 1e-3) / 1e9, 2),
                     edge_TBs=round(per_edge * E * B * ROUNDS / (best * 1e-3) / 1e12, 3),
                     kernels={k["name"]: [k["launches"], round(k["ms_total"] / max(k["launches"], 1), 4),
                                          round(k["bytes_total"] / (k["ms_total"] * 1e-3) / 1e12, 2) if k["ms_total"] > 0 else None]
                              for k in kt})


def per_degree(m):
    """{row degree: ms per launch} of the layer kernels of decoder m"""
    t = {}
    for name, (_, ms, _) in res[m]["kernels"].items():
        k = re.match(r"layer_kernel<\w+,(\d+),\d+>", name)
        if k:
            t[int(k.group(1))] = ms
    return t


fx_t, bpfx_t, bp_t = per_degree("fx"), per_degree("bpfx"), per_degree("bp")
res["bpfx_over_fx_time"] = round(min(res["bpfx"]["ms_per_batch"]) / min(res["fx"]["ms_per_batch"]), 4)
res["bpfx_over_bp_time"] = round(min(res["bpfx"]["ms_per_batch"]) / min(res["bp"]["ms_per_batch"]), 4)
res["bpfx_over_fx_by_degree"] = {d: round(bpfx_t[d] / fx_t[d], 3) for d in sorted(fx_t) if d in bpfx_t and fx_t[d] > 0}
res["bpfx_over_bp_by_degree"] = {d: round(bpfx_t[d] / bp_t[d], 3) for d in sorted(bp_t) if d in bpfx_t and bp_t[d] > 0}
lines.append(json.dumps(res))
print(lines[-1], flush=True)
for d in dec.values():
    d.close()
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
