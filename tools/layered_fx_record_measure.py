#!/usr/bin/env python3
"""What the fixed-point record kernel (algo layered_fx with tune fx_record) costs against the
streaming layered engine that runs the same rule and against the fp32 record kernel: the same code, batch and channel
decoded by decoders that live in the same process, alternating, two windows of --steps calls each after warm-up.  The
result lines are printed and written to --out (profiles/layered_fx_record.txt).

    python tools/layered_fx_record_measure.py [--steps 5] [--warmup 2] [--frames 8192] [--z 384,64,128,256] [--out PATH]

Per circulant size of --z, the BG1-profile code (a PROFILE SURROGATE, codes.py), --frames frames, 20 rounds at full work
(early_term = 0), sigma 0.8, q = 6 / p = 8, llr_scale 8, one-LSB offset:
  A  layered_fx on the streaming layered engine (the only way to run the rule without the field)
  B  layered_fx with fx_record: layered_ldsp_fx_kernel
  C  layered, fp32, offset 0.15: layered_ldsp_kernel
and that B's bytes and iteration counts are A's.  Per size also B with ldsp_per_cu = 2 ... 6 forced, beside the plan's own choice,
alternating over two windows as well.  Then one early-termination point: WiMAX (2304, 1152) at Eb/N0 = 2.0 dB, 20 rounds at most."""
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
ap.add_argument("--frames", type=int, default=8192)
ap.add_argument("--z", default="384,64,128,256")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "layered_fx_record.txt"))
args = ap.parse_args()

B = args.frames
s = torch.cuda.current_stream().cuda_stream
lines = [json.dumps({"float4_copy_GBs": round(L.capi.hbm_probe(0), 1), "frames": B, "rounds": ROUNDS, "steps": args.steps,
                     "warmup": args.warmup})]
print(lines[-1], flush=True)
FX = dict(algo="layered_fx", msg_dtype="i8", msg_bits=6, post_bits=8, llr_scale=8.0, ms_offset=1.0)


def timed(d, y, out, it):
    def call():
        d.decode_device(y.data_ptr(), B, out.data_ptr(), out.numel(), it.data_ptr(), s)
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        call()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / args.steps * 1e3, 3)


def launch_names(d, y, out, it):
    d.set_timing(True)                          # one more call, timed per launch (not part of the times above)
    d.decode_device(y.data_ptr(), B, out.data_ptr(), out.numel(), it.data_ptr(), s)
    torch.cuda.synchronize()
    names = sorted({k["name"] for k in d.kernel_times() if k["phase"] == 2})
    d.set_timing(False)
    return names if len(names) <= 2 else names[:2] + ["... %d names" % len(names)]


def compare(label, g, N, K, common, y, sweep):
    """A, B and C alternating over two windows; B's output against A's; with `sweep`, B at forced workgroups per CU"""
    kw = {"A": dict(FX), "B": dict(FX, tune={"fx_record": True}), "C": dict(algo="layered", ms_offset=0.15)}
    dec = {m: L.Decoder(g, K, **common, **k) for m, k in kw.items()}
    out = {m: torch.empty(L.out_bytes(K, B), dtype=torch.uint8, device="cuda") for m in dec}
    it = {m: torch.empty(B, dtype=torch.int32, device="cuda") for m in dec}
    res = dict(label, N=N, K=K, ms={m: [] for m in dec})
    for window in range(2):
        for m in dec:                           # alternating
            res["ms"][m].append(timed(dec[m], y, out[m], it[m]))
    res["kernels"] = {m: launch_names(dec[m], y, out[m], it[m]) for m in dec}
    res["B_equals_A"] = bool(torch.equal(out["A"], out["B"]) and torch.equal(it["A"], it["B"]))
    res["frame_errors"] = {m: int((out[m].view(B, -1) != 0).any(dim=1).sum()) for m in dec}
    res["mean_rounds"] = {m: round(float(it[m].float().mean()), 3) for m in dec}
    a, b, c = res["ms"]["A"], res["ms"]["B"], res["ms"]["C"]
    res["A_spread_ms"] = round(max(a) - min(a), 3)
    res["B_below_A_in_both_windows_by_more_than_A_spread"] = bool(all(a[w] - b[w] > max(a) - min(a) for w in range(2)))
    res["B_over_A_time"] = round(min(b) / min(a), 4)
    res["B_over_C_time"] = round(min(b) / min(c), 4)
    for d in dec.values():
        d.close()
    if sweep:                                   # alternating as well: two windows, all forms alive
        forms = {("auto" if k == 0 else str(k)): L.Decoder(g, K, **common, **dict(FX, tune={"fx_record": True, "ldsp_per_cu": k}))
                 for k in (0, 2, 3, 4, 5, 6)}   # 0: the plan's own choice
        res["B_per_cu_ms"] = {k: [] for k in forms}
        for window in range(2):
            for k, d in forms.items():
                res["B_per_cu_ms"][k].append(timed(d, y, out["B"], it["B"]))
        for k, d in forms.items():
            res["B_per_cu_ms"][k].append(launch_names(d, y, out["B"], it["B"])[0])
            d.close()
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)


for i, Z in enumerate(int(v) for v in args.z.split(",")):
    N, K = 68 * Z, 22 * Z
    rows, cols = codes.nr_bg1_profile_edges(Z)
    y = channel.awgn_device(N, 0, B, SIGMA, seed=SEED)
    compare({"code": "bg1-profile", "Z": Z, "E": len(rows), "sigma": SIGMA, "early_term": 0}, L.Graph(rows, cols, N - K, N), N, K,
            dict(max_batch=B, max_iter=ROUNDS, early_term=False, layer_rows=Z), y, sweep=True)
    del y
    torch.cuda.empty_cache()

# early termination: WiMAX (2304, 1152), BPSK at Eb/N0 = 2.0 dB, rate 1/2: sigma^2 = 1 / (2 R 10^(dB / 10))
rate, N = codes.RATE_1_2, 2304
K, M, z = codes.wimax_dims(rate, N)
rows, cols = codes.wimax_edges(rate, N)
sigma = (1.0 / (2 * 0.5 * 10 ** 0.2)) ** 0.5
y = channel.awgn_device(N, 0, B, sigma, seed=SEED)
compare({"code": "wimax(2304,1152)", "Z": z, "E": len(rows), "sigma": round(sigma, 4), "EbN0_dB": 2.0, "early_term": 1},
        L.Graph(rows, cols, M, N), N, K, dict(max_batch=B, max_iter=ROUNDS, early_term=True, layer_rows=z), y, sweep=False)

with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
