#!/usr/bin/env python3
"""What soft output costs (profiles/soft_output.txt): the same decoder's plain call against its soft
call, per call (wall clock over the timed steps) and per round (ldpc_decoder_set_timing: the soft_settle_kernel span and,
on a code with column-fused rows, the check_link kernel that now stores the fused columns' R).

    python tools/soft_output_measure.py [--steps 5] [--warmup 2] [--only NAME] [--frames N]

Configurations:
  dvbs2_12_et    (64800, 32400) min-sum fp32, 4096 frames, early termination at 2.0 dB, 50 iterations, polled every 2 rounds
  dvbs2_12_full  the same at full work (early_term = 0)
  dvbs2_910_f16  (64800, 58320) min-sum fp16, 4096 frames, sigma 0.43 (bench.py: dvbs2_910_f16)
  bg1_layered    BG1-profile Z = 384 layered record kernel, 8192 frames, sigma 1.1 (bench.py: bg1_layered)
Orientation: at full work a soft call adds one pass of about msg * (E + N) + 4 N bytes per frame to max_iter * (16 E + 4 N);
with early termination it adds the fused columns' stores in every round plus that pass over the lines of the settling frames.
The DVB-S2 / BG1 codes are PROFILE SURROGATES (codes.py)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes

SEED = 20260101
CONFIGS = {
    "dvbs2_12_et": dict(code=(64800, 32400), frames=4096, algo="ms", msg="f32", iters=50, sigma=10.0 ** (-2.0 / 20.0), early=True, poll=2),
    "dvbs2_12_full": dict(code=(64800, 32400), frames=4096, algo="ms", msg="f32", iters=50, sigma=10.0 ** (-2.0 / 20.0), early=False, poll=0),
    "dvbs2_910_f16": dict(code=(64800, 58320), frames=4096, algo="ms", msg="f16", iters=50, sigma=0.43, early=True, poll=2),
    "bg1_layered": dict(code="bg1", frames=8192, algo="layered", msg="f32", iters=20, sigma=1.1, early=True, poll=0),
}

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--only", default=None)
ap.add_argument("--frames", type=int, default=0, help="override the batch size (smaller boxes)")
args = ap.parse_args()

for name, c in CONFIGS.items():
    if args.only and name != args.only:
        continue
    if c["code"] == "bg1":
        Z = 384
        rows, cols = codes.nr_bg1_profile_edges(Z)
        N, K, M, layer = 68 * Z, 22 * Z, 46 * Z, Z
    else:
        N, K = c["code"]
        rows, cols = codes.dvbs2_profile_edges(N, K)
        M, layer = N - K, 0
    B = args.frames or c["frames"]
    g = L.Graph(rows, cols, M, N)
    dec = L.Decoder(g, K, max_batch=B, algo=c["algo"], max_iter=c["iters"], early_term=c["early"], layer_rows=layer,
                    msg_dtype=c["msg"], poll_interval=c["poll"])
    y = channel.awgn_device(N, 0, B, c["sigma"], seed=SEED)
    out = torch.empty(L.out_bytes(K, B), dtype=torch.uint8, device="cuda")
    it = torch.empty(B, dtype=torch.int32, device="cuda")
    soft = torch.empty(B * N, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(with_soft):
        if with_soft:
            dec.decode_device(y.data_ptr(), B, out.data_ptr(), out.numel(), it.data_ptr(), s, soft_ptr=soft.data_ptr(),
                              soft_floats=soft.numel(), soft="posterior")
        else:
            dec.decode_device(y.data_ptr(), B, out.data_ptr(), out.numel(), it.data_ptr(), s)

    res = {"config": name, "frames": B, "N": N, "E": len(rows), "max_iter": c["iters"], "early_term": c["early"]}
    for with_soft in (False, True, False, True):           # interleaved: plain, soft, plain, soft
        for _ in range(args.warmup):
            call(with_soft)
        torch.cuda.synchronize()
        dec.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call(with_soft)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        st = dec.stats()
        kt = dec.kernel_times()
        dec.set_timing(False)
        key = "soft" if with_soft else "plain"
        res.setdefault(key + "_ms_per_call", []).append(round(ms, 3))
        res[key + "_rounds"] = st["iterations_launched"]
        res[key + "_kernels"] = {k["name"]: [k["launches"] // args.steps, round(k["ms_total"] / max(k["launches"], 1), 4)] for k in kt}
    p, q = min(res["plain_ms_per_call"]), min(res["soft_ms_per_call"])
    res["soft_over_plain"] = round(q / p, 4)
    print(json.dumps(res), flush=True)
    dec.close()
    del y, out, it, soft
    torch.cuda.empty_cache()
