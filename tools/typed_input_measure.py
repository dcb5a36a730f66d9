#!/usr/bin/env python3
"""What int8 / fp16 channel values buy a host caller (profiles/typed_input.txt).

    python tools/typed_input_measure.py [--part gpu|loss] [--calls 3] [--frames 4096] [--groups 3] [--out profiles/typed_input.txt]

Everything on the (64800, 58320) rate-9/10 DVB-S2-profile code (a PROFILE SURROGATE, codes.py), fp16 messages, early
termination, max 50 rounds, sigma 0.43, polled every 2 rounds: bench.py's dvbs2_910_f16.
  host   (--part gpu) ldpc_decode / ldpc_decode_typed on pageable host buffers, PCIe included, --groups x --frames frames per
         call in launch groups of --frames, f32, f16 and i8 input through ONE handle in the same process, alternating, best
         and median of --calls calls; frame errors of each; the device-resident time of one launch group next to it
  init   (--part gpu) a handle that runs one round without early termination: its "other" spans are init_kernel + the
         state launch and one syndrome launch, so the difference between the input types is the init kernel's
  loss   (--part loss, CPU only) WiMAX (2304, 1152), 1.6 dB, BP restated in numpy (tests/bp_ref.py), 20 rounds: frame
         errors with f32 input and with int8 input at four units
Each part appends its lines to --out."""
import argparse, json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes

SEED = 20260101
N, K = 64800, 58320
SIGMA, ITERS, POLL = 0.43, 50, 2
UNITS = {"f32": 1.0, "f16": 1.0 / 256, "i8": 1.0 / 32}          # +-127 / 32 = +-3.97: the clamp sits beyond 1 + 6 sigma

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "typed_input.txt"))
ap.add_argument("--groups", type=int, default=3)
ap.add_argument("--part", choices=("gpu", "loss"), default="gpu")
args = ap.parse_args()
lines = []


def emit(d):
    s = json.dumps(d)
    print(s, flush=True)
    lines.append(s)


if args.part == "gpu":
    import torch
    DT = {"f16": torch.float16, "i8": torch.int8}
    rows, cols = codes.dvbs2_profile_edges(N, K)
    B, F = args.frames, args.frames * args.groups                  # frames per launch group, per host call
    g = L.Graph(rows, cols, N - K, N)
    s = torch.cuda.current_stream().cuda_stream
    emit({"code": "dvbs2_910 profile", "N": N, "K": K, "frames_per_call": F, "max_batch": B, "sigma": SIGMA, "max_iter": ITERS, "msg_dtype": "f16", "units": UNITS})

    # ---- inputs: one float batch, quantised on the device, copied to pageable host memory --------------------------------
    y = channel.awgn_device(N, 0, F, SIGMA, seed=SEED)
    dev = {"f32": y}
    for k in ("f16", "i8"):
        q = torch.empty((F, N), dtype=DT[k], device="cuda")
        L.quantize_device(y.data_ptr(), y.numel(), k, UNITS[k], q.data_ptr(), 0, s)
        dev[k] = q
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in dev.items()}                # pageable
    nb = L.out_bytes(K, B)
    dec = L.Decoder(g, K, max_batch=B, algo="ms", max_iter=ITERS, early_term=True, msg_dtype="f16", poll_interval=POLL)

    # ---- host path ---------------------------------------------------------------------------------------------------------
    times = {k: [] for k in host}
    errs = {}
    for call in range(args.calls + 1):                                  # the first round of calls is warm-up
        for k in ("f32", "f16", "i8"):
            t0 = time.perf_counter()
            out, iters = dec.decode(host[k], llr_unit=None if k == "f32" else UNITS[k])
            dt = (time.perf_counter() - t0) * 1e3
            if call:
                times[k].append(dt)
            errs[k] = int(np.count_nonzero(out.reshape(F, K // 8).any(axis=1)))
    dev_ms = {}
    o = torch.empty(nb, dtype=torch.uint8, device="cuda")
    it = torch.empty(B, dtype=torch.int32, device="cuda")
    for k in ("f32", "f16", "i8"):
        best = 1e9
        for call in range(args.calls + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.decode_device(dev[k].data_ptr(), B, o.data_ptr(), nb, it.data_ptr(), s,
                              **({} if k == "f32" else dict(llr_type=k, llr_unit=UNITS[k])))
            torch.cuda.synchronize()
            if call:
                best = min(best, (time.perf_counter() - t0) * 1e3)
        dev_ms[k] = best
    base = min(times["f32"])
    for k in ("f32", "f16", "i8"):
        emit({"host_path": k, "unit": UNITS[k], "input_MB": round(host[k].nbytes / 1e6, 1), "best_ms": round(min(times[k]), 2),
              "median_ms": round(float(np.median(times[k])), 2), "ratio_to_f32_host": round(min(times[k]) / base, 3),
              "device_resident_ms": round(dev_ms[k], 2), "frame_errors": errs[k], "info_Gbit_s": round(F * K / min(times[k]) / 1e6, 2)})

    # where the int8 call's time goes: the same call from memory the caller page-locked (no staging threads: direct copies),
    # and one launch group alone (its copy and its decode overlap nothing)
    pinned = torch.from_numpy(host["i8"]).pin_memory()
    for name, arr, fr in (("i8_pinned_direct", pinned.numpy(), F), ("i8_one_group", host["i8"][:B], B), ("f32_one_group", host["f32"][:B], B)):
        best = 1e9
        for call in range(args.calls + 1):
            t0 = time.perf_counter()
            dec.decode(arr, llr_unit=None if name.startswith("f32") else UNITS["i8"])
            if call:
                best = min(best, (time.perf_counter() - t0) * 1e3)
        emit({"host_path": name, "frames": fr, "best_ms": round(best, 2)})
    dec.close()

    # ---- init kernels alone: a second handle that runs ONE round without early termination, so that "other" is init + state + the last syndrome only
    dec1 = L.Decoder(g, K, max_batch=B, algo="ms", max_iter=1, early_term=False, msg_dtype="f16")
    for k in ("f32", "f16", "i8"):
        dec1.set_timing(True)
        for _ in range(5):
            dec1.decode_device(dev[k].data_ptr(), B, o.data_ptr(), nb, it.data_ptr(), s,
                               **({} if k == "f32" else dict(llr_type=k, llr_unit=UNITS[k])))
        torch.cuda.synchronize()
        dec1.stats()
        other = [t for t in dec1.kernel_times() if t["name"] == "other"]
        dec1.set_timing(False)
        emit({"one_round_handle": k, "other_ms_per_call": round(other[0]["ms_total"] / 5, 4) if other else None,
              "other_spans_per_call": other[0]["launches"] / 5 if other else None, "init_bytes_in": B * N * {"f32": 4, "f16": 2, "i8": 1}[k],
              "init_bytes_out": B * N * 2 + 2 * B * (len(rows)) })
    dec1.close()


# ---- quantisation loss on the CPU restatement --------------------------------------------------------------------------
if args.part == "loss":
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bp_ref as RB
    import typed_input_ref as T
    from ms_correction_ref import Code
    Nw = 2304
    Kw, Mw, zw = codes.wimax_dims(codes.RATE_1_2, Nw)
    r, c = codes.wimax_edges(codes.RATE_1_2, Nw)
    code = Code(r, c, Mw, Nw, Kw)
    sd = 10.0 ** (-1.6 / 20.0)
    frames = 400
    yw = channel.awgn_frames(Nw, 0, frames, sd, seed=SEED)
    scale = 2.0 / (sd * sd)

    def fer(v):
        w = RB.flood(code, v, 20, llr_scale=scale)
        return int(np.count_nonzero(w["hard"][:, :Kw].any(axis=1)))

    emit({"loss": "f32", "code": "wimax (2304, 1152)", "snr_db": 1.6, "frames": frames, "rounds": 20, "frame_errors": fer(yw)})
    for unit in (1.0 / 64, 1.0 / 32, 1.0 / 16, 1.0 / 8):
        x = T.quantize(yw, unit, "i8")
        emit({"loss": "i8", "unit": unit, "clamp_at": round(127 * unit, 3), "frame_errors": fer(T.dequantize(x, unit)),
              "clamped_values": int(np.count_nonzero(np.abs(x) == 127))})

with open(args.out, "a") as f:
    f.write("# tools/typed_input_measure.py --part %s --calls %d --frames %d --groups %d   (one JSON line per measurement)\n" % (
        args.part, args.calls, args.frames, args.groups))
    f.write("\n".join(lines) + "\n")
