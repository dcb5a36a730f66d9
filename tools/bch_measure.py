#!/usr/bin/env python3
"""Times the outer-code kernels (ldpc_bch_encode_device, ldpc_bch_decode_device) on 4096 frames of the two DVB-S2-profile
shapes -- (m, t, n) = (16, 12, 32400) and (16, 8, 58320), rows of n / 8 bytes -- next to the yardstick: ldpc_tb_check_device
(tb_check_kernel: the same walk with two 24-bit registers) on the same bytes in the same process, taken as one code block
of K = n bits per transport block.

Cases: encode; decode with every frame clean; decode with 1 % of the frames dirty (one wrong bit each, every hundredth
frame); decode with every frame dirty at weight t.  Per call: HIP-event time, median and minimum of 20 after 3 warm-up
calls, the ratio to the yardstick's median, and the time as a share of the LDPC decode of the batch (7.7 ms at
rate 9/10 with fp16 messages, 41 - 48 ms at rate 1/2).  The decoded payload and status are checked against what was
planted.  One JSON line per measurement.

    python tools/bch_measure.py [--frames 4096]"""
import argparse, json, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
import myldpccppapi_amd as L

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=4096)
args = ap.parse_args()
SHAPES = {"rate_1_2": dict(t=12, n=32400, ldpc_ms=(41.0, 48.0)), "rate_9_10": dict(t=8, n=58320, ldpc_ms=(7.7, 7.7))}


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


stream = torch.cuda.current_stream().cuda_stream
frames = args.frames
for name, shape in SHAPES.items():
    t, n = shape["t"], shape["n"]
    code = L.BchCode(n, t)
    kb, nb = code.k // 8, n // 8
    pay = torch.randint(0, 256, (frames, kb), dtype=torch.uint8, device="cuda")
    rows = torch.empty((frames, nb), dtype=torch.uint8, device="cuda")
    back = torch.empty_like(pay)
    status = torch.empty(frames, dtype=torch.int32, device="cuda")
    code.encode_device(pay.data_ptr(), frames, rows.data_ptr(), rows.numel(), stream)
    torch.cuda.synchronize()
    # the yardstick on the same bytes: one code block of n bits, no CRC expected to pass, flags only and with the payload copy
    tb = L.TransportBlock(n - 24, n, C=1, tb_crc=24, cb_crc=0)
    tb_pay = torch.empty((frames, (n - 24) // 8), dtype=torch.uint8, device="cuda")
    cb_ok = torch.empty(frames, dtype=torch.uint8, device="cuda")
    tb_ok = torch.empty(frames, dtype=torch.uint8, device="cuda")
    yard, yard_min = event_ms(lambda: tb.check_device(rows.data_ptr(), frames, tb_pay.data_ptr(), cb_ok.data_ptr(), tb_ok.data_ptr(), stream))

    def report(what, call, moved):
        med, fastest = event_ms(call)
        lo, hi = shape["ldpc_ms"]
        print(json.dumps({"shape": name, "m": code.m, "t": t, "n": n, "k": code.k, "frames": frames, "call": what, "ms_median": round(med, 4),
                          "ms_min": round(fastest, 4), "bytes_moved": moved, "gbs": round(moved / med / 1e6, 1),
                          "ratio_to_tb_check": round(med / yard, 2),
                          "share_of_ldpc_decode": [round(med / hi, 4), round(med / lo, 4)]}), flush=True)

    print(json.dumps({"shape": name, "n": n, "frames": frames, "call": "tb_check_kernel payload+cb_ok+tb_ok (yardstick)",
                      "ms_median": round(yard, 4), "ms_min": round(yard_min, 4)}), flush=True)
    report("encode", lambda: code.encode_device(pay.data_ptr(), frames, rows.data_ptr(), rows.numel(), stream), pay.numel() + rows.numel())
    decode = lambda src: code.decode_device(src.data_ptr(), frames, back.data_ptr(), status.data_ptr(), stream)
    report("decode, all clean", lambda: decode(rows), rows.numel() + pay.numel() + 4 * frames)
    torch.cuda.synchronize()
    assert bool((back == pay).all()) and not bool(status.any())
    report("decode, all clean, status only", lambda: code.decode_device(rows.data_ptr(), frames, None, status.data_ptr(), stream),
           rows.numel() + 4 * frames)
    rng = np.random.default_rng(1)
    some = rows.clone()
    dirty = torch.arange(0, frames, 100, device="cuda")
    some[dirty, 17] ^= 4
    report("decode, 1 % dirty (weight 1)", lambda: decode(some), rows.numel() + pay.numel() + 4 * frames)
    torch.cuda.synchronize()
    assert bool((back == pay).all()) and int(status.sum()) == len(dirty) and int(status.max()) == 1
    every = rows.cpu().numpy().copy()
    for f in range(frames):
        for b in rng.choice(n, t, replace=False):
            every[f, b >> 3] ^= 1 << (b & 7)
    every = torch.from_numpy(every).cuda()
    report("decode, all dirty (weight t)", lambda: decode(every), rows.numel() + pay.numel() + 4 * frames)
    torch.cuda.synchronize()
    assert bool((back == pay).all()) and bool((status == t).all())
    junk = torch.randint(0, 256, (frames, nb), dtype=torch.uint8, device="cuda")
    report("decode, all hopeless (random rows)", lambda: decode(junk), rows.numel() + pay.numel() + 4 * frames)
    torch.cuda.synchronize()
    assert bool((status == -1).all()) and bool((back == junk[:, :kb]).all())
    del pay, rows, back, status, some, every, junk, tb_pay, cb_ok, tb_ok
    torch.cuda.empty_cache()
