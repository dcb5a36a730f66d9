#!/usr/bin/env python3
"""Times ordered-statistics decoding (ldpc_osd_device) on the 802.16e codes (576, 288) and (1152, 576) and, for the
dirty frames alone, on the BG1-profile test code (1088, M = 736: the most rows and the largest LDS footprint).

Per code: 1000 frames that are all dirty (the all-zero codeword in noise of sd 0.9, as LLR-like values) at orders 0 and 1 --
milliseconds per 1000 dirty frames -- and a batch of 4096 frames at a frame error rate near 5 % behind 20 rounds of min-sum
(the noise level is searched for on the device): the OSD call of that batch, its flag pass alone (a batch with every frame
clean) and the batch's own decode (ldpc_decode_soft_device).  HIP events on the calling stream, 3 warm-up calls, then the
median and the minimum of 20.  One JSON line per measurement.

    python tools/osd_measure.py"""
import json, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes


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
    return round(float(np.median(times)), 4), round(float(min(times)), 4)


stream = torch.cuda.current_stream().cuda_stream
for N in (576, 1152, 1088):
    if N == 1088:
        K, M, z = 22 * 16, 46 * 16, 16
        rows, cols = codes.nr_bg1_profile_edges(z)
    else:
        K, M, z = codes.wimax_dims(0, N)
        rows, cols = codes.wimax_edges(0, N)
    g = L.Graph(rows, cols, M, N)
    B = 4096
    osd = L.Osd(g, K, max_frames=B)
    info = osd.info()
    out = torch.empty(B * K // 8, dtype=torch.uint8, device="cuda")
    status = torch.empty(B, dtype=torch.int32, device="cuda")

    def run(soft, frames, order):
        osd.run_device(soft.data_ptr(), frames, order, 256.0, out.data_ptr(), out.numel(), None, status.data_ptr(), None, stream)

    # ---- 1000 dirty frames
    y = channel.awgn_device(N, 0, 1000, 0.9, seed=7) * 4.0
    for order in (0, 1):
        med, fastest = event_ms(lambda: run(y, 1000, order))
        torch.cuda.synchronize()
        print(json.dumps({"code": [N, K], "case": "1000 dirty frames", "order": order, "dirty": int((status[:1000] > 0).sum()),
                          "flipped": int((status[:1000] == 2).sum()), "ms_median": med, "ms_min": fastest, "lds_bytes": info["lds_bytes"]}), flush=True)

    if N == 1088:
        osd.close()
        continue

    # ---- a batch of 4096 frames near 5 % frame errors behind 20 rounds of min-sum
    dec = L.Decoder(g, K, max_batch=B, algo="ms", max_iter=20, layer_rows=z)
    soft = torch.empty((B, N), dtype=torch.float32, device="cuda")
    dout = torch.empty(B * K // 8, dtype=torch.uint8, device="cuda")

    def decode(llr):
        dec.decode_device(llr.data_ptr(), B, dout.data_ptr(), dout.numel(), None, stream, soft_ptr=soft.data_ptr(), soft_floats=soft.numel())

    best = None
    for sd in np.arange(0.60, 0.90, 0.01):
        llr = channel.awgn_device(N, 0, B, float(sd), seed=11)
        decode(llr)
        fer = channel.count_errors_device(dout, None, B)[2] / B
        if best is None or abs(fer - 0.05) < abs(best[1] - 0.05):
            best = (float(sd), fer)
    llr = channel.awgn_device(N, 0, B, best[0], seed=11)
    dec_med, dec_min = event_ms(lambda: decode(llr))
    for order in (0, 1):
        med, fastest = event_ms(lambda: run(soft, B, order))
        torch.cuda.synchronize()
        after = channel.count_errors_device(out, None, B)[2]
        print(json.dumps({"code": [N, K], "case": "4096 frames behind min-sum", "sd": round(best[0], 2), "order": order,
                          "frame_errors_before": int(round(best[1] * B)), "frame_errors_after": after, "dirty": int((status > 0).sum()),
                          "flipped": int((status == 2).sum()), "osd_ms_median": med, "osd_ms_min": fastest, "decode_ms_median": dec_med,
                          "decode_ms_min": dec_min, "osd_share_of_decode": round(med / dec_med, 3)}), flush=True)
    clean = torch.full((B, N), 4.0, dtype=torch.float32, device="cuda")
    med, fastest = event_ms(lambda: run(clean, B, 1))
    print(json.dumps({"code": [N, K], "case": "4096 clean frames (flag pass, idle workgroups)", "ms_median": med, "ms_min": fastest}), flush=True)
    dec.close()
    osd.close()
