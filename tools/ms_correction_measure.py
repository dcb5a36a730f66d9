"""Normalized / offset min-sum measurements (profiles/ms_correction.txt).
    python tools/ms_correction_measure.py fer
        frame errors of layered min-sum on WiMAX (2304, 1152) rate 1/2, 2048 frames of the seeded device channel,
        20 iterations, plain against several corrections
    python tools/ms_correction_measure.py time <bg1|dvbs2> <algo> <frames> <iters> <f32|f16> <ms_scale> <ms_offset>
        decode time at full work (early termination off) of the BG1-profile code (Z = 384) or the DVB-S2-profile
        rate-9/10 code, median of 5 calls after one warm-up"""
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import json
import time
import numpy as np
import torch
import myldpccppapi_amd as L
from myldpccppapi_amd import channel, codes

what = sys.argv[1]
if what == "fer":
    K, M, z = codes.wimax_dims(codes.RATE_1_2, 2304)
    rows, cols = codes.wimax_edges(codes.RATE_1_2, 2304)
    g = L.Graph(rows, cols, M, 2304)
    for sd in (0.832, 0.81, 0.79):
        y = channel.awgn_device(2304, 0, 2048, sd, seed=20261016).cpu().numpy()
        res = {"sd": sd}
        for scale, offset in ((0.0, 0.0), (0.75, 0.0), (0.8, 0.0), (0.7, 0.0), (0.0, 0.15)):
            dec = L.Decoder(g, K, max_batch=2048, algo="layered", layer_rows=z, max_iter=20, ms_scale=scale, ms_offset=offset)
            out, _ = dec.decode(y)
            dec.close()
            res["%g/%g" % (scale, offset)] = int(np.any(out.reshape(2048, K // 8) != 0, axis=1).sum())
        print(json.dumps(res), flush=True)
else:
    # time: <code> <algo> <frames> <iters> <msg> <scale> <offset>
    code, algo, B, iters, msg, scale, offset = sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), sys.argv[6], float(sys.argv[7]), float(sys.argv[8])
    if code == "bg1":
        Z = 384; N, K, layer = 68 * Z, 22 * Z, Z
        rows, cols = codes.nr_bg1_profile_edges(Z)
    else:
        N, K = 64800, 58320; layer = 0
        rows, cols = codes.dvbs2_profile_edges(N, K)
    g = L.Graph(rows, cols, N - K, N)
    dec = L.Decoder(g, K, max_batch=B, algo=algo, max_iter=iters, layer_rows=layer, msg_dtype=msg,
                    early_term=False, ms_scale=scale, ms_offset=offset)
    y = channel.awgn_device(N, 0, B, 0.5, seed=1)
    out = torch.empty(L.out_bytes(K, B), dtype=torch.uint8, device="cuda")
    ts = []
    for r in range(6):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        dec.decode_device(y.data_ptr(), B, out.data_ptr(), out.numel(), None, None)
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    ts = sorted(ts[1:])
    print(json.dumps({"code": code, "algo": algo, "frames": B, "iters": iters, "msg": msg, "ms_scale": scale,
                      "ms_offset": offset, "median_ms": round(1e3 * ts[len(ts) // 2], 3), "min_ms": round(1e3 * ts[0], 3),
                      "Mbit_s": round(B * K / ts[len(ts) // 2] / 1e6, 1)}), flush=True)
