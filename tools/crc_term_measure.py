#!/usr/bin/env python3
"""What CRC-aided early termination (include/ldpc_hip.h: crc_kind / crc_bits) costs and what it saves, on one MI355X.

cost     The extra launch per round (crc_term_kernel), from ldpc_decoder_set_timing: the `ms_other` share per round of a
         decoder with the CRC on against the same decoder with it off, as a fraction of the round time with it off.  Noise
         so strong that no frame stops under either rule within the rounds run, so both decoders launch the same rounds at
         full work.  (a) DVB-S2-profile (64800, 32400), flooding min-sum fp32; (b) DVB-S2-profile (64800, 58320) rate 9/10,
         flooding min-sum with fp16 messages; 4096 frames, CRC24A over all K information bits.
benefit  The device chain of tools/ber_sweep.py --payload random --transport-block A with and without --crc-stop at three
         SNR points per code: mean iterations, frame_rounds, decode milliseconds per batch, the transport-block tally.
         Also the BG1-profile code (Z = 384, K = 8448) under the layered schedule.

One JSON line per measurement.
    python tools/crc_term_measure.py [--parts cost,benefit] [--codes dvbs2_12,dvbs2_910,bg1] [--frames 4096] [--rounds 10]"""
import argparse, json, os, subprocess, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--parts", default="cost,benefit")
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--codes", default="", help="comma-separated first words of the code names (default: all)")
args = ap.parse_args()
parts = args.parts.split(",")
#: name -> (K, message dtype, noise sd at which nothing stops (None: no cost measurement), ber_sweep --code, --algo, SNR points
#: around the waterfall)
CODES = {"dvbs2_12 ms f32": (32400, "f32", 1.1, "dvbs2_12", "ms", "1.5,1.6,2.0"),
         "dvbs2_910 ms f16": (58320, "f16", 0.62, "dvbs2_910", "ms", "7.0,7.3,7.6"),
         "bg1 layered f32": (8448, "f32", None, "bg1", "layered", "-0.5,-0.2,0.0")}
CODES = {k: v for k, v in CODES.items() if not args.codes or k.split()[0] in args.codes.split(",")}
N = 64800

if "cost" in parts:
    import torch
    import myldpccppapi_amd as L
    from myldpccppapi_amd import channel, codes
    B = args.frames
    s = torch.cuda.current_stream().cuda_stream
    for name, (K, msg, sd, _, _, _) in CODES.items():
        if sd is None:
            continue
        rows, cols = codes.dvbs2_profile_edges(N, K)
        g = L.Graph(rows, cols, N - K, N)
        y = channel.awgn_device(N, 0, B, sd, seed=7)
        out = torch.empty(L.out_bytes(K, B), dtype=torch.uint8, device="cuda")
        it = torch.empty(B, dtype=torch.int32, device="cuda")
        res = {}
        for on in (0, 1, 0, 1):                        # interleaved: off, on, off, on
            dec = L.Decoder(g, K, max_batch=B, algo="ms", max_iter=args.rounds, msg_dtype=msg, poll_interval=0,
                            crc_kind=24 * on, crc_bits=K * on, tune={"place": 1, "device_tail": False})
            for _ in range(2):
                dec.decode_device(y.data_ptr(), B, out.data_ptr(), out.numel(), it.data_ptr(), s)
            torch.cuda.synchronize()
            dec.set_timing(True)
            for _ in range(args.steps):
                dec.decode_device(y.data_ptr(), B, out.data_ptr(), out.numel(), it.data_ptr(), s)
            torch.cuda.synchronize()
            st = dec.stats()
            rounds = args.steps * st["iterations_launched"]
            r = {"ms_other_per_round": st["ms_other"] / rounds, "ms_round": (st["ms_check"] + st["ms_var"] + st["ms_other"]) / rounds,
                 "stopped": int((it < args.rounds).sum()) + dec.crc_stops()}      # 0: both decoders did the same work
            res.setdefault(on, []).append(r)
            dec.close()
        off = min(r["ms_round"] for r in res[0])
        d_other = min(r["ms_other_per_round"] for r in res[1]) - min(r["ms_other_per_round"] for r in res[0])
        print(json.dumps({"part": "cost", "code": name, "frames": B, "rounds": args.rounds, "crc_bits": K,
                          "ms_other_per_round_off": [round(r["ms_other_per_round"], 5) for r in res[0]],
                          "ms_other_per_round_on": [round(r["ms_other_per_round"], 5) for r in res[1]],
                          "ms_round_off": [round(r["ms_round"], 4) for r in res[0]], "ms_round_on": [round(r["ms_round"], 4) for r in res[1]],
                          "frames_stopped": sum(r["stopped"] for v in res.values() for r in v),
                          "launch_us": round(1e3 * d_other, 2), "fraction_of_round_off": round(d_other / off, 5)}), flush=True)
        del y, out, it
        torch.cuda.empty_cache()

if "benefit" in parts:
    for name, (K, msg, _, code, algo, snr) in CODES.items():
        for stop in (False, True):
            cmd = [sys.executable, os.path.join(ROOT, "tools", "ber_sweep.py"), "--code", code, "--algo", algo, "--msg-dtype", msg,
                   "--payload", "random", "--transport-block", str(K - 24), "--frames", str(args.frames), "--iters", "50",
                   "--snr=" + snr] + (["--crc-stop"] if stop else [])
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode:
                sys.exit("ber_sweep failed: " + p.stdout[-2000:] + p.stderr[-2000:])
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    print(json.dumps({"part": "benefit", "code": name, "crc_stop": stop, "snr_db": r["snr_db"], "avg_iters": r["avg_iters"],
                                      "frame_rounds": r["frame_rounds"], "decode_ms_per_batch": r["decode_ms_per_batch"],
                                      "fer": r["fer"], "blocks": r["blocks"], "bler": r["bler"], "blocks_crc_failed": r["blocks_crc_failed"],
                                      "blocks_undetected": r["blocks_undetected"], "blocks_parity_only": r["blocks_parity_only"],
                                      "crc_stops": r["crc_stops"]}), flush=True)
