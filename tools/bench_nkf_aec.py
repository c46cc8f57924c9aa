#!/usr/bin/env python3
"""NKF-AEC throughput on one GPU: one JSON line per batch size (B x 2 s calls per step).

    python tools/bench_nkf_aec.py [--steps 20] [--warmup 3] [--batches 1,16,64,256]
    python tools/bench_nkf_aec.py --stream [--steps 20] [--warmup 3] [--streams 1,16,256,1024] [--hops 1,4,62,125] [--out profiles/nkf_aec_stream_bench.jsonl]

ms per step (device-resident buffers, ade_run_device), audio-s/s, RTF and the fraction of the MI355X's 157.3 TFLOP/s fp32 vector rate at ~17.9 kFLOP per (bin, frame) of the Kalman recurrence.
The sub-engine reports no per-stage times through ade_kernel_ms, so there is no per-kernel field: run the tool under
``rocprofv3 --kernel-trace --stats`` for the device time of each kernel (profiles/nkf_aec_b256_kernel_stats.csv).  Seeded weights (tests/golden/nkf_aec_seed0.adew): the arithmetic does not depend on the values.

``--stream``: ms per push of a stateful stream (ade_stream_push_device on device-resident buffers, pushes enqueued back to back, one synchronise at the end) for every
(n_streams, frames_per_push) pair, and from it the number of real-time streams one GPU sustains, n_streams * 16 ms * frames_per_push / push_ms.  One JSON line per
pair, printed and appended to ``--out``.  For the per-kernel device times of one case run it under the profiler on its own, program after ``--``:
``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_nkf_aec.py --stream --streams 256 --hops 125 --out /dev/null``.
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FLOP_PER_BIN_FRAME = 648 + 15552 + 1584 + 100
PEAK = 157.3e12


def stream_main(args):
    import torch
    from audio_denoiser_onnx_amd import nkf_aec
    from audio_denoiser_onnx_amd.session import InferenceSession, StreamingSession
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 20
    warm = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 3
    streams = [int(b) for b in (args[args.index("--streams") + 1] if "--streams" in args else "1,16,256,1024").split(",")]
    hops = [int(b) for b in (args[args.index("--hops") + 1] if "--hops" in args else "1,4,62,125").split(",")]
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(REPO, "profiles", "nkf_aec_stream_bench.jsonl")
    with open(os.path.join(REPO, "tests", "golden", "nkf_aec_seed0.adew"), "rb") as f:
        blob = f.read()
    sess = InferenceSession(weights=blob, metadata=nkf_aec.metadata(32000), device_id=0)
    side = torch.cuda.Stream()
    with open(out_path, "a") as log:
        for S in streams:
            for F in hops:
                P = F * 256
                g = torch.Generator().manual_seed(S * 1000 + F)
                x = (torch.randn(S, 2, P, generator=g) * 3000).round().clamp(-32768, 32767).to(torch.int16).cuda()
                y = torch.empty(S, P, dtype=torch.int16, device="cuda")
                with StreamingSession(sess, S, F) as st:
                    with torch.cuda.stream(side):
                        for _ in range(warm + 1):                  # (the first push of a stream runs one frame less)
                            st.push_device(x, y, stream=side.cuda_stream)
                        side.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(steps):
                            st.push_device(x, y, stream=side.cuda_stream)
                        side.synchronize()
                        ms = (time.perf_counter() - t0) * 1e3 / steps
                flop = FLOP_PER_BIN_FRAME * 513.0 * F * S
                line = json.dumps({"model": "nkf_aec", "mode": "stream", "n_streams": S, "frames_per_push": F, "ms_per_push": round(ms, 4),
                                   "us_per_frame_step": round(ms * 1e3 / F, 2), "realtime_streams": int(S * 16.0 * F / ms), "rtf": ms / (16.0 * F * S),
                                   "frac_fp32_peak": round(flop / (ms * 1e-3) / PEAK, 4)})
                print(line, flush=True)
                log.write(line + "\n")
                log.flush()


def main():
    if "--stream" in sys.argv[1:]:
        return stream_main(sys.argv[1:])
    import torch
    from audio_denoiser_onnx_amd import nkf_aec
    from audio_denoiser_onnx_amd.session import InferenceSession
    args = sys.argv[1:]
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 20
    warm = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 3
    batches = [int(b) for b in (args[args.index("--batches") + 1] if "--batches" in args else "1,16,64,256").split(",")]
    with open(os.path.join(REPO, "tests", "golden", "nkf_aec_seed0.adew"), "rb") as f:
        blob = f.read()
    L = 32000
    sess = InferenceSession(weights=blob, metadata=nkf_aec.metadata(L), device_id=0)
    T = sess.frames
    for B in batches:
        g = torch.Generator().manual_seed(B)
        x = (torch.randn(B, 2 * L, generator=g) * 3000).round().clamp(-32768, 32767).to(torch.int16).cuda()
        y = torch.empty(B, L, dtype=torch.int16, device="cuda")
        sess.reserve(B)
        for _ in range(warm):
            sess.run_device(x, y)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            sess.run_device(x, y)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        flop = FLOP_PER_BIN_FRAME * 513.0 * T * B
        audio_s = B * L / 16000.0
        print(json.dumps({"model": "nkf_aec", "batch": B, "seconds_per_row": L / 16000.0, "ms_per_step": round(ms, 4),
                          "audio_s_per_s": round(audio_s / (ms * 1e-3), 1), "rtf": ms * 1e-3 / audio_s,
                          "gflop_per_step": round(flop / 1e9, 2), "frac_fp32_peak": round(flop / (ms * 1e-3) / PEAK, 4)}), flush=True)


if __name__ == "__main__":
    main()
