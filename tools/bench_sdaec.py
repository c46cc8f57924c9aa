#!/usr/bin/env python3
"""SDAEC throughput on one GPU: one JSON line per batch size (B x 2 s calls per step), printed and appended to ``--out``.

    python tools/bench_sdaec.py [--steps 10] [--warmup 2] [--batches 1,256] [--out profiles/sdaec_bench.jsonl]

ms per step (device-resident buffers, ade_run_device, the captured graph), audio-s/s and RTF.  ~55 MFLOP per frame: 0.5 M for the in / out LSTMs and Linears,
ten CFBs of 4.3 M each (gate / input Linears 0.26 - 0.51 M, convolution 0.38 M, the two cepstral tables 2 x 1.04 M, the cepstral LSTM 0.78 M input + 0.52 M
recurrent, Linear 0.26 M), 10.8 M for the three LSTM layers along time.  The sub-engine reports no per-stage times through ade_kernel_ms: for the device time
of each kernel run one case under the profiler on its own, program after ``--``:
``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_sdaec.py --batches 256 --steps 3 --out /dev/null``.
Seeded weights (weightgen.sdaec_state): the arithmetic does not depend on the values.
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MFLOP_PER_FRAME = 55.0


def main():
    import torch
    from audio_denoiser_onnx_amd import sdaec, weightgen, weights
    from audio_denoiser_onnx_amd.session import InferenceSession
    args = sys.argv[1:]
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 10
    warm = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 2
    batches = [int(b) for b in (args[args.index("--batches") + 1] if "--batches" in args else "1,256").split(",")]
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(REPO, "profiles", "sdaec_bench.jsonl")
    blob = weights.pack_blob(sdaec.state_to_blob_tensors(*weightgen.sdaec_state(0)))
    L = 32000
    sess = InferenceSession(weights=blob, metadata=sdaec.metadata(L), device_id=0)
    T = sess.frames
    with open(out_path, "a") as log:
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
            audio_s = B * L / 16000.0
            line = json.dumps({"model": "sdaec", "batch": B, "seconds_per_row": L / 16000.0, "frames": T, "ms_per_step": round(ms, 3),
                               "audio_s_per_s": round(audio_s / (ms * 1e-3), 1), "rtf": ms * 1e-3 / audio_s,
                               "gflop_per_step": round(MFLOP_PER_FRAME * 1e-3 * T * B, 2),
                               "tflops": round(MFLOP_PER_FRAME * 1e6 * T * B / (ms * 1e-3) / 1e12, 3)})
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()


if __name__ == "__main__":
    main()
