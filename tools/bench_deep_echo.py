#!/usr/bin/env python3
"""Deep Echo AEC throughput on one GPU: one JSON line per batch size and repeat (B x 2 s calls per step), printed and appended to ``--out``.

    python tools/bench_deep_echo.py [--steps 10] [--warmup 2] [--batches 1,256] [--repeats 2] [--sdaec] [--out profiles/deep_echo_bench.jsonl]
    python tools/bench_deep_echo.py --reference [--threads 16]        (CPU only, where the reference tree is present: its eager fp32 forward of one 2 s clip)

ms per step (device-resident buffers, ade_run_device, the captured graph), audio-s/s and RTF.  ~20 MFLOP per frame: 0.5 M for the in / out LSTMs and the in-Linear,
two CFBs of 4.3 M each (see tools/bench_sdaec.py), 10.8 M for the three LSTM layers along time, 0.27 M for the echo path and its ten taps.  ``--sdaec`` measures
SDAEC on the same shape in the same process (the yardstick for a family without a parent-commit number).  The sub-engine reports no per-stage times through
ade_kernel_ms: for the device time of each kernel run one case under the profiler on its own, program after ``--``:
``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_deep_echo.py --batches 256 --steps 3 --repeats 1 --out /dev/null``.
Seeded weights (weightgen.deep_echo_state): the arithmetic does not depend on the values.
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MFLOP_PER_FRAME = {"deep_echo": 20.2, "sdaec": 55.0}
L = 32000


def reference_cpu(threads):
    """The reference's eager fp32 forward of one 2 s clip on the CPU (the export's own default length)."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import make_golden_deep_echo as gold
    torch.set_num_threads(threads)
    model, _ = gold.build(gold.import_namespace(L), 0)
    rng = np.random.default_rng(1)
    near, far = (np.round(rng.standard_normal(L) * 700).astype(np.int16) for _ in range(2))
    gold.run(model, near, far)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        gold.run(model, near, far)
        times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"model": "deep_echo", "what": "reference eager fp32 forward, one 2 s clip", "cpu_threads": threads, "ms_min": round(min(times), 1),
                      "ms_max": round(max(times), 1)}))


def main():
    args = sys.argv[1:]
    if "--reference" in args:
        return reference_cpu(int(args[args.index("--threads") + 1]) if "--threads" in args else 16)
    import torch
    from audio_denoiser_onnx_amd import deep_echo, sdaec, weightgen, weights
    from audio_denoiser_onnx_amd.session import InferenceSession
    steps = int(args[args.index("--steps") + 1]) if "--steps" in args else 10
    warm = int(args[args.index("--warmup") + 1]) if "--warmup" in args else 2
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 2
    batches = [int(b) for b in (args[args.index("--batches") + 1] if "--batches" in args else "1,256").split(",")]
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(REPO, "profiles", "deep_echo_bench.jsonl")
    sessions = [("deep_echo", InferenceSession(weights=weights.pack_blob(deep_echo.state_to_blob_tensors(weightgen.deep_echo_state(0))),
                                               metadata=deep_echo.metadata(L), device_id=0))]
    if "--sdaec" in args:
        sessions.append(("sdaec", InferenceSession(weights=weights.pack_blob(sdaec.state_to_blob_tensors(*weightgen.sdaec_state(0))), metadata=sdaec.metadata(L),
                                                   device_id=0)))
    with open(out_path, "a") as log:
        for B in batches:
            g = torch.Generator().manual_seed(B)
            x = (torch.randn(B, 2 * L, generator=g) * 700).round().clamp(-32768, 32767).to(torch.int16).cuda()
            y = torch.empty(B, L, dtype=torch.int16, device="cuda")
            for name, sess in sessions:
                T = sess.frames
                sess.reserve(B)
                for rep in range(repeats):
                    for _ in range(warm):
                        sess.run_device(x, y)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        sess.run_device(x, y)
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t0) * 1e3 / steps
                    audio_s = B * L / 16000.0
                    line = json.dumps({"model": name, "batch": B, "repeat": rep, "seconds_per_row": L / 16000.0, "frames": T, "ms_per_step": round(ms, 3),
                                       "audio_s_per_s": round(audio_s / (ms * 1e-3), 1), "rtf": ms * 1e-3 / audio_s,
                                       "gflop_per_step": round(MFLOP_PER_FRAME[name] * 1e-3 * T * B, 2),
                                       "tflops": round(MFLOP_PER_FRAME[name] * 1e6 * T * B / (ms * 1e-3) / 1e12, 3)})
                    print(line, flush=True)
                    log.write(line + "\n")
                    log.flush()


if __name__ == "__main__":
    main()
