#!/usr/bin/env python3
"""DFSMN-AEC throughput on one GPU, next to its own NKF stage: JSON lines, printed and appended to ``--out`` (default profiles/dfsmn_aec_bench.jsonl).

    python tools/bench_dfsmn_aec.py [--steps 10] [--warmup 3] [--reps 5] [--calls 128,1] [--tables reference,exact] [--skip-nkf] [--out FILE]
    python tools/bench_dfsmn_aec.py --stream [--steps 20] [--warmup 10] [--reps 5] [--streams 1,16,256,1024] [--hops 1,5,62,125] [--tables reference,exact] [--skip-nkf]
                                    [--out profiles/dfsmn_aec_stream_bench.jsonl]

Each case is a folded export of 2 windows of 1.5 s (24000 samples) per call, ``--calls`` calls per step on device-resident buffers (ade_run_device): 128 calls
are 256 windows.  For every case the same number of windows and samples is also timed through ``nkf_aec`` (the linear canceller alone, 24000-sample calls), in
the same process, and the ratio of the two is written as a third line.  Timing: ``--warmup`` untimed steps, then ``--reps`` repetitions of ``--steps`` steps
each; the mean and the standard deviation over the repetitions are reported.  The sub-engine reports no per-stage times, so for the device time of each kernel
run one case under the profiler on its own, program after ``--``:
``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_dfsmn_aec.py --calls 128 --tables reference --reps 1 --skip-nkf --out /dev/null``.
Seeded weights (tests/golden): the arithmetic does not depend on the values.

``--stream``: ms per push of a stateful stream (ade_stream_push_device on device-resident buffers, a caller's stream, pushes enqueued back to back, one synchronise
at the end) for every (n_streams, frames_per_push) pair and table mode, the ``nkf_aec`` stream of the same shape in the same process as the yardstick, their
ratio, and the real-time streams one GPU sustains, n_streams * 16 ms * frames_per_push / push_ms.  The mask frames a push completes follow a pattern of period
five pushes (frames_per_push = 1: 1, 1, 1, 1, 0), so ``--steps`` and ``--warmup`` are rounded up to multiples of 5 and a repetition is a whole number of periods; the mean and the standard deviation over
``--reps`` repetitions of ``--steps`` pushes are reported, as in the one-shot mode.
For the per-kernel device times of one case run it under the profiler on its own:
``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_dfsmn_aec.py --stream --streams 256 --hops 125 --tables reference --skip-nkf --out /dev/null``.
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

W, N_WIN = 24000, 2


def timed(fn, sync, warm, reps, steps):
    for _ in range(warm):
        fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / steps)
    return float(np.mean(out)), float(np.std(out))


def stream_main(args):
    import torch
    from audio_denoiser_onnx_amd import dfsmn_aec, nkf_aec
    from audio_denoiser_onnx_amd.session import InferenceSession, StreamingSession
    opt = lambda k, d: args[args.index(k) + 1] if k in args else d
    up5 = lambda n: -(-int(n) // 5) * 5
    steps, warm, reps = up5(opt("--steps", 20)), up5(opt("--warmup", 10)), int(opt("--reps", 5))
    streams = [int(b) for b in str(opt("--streams", "1,16,256,1024")).split(",")]
    hops = [int(b) for b in str(opt("--hops", "1,5,62,125")).split(",")]
    tables = str(opt("--tables", "reference,exact")).split(",")
    out_path = opt("--out", os.path.join(REPO, "profiles", "dfsmn_aec_stream_bench.jsonl"))
    gold = os.path.join(REPO, "tests", "golden")
    with open(os.path.join(gold, "dfsmn_aec_seed0.adew"), "rb") as f:
        blob = f.read()
    with open(os.path.join(gold, "nkf_aec_seed0.adew"), "rb") as f:
        nkf_blob = f.read()
    sessions = [] if "--skip-nkf" in args else [("nkf_aec", None, InferenceSession(weights=nkf_blob, metadata=nkf_aec.metadata(32000), device_id=0))]
    sessions += [("dfsmn_aec", tb, InferenceSession(weights=blob, metadata=dfsmn_aec.metadata(32000, use_batch_fold=False, dft_tables=tb), device_id=0)) for tb in tables]
    side = torch.cuda.Stream()

    def push_ms(sess, x, y, S, F):
        with StreamingSession(sess, S, F) as st:
            with torch.cuda.stream(side):
                return timed(lambda: st.push_device(x, y, stream=side.cuda_stream), side.synchronize, warm, reps, steps)

    with open(out_path, "a") as log:
        for S in streams:
            for F in hops:
                P = F * 256
                g = torch.Generator().manual_seed(S * 1000 + F)
                x = (torch.randn(S, 2, P, generator=g) * 3000).round().clamp(-32768, 32767).to(torch.int16).cuda()     # the two families only differ in which row is which
                y = torch.empty(S, P, dtype=torch.int16, device="cuda")
                n_ms = 0.0
                for model, tb, sess in sessions:
                    ms, sd = push_ms(sess, x, y, S, F)
                    d = {"model": model, "mode": "stream", "n_streams": S, "frames_per_push": F, "ms_per_push": round(ms, 4), "ms_std": round(sd, 4), "us_per_hop": round(ms * 1e3 / F, 2),
                         "realtime_streams": int(S * 16.0 * F / ms), "rtf": ms / (16.0 * F * S)}
                    if model == "nkf_aec":
                        n_ms = ms
                    else:
                        d["dft_tables"] = tb
                        if n_ms > 0.0:
                            d["ratio_to_nkf_aec_stream"] = round(ms / n_ms, 4)
                    line = json.dumps(d)
                    print(line, flush=True)
                    log.write(line + "\n")
                    log.flush()


def main():
    if "--stream" in sys.argv[1:]:
        return stream_main(sys.argv[1:])
    import torch
    from audio_denoiser_onnx_amd import dfsmn_aec, nkf_aec
    from audio_denoiser_onnx_amd.session import InferenceSession
    args = sys.argv[1:]
    opt = lambda k, d: args[args.index(k) + 1] if k in args else d
    steps, warm, reps = int(opt("--steps", 10)), int(opt("--warmup", 3)), int(opt("--reps", 5))
    calls = [int(c) for c in str(opt("--calls", "128,1")).split(",")]
    tables = str(opt("--tables", "reference,exact")).split(",")
    out_path = opt("--out", os.path.join(REPO, "profiles", "dfsmn_aec_bench.jsonl"))
    gold = os.path.join(REPO, "tests", "golden")
    with open(os.path.join(gold, "dfsmn_aec_seed0.adew"), "rb") as f:
        blob = f.read()
    with open(os.path.join(gold, "nkf_aec_seed0.adew"), "rb") as f:
        nkf_blob = f.read()
    nkf = InferenceSession(weights=nkf_blob, metadata=nkf_aec.metadata(W), device_id=0)
    sync = torch.cuda.synchronize
    with open(out_path, "a") as log:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
        for C in calls:
            windows = C * N_WIN
            g = torch.Generator().manual_seed(C)
            xn = (torch.randn(windows, 2 * W, generator=g) * 3000).round().clamp(-32768, 32767).to(torch.int16).cuda()
            yn = torch.empty(windows, nkf.out_len, dtype=torch.int16, device="cuda")
            audio_s = windows * W / 16000.0
            n_ms = 0.0
            if "--skip-nkf" not in args:
                nkf.reserve(windows)
                n_ms, n_sd = timed(lambda: nkf.run_device(xn, yn), sync, warm, reps, steps)
                emit({"model": "nkf_aec", "windows": windows, "samples_per_window": W, "ms_per_step": round(n_ms, 4), "ms_std": round(n_sd, 4),
                      "audio_s_per_s": round(audio_s / (n_ms * 1e-3), 1)})
            for tb in tables:
                sess = InferenceSession(weights=blob, metadata=dfsmn_aec.metadata(N_WIN * W, use_batch_fold=True, dft_tables=tb), device_id=0)
                assert sess.in_len == N_WIN * W
                x = xn.reshape(C, 2 * N_WIN * W)              # the same samples; the two families only differ in which channel is which
                y = torch.empty(C, sess.out_len, dtype=torch.int16, device="cuda")
                sess.reserve(C)
                ms, sd = timed(lambda: sess.run_device(x, y), sync, warm, reps, steps)
                emit({"model": "dfsmn_aec", "dft_tables": tb, "calls": C, "windows": windows, "samples_per_window": W, "ms_per_step": round(ms, 4), "ms_std": round(sd, 4),
                      "audio_s_per_s": round(audio_s / (ms * 1e-3), 1), "rtf": ms * 1e-3 / audio_s})
                if n_ms > 0.0:
                    emit({"ratio": "dfsmn_aec / nkf_aec", "dft_tables": tb, "windows": windows, "value": round(ms / n_ms, 4)})
                sess.close()


if __name__ == "__main__":
    main()
