#!/usr/bin/env python3
"""UL-UNAS throughput on one MI355X (seeded reference-architecture weights from the golden fixture, synthetic PCM resident in HBM).

    python tools/bench_ulunas.py [--batches 64,256,1024] [--steps 10]
    python tools/bench_ulunas.py --stream [--steps 20] [--warmup 5] [--reps 5] [--shapes 256x62,1024x2,1024x8,1024x62,1x2] [--out profiles/ulunas_stream_bench.jsonl]

``--stream``: ms per push of a stateful stream (ade_stream_push_device on device-resident buffers, a caller's stream, ``--steps`` pushes enqueued back to back,
one synchronise at the end; mean and spread over ``--reps`` such windows after a warm-up) for every n_streams x hops-per-push shape, next to the one-shot
ade_process_device call on the same audio in the same process, timed the same way (n_streams rows of 256 x hops samples), the real-time streams one GPU sustains,
n_streams * 16 ms * hops / push_ms, and the kernel launches of one push (a count of the launch sequence, the same for every shape).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.chdir(REPO)

import torch  # noqa: E402

from audio_denoiser_onnx_amd import ulunas  # noqa: E402
from audio_denoiser_onnx_amd.session import InferenceSession  # noqa: E402
from audio_denoiser_onnx_amd.weights import pack_blob  # noqa: E402


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


def launches_per_push():
    """analysis + feature kernel + per block (its convolutions + time attention, frequency attention, apply) + 2 x 4 DPGRNN + mask + synthesis + output"""
    convs = {0: 1, 1: 2, 2: 3}
    return 1 + 1 + sum(convs[p[1]] + 3 for p in ulunas.block_plan()) + 2 * 4 + 1 + 1 + 1


def stream_main(args):
    from audio_denoiser_onnx_amd.session import StreamingSession
    opt = lambda k, d: args[args.index(k) + 1] if k in args else d      # noqa: E731
    steps, warm, reps = int(opt("--steps", 20)), int(opt("--warmup", 5)), int(opt("--reps", 5))
    shapes = [tuple(int(v) for v in sh.split("x")) for sh in str(opt("--shapes", "256x62,1024x2,1024x8,1024x62,1x2")).split(",")]
    out_path = opt("--out", os.path.join(REPO, "profiles", "ulunas_stream_bench.jsonl"))
    z = np.load(os.path.join(REPO, "tests", "golden", "ulunas_seed0.npz"))
    blob = pack_blob(ulunas.fold_state_dict({str(k): z["w:" + str(k)] for k in z["keys"]}))
    side = torch.cuda.Stream()
    with open(out_path, "a") as log:
        for S, F in shapes:
            P = F * 256
            g = torch.Generator().manual_seed(S * 1000 + F)
            x = (torch.randn(S, P, generator=g) * 3000).round().clamp(-32768, 32767).to(torch.int16).cuda()
            y = torch.empty(S, P, dtype=torch.int16, device="cuda")
            with InferenceSession(weights=blob, metadata=ulunas.metadata(P), device_id=0) as sess:
                yo = torch.empty(S, sess.row_out, dtype=torch.int16, device="cuda")
                sess.reserve(S)
                with torch.cuda.stream(side):
                    o_ms, o_sd = timed(lambda: sess.run_device(x, yo, stream=side.cuda_stream), side.synchronize, warm, reps, steps)
                    with StreamingSession(sess, S, F) as st:
                        ms, sd = timed(lambda: st.push_device(x, y, stream=side.cuda_stream), side.synchronize, warm, reps, steps)
            d = {"model": "ul_unas", "mode": "stream", "n_streams": S, "frames_per_push": F, "ms_per_push": round(ms, 4), "ms_std": round(sd, 4), "us_per_hop": round(ms * 1e3 / F, 2),
                 "realtime_streams": int(S * 16.0 * F / ms), "rtf": ms / (16.0 * F * S), "launches_per_push": launches_per_push(), "oneshot_batch": S, "oneshot_length": P,
                 "oneshot_ms": round(o_ms, 4), "oneshot_ms_std": round(o_sd, 4), "ratio_to_oneshot": round(ms / o_ms, 4)}
            line = json.dumps(d)
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,256,1024")
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    z = np.load(os.path.join(REPO, "tests", "golden", "ulunas_seed0.npz"))
    fused = ulunas.fold_state_dict({str(k): z["w:" + str(k)] for k in z["keys"]})
    sess = InferenceSession(weights=pack_blob(fused), metadata=ulunas.metadata(16000))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    for B in [int(x) for x in a.batches.split(",")]:
        pcm = torch.from_numpy((np.random.default_rng(B).standard_normal((B, sess.row_in)) * 3000).astype(np.int16)).to(dev)
        out = torch.empty((B, sess.row_out), dtype=torch.int16, device=dev)
        sess.reserve(B)
        with torch.cuda.stream(stream):
            sess.run_device(pcm, out, stream=stream.cuda_stream)
            stream.synchronize()
            t = time.perf_counter()
            for _ in range(a.steps):
                sess.run_device(pcm, out, stream=stream.cuda_stream)
            stream.synchronize()
            ms = (time.perf_counter() - t) / a.steps * 1e3
        print(f"B={B:5d} x 1 s: {ms:9.3f} ms/step  {B / (ms * 1e-3):10.0f} audio-s/s  RTF {ms * 1e-3 / B:.2e}", flush=True)


if __name__ == "__main__":
    if "--stream" in sys.argv[1:]:
        stream_main(sys.argv[1:])
    else:
        main()
