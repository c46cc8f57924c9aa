#!/usr/bin/env python3
"""DFSMN throughput on one MI355X (informational; BASELINE.json has no DFSMN configuration): batch x 2 s chunks @ 48 kHz,
int16 PCM resident in HBM, steps enqueued back to back on one stream.

    python tools/bench_dfsmn.py
    python tools/bench_dfsmn.py --stream [--steps 20] [--warmup 5] [--reps 5] [--shapes 1024x1,1024x5,1024x50,256x100,1x1] [--out profiles/dfsmn_stream_bench.jsonl]

``--stream``: ms per push of a stateful stream (ade_stream_push_device on device-resident buffers, a caller's stream, ``--steps`` pushes enqueued back to back,
one synchronise at the end; mean and spread over ``--reps`` such windows after a warm-up) for every n_streams x hops-per-push shape, next to the one-shot
ade_process_device call on the same amount of audio in the same process, timed the same way: n_streams rows of 960 x hops samples (one-hop pushes: half as many
rows of one 1920-sample frame, the shortest call there is; 1 x 1 has no such call and is given next to one row of one frame, twice its audio), and the real-time
streams one GPU sustains, n_streams * 20 ms * hops / push_ms.  Kernel times come from a run of their own:
``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_dfsmn.py --stream --shapes 256x100 --out /dev/null``."""
import json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.chdir(REPO)
import numpy as np
import torch
from audio_denoiser_onnx_amd.metadata import build_audio_metadata
from audio_denoiser_onnx_amd.session import InferenceSession



def dfsmn_meta(length):
    return build_audio_metadata(producer="bench_dfsmn", model_name="DFSMN", task="denoise", model_family="dfsmn", input_audio_length=length,
                                in_sample_rate=48000, nfft=1920, window_length=1920, hop_length=960, window_type="hamming",
                                center_pad=False, pad_mode="constant", feature_kind="kaldi_fbank_stft")


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
    from audio_denoiser_onnx_amd.session import StreamingSession
    opt = lambda k, d: args[args.index(k) + 1] if k in args else d
    steps, warm, reps = int(opt("--steps", 20)), int(opt("--warmup", 5)), int(opt("--reps", 5))
    shapes = [tuple(int(v) for v in sh.split("x")) for sh in str(opt("--shapes", "1024x1,1024x5,1024x50,256x100,1x1")).split(",")]
    out_path = opt("--out", os.path.join(REPO, "profiles", "dfsmn_stream_bench.jsonl"))
    with open(os.path.join("tests", "golden", "dfsmn_seed0.adew"), "rb") as f:
        blob = f.read()
    side = torch.cuda.Stream()
    with open(out_path, "a") as log:
        for S, F in shapes:
            P = F * 960
            g = torch.Generator().manual_seed(S * 1000 + F)
            x = (torch.randn(S, P, generator=g) * 1500).round().clamp(-32768, 32767).to(torch.int16).cuda()
            y = torch.empty(S, P, dtype=torch.int16, device="cuda")
            B, L = (S, P) if F >= 2 else (max(1, S // 2), 1920)            # the one-shot call on the same amount of audio (1 x 1: one frame, twice the audio)
            with InferenceSession(weights=blob, metadata=dfsmn_meta(L), device_id=0) as sess:
                xo = (torch.randn(B, L, generator=g) * 1500).round().clamp(-32768, 32767).to(torch.int16).cuda()
                yo = torch.empty(B, sess.out_len, dtype=torch.int16, device="cuda")
                with torch.cuda.stream(side):
                    o_ms, o_sd = timed(lambda: sess.run_device(xo, yo, stream=side.cuda_stream), side.synchronize, warm, reps, steps)
                    with StreamingSession(sess, S, F) as st:
                        ms, sd = timed(lambda: st.push_device(x, y, stream=side.cuda_stream), side.synchronize, warm, reps, steps)
            d = {"model": "dfsmn", "mode": "stream", "n_streams": S, "frames_per_push": F, "ms_per_push": round(ms, 4), "ms_std": round(sd, 4), "us_per_hop": round(ms * 1e3 / F, 2),
                 "realtime_streams": int(S * 20.0 * F / ms), "rtf": ms / (20.0 * F * S), "oneshot_batch": B, "oneshot_length": L, "oneshot_ms": round(o_ms, 4),
                 "oneshot_ms_std": round(o_sd, 4), "oneshot_same_audio": B * L == S * P, "ratio_to_oneshot": round(ms / o_ms, 4)}
            line = json.dumps(d)
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()


if "--stream" in sys.argv[1:]:
    stream_main(sys.argv[1:])
    sys.exit(0)

L = 96000
meta = build_audio_metadata(producer="bench_dfsmn", model_name="DFSMN", task="denoise", model_family="dfsmn", input_audio_length=L,
                            in_sample_rate=48000, nfft=1920, window_length=1920, hop_length=960, window_type="hamming",
                            center_pad=False, pad_mode="constant", feature_kind="kaldi_fbank_stft")
with open(os.path.join("tests", "golden", "dfsmn_seed0.adew"), "rb") as f:
    blob = f.read()
sess = InferenceSession(weights=blob, metadata=meta)
for B in (8, 64, 256):
    x = torch.from_numpy((np.random.default_rng(0).standard_normal((B, L)) * 1500).astype(np.int16)).cuda()
    y = torch.empty((B, sess.out_len), dtype=torch.int16, device="cuda")
    st = torch.cuda.Stream()
    for _ in range(3):
        sess.run_device(x, y, stream=st.cuda_stream)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(10):
        sess.run_device(x, y, stream=st.cuda_stream)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 10
    N = B * sess.frames
    macs = N * (120 * 1025 + 256 * 120 + 9 * 2 * 256 * 256 + 961 * 256)          # the mask network's matrix products (the transforms are FFTs: ~0.3 MFLOP per frame)
    print(f"B={B:4d}: {dt*1e3:8.3f} ms/step  {B*2.0/dt:10.0f} audio-s/s  RTF {dt/(B*2.0):.2e}  {2*macs/dt/1e12:6.1f} TFLOP/s fp32 in the mask network's GEMMs")
