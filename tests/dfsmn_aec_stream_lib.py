"""Shared pieces of the DFSMN-AEC streaming tests (tests/test_dfsmn_aec_stream.py, tests/test_dfsmn_aec_stream_gpu.py)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
HOP, DELAY = 256, 1344


def mask_frames_after(hops: int) -> int:
    """M(k) of include/ade.h: the mask frames that are complete after k hops of input."""
    nt = HOP * max(0, hops - 3)
    return 0 if nt < 640 else (nt - 640) // 320 + 1


def seed0_blob() -> bytes:
    with open(os.path.join(GOLD, "dfsmn_aec_seed0.adew"), "rb") as f:
        return f.read()


def seed0_tensors():
    from audio_denoiser_onnx_amd.weights import load_blob
    return load_blob(os.path.join(GOLD, "dfsmn_aec_seed0.adew"))


def seed0_io():
    """tests/golden/dfsmn_aec_seed0_io.npz: four rows of 32 000 samples (speech, noise, silent far end, zeros) and the reference's unfolded outputs."""
    io = np.load(os.path.join(GOLD, "dfsmn_aec_seed0_io.npz"))
    near, far, out = (np.stack([io[f"{k}{i}"][:32000] for i in range(4)]) for k in ("near", "far", "out"))
    return near, far, out


def stream_fixture():
    """tests/golden/dfsmn_aec_seed0_stream.npz (tools/make_golden_dfsmn_aec.py --stream): the reference's unfolded forward, ONE call, on two clips of 40 960 samples."""
    return np.load(os.path.join(GOLD, "dfsmn_aec_seed0_stream.npz"))


def run_stream(st, near, far, flush=True):
    """Whole (n_streams, n) signals through an open StreamingSession in pushes of its size, then the flush -> (pcm, f32), each (n_streams, n + delay)
    (flush=False: the pushes alone, (n_streams, n))."""
    P = st.samples_per_push
    assert far.shape == near.shape and far.shape[1] % P == 0
    parts = [st.push_aec(far[:, o:o + P], near[:, o:o + P], want_f32=True) for o in range(0, far.shape[1], P)]
    if flush:
        parts.append(st.flush(want_f32=True))
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)
