"""Shared pieces of the NKF-AEC streaming tests (tests/test_nkf_aec_stream.py, tests/test_nkf_aec_stream_gpu.py)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
HOP, DELAY = 256, 768


def fixture():
    """tests/golden/nkf_aec_seed0_stream.npz (tools/make_golden_nkf_aec.py --stream): the reference's NKF.forward on two zero-sum clips of 49 152 samples."""
    return np.load(os.path.join(GOLD, "nkf_aec_seed0_stream.npz"))


def seed0_blob() -> bytes:
    with open(os.path.join(GOLD, "nkf_aec_seed0.adew"), "rb") as f:
        return f.read()


def seed0_tensors():
    from audio_denoiser_onnx_amd.weights import load_blob
    return load_blob(os.path.join(GOLD, "nkf_aec_seed0.adew"))


def zero_sum(x):
    """int16 signal -> the same signal with an exactly zero integer sum: the reference's whole-call mean is then exactly 0."""
    x = np.asarray(x).astype(np.int64)
    x -= int(x.sum()) // len(x)
    x[:int(x.sum())] -= 1                               # 0 <= remainder < n: take it off one LSB at a time
    assert x.sum() == 0 and np.abs(x).max() < 32768
    return x.astype(np.int16)


def run_stream(st, far, near):
    """Whole (n_streams, n) signals through an open StreamingSession in pushes of its size, then the flush -> (pcm, f32), each (n_streams, n + delay)."""
    P = st.samples_per_push
    assert far.shape == near.shape and far.shape[1] % P == 0
    parts = [st.push_aec(far[:, o:o + P], near[:, o:o + P], want_f32=True) for o in range(0, far.shape[1], P)]
    parts.append(st.flush(want_f32=True))
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)
