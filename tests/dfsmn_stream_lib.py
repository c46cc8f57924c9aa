"""Shared pieces of the DFSMN streaming tests (tests/test_dfsmn_stream.py, tests/test_dfsmn_stream_gpu.py)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
HOP = DELAY = 960
NAMES = ("speech0", "speech1", "randn", "zeros")


def blob_bytes() -> bytes:
    with open(os.path.join(GOLD, "dfsmn_seed0.adew"), "rb") as f:
        return f.read()


def tensors():
    from audio_denoiser_onnx_amd.weights import load_blob
    return load_blob(os.path.join(GOLD, "dfsmn_seed0.adew"))


def meta(length, in_rate=48000, out_rate=48000, **kw):
    from audio_denoiser_onnx_amd.metadata import build_audio_metadata
    return build_audio_metadata(producer="tests", model_name="DFSMN", task="denoise", model_family="dfsmn", input_audio_length=length,
                                in_sample_rate=in_rate, out_sample_rate=out_rate, model_sample_rate=48000, nfft=1920, window_length=1920,
                                hop_length=960, window_type="hamming", center_pad=False, pad_mode="constant", feature_kind="kaldi_fbank_stft", **kw)


def seed0_io():
    """tests/golden/dfsmn_seed0_io.npz: four rows of 24 000 samples (two speech clips, noise, zeros) and the reference's one-call outputs."""
    g = np.load(os.path.join(GOLD, "dfsmn_seed0_io.npz"))
    return np.stack([g[f"{n}.pcm_in"] for n in NAMES]), np.stack([g[f"{n}.pcm_out"] for n in NAMES])


def stream_fixture():
    """tests/golden/dfsmn_seed0_stream.npz (tools/make_golden_dfsmn.py --stream): the reference's forward, ONE call, on a speech clip of 48 000 samples."""
    return np.load(os.path.join(GOLD, "dfsmn_seed0_stream.npz"))


def run_stream(st, x, flush=True):
    """A whole (n_streams, n) signal through an open StreamingSession in pushes of its size, then the flush -> (pcm, f32), each (n_streams, n + delay)
    (flush=False: the pushes alone, (n_streams, n))."""
    P = st.samples_per_push
    assert x.shape[1] % P == 0
    parts = [st.push(x[:, o:o + P], want_f32=True) for o in range(0, x.shape[1], P)]
    if flush:
        parts.append(st.flush(want_f32=True))
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)


def lsb(a, b):
    return np.abs(a.astype(np.int32) - b.astype(np.int32))
