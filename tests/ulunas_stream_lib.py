"""Shared pieces of the UL-UNAS streaming tests (tests/test_ulunas_stream.py, tests/test_ulunas_stream_gpu.py)."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
HOP = DELAY = 256


@functools.lru_cache(maxsize=None)
def seed0():
    """tests/golden/ulunas_seed0.npz: (pcm_in, pcm_out) = three rows of 16 000 samples (speech, noise, silence) and the reference's one-call outputs of 15 872 samples,
    and the folded seed-0 network."""
    from audio_denoiser_onnx_amd import ulunas
    z = np.load(os.path.join(GOLD, "ulunas_seed0.npz"))
    fused = ulunas.fold_state_dict({str(k): z["w:" + str(k)] for k in z["keys"]})
    return z["pcm_in"], z["pcm_out"], fused


def stream_fixture():
    """tests/golden/ulunas_seed0_stream.npz (tools/make_golden_ulunas.py --stream): the reference's forward, ONE call, on a clip of 20 480 samples; same network."""
    return np.load(os.path.join(GOLD, "ulunas_seed0_stream.npz"))


@functools.lru_cache(maxsize=None)
def blob_bytes() -> bytes:
    from audio_denoiser_onnx_amd.weights import pack_blob
    return pack_blob(seed0()[2])


def meta(length, **kw):
    """ulunas.metadata() plus any other manifest key (audio dtypes, batch-fold, dynamic_axes, sample rates)."""
    from audio_denoiser_onnx_amd import ulunas
    from audio_denoiser_onnx_amd.metadata import build_audio_metadata
    args = dict(producer="tests", model_name="UL_UNAS", task="denoise", model_family="ul_unas", input_audio_length=length, in_sample_rate=16000, out_sample_rate=16000,
                model_sample_rate=16000, nfft=ulunas.NFFT, window_length=ulunas.NFFT, hop_length=ulunas.HOP, window_type="hann", center_pad=True, pad_mode="reflect",
                extra={"n_mels": 100, "remove_dc_offset": 0})
    args.update(kw)
    return build_audio_metadata(**args)


def oracle(length):
    """The float64-table oracle of the whole network on one call of `length` samples (the engine's DFT tables use exactly reduced angles)."""
    from audio_denoiser_onnx_amd import ulunas
    from ulunas_oracle import UlunasOracle
    return UlunasOracle(seed0()[2], ulunas.block_plan(), length, True)


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
