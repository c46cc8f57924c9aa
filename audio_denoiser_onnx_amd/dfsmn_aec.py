"""DFSMN-AEC (DFSMN_AEC/Export_DFSMN_AEC.py, ``light_aec_model = "NKF"``): the NKF linear echo canceller followed by a DFSMN residual-echo mask.

Two graph inputs, ``near_end_audio`` then ``far_end_audio`` (:1519 -- the OPPOSITE of nkf_aec), one output ``aec_audio`` and, with ``output_vad_result``, a
per-frame speech probability ``vad_results``.  At the C ABI a call is a two-channel row: channel 0 the near end, channel 1 the far end.

Blob tensors:
    the NKF tensors of ``nkf_aec.state_to_blob_tensors`` (fc_in_w ... fc_out2_b), from the NKF checkpoint's own key names;
    feature_linear_weight (D, 240), feature_linear_bias (D)      linear1 with the feature shift / scale folded in (:1114-1124)
    deepfsmn.{i}.linear.weight (H, D), .linear.bias (H), deepfsmn.{i}.project.weight (D, H)
    fsmn_conv_weight_{i} (D, 1, lorder)                           the causal depthwise memory (:1100-1103)
    fsmn_skip (depth), fsmn_dilation (depth)                      per layer: skip_connect as 0 / 1, the memory's dilation
    linear2.weight (321, D), linear2.bias (321)                   mask;   linear3.weight (1, D), linear3.bias (1)   VAD
    mel_banks (80, 513)                                           kaldi_mel.get_mel_banks(80, 1024, 16000, 20, 0) with the zero Nyquist column (:1066-1067)
Every network dimension (D, H, lorder, depth) is read from the blob.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Mapping, Sequence

import numpy as np

from . import kaldi_mel
from .metadata import build_audio_metadata
from .nkf_aec import state_to_blob_tensors as nkf_state_to_blob_tensors

MODEL_SAMPLE_RATE = 16000
NFFT_A, NFFT_A2, WINDOW_LENGTH_A, HOP_LENGTH_A, N_MELS = 1024, 640, 640, 320, 80      # (Export_DFSMN_AEC.py:56-60)
NFFT_B, WINDOW_LENGTH_B, HOP_LENGTH_B, FILTER_ORDER = 1024, 1024, 256, 4                # (:103-107)
N_BINS = NFFT_A2 // 2 + 1
FEAT_DIM = 3 * N_MELS
PRE_EMPHASIZE = 0.97
FUSION_THRESHOLD, MIN_SPEECH_DURATION, SPEAKING_SCORE, SILENCE_SCORE, LOOK_AHEAD = 0.3, 0.2, 0.5, 0.5, 0.3      # (:62-66)


def mel_banks() -> np.ndarray:
    """(80, 513): the Kaldi bank on the first 512 bins, a zero column for Nyquist."""
    return np.pad(kaldi_mel.get_mel_banks(N_MELS, NFFT_A, float(MODEL_SAMPLE_RATE), 20.0, 0.0), ((0, 0), (0, 1))).astype(np.float32)


def mask_frames(window: int) -> int:
    return (window - WINDOW_LENGTH_A) // HOP_LENGTH_A + 1


def state_to_blob_tensors(nkf_sd: Mapping[str, np.ndarray], dfsmn_sd: Mapping[str, np.ndarray], skip_connect: Sequence[bool],
                          dilation: Sequence[int]) -> "OrderedDict[str, np.ndarray]":
    """``nkf_sd``: the NKF checkpoint (``kg_net.fc_in.0.linear_real.weight`` ...).  ``dfsmn_sd``: the DFSMN network's state dict (``linear1.linear.weight``,
    ``deepfsmn.{i}.linear.weight`` / ``.linear.bias`` / ``.project.weight`` / ``.conv1.weight``, ``linear2.*``, ``linear3.*``) plus the preprocessor's
    ``feature.shift`` / ``feature.scale``.  ``skip_connect`` / ``dilation``: one entry per deepfsmn layer (module attributes, not tensors)."""
    def g(k):
        if k not in dfsmn_sd:
            raise KeyError(f"DFSMN-AEC state: missing tensor {k}")
        return np.asarray(dfsmn_sd[k])

    out = nkf_state_to_blob_tensors(nkf_sd)
    w1, b1 = g("linear1.linear.weight").astype(np.float64), g("linear1.linear.bias").astype(np.float64)
    shift, scale = g("feature.shift").astype(np.float32).astype(np.float64), g("feature.scale").astype(np.float32).astype(np.float64)
    if w1.shape[1] != FEAT_DIM:
        raise ValueError(f"DFSMN-AEC state: linear1 takes {w1.shape[1]} features, expected {FEAT_DIM}")
    out["feature_linear_weight"] = (w1 * scale[None, :]).astype(np.float32)              # (x + shift) * scale folded into linear1 (:1117-1122)
    out["feature_linear_bias"] = (b1 + w1 @ (shift * scale)).astype(np.float32)
    depth = len(skip_connect)
    if len(dilation) != depth:
        raise ValueError("skip_connect and dilation must have one entry per deepfsmn layer")
    D = w1.shape[0]
    for i in range(depth):
        out[f"deepfsmn.{i}.linear.weight"] = g(f"deepfsmn.{i}.linear.weight").astype(np.float32)
        out[f"deepfsmn.{i}.linear.bias"] = g(f"deepfsmn.{i}.linear.bias").astype(np.float32)
        out[f"deepfsmn.{i}.project.weight"] = g(f"deepfsmn.{i}.project.weight").astype(np.float32)
        cw = g(f"deepfsmn.{i}.conv1.weight").astype(np.float32)
        out[f"fsmn_conv_weight_{i}"] = cw.reshape(D, 1, -1)                               # conv1.weight.squeeze(-1) (:1102)
    out["fsmn_skip"] = np.asarray([1.0 if s else 0.0 for s in skip_connect], np.float32)
    out["fsmn_dilation"] = np.asarray(dilation, np.float32)
    for k in ("linear2.weight", "linear2.bias", "linear3.weight", "linear3.bias"):
        out[k] = g(k).astype(np.float32)
    if out["linear2.weight"].shape != (N_BINS, D) or out["linear3.weight"].shape != (1, D):
        raise ValueError("DFSMN-AEC state: linear2 must be (321, D) and linear3 (1, D)")
    out["mel_banks"] = mel_banks()
    return out


def metadata(input_audio_length: int = 32000, use_batch_fold: bool = True, batch_window_seconds: float = 1.5, in_sample_rate: int = 16000,
             out_sample_rate: int = 16000, input_audio_dtype: str = "INT16", output_audio_dtype: str = "INT16", output_vad_result: bool = False,
             light_aec_model: str = "NKF", dft_tables: str = "reference", name: str = "DFSMN_AEC") -> Dict[str, str]:
    """The manifest Export_DFSMN_AEC.py:1538-1555 stamps.  The folded export (the folder's default) rounds its input up to whole windows of
    ``batch_window_seconds`` rounded up to the 320-sample mask hop (:118-123).  ``dft_tables``: the engine's ``ade_dft_tables`` key -- "reference" (the back end's
    transforms as dense products with the reference's fp32-angle tables: the parity path) or "exact" (its FFT kernels)."""
    meta = build_audio_metadata(producer="export.py", model_name=name, task="aec", model_family="dfsmn_aec", input_audio_length=input_audio_length,
                                in_sample_rate=in_sample_rate, out_sample_rate=out_sample_rate, model_sample_rate=MODEL_SAMPLE_RATE, nfft=NFFT_A2,
                                window_length=WINDOW_LENGTH_A, hop_length=HOP_LENGTH_A, window_type="hamming_symmetric", center_pad=False, pad_mode="constant",
                                dynamic_axes=False, input_audio_dtype=input_audio_dtype, output_audio_dtype=output_audio_dtype, max_dynamic_audio_seconds=30,
                                batch_window_seconds=batch_window_seconds, use_batch_fold=use_batch_fold, input_channels=1, output_channels=1,
                                num_audio_inputs=2, feature_kind="kaldi_fbank_stft_aec",
                                extra={"light_aec_model": light_aec_model, "n_mels": N_MELS, "nfft_a": NFFT_A, "nfft_a2": NFFT_A2, "window_length_a": WINDOW_LENGTH_A,
                                       "hop_length_a": HOP_LENGTH_A, "nfft_b": NFFT_B, "window_length_b": WINDOW_LENGTH_B, "hop_length_b": HOP_LENGTH_B,
                                       "window_type_b": "hann", "preemphasize": PRE_EMPHASIZE, "filter_order": FILTER_ORDER,
                                       "output_vad_result": bool(output_vad_result), "num_outputs": 2 if output_vad_result else 1,
                                       "output_frame_shift_seconds": HOP_LENGTH_A / MODEL_SAMPLE_RATE, "output_frame_shift_samples": HOP_LENGTH_A,
                                       "fbank_window_length_samples": WINDOW_LENGTH_A, "speaking_score": SPEAKING_SCORE, "silence_score": SILENCE_SCORE,
                                       "look_ahead_seconds": LOOK_AHEAD, "fusion_threshold_seconds": FUSION_THRESHOLD,
                                       "min_speech_duration_seconds": MIN_SPEECH_DURATION})
    if dft_tables != "reference":
        meta["ade_dft_tables"] = dft_tables
    return meta
