"""numpy (float64) restatement of DFSMN-AEC's forward (DFSMN_AEC/Export_DFSMN_AEC.py:1268-1352 with NKF_Inner :897-1000 and the folder's STFT_Process), for the parity tests.

Per window of W samples (a folded call is a batch of independent windows):
    near, far (int16 * 2^-15, or normalised floats; NO DC removal) -> NKF back end: stft 1024 / 1024 / 256 periodic hann, constant centre pad; the Kalman
    recurrence of nkf_aec_oracle.NkfAecOracle.kalman; istft with the static window-square sum, raw overlap-add samples [512, 512 + W) -> temp_aec (W floats)
    -> mask STFT of temp_aec: 640 / 640 / 320 symmetric hamming, no centre pad -> 321 bins x Tm frames
    -> Kaldi fbank of near and temp_aec per 640-sample frame at hop 320: mean removal, 0.97 pre-emphasis, symmetric hamming, zero pad to 1024, DFT (513 bins);
       echo = near_spec - 1.15 temp_spec; the three powers * 2^30 -> mel(80, 513) -> max(., eps) -> log -> [near | temp | echo] = 240 per frame
    -> relu(feature_linear) -> deepfsmn[i]: x + causal depthwise memory(project(relu(linear(x)))) [+ that hidden if skip_connect] -> sigmoid(linear2) = mask (321),
       sigmoid(linear3) = vad (1)
    -> mask * spectrum -> istft 640 / 320 symmetric hamming, static window-square sum (raw length == W) -> * 32767, clamp, truncate -> int16.

``tables="reference"`` builds the STFT_Process DFT kernels from fp32 angles as the reference does; ``"exact"`` uses exact trigonometry (what an FFT computes).
``tables`` is the back end's 1024-point pair, ``mask_tables`` (default: the same) the 640-point mask pair.  The engine's default is ``("reference", "exact")``:
dense reference tables in the back end, FFTs for the mask transforms; with ``ade_dft_tables = exact`` it is ``("exact", "exact")``.
The Kaldi fbank kernel is built in float64 by the reference, so it is exact in every mode.
"""
from __future__ import annotations

import numpy as np

from nkf_aec_oracle import NkfAecOracle, hann_periodic_f32

NB, HB, FB = 1024, 256, 513                  # back end (NKF) STFT
NA, HA, FA = 640, 320, 321                   # mask STFT
NK, FK, NMEL = 1024, 513, 80                 # Kaldi fbank
ECHO_FACTOR = 1.15
EPS = float(np.finfo(np.float32).eps)


def hamming_symmetric_f32(n):
    import torch
    return torch.hamming_window(n, periodic=False, alpha=0.54, beta=0.46).double().numpy()


def _dft(kind, n_fft, bins):
    if kind == "reference":                  # STFT_Process._build_stft_kernels: fp32 angles
        f32 = np.float32
        om = (f32(2.0 * np.pi / n_fft) * np.arange(bins, dtype=f32)[:, None] * np.arange(n_fft, dtype=f32)[None, :]).astype(f32)
        return np.cos(om).astype(np.float64), np.sin(om).astype(np.float64)
    om = 2.0 * np.pi * (np.outer(np.arange(bins), np.arange(n_fft)) % n_fft) / n_fft
    return np.cos(om), np.sin(om)


def _stft(x, w, cos, sin, hop, pad):
    """x (R, L) -> complex (R, T, bins)"""
    n = w.size
    xp = np.pad(x, ((0, 0), (pad, pad)))
    T = (xp.shape[1] - n) // hop + 1
    idx = np.arange(T)[:, None] * hop + np.arange(n)[None, :]
    fr = xp[:, idx] * w
    return fr @ cos.T - 1j * (fr @ sin.T)


def _istft(spec, w, cos, sin, hop, start, length):
    """spec complex (R, T, bins) -> (R, length): overlap-add samples [start, start + length) over the window-square sum of the same T frames"""
    n = w.size
    R, T, bins = spec.shape
    scale = np.full((bins, 1), 2.0)
    scale[0] = scale[-1] = 1.0
    frames = (spec.real @ (scale * cos / n) + spec.imag @ (scale * -sin / n)) * w
    raw = np.zeros((R, n + hop * (T - 1)))
    ws = np.zeros(n + hop * (T - 1))
    for t in range(T):
        raw[:, t * hop:t * hop + n] += frames[:, t]
        ws[t * hop:t * hop + n] += w * w
    return raw[:, start:start + length] / ws[start:start + length]


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


class DfsmnAecOracle:
    def __init__(self, blob_tensors, tables="reference", mask_tables=None):
        self.w = {k: np.asarray(v, np.float64) for k, v in blob_tensors.items()}
        self.nkf = NkfAecOracle(blob_tensors, tables=tables)
        self.tables, self.mask_tables = tables, mask_tables or tables
        self.depth = int(self.w["fsmn_skip"].size)

    def fbank_spectrum(self, x):
        """x (R, W) -> complex (R, Tm, 513): the Kaldi frame transform (build_kaldi_fbank_conv, :1032-1068)"""
        T = (x.shape[1] - NA) // HA + 1
        idx = np.arange(T)[:, None] * HA + np.arange(NA)[None, :]
        fr = x[:, idx]
        fr = fr - fr.mean(axis=2, keepdims=True)
        prev = np.concatenate([fr[..., :1], fr[..., :-1]], axis=2)
        fr = (fr - 0.97 * prev) * (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(NA) / (NA - 1)))
        return np.fft.rfft(fr, n=NK, axis=2)

    def network(self, feat):
        """feat (R, Tm, 240) -> mask (R, Tm, 321), vad (R, Tm)"""
        w = self.w
        x = np.maximum(feat @ w["feature_linear_weight"].T + w["feature_linear_bias"], 0.0)
        T = x.shape[1]
        for i in range(self.depth):
            h = np.maximum(x @ w[f"deepfsmn.{i}.linear.weight"].T + w[f"deepfsmn.{i}.linear.bias"], 0.0) @ w[f"deepfsmn.{i}.project.weight"].T
            cw = w[f"fsmn_conv_weight_{i}"].reshape(h.shape[2], -1)           # (D, lorder)
            lo, dil = cw.shape[1], int(w["fsmn_dilation"][i])
            hp = np.pad(h, ((0, 0), (dil * (lo - 1), 0), (0, 0)))
            mem = sum(hp[:, k * dil:k * dil + T] * cw[:, k] for k in range(lo))
            if w["fsmn_skip"][i] != 0:
                mem = mem + h
            x = x + mem
        mask = _sig(x @ w["linear2.weight"].T + w["linear2.bias"])
        vad = _sig(x @ w["linear3.weight"].T + w["linear3.bias"])[..., 0]
        return mask, vad

    def forward(self, near, far, fold_window=0, int_in=True, int_out=True):
        """near, far: (B, L) int16 (or normalised floats with int_in=False) -> (output (B, L) int16 / float32, dict of taps).
        Taps (rows = B * windows): temp_aec (rows, W), spec complex (rows, Tm, 321), feat (rows, Tm, 240), mask (rows, Tm, 321), vad_results (rows * Tm), wave (B, L)."""
        near, far = np.asarray(near, np.float64), np.asarray(far, np.float64)
        if int_in:
            near, far = near / 32768.0, far / 32768.0
        B, L = near.shape
        W = fold_window or L
        near, far = near.reshape(-1, W), far.reshape(-1, W)
        R = near.shape[0]
        # NKF back end (:1236-1238, :931-1000)
        wb = hann_periodic_f32(NB)
        cb, sb = _dft(self.tables, NB, FB)
        spec = _stft(np.concatenate([far, near]), wb, cb, sb, HB, NB // 2).transpose(0, 2, 1)      # (2R, F, Tb)
        ref, mic = spec[:R], spec[R:]
        echo, _ = self.nkf.kalman(ref, mic)
        temp = _istft((mic - echo).transpose(0, 2, 1), wb, cb, sb, HB, NB // 2, W)
        # mask STFT of temp_aec and the Kaldi features (:1288-1311)
        wa = hamming_symmetric_f32(NA)
        ca, sa = _dft(self.mask_tables, NA, FA)
        spec_a = _stft(temp, wa, ca, sa, HA, 0)                                                          # (R, Tm, 321)
        near_k, temp_k = self.fbank_spectrum(near), self.fbank_spectrum(temp)
        echo_k = near_k - ECHO_FACTOR * temp_k
        power = np.stack([np.abs(near_k) ** 2, np.abs(temp_k) ** 2, np.abs(echo_k) ** 2], axis=2) * 2.0 ** 30      # (R, Tm, 3, 513)
        feat = np.log(np.maximum(power @ self.w["mel_banks"].T, EPS)).reshape(R, -1, 3 * NMEL)
        mask, vad = self.network(feat)
        wave = _istft(spec_a * mask, wa, ca, sa, HA, 0, W).reshape(B, L)
        out = np.trunc(np.clip(wave * 32767.0, -32768, 32767)).astype(np.int16) if int_out else wave.astype(np.float32)
        return out, {"temp_aec": temp, "spec": spec_a, "feat": feat, "mask": mask, "vad_results": vad.reshape(-1), "wave": wave}


def load_blob_tensors(path):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from audio_denoiser_onnx_amd.weights import load_blob
    return load_blob(path)
