"""numpy restatement of NKF-AEC's forward (NKF_AEC/Export_NKF_AEC.py:246-411 with its STFT_Process), for the parity tests.

Per call: both inputs minus their own DC mean (int16 units, :259-269) -> stft_B (1024 / 1024 / 256, periodic hann, constant centre pad, the 2^-15 input scale
folded, :482-486) -> per bin, the Kalman recurrence over all frames (:302-373) -> error spectrum mic - echo_hat -> istft_B with the static 1 / window-square
sum (:487-492) -> [:audio_len] -> * 32767 and .to(int16) (:389-408).

The KGNet step of one bin (:182-197), every product a real 2-group dense layer (ComplexDense_Real is two independent Linear layers, :93-122):
    fc_in:   u_c = leaky(W_in[c] x_c + b_in[c], slope_in),        x_c = [xt_c (4), e_c, dh_c (4)],  c in (re, im)
    GRU:     h_rr = gru_r(u_re), h_ir = gru_r(u_im), h_ri = gru_i(u_re), h_ii = gru_i(u_im)      (PyTorch nn.GRU, gates r, z, n)
             g = (h_rr - h_ii, h_ri + h_ir)
    fc_out:  v_c = leaky(W_o1[c] g_c + b_o1[c], slope_out);  kg_c = W_o2[c] v_c + b_o2[c]
The Kalman update (:344-373), complex:  dh = h_post - h_prior;  h_prior <- h_post;  e = mic - <xt, h_prior>;  h_post = h_prior + kg e;  echo = <xt, h_post>
with xt the last 4 reference frames (oldest first, zeros before frame 0).  Frame 0 of the reference (:309-335) is this step with zero state.

``tables="reference"`` builds the DFT kernels as the reference does (fp32 angles); ``"exact"`` uses exact (float64) trigonometry, which is what the engine's FFT
computes.
"""
from __future__ import annotations

import numpy as np

NFFT, HOP, F, LTAPS, H = 1024, 256, 513, 4, 18


def hann_periodic_f32(n):
    import torch
    return torch.hann_window(n, periodic=True).double().numpy()


def _tables(kind, input_scale, output_scale, frames):
    w = hann_periodic_f32(NFFT)
    if kind == "reference":                                          # STFT_Process._build_stft_kernels / _build_istft_kernels, fp32
        f32 = np.float32
        om = (f32(2.0 * np.pi / NFFT) * np.arange(F, dtype=f32)[:, None] * np.arange(NFFT, dtype=f32)[None, :]).astype(f32)
        cos, sin = np.cos(om).astype(np.float64), np.sin(om).astype(np.float64)
    else:
        om = 2.0 * np.pi * (np.outer(np.arange(F), np.arange(NFFT)) % NFFT) / NFFT
        cos, sin = np.cos(om), np.sin(om)
    ka_re, ka_im = cos * w * input_scale, -sin * w * input_scale
    scale = np.full((F, 1), 2.0)
    scale[0] = scale[-1] = 1.0
    ks_re, ks_im = scale * cos / NFFT * w, scale * -sin / NFFT * w
    raw = NFFT + HOP * (frames - 1)
    ws = np.zeros(raw)
    for t in range(frames):
        ws[t * HOP:t * HOP + NFFT] += w * w
    inv_ws = output_scale / ws[NFFT // 2:raw - NFFT // 2]
    return ka_re, ka_im, ks_re, ks_im, inv_ws


def _leaky(x, s):
    return np.where(x > 0, x, x * s)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


class NkfAecOracle:
    def __init__(self, blob_tensors, tables="reference"):
        self.w = {k: np.asarray(v, np.float64) for k, v in blob_tensors.items()}
        self.tables = tables

    def _gru(self, g, x, h):
        w = self.w
        gi = x @ w["gru_w_ih"][g].T + w["gru_b_ih"][g]
        gh = h @ w["gru_w_hh"][g].T + w["gru_b_hh"][g]
        r = _sig(gi[..., :H] + gh[..., :H])
        z = _sig(gi[..., H:2 * H] + gh[..., H:2 * H])
        n = np.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
        return (1.0 - z) * n + z * h

    def kalman(self, ref, mic):
        """ref, mic: complex (N, F, T) -> echo_hat complex (N, F, T), and the last frame's gain (N, F, 4)"""
        w = self.w
        N, _, T = ref.shape
        pad = np.concatenate([np.zeros((N, F, LTAPS - 1), complex), ref], axis=2)
        hp = np.zeros((N, F, LTAPS), complex)
        hq = np.zeros((N, F, LTAPS), complex)
        hs = [np.zeros((N, F, H)) for _ in range(4)]               # h_rr, h_ir, h_ri, h_ii
        echo = np.zeros((N, F, T), complex)
        s_in, s_out = float(w["fc_in_slope"][0]), float(w["fc_out_slope"][0])
        kg = None
        for t in range(T):
            xt = pad[..., t:t + LTAPS]
            dh = hq - hp
            hp = hq
            e = mic[..., t] - np.sum(xt * hp, axis=2)
            feat = [np.concatenate([xt.real, e.real[..., None], dh.real], axis=2), np.concatenate([xt.imag, e.imag[..., None], dh.imag], axis=2)]
            u = [_leaky(feat[c] @ w["fc_in_w"][c].T + w["fc_in_b"][c], s_in) for c in range(2)]
            hs = [self._gru(0, u[0], hs[0]), self._gru(0, u[1], hs[1]), self._gru(1, u[0], hs[2]), self._gru(1, u[1], hs[3])]
            gx = [hs[0] - hs[3], hs[2] + hs[1]]
            v = [_leaky(gx[c] @ w["fc_out1_w"][c].T + w["fc_out1_b"][c], s_out) for c in range(2)]
            kg = (v[0] @ w["fc_out2_w"][0].T + w["fc_out2_b"][0]) + 1j * (v[1] @ w["fc_out2_w"][1].T + w["fc_out2_b"][1])
            hq = hp + kg * e[..., None]
            echo[..., t] = np.sum(xt * hq, axis=2)
        return echo, kg

    def forward(self, far, near, fold_window=0, int_in=True, int_out=True, want_taps=False, audio_len=None):
        """far, near: (B, L) int16 (or normalised float with int_in=False) -> (int16 or float output (B, audio_len), waveform before the PCM scale, taps).
        fold_window: USE_BATCH_FOLD -- each window of the row is an independent call; audio_len: the [:audio_len] trim (default L)."""
        far, near = np.asarray(far, np.float64), np.asarray(near, np.float64)
        B, L = far.shape
        Wn = fold_window or L
        n_win = L // Wn
        x = np.concatenate([far.reshape(B * n_win, Wn), near.reshape(B * n_win, Wn)])           # audio_pair: far rows, then near rows (:259)
        x = x - x.mean(axis=1, keepdims=True)
        T = Wn // HOP + 1
        ka_re, ka_im, ks_re, ks_im, inv_ws = _tables(self.tables, 1.0 / 32768.0 if int_in else 1.0, 1.0, T)
        xp = np.pad(x, ((0, 0), (NFFT // 2, NFFT // 2)))
        idx = np.arange(T)[:, None] * HOP + np.arange(NFFT)[None, :]
        fr = xp[:, idx]                                                   # (rows, T, NFFT)
        spec = (fr @ ka_re.T + 1j * (fr @ ka_im.T)).transpose(0, 2, 1)     # (rows, F, T)
        ref, mic = spec[:B * n_win], spec[B * n_win:]
        echo, kg = self.kalman(ref, mic)
        err = mic - echo
        frames = err.real.transpose(0, 2, 1) @ ks_re + err.imag.transpose(0, 2, 1) @ ks_im      # (rows, T, NFFT)
        raw = np.zeros((B * n_win, NFFT + HOP * (T - 1)))
        for t in range(T):
            raw[:, t * HOP:t * HOP + NFFT] += frames[:, t]
        y = raw[:, NFFT // 2:NFFT // 2 + HOP * (T - 1)] * inv_ws
        wave = y.reshape(B, -1)[:, :audio_len or L]
        if int_out:
            out = np.trunc(np.clip(wave * 32767.0, -32768, 32767)).astype(np.int16)
        else:
            out = wave.astype(np.float32)
        taps = {"ref": ref, "mic": mic, "echo_hat": echo, "kg": kg} if want_taps else None
        return out, wave, taps


def load_blob_tensors(path):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from audio_denoiser_onnx_amd.weights import load_blob
    return load_blob(path)
