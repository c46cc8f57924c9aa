"""float64 numpy restatement of Deep Echo's forward (Deep_Echo_AEC/Export_Deep_Echo.py:303-342, :372-426 with its STFT_Process), from the engine's blob, for the
parity tests.

Per clip (a call, or one fold window): both rows / 32768 (int16 input) minus their own mean -> stft_B (319 / 319 / 160, periodic Hamming, constant centre pad; the
DFT tables with the reference's fp32 angles) -> the four inputs [near re, far re, near im, far im] -> NET (bidirectional LSTM along the bins, cfb_e1, the two-layer
LSTM along time, cfb_d1 on e1 * lstm_out, out_ch_lstm along time, the 10-tap echo path) -> mix - sum_k far[t - 9 + k] * path_k[t] -> istft_B, the overlap-add
DIVIDED by the window-square sum, samples [159, 159 + L) -> * 32767, clamp, truncate.  Layout of every activation: (clip, frame, bin, channel).  The building blocks
(LayerNorm in its folded form, the LSTMs, the CFB, the STFT tables) are tests/sdaec_oracle.py's: the two networks share them.
"""
from __future__ import annotations

import glob
import os

import numpy as np

from sdaec_oracle import HOP, NFFT, SdaecOracle, stft_tables

ORDER = 10

# The reference's own fp32 forward against this float64 restatement, measured on the CPU over the fixture (tests/test_deep_echo.py asserts that the figures still
# hold).  WAVE_REF_DISTANCE is the largest over the four L = 8000 rows, the three short lengths, the F32 case and the fold; it lies below 2.5e-5, so the family
# gate is the project's: waveform <= 1e-4, PCM <= 1 LSB.
WAVE_REF_DISTANCE = 5.0e-7
WAVE_GATE = 1e-4
# Tap gates (row 0 of the L = 8000 fixture): gate = max(1e-5 * max |reference tap|, 4 * the distance between the reference's fp32 tap and this restatement); the
# factor 4 covers an engine's different summation order at fp32 noise of the same size as the reference's own.
TAP_REF_DISTANCE = {"e0": 3.5e-7, "e1": 1.6e-6, "lstm_out": 6.3e-8, "d1": 1.5e-6, "path": 4.0e-7, "spec_out": 2.3e-6}


def tap_gate(name, ref_absmax):
    return max(1e-5 * float(ref_absmax), 4.0 * TAP_REF_DISTANCE[name])


class DeepEchoOracle(SdaecOracle):
    def net(self, x, taps=None):
        """x: (N, T, 160, 4) [near re, far re, near im, far im] -> the echo path (N, T, 160, 20): [re taps 0 .. 9 | im taps 0 .. 9]"""
        w = self.w
        e0 = np.concatenate([self._bilstm_f(x, "in_lstm"), x], axis=-1) @ w["in_fused_w"].T + w["in_fused_b"]
        e1 = self._cfb(e0, "e1")
        h = self._ln(e1, "ln")
        for layer in range(2):
            h = self._lstm_t(h, w[f"t_lstm.w_ih{layer}"], w[f"t_lstm.w_hh{layer}"], w[f"t_lstm.b_ih{layer}"], w[f"t_lstm.b_hh{layer}"])
        lstm_out = h @ w["t_lin_w"].T + w["t_lin_b"]
        d1 = self._cfb(e1 * lstm_out, "d1")
        d0 = self._lstm_t(np.concatenate([e0, d1], axis=-1), w["out_lstm.w_ih"], w["out_lstm.w_hh"], w["out_lstm.b_ih"], w["out_lstm.b_hh"])
        path = np.concatenate([d0, d1], axis=-1) @ w["echo_w"].T + w["echo_b"]
        if taps is not None:
            taps.update(e0=e0, e1=e1, lstm_out=lstm_out, d1=d1, path=path)
        return path

    @staticmethod
    def apply_echo_path(far_re, far_im, path):
        """far: (N, T, 160), path: (N, T, 160, 20) -> est (re, im): tap k multiplies the far-end frame t - 9 + k, zeros before frame 0 (:279, :303-311)"""
        T = far_re.shape[1]
        fr, fi = (np.pad(v, ((0, 0), (ORDER - 1, 0), (0, 0))) for v in (far_re, far_im))
        er, ei = np.zeros_like(far_re), np.zeros_like(far_im)
        for k in range(ORDER):
            dr, di, pr, pi = fr[:, k:k + T], fi[:, k:k + T], path[..., k], path[..., ORDER + k]
            er += dr * pr - di * pi
            ei += dr * pi + di * pr
        return er, ei

    def forward(self, near, far, fold_window=0, int_in=True, int_out=True, want_taps=False):
        """near, far: (B, L) int16 (or normalised float with int_in=False) -> (int16 or float output (B, L), the waveform before the PCM scale, taps).
        fold_window: USE_BATCH_FOLD -- each window of a row is an independent clip."""
        near, far = np.asarray(near, np.float64), np.asarray(far, np.float64)
        B, L = near.shape
        Wn = fold_window or L
        n_win = L // Wn
        N = B * n_win
        x = np.concatenate([near.reshape(N, Wn), far.reshape(N, Wn)])
        if int_in:
            x = x / 32768.0
        x = x - x.mean(axis=1, keepdims=True)
        T = (Wn - 1) // HOP + 1
        ka_re, ka_im, ks_re, ks_im, inv_ws = stft_tables(T, Wn)
        xp = np.pad(x, ((0, 0), (NFFT // 2, NFFT)))
        fr = xp[:, np.arange(T)[:, None] * HOP + np.arange(NFFT)[None, :]]             # (2 N, T, 319)
        re, im = fr @ ka_re.T, fr @ ka_im.T                                             # (2 N, T, 160)
        feat = np.stack([re[:N], re[N:], im[:N], im[N:]], axis=-1)                      # (N, T, 160, 4)
        taps = {} if want_taps else None
        path = self.net(feat, taps)
        er, ei = self.apply_echo_path(re[N:], im[N:], path)
        out = np.stack([re[:N] - er, im[:N] - ei], axis=-1)                             # (N, T, 160, 2)
        if want_taps:
            taps["spec_out"] = out
        frames = out[..., 0] @ ks_re + out[..., 1] @ ks_im                              # (N, T, 319)
        raw = np.zeros((N, NFFT + HOP * (T - 1)))
        for t in range(T):
            raw[:, t * HOP:t * HOP + NFFT] += frames[:, t]
        wave = (raw[:, NFFT // 2:NFFT // 2 + Wn] * inv_ws).reshape(B, L)               # inv_ws = 1 / window-square sum in float64: the reference's division
        res = np.trunc(np.clip(wave * 32767.0, -32768, 32767)).astype(np.int16) if int_out else wave.astype(np.float32)
        return res, wave, taps


def fixture_state(gold_dir, seed=0):
    """The checkpoint-named fixture -> the state of NET."""
    state = {}
    for p in sorted(glob.glob(os.path.join(gold_dir, f"deep_echo_seed{seed}_state_*.npz"))):
        with np.load(p) as z:
            state.update({k: z[k] for k in z.files})
    return state
