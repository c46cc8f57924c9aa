"""float64 numpy restatement of SDAEC's forward (SDAEC/Export_SDAEC.py:261-284, :382-444 with its STFT_Process), from the engine's blob, for the parity tests.

Per clip (a call, or one fold window): both rows / 32768 (int16 input) minus their own mean -> stft_B (319 / 319 / 160, periodic Hamming, constant centre
pad; the DFT tables with the reference's fp32 angles) -> frame powers -> alpha = causal 10-tap, 2-channel convolution -> far spectrum * |alpha| ->
NET (bidirectional LSTM along the bins, ten CFB blocks with their cepstral units, the two LSTM stacks along time) -> istft_B with the static window-square
norm, samples [159, 159 + L) -> * 32767, clamp, truncate.  Layout of every activation: (clip, frame, bin, channel).
"""
from __future__ import annotations

import glob
import os

import numpy as np

NFFT, HOP, F, C, K = 319, 160, 160, 20, 10
CFB_NAMES = ("e1", "e2", "e3", "e4", "e5", "d5", "d4", "d3", "d2", "d1")


# Tap gates (row 0 of the L = 32000 fixture): gate = max(1e-5 * max |reference tap|, 4 * the distance between the reference's fp32 tap and this float64
# restatement).  The distances below were measured with this file against tests/golden/sdaec_seed0_taps.npz (tests/test_sdaec.py asserts that they still hold);
# the factor 4 covers an engine's different summation order at fp32 noise of the same size as the reference's own.
TAP_REF_DISTANCE = {"alpha": 2.3e-4, "e0": 1.1e-4, "e5": 7.7e-6, "lstm_out": 2.3e-7, "d1": 8.0e-6, "spec_out": 1.4e-6}


def tap_gate(name, ref_absmax):
    return max(1e-5 * float(ref_absmax), 4.0 * TAP_REF_DISTANCE[name])


def hamming_periodic_f32(n):
    import torch
    return torch.hamming_window(n, periodic=True).double().numpy()


def stft_tables(frames, out_len):
    """STFT_Process._build_stft_kernels / _build_istft_kernels: fp32 angles fl(fl(2 pi / N) f) t), the rest in float64."""
    f32 = np.float32
    w = hamming_periodic_f32(NFFT)
    om = ((f32(2.0 * np.pi / NFFT) * np.arange(F, dtype=f32)[:, None]).astype(f32) * np.arange(NFFT, dtype=f32)[None, :]).astype(f32).astype(np.float64)
    cos, sin = np.cos(om), np.sin(om)
    scale = np.full((F, 1), 2.0)
    scale[0] = 1.0                                                  # odd n_fft: no Nyquist bin
    ws = np.zeros(NFFT + HOP * (frames - 1))
    for t in range(frames):
        ws[t * HOP:t * HOP + NFFT] += w * w
    return cos * w, -sin * w, scale * cos / NFFT * w, scale * -sin / NFFT * w, 1.0 / ws[NFFT // 2:NFFT // 2 + out_len]


def _sig(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def lstm(x, w_ih, w_hh, b_ih, b_hh, reverse=False):
    """x: (steps, n, in) -> (steps, n, hidden); PyTorch gate order i, f, g, o; zero initial state."""
    H = w_hh.shape[1]
    S, n, _ = x.shape
    xg = x @ w_ih.T + b_ih + b_hh
    h, c = np.zeros((n, H)), np.zeros((n, H))
    out = np.zeros((S, n, H))
    for s in (range(S - 1, -1, -1) if reverse else range(S)):
        g = xg[s] + h @ w_hh.T
        i, f, gg, o = _sig(g[:, :H]), _sig(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sig(g[:, 3 * H:])
        c = f * c + i * gg
        h = o * np.tanh(c)
        out[s] = h
    return out


class SdaecOracle:
    def __init__(self, blob_tensors):
        self.w = {k: np.asarray(v, np.float64) for k, v in blob_tensors.items()}

    def _ln(self, x, name):
        w = self.w
        ax = (-2, -1)
        mu = x.mean(axis=ax, keepdims=True)
        var = ((x - mu) ** 2).mean(axis=ax, keepdims=True)
        return (x - mu) / np.sqrt(var + w[name + "_eps"][0]) * w[name + "_w"] + w[name + "_b"]

    def _bilstm_f(self, x, p):
        """x: (N, T, bins, in) -> (N, T, bins, 2 H), the recurrence along the bins"""
        w = self.w
        N, T, Fb, D = x.shape
        xs = x.reshape(N * T, Fb, D).transpose(1, 0, 2)
        out = [lstm(xs, w[p + ".w_ih"][d], w[p + ".w_hh"][d], w[p + ".b_ih"][d], w[p + ".b_hh"][d], reverse=bool(d)) for d in range(2)]
        return np.concatenate(out, axis=2).transpose(1, 0, 2).reshape(N, T, Fb, -1)

    def _lstm_t(self, x, w_ih, w_hh, b_ih, b_hh):
        """x: (N, T, bins, in) -> (N, T, bins, H), the recurrence along time"""
        N, T, Fb, D = x.shape
        out = lstm(x.transpose(1, 0, 2, 3).reshape(T, N * Fb, D), w_ih, w_hh, b_ih, b_hh)
        return out.reshape(T, N, Fb, -1).transpose(1, 0, 2, 3)

    def _cfb(self, x, n):
        w = self.w
        g = _sig(self._ln(x, n + ".ln0") @ w[n + ".gate_w"].T + w[n + ".gate_b"])
        xi = x @ w[n + ".input_w"].T + w[n + ".input_b"]
        gx = g * xi
        y = self._ln(gx, n + ".ln1")
        yp = np.pad(y, ((0, 0), (0, 0), (1, 1), (0, 0)))
        cw = w[n + ".conv_w"]                                        # (out, in, tap)
        y = sum(yp[:, :, k:k + F] @ cw[:, :, k].T for k in range(3)) + w[n + ".conv_b"]
        z = self._ln(xi - gx, n + ".ln2")
        sp = np.einsum("mf,ntfc->ntmc", w["ceps_dft"], z)            # (N, T, 162, C): rows interleaved (re, im)
        N, T = sp.shape[:2]
        sp = sp.reshape(N, T, 81, 2 * C)                             # [re C | im C] per cepstral bin
        sr, si = sp[..., :C], sp[..., C:]
        lo = self._bilstm_f(self._ln(sp, n + ".ceps_ln"), n + ".lstm") @ w[n + ".lin_w"].T + w[n + ".lin_b"]
        pr, pi = lo[..., :C], lo[..., C:]
        packed = np.concatenate([pr * sr - pi * si, pr * si + pi * sr], axis=2)      # (N, T, 162, C)
        return y + np.einsum("fm,ntmc->ntfc", w["ceps_idft"], packed)

    def net(self, x, taps=None):
        """x: (N, T, 160, 4) [mix re, mix im, far re, far im] -> (N, T, 160, 2)"""
        w = self.w
        e0 = np.concatenate([self._bilstm_f(x, "in_lstm"), x], axis=-1) @ w["in_fused_w"].T + w["in_fused_b"]
        e = [e0]
        for n in CFB_NAMES[:5]:
            e.append(self._cfb(e[-1], n))
        h = self._ln(e[5], "ln")
        for layer in range(2):
            h = self._lstm_t(h, w[f"t_lstm.w_ih{layer}"], w[f"t_lstm.w_hh{layer}"], w[f"t_lstm.b_ih{layer}"], w[f"t_lstm.b_hh{layer}"])
        lstm_out = h @ w["t_lin_w"].T + w["t_lin_b"]
        d = self._cfb(e[5] * lstm_out, "d5")
        for k, n in zip((4, 3, 2, 1), CFB_NAMES[6:]):
            d = self._cfb(np.concatenate([e[k], d], axis=-1), n)
        d0 = self._lstm_t(np.concatenate([e0, d], axis=-1), w["out_lstm.w_ih"], w["out_lstm.w_hh"], w["out_lstm.b_ih"], w["out_lstm.b_hh"])
        out = np.concatenate([d0, d], axis=-1) @ w["out_fused_w"].T + w["out_fused_b"]
        if taps is not None:
            taps.update(e0=e0, e5=e[5], lstm_out=lstm_out, d1=d, spec_out=out)
        return out

    def forward(self, near, far, fold_window=0, int_in=True, int_out=True, want_taps=False):
        """near, far: (B, L) int16 (or normalised float with int_in=False) -> (int16 or float output (B, L), the waveform before the PCM scale, taps).
        fold_window: USE_BATCH_FOLD -- each window of a row is an independent clip."""
        w = self.w
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
        power = (re * re + im * im).sum(axis=2)                                         # (2 N, T)
        pp = np.pad(np.stack([power[:N], power[N:]], axis=1), ((0, 0), (0, 0), (K - 1, 0)))      # (N, [mix, far], K - 1 + T)
        alpha = w["alpha_bias"][0] + sum(pp[:, c, k:k + T] * w["alpha_kernel"][c, k] for c in range(2) for k in range(K))
        a = np.abs(alpha)[:, :, None]
        feat = np.stack([re[:N], im[:N], re[N:] * a, im[N:] * a], axis=-1)              # (N, T, 160, 4)
        taps = {"alpha": alpha} if want_taps else None
        out = self.net(feat, taps)
        frames = out[..., 0] @ ks_re + out[..., 1] @ ks_im                              # (N, T, 319)
        raw = np.zeros((N, NFFT + HOP * (T - 1)))
        for t in range(T):
            raw[:, t * HOP:t * HOP + NFFT] += frames[:, t]
        wave = (raw[:, NFFT // 2:NFFT // 2 + Wn] * inv_ws).reshape(B, L)
        res = np.trunc(np.clip(wave * 32767.0, -32768, 32767)).astype(np.int16) if int_out else wave.astype(np.float32)
        return res, wave, taps


def fixture_state(gold_dir, seed=0):
    """The sharded checkpoint-named fixture -> (iccrn_state, alpha_state)."""
    state = {}
    for p in sorted(glob.glob(os.path.join(gold_dir, f"sdaec_seed{seed}_state_*.npz"))):
        with np.load(p) as z:
            state.update({k: z[k] for k in z.files})
    return ({k: v for k, v in state.items() if not k.startswith("alpha.")}, {k[6:]: v for k, v in state.items() if k.startswith("alpha.")})
