"""SDAEC (SDAEC/Export_SDAEC.py): the ICCRN echo canceller with its alpha predictor -- checkpoint keys -> engine blob, and the manifest.

Two inputs, the near-end microphone first and the far-end reference second (the export's input order, :501), one output (``aec_audio``).  At the C ABI
the call is a two-channel planar row (channel 0 = near end).  The engine is csrc/ade_sdaec.hip.

``state_to_blob_tensors`` does on the host what the reference does after loading the two checkpoints:
    * every LayerNorm: ``fuse_var_scale_`` (:144-149) and ``prepare_for_export_`` (:151-163) -> ``*_w`` / ``*_b`` in (bins, channels) layout and ``*_eps``;
    * the Linear behind ``in_ch_lstm`` folded into ``in_conv`` and the one behind ``out_ch_lstm`` into ``out_conv``, in float64 (:239-259);
    * the alpha predictor's two Linears as one causal 10-tap, 2-channel kernel and bias (:372-379);
    * the two cepstral tables, the 160-point real DFT (162 x 160) and its pseudo-inverse (160 x 162) (:208-221).

Blob tensors (LSTMs keep PyTorch's layout, gate order i, f, g, o; a leading axis of 2 is (forward, reverse)):
    alpha_kernel (2, 10) [mix, far]   alpha_bias (1)
    in_lstm.{w_ih (2, 80, 4), w_hh (2, 80, 20), b_ih (2, 80), b_hh (2, 80)}    in_fused_w (20, 44)  in_fused_b (20)
    per CFB n in e1..e5, d5..d1 (C_in = 20, or 40 for d4..d1):
        n.ln0_{w,b} (160, C_in)  n.ln1_{w,b}, n.ln2_{w,b} (160, 20)  n.ceps_ln_{w,b} (81, 40)  n.*_eps (1)
        n.gate_{w (20, C_in), b (20)}  n.input_{w, b}  n.conv_w (20, 20, 3)  n.conv_b (20)
        n.lstm.{w_ih (2, 80, 40), w_hh (2, 80, 20), b_ih, b_hh (2, 80)}  n.lin_w (40, 40)  n.lin_b (40)
    ln_{w,b} (160, 20)  ln_eps (1)
    t_lstm.{w_ih0 (160, 20), w_hh0 (160, 40), b_ih0, b_hh0 (160), w_ih1 (160, 40), w_hh1 (160, 40), b_ih1, b_hh1}  t_lin_w (20, 40)  t_lin_b (20)
    out_lstm.{w_ih (80, 40), w_hh (80, 20), b_ih, b_hh (80)}    out_fused_w (2, 40)  out_fused_b (2)
    ceps_dft (162, 160)   ceps_idft (160, 162)
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Mapping

import numpy as np

from .metadata import build_audio_metadata

NFFT, HOP, BINS, CH, ALPHA_K = 319, 160, 160, 20, 10
CEPS_BINS = BINS // 2 + 1
CFB_NAMES = ("e1", "e2", "e3", "e4", "e5", "d5", "d4", "d3", "d2", "d1")
CFB_IN = {n: (2 * CH if n in ("d4", "d3", "d2", "d1") else CH) for n in CFB_NAMES}


def frames_of(length: int) -> int:
    """STATIC_SIGNAL_LENGTH (:33): frames of the centred 319 / 160 STFT."""
    return (length - 1) // HOP + 1


def cepstral_tables():
    """The 160-point real DFT with interleaved (re, im) rows, fp32 angles as :210-215 forms them, and the pseudo-inverse of the stacked
    (re rows | im rows) basis (:216-221), computed in float64."""
    t = np.arange(BINS, dtype=np.float32)[None, :]
    f = np.arange(CEPS_BINS, dtype=np.float32)[:, None]
    omega = (np.float32(2.0 * np.pi) * f * t / np.float32(BINS)).astype(np.float32)
    dft = np.stack([np.cos(omega.astype(np.float64)), -np.sin(omega.astype(np.float64))], axis=1).reshape(2 * CEPS_BINS, BINS).astype(np.float32)
    basis = np.fft.fft(np.eye(BINS))[:CEPS_BINS]
    idft = np.linalg.pinv(np.vstack([basis.real, basis.imag])).astype(np.float32)          # (160, 162): columns [re bins | im bins]
    return dft, np.ascontiguousarray(idft)


def fold_layernorm(w: np.ndarray, b: np.ndarray):
    """LayerNorm.w / .b of shape (1, c, f, 1) -> (export_w, export_b, export_eps) in (f, c) layout (:144-163)."""
    w, b = np.asarray(w, np.float32), np.asarray(b, np.float32)
    reduced = w.shape[1] * w.shape[2]
    scale = np.float32(float(max(reduced - 1, 1)) ** 0.5)
    ew = ((w * scale)[0, :, :, 0].T / np.float32(float(reduced) ** 0.5)).astype(np.float32)
    return np.ascontiguousarray(ew), np.ascontiguousarray(b[0, :, :, 0].T), np.asarray([1e-6 * float(reduced - 1) / float(reduced)], np.float32)


def fuse_linear(conv_w: np.ndarray, conv_b: np.ndarray, lin_w: np.ndarray, lin_b: np.ndarray):
    """conv(cat([linear(h), x])) -> one Linear on cat([h, x]), in float64 (:239-259)."""
    cw, lw = np.asarray(conv_w, np.float32).astype(np.float64), np.asarray(lin_w, np.float32).astype(np.float64)
    proj = cw[:, :lw.shape[0]]
    w = np.concatenate([proj @ lw, cw[:, lw.shape[0]:]], axis=1).astype(np.float32)
    b = (np.asarray(conv_b, np.float32).astype(np.float64) + proj @ np.asarray(lin_b, np.float32).astype(np.float64)).astype(np.float32)
    return np.ascontiguousarray(w), b


def fuse_alpha(l1w, l1b, l2w, l2b):
    """AlphaPredictor's linear1 (2 -> 1) and linear2 (k -> 1) as a (2, k) kernel [mix, far] and a bias, in fp32 as :372-377."""
    l1w, l1b = np.asarray(l1w, np.float32).reshape(2), np.asarray(l1b, np.float32).reshape(1)
    l2w, l2b = np.asarray(l2w, np.float32).reshape(-1), np.asarray(l2b, np.float32).reshape(1)
    bias = (l2b + l2w.sum(dtype=np.float32) * l1b[0]).astype(np.float32)
    return np.stack([l2w * l1w[1], l2w * l1w[0]]).astype(np.float32), bias


def state_to_blob_tensors(iccrn_state: Mapping[str, np.ndarray], alpha_state: Mapping[str, np.ndarray]) -> "OrderedDict[str, np.ndarray]":
    """``ICCRN.ckpt`` (module paths of ``NET``) and ``alpha.ckpt`` (``AlphaPredictor``) -> the blob tensors."""
    def g(k, shape, sd=iccrn_state, what="ICCRN"):
        if k not in sd:
            raise KeyError(f"SDAEC {what} checkpoint: missing tensor {k}")
        v = np.asarray(sd[k], np.float32)
        if v.shape != tuple(shape):
            raise ValueError(f"SDAEC {what} checkpoint: {k} has shape {v.shape}, expected {tuple(shape)}")
        return v

    def lstm(prefix, n_in, hid, suffixes):
        return {p: np.stack([g(f"{prefix}.{q}_l0{s}", sh) for s in suffixes]) if len(suffixes) > 1 else g(f"{prefix}.{q}_l0", sh)
                for p, q, sh in (("w_ih", "weight_ih", (4 * hid, n_in)), ("w_hh", "weight_hh", (4 * hid, hid)), ("b_ih", "bias_ih", (4 * hid,)),
                                 ("b_hh", "bias_hh", (4 * hid,)))}

    def ln(dst, name, prefix, c, f):
        dst[name + "_w"], dst[name + "_b"], dst[name + "_eps"] = fold_layernorm(g(prefix + ".w", (1, c, f, 1)), g(prefix + ".b", (1, c, f, 1)))

    out = OrderedDict()
    ga = lambda k, shape: g(k, shape, alpha_state, "alpha")        # noqa: E731
    out["alpha_kernel"], out["alpha_bias"] = fuse_alpha(ga("linear1.weight", (1, 2)), ga("linear1.bias", (1,)), ga("linear2.weight", (1, ALPHA_K)),
                                                        ga("linear2.bias", (1,)))
    for p, v in lstm("in_ch_lstm.lstm2", 4, CH, ("", "_reverse")).items():
        out["in_lstm." + p] = v
    out["in_fused_w"], out["in_fused_b"] = fuse_linear(g("in_conv.weight", (CH, CH + 4, 1, 1))[:, :, 0, 0], g("in_conv.bias", (CH,)),
                                                       g("in_ch_lstm.linear.weight", (CH, 2 * CH)), g("in_ch_lstm.linear.bias", (CH,)))
    for n in CFB_NAMES:
        m, cin = "cfb_" + n, CFB_IN[n]
        ln(out, f"{n}.ln0", m + ".LN0", cin, BINS)
        ln(out, f"{n}.ln1", m + ".LN1", CH, BINS)
        ln(out, f"{n}.ln2", m + ".LN2", CH, BINS)
        ln(out, f"{n}.ceps_ln", m + ".ceps_unit.LN", 2 * CH, CEPS_BINS)
        out[f"{n}.gate_w"], out[f"{n}.gate_b"] = g(m + ".conv_gate.weight", (CH, cin, 1, 1))[:, :, 0, 0].copy(), g(m + ".conv_gate.bias", (CH,))
        out[f"{n}.input_w"], out[f"{n}.input_b"] = g(m + ".conv_input.weight", (CH, cin, 1, 1))[:, :, 0, 0].copy(), g(m + ".conv_input.bias", (CH,))
        out[f"{n}.conv_w"], out[f"{n}.conv_b"] = g(m + ".conv.weight", (CH, CH, 3, 1))[:, :, :, 0].copy(), g(m + ".conv.bias", (CH,))
        for p, v in lstm(m + ".ceps_unit.ch_lstm_f.lstm2", 2 * CH, CH, ("", "_reverse")).items():
            out[f"{n}.lstm.{p}"] = v
        out[f"{n}.lin_w"], out[f"{n}.lin_b"] = g(m + ".ceps_unit.ch_lstm_f.linear.weight", (2 * CH, 2 * CH)), g(m + ".ceps_unit.ch_lstm_f.linear.bias", (2 * CH,))
    ln(out, "ln", "ln", CH, BINS)
    for layer, n_in in ((0, CH), (1, 2 * CH)):
        for p, q, sh in (("w_ih", "weight_ih", (8 * CH, n_in)), ("w_hh", "weight_hh", (8 * CH, 2 * CH)), ("b_ih", "bias_ih", (8 * CH,)), ("b_hh", "bias_hh", (8 * CH,))):
            out[f"t_lstm.{p}{layer}"] = g(f"ch_lstm.lstm2.{q}_l{layer}", sh)
    out["t_lin_w"], out["t_lin_b"] = g("ch_lstm.linear.weight", (CH, 2 * CH)), g("ch_lstm.linear.bias", (CH,))
    for p, v in lstm("out_ch_lstm.lstm2", 2 * CH, CH, ("",)).items():
        out["out_lstm." + p] = v
    out["out_fused_w"], out["out_fused_b"] = fuse_linear(g("out_conv.weight", (2, 3 * CH, 1, 1))[:, :, 0, 0], g("out_conv.bias", (2,)),
                                                         g("out_ch_lstm.linear.weight", (2 * CH, CH)), g("out_ch_lstm.linear.bias", (2 * CH,)))
    out["ceps_dft"], out["ceps_idft"] = cepstral_tables()
    return OrderedDict((k, np.ascontiguousarray(v, np.float32)) for k, v in out.items())


def metadata(input_audio_length: int = 32000, use_batch_fold: bool = False, out_sample_rate: int = 16000, input_audio_dtype: str = "INT16",
             output_audio_dtype: str = "INT16", name: str = "SDAEC") -> Dict[str, str]:
    """The manifest Export_SDAEC.py:517-521 stamps: static axes only, 16 kHz in and model rate, any output rate.  A folded export (1.5 s windows of
    24000 samples, :42-51) sizes its frames from one window."""
    fold = ((int(1.5 * 16000) + HOP - 1) // HOP) * HOP
    return build_audio_metadata(producer="export.py", model_name=name, task="aec", model_family="sdaec", input_audio_length=input_audio_length,
                                in_sample_rate=16000, out_sample_rate=out_sample_rate, model_sample_rate=16000, nfft=NFFT, window_length=NFFT,
                                hop_length=HOP, window_type="hamming", center_pad=True, pad_mode="constant", dynamic_axes=False,
                                input_audio_dtype=input_audio_dtype, output_audio_dtype=output_audio_dtype, max_dynamic_audio_seconds=30,
                                use_batch_fold=use_batch_fold, input_channels=1, output_channels=1, num_audio_inputs=2,
                                feature_kind="stft_alpha_predictor",
                                extra={"alpha_k": ALPHA_K, "max_signal_length": frames_of(fold if use_batch_fold else input_audio_length)})
