"""Deep Echo AEC (Deep_Echo_AEC/Export_Deep_Echo.py): the ICCRN echo-path estimator -- checkpoint keys -> engine blob, and the manifest.

Two inputs, the near-end microphone first and the far-end reference second (the export's input order, :490), one output (``aec_audio``).  At the C ABI
the call is a two-channel planar row (channel 0 = near end).  The engine is csrc/ade_deep_echo.hip.

``state_to_blob_tensors`` does on the host what the reference does after loading the checkpoint, and what the engine's kernels expect:
    * every LayerNorm (:181-208, with ``fuse_layer_norm_scales_``, :211-214) as the ``(w, b, eps)`` triple of the (x - mean) * rsqrt(var + eps) * w + b form
      -> ``*_w`` / ``*_b`` in (bins, channels) layout and ``*_eps`` (``fold_layernorm``);
    * the Linear behind ``in_ch_lstm`` folded into ``in_conv`` (:319-320) and the one behind ``out_ch_lstm`` into ``out_conv`` (:338-339), in float64
      (``sdaec.fuse_linear``: the two networks agree here);
    * the two cepstral tables, the 160-point real DFT (162 x 160) and its pseudo-inverse (160 x 162) (:133-153), shared by both CFBs (:316).

Blob tensors (LSTMs keep PyTorch's layout, gate order i, f, g, o; a leading axis of 2 is (forward, reverse)):
    in_lstm.{w_ih (2, 80, 4), w_hh (2, 80, 20), b_ih (2, 80), b_hh (2, 80)}    in_fused_w (20, 44)  in_fused_b (20)
        the 4 inputs are [near re, far re, near im, far im] (:398-401)
    per CFB n in e1, d1:
        n.ln0_{w,b}, n.ln1_{w,b}, n.ln2_{w,b} (160, 20)  n.ceps_ln_{w,b} (81, 40)  n.*_eps (1)
        n.gate_{w (20, 20), b (20)}  n.input_{w, b}  n.conv_w (20, 20, 3)  n.conv_b (20)
        n.lstm.{w_ih (2, 80, 40), w_hh (2, 80, 20), b_ih, b_hh (2, 80)}  n.lin_w (40, 40)  n.lin_b (40)
    ln_{w,b} (160, 20)  ln_eps (1)
    t_lstm.{w_ih0 (160, 20), w_hh0 (160, 40), b_ih0, b_hh0 (160), w_ih1 (160, 40), w_hh1 (160, 40), b_ih1, b_hh1}  t_lin_w (20, 40)  t_lin_b (20)
    out_lstm.{w_ih (80, 40), w_hh (80, 20), b_ih, b_hh (80)}
    echo_w (20, 40)  echo_b (20)      the echo path from [h of out_ch_lstm | d1]: row c is (re / im = c // 10, tap = c % 10) (:340)
    ceps_dft (162, 160)   ceps_idft (160, 162)
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Mapping

import numpy as np

from .metadata import build_audio_metadata
from .sdaec import BINS, CEPS_BINS, CH, HOP, NFFT, cepstral_tables, frames_of, fuse_linear  # noqa: F401  (frames_of: MODEL_STFT_FRAMES, :49)

ECHO_ORDER = 10
CFB_NAMES = ("e1", "d1")


def fold_layernorm(w: np.ndarray, b: np.ndarray):
    """LayerNorm.w / .b of shape (1, c, f, 1) -> (w', b', eps') in (f, c) layout, for (x - mean) * rsqrt(var + eps') * w' + b' with var the MEAN of the
    centred squares over the n = c * f elements.

    The reference computes (x - mean) * rsqrt(sum((x - mean)^2) + 1e-8 (n - 1)) * w sqrt(n - 1) + b (:200-208 with :193-198).  The sum is n * var, so
    rsqrt(sum + E) = rsqrt(var + E / n) / sqrt(n):  w' = w sqrt((n - 1) / n),  eps' = 1e-8 (n - 1) / n.  Folded in float64, rounded once.

    The cepstral LayerNorm's sum_scale = 0.25 (:129, :204-206) multiplies x by 2^-2 and eps by 2^-4: rsqrt(2^-4 (sum + E)) = 4 rsqrt(sum + E), and
    0.25 x * 4 rsqrt(.) = x rsqrt(.).  Powers of two rescale fp32 values exactly, so the factor folds away without a trace and is not an argument here."""
    w, b = np.asarray(w, np.float32), np.asarray(b, np.float32)
    n = float(w.shape[1] * w.shape[2])
    ew = (w[0, :, :, 0].T.astype(np.float64) * np.sqrt((n - 1.0) / n)).astype(np.float32)
    return np.ascontiguousarray(ew), np.ascontiguousarray(b[0, :, :, 0].T), np.asarray([1e-8 * (n - 1.0) / n], np.float32)


def state_to_blob_tensors(state: Mapping[str, np.ndarray]) -> "OrderedDict[str, np.ndarray]":
    """``model.ckpt`` (module paths of ``NET``, after ``export.extract_state_dict``) -> the blob tensors."""
    def g(k, shape):
        if k not in state:
            raise KeyError(f"Deep Echo checkpoint: missing tensor {k}")
        v = np.asarray(state[k], np.float32)
        if v.shape != tuple(shape):
            raise ValueError(f"Deep Echo checkpoint: {k} has shape {v.shape}, expected {tuple(shape)}")
        return v

    def lstm(prefix, n_in, hid, suffixes):
        return {p: np.stack([g(f"{prefix}.{q}_l0{s}", sh) for s in suffixes]) if len(suffixes) > 1 else g(f"{prefix}.{q}_l0", sh)
                for p, q, sh in (("w_ih", "weight_ih", (4 * hid, n_in)), ("w_hh", "weight_hh", (4 * hid, hid)), ("b_ih", "bias_ih", (4 * hid,)),
                                 ("b_hh", "bias_hh", (4 * hid,)))}

    def ln(dst, name, prefix, c, f):
        dst[name + "_w"], dst[name + "_b"], dst[name + "_eps"] = fold_layernorm(g(prefix + ".w", (1, c, f, 1)), g(prefix + ".b", (1, c, f, 1)))

    out = OrderedDict()
    for p, v in lstm("in_ch_lstm.lstm2", 4, CH, ("", "_reverse")).items():
        out["in_lstm." + p] = v
    out["in_fused_w"], out["in_fused_b"] = fuse_linear(g("in_conv.weight", (CH, CH + 4, 1, 1))[:, :, 0, 0], g("in_conv.bias", (CH,)),
                                                       g("in_ch_lstm.linear.weight", (CH, 2 * CH)), g("in_ch_lstm.linear.bias", (CH,)))
    for n in CFB_NAMES:
        m = "cfb_" + n
        ln(out, f"{n}.ln0", m + ".LN0", CH, BINS)
        ln(out, f"{n}.ln1", m + ".LN1", CH, BINS)
        ln(out, f"{n}.ln2", m + ".LN2", CH, BINS)
        ln(out, f"{n}.ceps_ln", m + ".ceps_unit.LN", 2 * CH, CEPS_BINS)
        out[f"{n}.gate_w"], out[f"{n}.gate_b"] = g(m + ".conv_gate.weight", (CH, CH, 1, 1))[:, :, 0, 0].copy(), g(m + ".conv_gate.bias", (CH,))
        out[f"{n}.input_w"], out[f"{n}.input_b"] = g(m + ".conv_input.weight", (CH, CH, 1, 1))[:, :, 0, 0].copy(), g(m + ".conv_input.bias", (CH,))
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
    out["echo_w"], out["echo_b"] = fuse_linear(g("out_conv.weight", (2 * ECHO_ORDER, 3 * CH, 1, 1))[:, :, 0, 0], g("out_conv.bias", (2 * ECHO_ORDER,)),
                                               g("out_ch_lstm.linear.weight", (2 * CH, CH)), g("out_ch_lstm.linear.bias", (2 * CH,)))
    out["ceps_dft"], out["ceps_idft"] = cepstral_tables()
    return OrderedDict((k, np.ascontiguousarray(v, np.float32)) for k, v in out.items())


def metadata(input_audio_length: int = 32000, use_batch_fold: bool = False, out_sample_rate: int = 16000, input_audio_dtype: str = "INT16",
             output_audio_dtype: str = "INT16", name: str = "Deep_Echo_AEC") -> Dict[str, str]:
    """The manifest Export_Deep_Echo.py:505-510 stamps for its static export: 16 kHz in and model rate, any output rate.  A folded export (1.5 s windows
    of 24000 samples, :39-47) sizes its frames from one window."""
    fold = ((int(1.5 * 16000) + HOP - 1) // HOP) * HOP
    return build_audio_metadata(producer="export.py", model_name=name, task="aec", model_family="deep_echo", input_audio_length=input_audio_length,
                                in_sample_rate=16000, out_sample_rate=out_sample_rate, model_sample_rate=16000, nfft=NFFT, window_length=NFFT,
                                hop_length=HOP, window_type="hamming", center_pad=True, pad_mode="constant", dynamic_axes=False,
                                input_audio_dtype=input_audio_dtype, output_audio_dtype=output_audio_dtype, max_dynamic_audio_seconds=30,
                                use_batch_fold=use_batch_fold, input_channels=1, output_channels=1, num_audio_inputs=2, feature_kind="stft",
                                extra={"echo_order": ECHO_ORDER, "max_signal_length": frames_of(fold if use_batch_fold else input_audio_length)})
