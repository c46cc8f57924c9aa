"""NKF-AEC (NKF_AEC/Export_NKF_AEC.py): the neural Kalman filter for acoustic echo cancellation -- checkpoint keys -> engine blob, and the manifest.

The model takes two signals, the far-end reference and the near-end microphone, and returns the microphone with the echo of the far end removed.
At the C ABI it is a two-channel input (channel 0 = ``far_end_audio``, channel 1 = ``near_end_audio``, the export's input order :524) and a one-channel
output (``aec_audio``).  The engine (csrc/ade_nkf_aec.hip) holds the whole per-bin Kalman recurrence of one call in one kernel launch.

Blob tensors (real part first, imaginary part second on the leading axis of 2; the GRUs ``gru_r`` first, ``gru_i`` second):

    fc_in_w (2, 18, 9)    fc_in_b (2, 18)    fc_in_slope (1)          ComplexDense(2L+1, 18) + ComplexPReLU   (:160-162)
    gru_w_ih (2, 54, 18)  gru_w_hh (2, 54, 18)  gru_b_ih (2, 54)  gru_b_hh (2, 54)     the two nn.GRU of ComplexGRU (:68-69), PyTorch gate order r, z, n
    fc_out1_w (2, 18, 18) fc_out1_b (2, 18)  fc_out_slope (1)         ComplexDense(18, 18) + ComplexPReLU     (:168-169)
    fc_out2_w (2, 4, 18)  fc_out2_b (2, 4)                             ComplexDense(18, L)                      (:170)
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Mapping

import numpy as np

from .metadata import build_audio_metadata

FILTER_ORDER, FC_DIM, RNN_DIM = 4, 18, 18          # (Export_NKF_AEC.py:51-54)
NFFT, HOP = 1024, 256
N_BINS = NFFT // 2 + 1


def state_to_blob_tensors(sd: Mapping[str, np.ndarray]) -> "OrderedDict[str, np.ndarray]":
    """The checkpoint's state dict (``nkf_epoch70.pt``; key names of ``load_nkf_weights``, Export_NKF_AEC.py:414-455) -> the blob tensors."""
    def g(k):
        if k not in sd:
            raise KeyError(f"NKF checkpoint: missing tensor {k}")
        return np.asarray(sd[k], np.float32)

    def dense(prefix):
        return (np.stack([g(prefix + ".linear_real.weight"), g(prefix + ".linear_imag.weight")]),
                np.stack([g(prefix + ".linear_real.bias"), g(prefix + ".linear_imag.bias")]))
    out = OrderedDict()
    out["fc_in_w"], out["fc_in_b"] = dense("kg_net.fc_in.0")
    out["fc_in_slope"] = g("kg_net.fc_in.1.prelu.weight").reshape(1)            # nn.PReLU(): one slope (:136)
    for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
        name = {"weight_ih": "gru_w_ih", "weight_hh": "gru_w_hh", "bias_ih": "gru_b_ih", "bias_hh": "gru_b_hh"}[p]
        out[name] = np.stack([g(f"kg_net.complex_gru.gru_r.{p}_l0"), g(f"kg_net.complex_gru.gru_i.{p}_l0")])
    out["fc_out1_w"], out["fc_out1_b"] = dense("kg_net.fc_out.0")
    out["fc_out_slope"] = g("kg_net.fc_out.1.prelu.weight").reshape(1)
    out["fc_out2_w"], out["fc_out2_b"] = dense("kg_net.fc_out.2")
    shapes = {"fc_in_w": (2, FC_DIM, 2 * FILTER_ORDER + 1), "fc_in_b": (2, FC_DIM), "gru_w_ih": (2, 3 * RNN_DIM, FC_DIM), "gru_w_hh": (2, 3 * RNN_DIM, RNN_DIM),
              "gru_b_ih": (2, 3 * RNN_DIM), "gru_b_hh": (2, 3 * RNN_DIM), "fc_out1_w": (2, FC_DIM, RNN_DIM), "fc_out1_b": (2, FC_DIM),
              "fc_out2_w": (2, FILTER_ORDER, FC_DIM), "fc_out2_b": (2, FILTER_ORDER)}
    for k, s in shapes.items():
        if out[k].shape != s:
            raise ValueError(f"NKF checkpoint: {k} has shape {out[k].shape}, expected {s}")
    return out


def metadata(input_audio_length: int = 32000, use_batch_fold: bool = False, out_sample_rate: int = 16000, input_audio_dtype: str = "INT16",
             output_audio_dtype: str = "INT16", name: str = "NKF_AEC") -> Dict[str, str]:
    """The manifest Export_NKF_AEC.py:543-548 stamps: static axes only, 16 kHz in and model rate, any output rate."""
    return build_audio_metadata(producer="export.py", model_name=name, task="aec", model_family="nkf_aec", input_audio_length=input_audio_length,
                                in_sample_rate=16000, out_sample_rate=out_sample_rate, model_sample_rate=16000, nfft=NFFT, window_length=NFFT,
                                hop_length=HOP, window_type="hann", center_pad=True, pad_mode="constant", dynamic_axes=False,
                                input_audio_dtype=input_audio_dtype, output_audio_dtype=output_audio_dtype, max_dynamic_audio_seconds=4,
                                use_batch_fold=use_batch_fold, input_channels=1, output_channels=1, num_audio_inputs=2,
                                feature_kind="stft_kalman_filter",
                                extra={"filter_order": FILTER_ORDER, "fc_dim": FC_DIM, "rnn_layers": 1, "rnn_dim": RNN_DIM})
