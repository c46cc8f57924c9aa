"""Counter-based weight generator: reproducible "seeded weights" for models whose tensors are too large to commit.

Mel-Band-Roformer's fused buffers hold ~208 M floats at depth 1 (the 60-band mask estimator alone is 141.6 M,
Mel_Band_Roformer/Stereo/Export_MelBandRoformer.py:499-502) -- 0.8 GB cannot be a fixture, and torch's RNG stream is
not reproducible outside torch.  Every value is instead a pure function of (tensor name, flat index, seed):

    value[i] = scale * (2 * u - 1),  u = top 24 bits of splitmix64(fnv1a64(name) ^ seed * GOLDEN + i) / 2^24

so the golden-vector script (which overwrites the reference module's buffers with these values before running it), the
oracle and the engine-side tests all materialise identical tensors from a (name, shape, scale) list.
"""
from __future__ import annotations

from typing import Dict, Iterable, Sequence, Tuple

import numpy as np

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def fnv1a64(name: str) -> np.uint64:
    h = 0xCBF29CE484222325
    for b in name.encode():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return np.uint64(h)


def splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = x + _GOLDEN
        z = x
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def tensor(name: str, shape: Sequence[int], scale: float, seed: int = 0) -> np.ndarray:
    n = int(np.prod(shape)) if len(shape) else 1
    with np.errstate(over="ignore"):
        base = fnv1a64(name) ^ (np.uint64(seed) * _GOLDEN)
        out = np.empty(n, np.float32)
        step = 1 << 24
        for lo in range(0, n, step):                       # chunked: bounds the uint64 scratch for the 141 M-float tensor
            idx = np.arange(lo, min(n, lo + step), dtype=np.uint64)
            bits = splitmix64(base + idx) >> np.uint64(40)                     # top 24 bits
            out[lo:lo + idx.size] = (bits.astype(np.float32) * np.float32(2.0 / (1 << 24)) - np.float32(1.0)) * np.float32(scale)
    return out.reshape(tuple(shape))


def materialise(spec: Iterable[Tuple[str, Sequence[int], float]], seed: int = 0) -> Dict[str, np.ndarray]:
    return {name: tensor(name, shape, scale, seed) for name, shape, scale in spec}


# NKF-AEC seeded weights (tools/make_golden_nkf_aec.py): PyTorch's default initialisation under torch.manual_seed(seed), with the Kalman-gain layer
# fc_out_dense2 (weight and bias) multiplied by this factor.  The per-bin Kalman recurrence is only stable with a small gain: default init, or more than
# about 0.03 x default on that layer, diverges (NaN or a 10 x output RMS), and fp32 evaluations of a diverging filter disagree by tens of LSB.
NKF_GAIN_LAYER_SCALE = 1e-2


def dfsmn_aec_state(seed: int = 0, width: int = 128, hidden: int = 64, depth: int = 6, lorder: int = 20, dilation: int = 2):
    """Seeded DFSMN-AEC weights for benchmarks and smoke runs: ``(nkf_state, dfsmn_state, skip_connect, dilation)``, the arguments of
    ``dfsmn_aec.state_to_blob_tensors``.  The NKF half is uniform in +- 1 / sqrt(fan_in) (PyTorch's default range) with the Kalman-gain layer scaled by
    NKF_GAIN_LAYER_SCALE (the stability rule above); the DFSMN half has the attribute paths of the ModelScope network, scaled so that activations stay of order
    one, and a feature shift / scale that centres int16-scale log-mel energies."""
    L, fc, rnn, feat, bins = 4, 18, 18, 240, 321
    nkf = {}

    def put(dst, name, shape, fan_in, gain=1.0):
        dst[name] = tensor(name, shape, gain / np.sqrt(fan_in), seed)

    for part in ("real", "imag"):
        put(nkf, f"kg_net.fc_in.0.linear_{part}.weight", (fc, 2 * L + 1), 2 * L + 1)
        put(nkf, f"kg_net.fc_in.0.linear_{part}.bias", (fc,), 2 * L + 1)
        put(nkf, f"kg_net.fc_out.0.linear_{part}.weight", (fc, rnn), rnn)
        put(nkf, f"kg_net.fc_out.0.linear_{part}.bias", (fc,), rnn)
        put(nkf, f"kg_net.fc_out.2.linear_{part}.weight", (L, fc), fc, NKF_GAIN_LAYER_SCALE)
        put(nkf, f"kg_net.fc_out.2.linear_{part}.bias", (L,), fc, NKF_GAIN_LAYER_SCALE)
    for g in ("gru_r", "gru_i"):
        put(nkf, f"kg_net.complex_gru.{g}.weight_ih_l0", (3 * rnn, fc), rnn)
        put(nkf, f"kg_net.complex_gru.{g}.weight_hh_l0", (3 * rnn, rnn), rnn)
        put(nkf, f"kg_net.complex_gru.{g}.bias_ih_l0", (3 * rnn,), rnn)
        put(nkf, f"kg_net.complex_gru.{g}.bias_hh_l0", (3 * rnn,), rnn)
    nkf["kg_net.fc_in.1.prelu.weight"] = np.full((1,), 0.25, np.float32)
    nkf["kg_net.fc_out.1.prelu.weight"] = np.full((1,), 0.25, np.float32)
    net = {}
    put(net, "linear1.linear.weight", (width, feat), feat, 1.0)
    put(net, "linear1.linear.bias", (width,), 100.0)
    for i in range(depth):
        put(net, f"deepfsmn.{i}.linear.weight", (hidden, width), width, 2.0)
        put(net, f"deepfsmn.{i}.linear.bias", (hidden,), 100.0)
        put(net, f"deepfsmn.{i}.project.weight", (width, hidden), hidden, 1.2)
        put(net, f"deepfsmn.{i}.conv1.weight", (width, 1, lorder, 1), 50.0)
    put(net, "linear2.weight", (bins, width), width, 0.9)
    put(net, "linear2.bias", (bins,), 100.0)
    put(net, "linear3.weight", (1, width), width, 0.9)
    put(net, "linear3.bias", (1,), 100.0)
    net["feature.shift"] = np.full((feat,), -15.0, np.float32)
    net["feature.scale"] = np.full((feat,), 0.2, np.float32)
    return nkf, net, [i % 2 == 0 for i in range(depth)], [dilation] * depth


def sdaec_state(seed: int = 0):
    """Seeded SDAEC weights for benchmarks and smoke runs: ``(iccrn_state, alpha_state)`` under the two checkpoints' key names, the arguments of
    ``sdaec.state_to_blob_tensors``.  Linear / Conv / LSTM tensors are uniform in +- 1 / sqrt(fan_in) (PyTorch's default range), every LayerNorm has unit
    weight and a bias of order 1e-4 (the module's own initialisation)."""
    C, F, FC, K = 20, 160, 81, 10
    net, alpha = {}, {}

    def put(dst, name, shape, fan_in):
        dst[name] = tensor(name, shape, 1.0 / np.sqrt(fan_in), seed)

    def lstm(prefix, n_in, hid, layers, bi):
        for layer in range(layers):
            for suffix in ("", "_reverse") if bi else ("",):
                put(net, f"{prefix}.weight_ih_l{layer}{suffix}", (4 * hid, n_in if layer == 0 else hid * (2 if bi else 1)), hid)
                put(net, f"{prefix}.weight_hh_l{layer}{suffix}", (4 * hid, hid), hid)
                put(net, f"{prefix}.bias_ih_l{layer}{suffix}", (4 * hid,), hid)
                put(net, f"{prefix}.bias_hh_l{layer}{suffix}", (4 * hid,), hid)

    def layernorm(prefix, c, f):
        net[prefix + ".w"] = np.ones((1, c, f, 1), np.float32)
        net[prefix + ".b"] = np.abs(tensor(prefix + ".b", (1, c, f, 1), 1e-4, seed))

    lstm("in_ch_lstm.lstm2", 4, C, 1, True)
    put(net, "in_ch_lstm.linear.weight", (C, 2 * C), 2 * C)
    put(net, "in_ch_lstm.linear.bias", (C,), 2 * C)
    put(net, "in_conv.weight", (C, C + 4, 1, 1), C + 4)
    put(net, "in_conv.bias", (C,), C + 4)
    for n in ("e1", "e2", "e3", "e4", "e5", "d5", "d4", "d3", "d2", "d1"):
        m, cin = "cfb_" + n, (2 * C if n in ("d4", "d3", "d2", "d1") else C)
        for conv in ("conv_gate", "conv_input"):
            put(net, f"{m}.{conv}.weight", (C, cin, 1, 1), cin)
            put(net, f"{m}.{conv}.bias", (C,), cin)
        put(net, f"{m}.conv.weight", (C, C, 3, 1), 3 * C)
        put(net, f"{m}.conv.bias", (C,), 3 * C)
        layernorm(m + ".LN0", cin, F)
        layernorm(m + ".LN1", C, F)
        layernorm(m + ".LN2", C, F)
        layernorm(m + ".ceps_unit.LN", 2 * C, FC)
        lstm(m + ".ceps_unit.ch_lstm_f.lstm2", 2 * C, C, 1, True)
        put(net, m + ".ceps_unit.ch_lstm_f.linear.weight", (2 * C, 2 * C), 2 * C)
        put(net, m + ".ceps_unit.ch_lstm_f.linear.bias", (2 * C,), 2 * C)
    layernorm("ln", C, F)
    lstm("ch_lstm.lstm2", C, 2 * C, 2, False)
    put(net, "ch_lstm.linear.weight", (C, 2 * C), 2 * C)
    put(net, "ch_lstm.linear.bias", (C,), 2 * C)
    lstm("out_ch_lstm.lstm2", 2 * C, C, 1, False)
    put(net, "out_ch_lstm.linear.weight", (2 * C, C), C)
    put(net, "out_ch_lstm.linear.bias", (2 * C,), C)
    put(net, "out_conv.weight", (2, 3 * C, 1, 1), 3 * C)
    put(net, "out_conv.bias", (2,), 3 * C)
    put(alpha, "linear1.weight", (1, 2), 2)
    put(alpha, "linear1.bias", (1,), 2)
    put(alpha, "linear2.weight", (1, K), K)
    put(alpha, "linear2.bias", (1,), K)
    return net, alpha


def deep_echo_state(seed: int = 0):
    """Seeded Deep Echo weights for benchmarks: the state of ``NET`` under the checkpoint's key names, the argument of ``deep_echo.state_to_blob_tensors``.
    SDAEC's ICCRN state cut down to the two CFBs this network has, with the 20-channel echo-path ``out_conv`` (10 taps x (re, im))."""
    C, K = 20, 10
    net, _ = sdaec_state(seed)
    net = {k: v for k, v in net.items() if not k.startswith("cfb_") or k.startswith(("cfb_e1.", "cfb_d1."))}
    for conv in ("conv_gate", "conv_input"):
        net[f"cfb_d1.{conv}.weight"] = tensor(f"deep_echo.cfb_d1.{conv}.weight", (C, C, 1, 1), 1.0 / np.sqrt(C), seed)
    net["cfb_d1.LN0.w"] = np.ones((1, C, 160, 1), np.float32)
    net["cfb_d1.LN0.b"] = np.abs(tensor("deep_echo.cfb_d1.LN0.b", (1, C, 160, 1), 1e-4, seed))
    net["out_conv.weight"] = tensor("deep_echo.out_conv.weight", (2 * K, 3 * C, 1, 1), 1.0 / np.sqrt(3 * C), seed)
    net["out_conv.bias"] = tensor("deep_echo.out_conv.bias", (2 * K,), 1.0 / np.sqrt(3 * C), seed)
    return net
