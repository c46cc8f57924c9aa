#!/usr/bin/env python3
"""SDAEC golden vectors, produced by RUNNING THE REFERENCE (SDAEC/Export_SDAEC.py: ``NET``, ``CFB``, ``CepsUnit``, ``CH_LSTM_F``, ``CH_LSTM_T``,
``LayerNorm``, ``AlphaPredictor``, ``SDAEC``, with the folder's own STFT_Process) in this container.

The reference ships no checkpoint (ICCRN.ckpt / alpha.ckpt are separate downloads), so the network is seeded: PyTorch's default initialisation under
``torch.manual_seed(0)``.  Every stage is LayerNorm-normalised, so the output is stable and non-trivial as it stands; the script prints peak, rms and
the clamped-sample count of every row.

Written under tests/golden/ (data only):
    sdaec_seed0_state_<i>.npz     the weights under the CHECKPOINTS' key names (``alpha.`` prefixes the alpha predictor's), in shards that each stay below 1 MiB
    sdaec_seed0_manifest.json     the manifest the reference stamps (:517-521), the SHA-256 of the blob ``sdaec.state_to_blob_tensors`` makes of the state
                                  (the 2 MB blob itself is not committed) and the reference's folded buffers' checksums
    sdaec_seed0_folds.npz         the reference's own folded buffers for a few LayerNorms, the two fused Linears, the alpha kernel
    sdaec_seed0_io.npz            six rows at L = 32000: near / far / out (int16)
    sdaec_seed0_wave.npz          the F32 outputs of the same rows
    sdaec_seed0_taps.npz          row 0: alpha (T), and e0 / e5 / lstm_out / d1 (frames TAP_FRAMES x 160 x 20), spec_out (TAP_FRAMES x 160 x 2); the two cepstral tables
    sdaec_seed0_extra.npz         L = 1600 / 2720 / 3000, F32 I/O, out_sample_rate = 48000
    sdaec_seed0_fold.npz          USE_BATCH_FOLD: 48000 samples, two windows of 24000

    python tools/make_golden_sdaec.py
"""
import ast
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

from ref_import import REF_ROOT, _stub_absent_modules, import_stft_process  # noqa: E402
from audio_denoiser_onnx_amd import weights as W  # noqa: E402
from audio_denoiser_onnx_amd.sdaec import state_to_blob_tensors  # noqa: E402
from audio_denoiser_onnx_amd.wavio import read_pcm16  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
L = 32000
TAP_FRAMES = [0, 1, 15, 16, 100, 199]


def import_namespace(length, in_dtype="INT16", out_dtype="INT16", out_rate=16000, fold=False):
    _stub_absent_modules()
    path = os.path.join(REF_ROOT, "SDAEC", "Export_SDAEC.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    over = {"INPUT_AUDIO_LENGTH": length, "IN_AUDIO_DTYPE": in_dtype, "OUT_AUDIO_DTYPE": out_dtype, "OUT_SAMPLE_RATE": out_rate, "USE_BATCH_FOLD": fold}
    keep = []
    for node in tree.body:
        if isinstance(node, ast.ClassDef):
            keep.append(node)
        elif isinstance(node, ast.If):                       # the two top-level `if`s: the DYNAMIC_AXES guard and the folded frame count (:47-51)
            keep.append(node)
        elif isinstance(node, ast.Assign):
            names = [t.id for t in node.targets if isinstance(t, ast.Name)]
            if names and all(n.upper() == n for n in names):
                if len(names) == 1 and names[0] in over:
                    node = ast.parse(f"{names[0]} = {over[names[0]]!r}").body[0]
                keep.append(node)
    module = ast.Module(body=keep, type_ignores=[])
    ast.fix_missing_locations(module)
    STFT_Process = import_stft_process("SDAEC").STFT_Process
    ns = {"torch": torch, "STFT_Process": STFT_Process, "__name__": "ref_export_sdaec"}
    exec(compile(module, path, "exec"), ns)
    return ns


def build(ns, seed=0):
    """The export's own construction sequence (:459-487) with seeded parameters instead of the two checkpoints."""
    STFT_Process = ns["STFT_Process"]
    stft = STFT_Process(model_type="stft_B", n_fft=ns["NFFT"], hop_len=ns["HOP_LENGTH"], win_length=ns["WINDOW_LENGTH"], max_frames=0,
                        window_type=ns["WINDOW_TYPE"], center_pad=True, pad_mode="constant", input_scale=1.0, packed_output=True).eval()
    out_len = ns["FOLD_WINDOW_LENGTH"] if ns["USE_BATCH_FOLD"] else int(round(ns["EXPORT_AUDIO_LENGTH"] * ns["MODEL_SAMPLE_RATE"] / ns["IN_SAMPLE_RATE"]))
    istft = STFT_Process(model_type="istft_B", n_fft=ns["NFFT"], hop_len=ns["HOP_LENGTH"], win_length=ns["WINDOW_LENGTH"], max_frames=ns["MAX_SIGNAL_LENGTH"],
                         window_type=ns["WINDOW_TYPE"], center_pad=True, pad_mode="constant", static_norm=True, output_scale=1.0, output_length=out_len).eval()
    torch.manual_seed(seed)
    net = ns["NET"](max_frames=ns["MAX_SIGNAL_LENGTH"], custom_istft=istft)
    alpha = ns["AlphaPredictor"](ns["ALPHA_K"])
    skip = ("mean_scale", "weight_scale", "norm_eps", "cepstral_", "initial_state", "custom_istft")
    state = {k: v.detach().clone().numpy() for k, v in net.state_dict().items() if not any(s in k for s in skip)}
    state.update({"alpha." + k: v.detach().clone().numpy() for k, v in alpha.state_dict().items()})
    for m in net.modules():
        if isinstance(m, ns["LayerNorm"]):
            m.fuse_var_scale_()
    net.prepare_for_export_()
    net = net.float().eval()
    alpha = alpha.float().eval()
    model = ns["SDAEC"](net, alpha, stft, ns["NFFT"], ns["ALPHA_K"], ns["MAX_SIGNAL_LENGTH"], ns["IN_SAMPLE_RATE"], ns["OUT_SAMPLE_RATE"],
                        ns["USE_BATCH_FOLD"], ns["FOLD_WINDOW_LENGTH"]).eval()
    return model, state


def run(model, near, far, dtype=torch.int16, want_taps=False):
    taps, hooks = {}, []
    net = model.iccrn
    if want_taps:
        hooks.append(net.cfb_e1.register_forward_pre_hook(lambda m, a: taps.__setitem__("e0", a[0].clone())))
        hooks.append(net.cfb_e5.register_forward_hook(lambda m, a, o: taps.__setitem__("e5", o.clone())))
        hooks.append(net.ch_lstm.register_forward_hook(lambda m, a, o: taps.__setitem__("lstm_out", o.clone())))
        hooks.append(net.cfb_d1.register_forward_hook(lambda m, a, o: taps.__setitem__("d1", o.clone())))
    conv1d, packed = torch.nn.functional.conv1d, net.custom_istft.forward_packed

    def conv1d_w(x, w, *a, **k):
        y = conv1d(x, w, *a, **k)
        if w is model.alpha_conv_kernel:
            taps["alpha"] = y.clone()
        return y

    def packed_w(x):
        taps["spec_out"] = x.clone()
        return packed(x)
    torch.nn.functional.conv1d, net.custom_istft.forward_packed = conv1d_w, packed_w
    try:
        with torch.inference_mode():
            out = model(torch.from_numpy(near).reshape(1, 1, -1).to(dtype), torch.from_numpy(far).reshape(1, 1, -1).to(dtype))
    finally:
        torch.nn.functional.conv1d = conv1d
        del net.custom_istft.forward_packed
        for h in hooks:
            h.remove()
    return out.numpy().reshape(-1), {k: v.numpy() for k, v in taps.items()}


def rows():
    far, _ = read_pcm16(os.path.join(REF_ROOT, "Test_Examples", "aec", "farend_speech1.wav"))
    near, _ = read_pcm16(os.path.join(REF_ROOT, "Test_Examples", "aec", "nearend_mic1.wav"))
    far, near = far[0], near[0]
    out = [(near[o:o + L], far[o:o + L]) for o in (48000, 160000)]
    rng = np.random.default_rng(7)
    f = np.clip(np.round(rng.standard_normal(L) * 3000.0), -32768, 32767)
    echo = np.convolve(f, np.exp(-np.arange(64) / 12.0) * rng.standard_normal(64) * 0.3)[:L]
    out.append((np.clip(np.round(echo + rng.standard_normal(L) * 800.0), -32768, 32767).astype(np.int16), f.astype(np.int16)))      # a seeded noise-echo pair
    out.append((near[96000:96000 + L], np.zeros(L, np.int16)))                    # far end silent
    out.append((np.zeros(L, np.int16), np.zeros(L, np.int16)))                    # both silent: every LayerNorm sees a constant plane
    out.append((np.clip(near[48000:48000 + L].astype(np.int32) * 8, -32768, 32767).astype(np.int16),
                np.clip(far[48000:48000 + L].astype(np.int32) * 8, -32768, 32767).astype(np.int16)))    # scaled up until the INPUT saturates
    return [(np.ascontiguousarray(n), np.ascontiguousarray(f)) for n, f in out], near, far


def stats(tag, pcm):
    x = pcm.astype(np.float64)
    print(f"{tag}: peak {int(np.abs(x).max())} rms {np.sqrt(np.mean(x * x)):.1f} LSB, clamped samples {int(np.sum((pcm == 32767) | (pcm == -32768)))}")


def main(seed=0):
    ns = import_namespace(L)
    assert ns["MAX_SIGNAL_LENGTH"] == 200
    model, state = build(ns, seed)
    shard, used, n_shards = {}, 0, 0                             # shards of at most ~0.75 MB of incompressible data: every committed file stays below 1 MiB
    for k in sorted(state):
        cost = 0 if k.endswith(".w") else state[k].nbytes        # a LayerNorm's .w is all ones at initialisation and compresses away
        if shard and used + cost > 750000:
            np.savez_compressed(os.path.join(GOLD, f"sdaec_seed{seed}_state_{n_shards}.npz"), **shard)
            shard, used, n_shards = {}, 0, n_shards + 1
        shard[k] = state[k]
        used += cost
    np.savez_compressed(os.path.join(GOLD, f"sdaec_seed{seed}_state_{n_shards}.npz"), **shard)
    blob = W.pack_blob(state_to_blob_tensors({k: v for k, v in state.items() if not k.startswith("alpha.")},
                                             {k[6:]: v for k, v in state.items() if k.startswith("alpha.")}))
    net = model.iccrn
    folds = {"in_fused_weight": net.in_fused_weight.numpy(), "in_fused_bias": net.in_fused_bias.numpy(), "out_fused_weight": net.out_fused_weight.numpy(),
             "out_fused_bias": net.out_fused_bias.numpy(), "alpha_conv_kernel": model.alpha_conv_kernel.detach().numpy(), "alpha_conv_bias": model.alpha_conv_bias.detach().numpy()}
    ln_sha = hashlib.sha256()
    for name, m in net.named_modules():
        if isinstance(m, ns["LayerNorm"]):
            ln_sha.update(name.encode() + m.export_w.numpy().tobytes() + m.export_b.numpy().tobytes() + np.float32(m.export_eps).tobytes())
            if name in ("cfb_e1.LN0", "cfb_d1.LN0", "cfb_e3.ceps_unit.LN", "ln"):
                folds[name + ".export_w"], folds[name + ".export_b"] = m.export_w.numpy(), m.export_b.numpy()
                folds[name + ".export_eps"] = np.asarray([m.export_eps], np.float64)
    np.savez_compressed(os.path.join(GOLD, f"sdaec_seed{seed}_folds.npz"), **folds)
    g = dict(ns)
    for k in ("BATCH_WINDOW_SECONDS",):
        g.setdefault(k, 1.5)
    sys.path.insert(0, REF_ROOT)
    from audio_onnx_metadata import build_audio_metadata_from_globals, build_model_metadata
    manifest = build_model_metadata(build_audio_metadata_from_globals(
        g, producer="Export_SDAEC.py", model_name="SDAEC", task="aec", model_family="sdaec", max_dynamic_audio_seconds=30, normalize_audio_default=False,
        input_channels=1, output_channels=1, num_audio_inputs=2, feature_kind="stft_alpha_predictor", center_pad=True, pad_mode="constant",
        extra={"alpha_k": ns["ALPHA_K"]}))
    with open(os.path.join(GOLD, f"sdaec_seed{seed}_manifest.json"), "w") as f:
        json.dump({"manifest": {k: str(v) for k, v in manifest.items()}, "blob_sha256": hashlib.sha256(blob).hexdigest(), "blob_nbytes": len(blob),
                   "layernorm_folds_sha256": ln_sha.hexdigest()}, f, indent=1, sort_keys=True)

    rs, near_all, far_all = rows()
    m32, _ = build(import_namespace(L, out_dtype="F32"), seed)
    io, wave, taps = {}, {}, {}
    for i, (n, f) in enumerate(rs):
        pcm, tp = run(model, n, f, want_taps=(i == 0))
        w32, _ = run(m32, n, f)
        io[f"near{i}"], io[f"far{i}"], io[f"out{i}"] = n, f, pcm.astype(np.int16)
        wave[f"wave{i}"] = w32.astype(np.float32)
        stats(f"row {i}", pcm)
        if i != 5:
            assert not np.any((pcm == 32767) | (pcm == -32768)), "a clamped sample would hide errors behind the clamp"
        if i == 0:
            taps["alpha"] = tp["alpha"].reshape(-1).astype(np.float32)
            taps["frames"] = np.asarray(TAP_FRAMES, np.int32)
            for k in ("e0", "e5", "lstm_out", "d1"):
                taps[k] = tp[k][0][TAP_FRAMES].astype(np.float32)                                  # (frames, 160, 20)
                taps[k + "_absmax"] = np.asarray([np.abs(tp[k]).max()], np.float32)
            so = tp["spec_out"].reshape(2, 160, -1).transpose(2, 1, 0)                             # (T, 160, re / im)
            taps["spec_out"] = so[TAP_FRAMES].astype(np.float32)
            taps["spec_out_absmax"] = np.asarray([np.abs(so).max()], np.float32)
            taps["ceps_dft"], taps["ceps_idft"] = net.cepstral_dft_weight.numpy(), net.cepstral_idft_weight.numpy()
    np.savez_compressed(os.path.join(GOLD, f"sdaec_seed{seed}_io.npz"), **io)
    np.savez_compressed(os.path.join(GOLD, f"sdaec_seed{seed}_wave.npz"), **wave)
    np.savez_compressed(os.path.join(GOLD, f"sdaec_seed{seed}_taps.npz"), **taps)

    extra = {}
    for Ls in (1600, 2720, 3000):
        n, f = near_all[64000:64000 + Ls], far_all[64000:64000 + Ls]
        o, _ = run(build(import_namespace(Ls), seed)[0], n, f)
        o32, _ = run(build(import_namespace(Ls, out_dtype="F32"), seed)[0], n, f)
        assert o.shape == (Ls,)
        extra.update({f"near_{Ls}": n, f"far_{Ls}": f, f"out_{Ls}": o.astype(np.int16), f"wave_{Ls}": o32.astype(np.float32)})
        stats(f"L = {Ls}", o)
    Ls = 16000
    n, f = near_all[64000:64000 + Ls], far_all[64000:64000 + Ls]
    n32, f32 = (n / 32768.0).astype(np.float32), (f / 32768.0).astype(np.float32)
    o32, _ = run(build(import_namespace(Ls, in_dtype="F32", out_dtype="F32"), seed)[0], n32, f32, dtype=torch.float32)
    extra.update(f32_near=n32, f32_far=f32, f32_out=o32.astype(np.float32))
    o48, _ = run(build(import_namespace(Ls, out_rate=48000), seed)[0], n, f)
    extra.update(r48_near=n, r48_far=f, r48_out=o48.astype(np.int16))
    np.savez_compressed(os.path.join(GOLD, f"sdaec_seed{seed}_extra.npz"), **extra)

    Lf = 48000
    nsf = import_namespace(Lf, fold=True)
    assert nsf["FOLD_WINDOW_LENGTH"] == 24000 and nsf["STATIC_MODEL_BATCH"] == 2 and nsf["MAX_SIGNAL_LENGTH"] == 150
    n, f = near_all[48000:48000 + Lf], far_all[48000:48000 + Lf]
    of, _ = run(build(nsf, seed)[0], n, f)
    of32, _ = run(build(import_namespace(Lf, out_dtype="F32", fold=True), seed)[0], n, f)
    stats("fold", of)
    np.savez_compressed(os.path.join(GOLD, f"sdaec_seed{seed}_fold.npz"), near=n, far=f, out=of.astype(np.int16), wave=of32.astype(np.float32))
    for fn in sorted(os.listdir(GOLD)):
        if fn.startswith("sdaec"):
            print(fn, os.path.getsize(os.path.join(GOLD, fn)))


if __name__ == "__main__":
    main()
