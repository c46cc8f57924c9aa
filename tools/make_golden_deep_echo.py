#!/usr/bin/env python3
"""Deep Echo AEC golden vectors, produced by RUNNING THE REFERENCE (Deep_Echo_AEC/Export_Deep_Echo.py: ``NET``, ``CFB``, ``CepsUnit``, ``CH_LSTM_F``,
``CH_LSTM_T``, ``LayerNorm``, ``DeepEchoAEC``, with the folder's own STFT_Process) in this container.

The reference ships no checkpoint (model.ckpt is a separate download), so the network is seeded: PyTorch's default initialisation under
``torch.manual_seed(0)``.  The output is ``mix - est`` with an unnormalised echo path; the script prints peak, rms and the clamped-sample count of every row
and refuses to write a fixture in which the reference's output clamps.  ``OUT_CONV_SCALE`` scales ``out_conv``'s weight and bias in the seeded state (1.0: the
state is PyTorch's initialisation as it stands, which is what the committed fixture uses); ``INPUT_SCALE`` = 0.25 scales every non-silent fixture input: at the
wav files' own level the estimated echo of the seeded path clamps 21 samples of row 0, at a quarter of it the largest output peak is 8059 LSB.  Both factors
are recorded in the manifest file.

Written under tests/golden/ (data only):
    deep_echo_seed0_state_0.npz       the weights under the CHECKPOINT's key names (about 0.5 MB; sharded if a file would pass 0.75 MB)
    deep_echo_seed0_manifest.json     the manifest the reference stamps (:505-510), the SHA-256 of the blob ``deep_echo.state_to_blob_tensors`` makes of the state
    deep_echo_seed0_io.npz            four rows at L = 8000 (T = 50): near / far / out (int16)
    deep_echo_seed0_wave.npz          the F32 outputs of the same rows
    deep_echo_seed0_taps.npz          row 0: e0 / e1 / lstm_out / d1 / path (frames TAP_FRAMES x 160 x 20), spec_out (TAP_FRAMES x 160 x 2), each with its
                                      whole-tensor maximum
    deep_echo_seed0_extra.npz         L = 1600 / 2720 / 3000, F32 I/O at 16000, out_sample_rate = 48000
    deep_echo_seed0_fold.npz          USE_BATCH_FOLD: 48000 samples, two windows of 24000

    python tools/make_golden_deep_echo.py
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
from audio_denoiser_onnx_amd.deep_echo import state_to_blob_tensors  # noqa: E402
from audio_denoiser_onnx_amd.wavio import read_pcm16  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
L = 8000
TAP_FRAMES = [0, 1, 8, 9, 10, 15, 16, 49]
OUT_CONV_SCALE = 1.0
INPUT_SCALE = 0.25          # every non-zero fixture input is scaled by this: at full level the seeded path's estimated echo clamps the output


def import_namespace(length, in_dtype="INT16", out_dtype="INT16", out_rate=16000, fold=False):
    _stub_absent_modules()
    path = os.path.join(REF_ROOT, "Deep_Echo_AEC", "Export_Deep_Echo.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    over = {"INPUT_AUDIO_LENGTH": length, "IN_AUDIO_DTYPE": in_dtype, "OUT_AUDIO_DTYPE": out_dtype, "OUT_SAMPLE_RATE": out_rate, "USE_BATCH_FOLD": fold}
    keep = []
    for node in tree.body:
        if isinstance(node, ast.ClassDef) or (isinstance(node, ast.FunctionDef) and node.name == "fuse_layer_norm_scales_"):
            keep.append(node)
        elif isinstance(node, ast.If):                       # the two top-level `if`s: the folded frame count and the static one (:44-45, :52-53)
            keep.append(node)
        elif isinstance(node, ast.Assign):
            names = [t.id for t in node.targets if isinstance(t, ast.Name)]
            if names and all(n.upper() == n for n in names):
                if len(names) == 1 and names[0] in over:
                    node = ast.parse(f"{names[0]} = {over[names[0]]!r}").body[0]
                keep.append(node)
    module = ast.Module(body=keep, type_ignores=[])
    ast.fix_missing_locations(module)
    STFT_Process = import_stft_process("Deep_Echo_AEC").STFT_Process
    ns = {"torch": torch, "STFT_Process": STFT_Process, "__name__": "ref_export_deep_echo"}
    exec(compile(module, path, "exec"), ns)
    return ns


def build(ns, seed=0):
    """The export's own construction sequence (:441-476) with seeded parameters instead of the checkpoint."""
    STFT_Process = ns["STFT_Process"]
    stft = STFT_Process(model_type="stft_B", n_fft=ns["NFFT"], hop_len=ns["HOP_LENGTH"], win_length=ns["WINDOW_LENGTH"], max_frames=0,
                        window_type=ns["WINDOW_TYPE"], center_pad=True, pad_mode="constant", packed_output=True, input_scale=1.0).eval()
    istft = STFT_Process(model_type="istft_B", n_fft=ns["NFFT"], hop_len=ns["HOP_LENGTH"], win_length=ns["WINDOW_LENGTH"], max_frames=ns["MODEL_STFT_FRAMES"],
                         window_type=ns["WINDOW_TYPE"], center_pad=True, pad_mode="constant", output_length=ns["MODEL_AUDIO_LENGTH"],
                         static_norm_divisor=True).eval()
    torch.manual_seed(seed)
    net = ns["NET"](order=ns["ECHO_ORDER"], custom_istft=istft, batch_size=ns["MODEL_BATCH_SIZE"], frames=ns["STATIC_STFT_FRAMES"])
    with torch.no_grad():
        net.out_conv.weight.mul_(OUT_CONV_SCALE)
        net.out_conv.bias.mul_(OUT_CONV_SCALE)
    skip = ("weight_scale", "norm_eps", "initial_state", "custom_istft", "delay_bank_kernel", "delay_pad", "stft_kernel", "inverse_basis")
    state = {k: v.detach().clone().numpy() for k, v in net.state_dict().items() if not any(s in k for s in skip)}      # before the LayerNorm scales are fused in place
    ns["fuse_layer_norm_scales_"](net)
    net = net.float().eval()
    model = ns["DeepEchoAEC"](net, stft, ns["IN_SAMPLE_RATE"], ns["OUT_SAMPLE_RATE"], ns["USE_BATCH_FOLD"], ns["FOLD_WINDOW_LENGTH"], ns["MODEL_BATCH_SIZE"],
                              ns["STATIC_AUDIO_LENGTH"], ns["STATIC_STFT_FRAMES"], input_scale_folded=False).eval()
    return model, state


def run(model, near, far, dtype=torch.int16, want_taps=False):
    taps, hooks = {}, []
    net = model.iccrn
    if want_taps:
        hooks.append(net.cfb_e1.register_forward_pre_hook(lambda m, a: taps.__setitem__("e0", a[0].clone())))
        hooks.append(net.cfb_e1.register_forward_hook(lambda m, a, o: taps.__setitem__("e1", o.clone())))
        hooks.append(net.ch_lstm.register_forward_hook(lambda m, a, o: taps.__setitem__("lstm_out", o.clone())))
        hooks.append(net.cfb_d1.register_forward_hook(lambda m, a, o: taps.__setitem__("d1", o.clone())))
        hooks.append(net.out_conv.register_forward_hook(lambda m, a, o: taps.__setitem__("path", o.clone())))
    packed = net.custom_istft.forward_packed

    def packed_w(x):
        taps["spec_out"] = x.clone()
        return packed(x)
    net.custom_istft.forward_packed = packed_w
    try:
        with torch.inference_mode():
            out = model(torch.from_numpy(near).reshape(1, 1, -1).to(dtype), torch.from_numpy(far).reshape(1, 1, -1).to(dtype))
    finally:
        del net.custom_istft.forward_packed
        for h in hooks:
            h.remove()
    return out.numpy().reshape(-1), {k: v.numpy() for k, v in taps.items()}


def rows():
    far, _ = read_pcm16(os.path.join(REF_ROOT, "Test_Examples", "aec", "farend_speech1.wav"))
    near, _ = read_pcm16(os.path.join(REF_ROOT, "Test_Examples", "aec", "nearend_mic1.wav"))
    far, near = np.round(far[0] * INPUT_SCALE).astype(np.int16), np.round(near[0] * INPUT_SCALE).astype(np.int16)
    out = [(near[o:o + L], far[o:o + L]) for o in (48000, 160000)]
    rng = np.random.default_rng(7)
    f = np.clip(np.round(rng.standard_normal(L) * 3000.0 * INPUT_SCALE), -32768, 32767)
    echo = np.convolve(f, np.exp(-np.arange(64) / 12.0) * rng.standard_normal(64) * 0.3)[:L]
    out.append((np.clip(np.round(echo + rng.standard_normal(L) * 800.0 * INPUT_SCALE), -32768, 32767).astype(np.int16), f.astype(np.int16)))      # a seeded noise-echo pair
    out.append((np.zeros(L, np.int16), np.zeros(L, np.int16)))                    # both silent: every LayerNorm sees a constant plane
    return [(np.ascontiguousarray(n), np.ascontiguousarray(f)) for n, f in out], near, far


def stats(tag, pcm):
    x = pcm.astype(np.float64)
    clamped = int(np.sum((pcm == 32767) | (pcm == -32768)))
    print(f"{tag}: peak {int(np.abs(x).max())} rms {np.sqrt(np.mean(x * x)):.1f} LSB, clamped samples {clamped}")
    assert clamped == 0, "a clamped sample would hide errors behind the clamp"


def main(seed=0):
    ns = import_namespace(L)
    assert ns["MODEL_STFT_FRAMES"] == 50 and ns["MODEL_BATCH_SIZE"] == 1
    model, state = build(ns, seed)
    shard, used, n_shards = {}, 0, 0                             # shards of at most ~0.75 MB of incompressible data: every committed file stays below 1 MiB
    for k in sorted(state):
        cost = 0 if k.endswith(".w") else state[k].nbytes        # a LayerNorm's .w is all ones at initialisation and compresses away
        if shard and used + cost > 750000:
            np.savez_compressed(os.path.join(GOLD, f"deep_echo_seed{seed}_state_{n_shards}.npz"), **shard)
            shard, used, n_shards = {}, 0, n_shards + 1
        shard[k] = state[k]
        used += cost
    np.savez_compressed(os.path.join(GOLD, f"deep_echo_seed{seed}_state_{n_shards}.npz"), **shard)
    blob = W.pack_blob(state_to_blob_tensors(state))
    sys.path.insert(0, REF_ROOT)
    from audio_onnx_metadata import build_audio_metadata_from_globals, build_model_metadata
    manifest = build_model_metadata(build_audio_metadata_from_globals(
        dict(import_namespace(32000)), producer="Export_Deep_Echo.py", model_name="Deep_Echo_AEC", task="aec", model_family="deep_echo", max_dynamic_audio_seconds=30,
        normalize_audio_default=False, batch_fold_inference_default=False, input_channels=1, output_channels=1, num_audio_inputs=2, feature_kind="stft",
        center_pad=True, pad_mode="constant", extra={"echo_order": ns["ECHO_ORDER"]}))               # the export's default length, as the reference stamps it
    with open(os.path.join(GOLD, f"deep_echo_seed{seed}_manifest.json"), "w") as f:
        json.dump({"manifest": {k: str(v) for k, v in manifest.items()}, "blob_sha256": hashlib.sha256(blob).hexdigest(), "blob_nbytes": len(blob),
                   "out_conv_scale": OUT_CONV_SCALE, "input_scale": INPUT_SCALE}, f, indent=1, sort_keys=True)

    rs, near_all, far_all = rows()
    m32, _ = build(import_namespace(L, out_dtype="F32"), seed)
    io, wave, taps = {}, {}, {}
    for i, (n, f) in enumerate(rs):
        pcm, tp = run(model, n, f, want_taps=(i == 0))
        w32, _ = run(m32, n, f)
        io[f"near{i}"], io[f"far{i}"], io[f"out{i}"] = n, f, pcm.astype(np.int16)
        wave[f"wave{i}"] = w32.astype(np.float32)
        stats(f"row {i}", pcm)
        if i == 0:
            taps["frames"] = np.asarray(TAP_FRAMES, np.int32)
            for k in ("e0", "e1", "lstm_out", "d1", "path"):
                full = tp[k][0].transpose(2, 1, 0)                                                 # (channels, 160, T) -> (T, 160, channels)
                taps[k] = np.ascontiguousarray(full[TAP_FRAMES]).astype(np.float32)
                taps[k + "_absmax"] = np.asarray([np.abs(full).max()], np.float32)
            so = tp["spec_out"].reshape(2, 160, -1).transpose(2, 1, 0)                             # (T, 160, re / im)
            taps["spec_out"] = so[TAP_FRAMES].astype(np.float32)
            taps["spec_out_absmax"] = np.asarray([np.abs(so).max()], np.float32)
    np.savez_compressed(os.path.join(GOLD, f"deep_echo_seed{seed}_io.npz"), **io)
    np.savez_compressed(os.path.join(GOLD, f"deep_echo_seed{seed}_wave.npz"), **wave)
    np.savez_compressed(os.path.join(GOLD, f"deep_echo_seed{seed}_taps.npz"), **taps)

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
    assert float(np.abs(o32).max()) < 1.0
    extra.update(f32_near=n32, f32_far=f32, f32_out=o32.astype(np.float32))
    o48, _ = run(build(import_namespace(Ls, out_rate=48000), seed)[0], n, f)
    stats("48 kHz out", o48)
    extra.update(r48_near=n, r48_far=f, r48_out=o48.astype(np.int16))
    np.savez_compressed(os.path.join(GOLD, f"deep_echo_seed{seed}_extra.npz"), **extra)

    Lf = 48000
    nsf = import_namespace(Lf, fold=True)
    assert nsf["FOLD_WINDOW_LENGTH"] == 24000 and nsf["MODEL_BATCH_SIZE"] == 2 and nsf["MODEL_STFT_FRAMES"] == 150
    n, f = near_all[48000:48000 + Lf], far_all[48000:48000 + Lf]
    of, _ = run(build(nsf, seed)[0], n, f)
    of32, _ = run(build(import_namespace(Lf, out_dtype="F32", fold=True), seed)[0], n, f)
    stats("fold", of)
    np.savez_compressed(os.path.join(GOLD, f"deep_echo_seed{seed}_fold.npz"), near=n, far=f, out=of.astype(np.int16), wave=of32.astype(np.float32))
    for fn in sorted(os.listdir(GOLD)):
        if fn.startswith("deep_echo"):
            print(fn, os.path.getsize(os.path.join(GOLD, fn)))


if __name__ == "__main__":
    main()
