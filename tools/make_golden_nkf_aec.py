#!/usr/bin/env python3
"""NKF-AEC golden vectors, produced by RUNNING THE REFERENCE (NKF_AEC/Export_NKF_AEC.py: ``KGNet_Real`` :150-197 and ``NKF.forward`` :246-411, with
the folder's own STFT_Process) in this container.

The reference ships no checkpoint (nkf_epoch70.pt is a separate download), so the network is seeded: PyTorch's default initialisation under
``torch.manual_seed(seed)``, then the gain layer ``fc_out_dense2`` (weight and bias) scaled by ``weightgen.NKF_GAIN_LAYER_SCALE`` (1e-2).  That is
the stability rule: with default init, or anything larger than about 0.03 x default on the gain layer, the Kalman recurrence diverges (NaN, or an
output RMS 10 x the microphone's), and two fp32 evaluations of a diverging filter differ by tens of LSB, so no parity test could hold on it.  With the
rule the filter is stable and the echo path is exercised well above every tolerance: on the two speech windows of the fixture rms(out - near) is
0.033 / 0.024 against a near-end RMS of 0.130 / 0.085 (normalised units; the script prints these per row).

``nkf_aec_seed0_state.npz`` holds the weights under the CHECKPOINT's key names (``kg_net.fc_in.0.linear_real.weight`` ..., Export_NKF_AEC.py:414-455);
the blob (``nkf_aec_seed0.adew``) is ``audio_denoiser_onnx_amd.nkf_aec.state_to_blob_tensors`` of it, so the export round-trip test pins that mapping.

    python tools/make_golden_nkf_aec.py     # writes tests/golden/nkf_aec_seed0*.npz and nkf_aec_seed0.adew
    python tools/make_golden_nkf_aec.py --stream     # writes tests/golden/nkf_aec_seed0_stream.npz only (the streaming tests' fixture)
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

from ref_import import REF_ROOT, _stub_absent_modules, import_stft_process  # noqa: E402
from audio_denoiser_onnx_amd import weights as W  # noqa: E402
from audio_denoiser_onnx_amd.nkf_aec import state_to_blob_tensors as nkf_aec_state_to_blob_tensors  # noqa: E402
from audio_denoiser_onnx_amd.wavio import read_pcm16  # noqa: E402
from audio_denoiser_onnx_amd.weightgen import NKF_GAIN_LAYER_SCALE  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
L = 32000


def import_namespace(length: int, in_dtype: str = "INT16", out_dtype: str = "INT16", out_rate: int = 16000) -> dict:
    _stub_absent_modules()
    path = os.path.join(REF_ROOT, "NKF_AEC", "Export_NKF_AEC.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    over = {"INPUT_AUDIO_LENGTH": length, "IN_AUDIO_DTYPE": in_dtype, "OUT_AUDIO_DTYPE": out_dtype, "OUT_SAMPLE_RATE": out_rate}
    keep = []
    for node in tree.body:
        if isinstance(node, ast.ClassDef):
            keep.append(node)
        elif isinstance(node, ast.Assign):
            names = [t.id for t in node.targets if isinstance(t, ast.Name)]
            if names and all(n.upper() == n for n in names):
                if len(names) == 1 and names[0] in over:
                    node = ast.parse(f"{names[0]} = {over[names[0]]!r}").body[0]
                keep.append(node)
    module = ast.Module(body=keep, type_ignores=[])
    ast.fix_missing_locations(module)
    STFT_Process = import_stft_process("NKF_AEC").STFT_Process
    ns = {"np": np, "torch": torch, "nn": nn, "STFT_Process": STFT_Process, "__name__": "ref_export_nkf_aec"}
    exec(compile(module, path, "exec"), ns)
    return ns


def build(ns, seed=0, state=None):
    """``state``: a checkpoint-named NKF state dict to load instead of the seeded initialisation (the geometry fixtures' generated weights)."""
    STFT_Process = ns["STFT_Process"]
    int_in, int_out = "int" in ns["IN_AUDIO_DTYPE"].lower(), "int" in ns["OUT_AUDIO_DTYPE"].lower()
    stft = STFT_Process(model_type="stft_B", n_fft=ns["NFFT"], hop_len=ns["HOP_LENGTH"], win_length=ns["WINDOW_LENGTH"], max_frames=0,
                        window_type=ns["WINDOW_TYPE"], center_pad=True, pad_mode="constant", input_scale=ns["INV_INT16"] if int_in else 1.0).eval()
    istft = STFT_Process(model_type="istft_B", n_fft=ns["NFFT"], hop_len=ns["HOP_LENGTH"], win_length=ns["WINDOW_LENGTH"],
                         max_frames=ns["MAX_SIGNAL_LENGTH"], window_type=ns["WINDOW_TYPE"], center_pad=True, pad_mode="constant",
                         static_norm=True, output_scale=32767.0 if int_out else 1.0).eval()          # (:482-492)
    torch.manual_seed(seed)
    model = ns["NKF"](L=ns["FILTER_ORDER"], fc_dim=ns["FC_DIM"], rnn_layers=ns["RNN_LAYERS"], rnn_dim=ns["RNN_DIM"], custom_stft=stft, custom_istft=istft,
                      max_frames=ns["MAX_SIGNAL_LENGTH"], in_sample_rate=ns["IN_SAMPLE_RATE"], out_sample_rate=ns["OUT_SAMPLE_RATE"],
                      use_batch_fold=ns["USE_BATCH_FOLD"], fold_window=ns["FOLD_WINDOW_LENGTH"]).eval()
    if state is not None:
        load_checkpoint(model, state)
    else:
        with torch.no_grad():
            for p in model.kg_net.fc_out_dense2.parameters():
                p.mul_(NKF_GAIN_LAYER_SCALE)
    state = {k: v.detach().clone().numpy() for k, v in model.state_dict().items() if k.startswith("kg_net.")}
    model.cache_export_constants_()                                                                    # (:509)
    return model, state


def checkpoint_names(state):
    """export-module names -> the checkpoint's (the inverse of load_nkf_weights, Export_NKF_AEC.py:414-455)"""
    ren = {"fc_in_dense": "fc_in.0", "fc_in_act": "fc_in.1", "fc_out_dense1": "fc_out.0", "fc_out_act": "fc_out.1", "fc_out_dense2": "fc_out.2"}
    out = {}
    for k, v in state.items():
        parts = k.split(".")
        parts[1] = ren.get(parts[1], parts[1])
        out[".".join(parts)] = v
    return out


def load_checkpoint(model, state):
    """checkpoint-named weights -> the export module, every ``kg_net.`` parameter (what load_nkf_weights does, Export_NKF_AEC.py:414-455)"""
    ren = {"fc_in.0": "fc_in_dense", "fc_in.1": "fc_in_act", "fc_out.0": "fc_out_dense1", "fc_out.1": "fc_out_act", "fc_out.2": "fc_out_dense2"}
    own = {k: v for k, v in model.state_dict().items() if k.startswith("kg_net.") and "buffer" not in k}
    new = {}
    for k, v in state.items():
        parts = k.split(".")
        two = ".".join(parts[1:3])
        parts = [parts[0], ren[two]] + parts[3:] if two in ren else parts
        new[".".join(parts)] = torch.from_numpy(np.asarray(v, np.float32).copy())
    assert set(new) == set(own), sorted(set(new) ^ set(own))
    model.load_state_dict(new, strict=False)
    for k, v in new.items():
        assert torch.equal(model.state_dict()[k], v.reshape(model.state_dict()[k].shape)), k


def run(model, far, near, dtype=torch.int16):
    taps = {}
    stft_f, istft_f = model.custom_stft.forward, model.custom_istft.forward

    def stft_w(x):
        y = stft_f(x)
        taps["spec"] = [t.clone() for t in y]
        return y

    def istft_w(re, im):
        taps["err"] = (re.clone(), im.clone())
        y = istft_f(re, im)
        taps["istft"] = y.clone()
        return y
    model.custom_stft.forward, model.custom_istft.forward = stft_w, istft_w
    with torch.inference_mode():
        out = model(torch.from_numpy(far).reshape(1, 1, -1).to(dtype), torch.from_numpy(near).reshape(1, 1, -1).to(dtype))
    model.custom_stft.forward, model.custom_istft.forward = stft_f, istft_f
    b = model.model_batch
    mic_re, mic_im = taps["spec"][0][b:], taps["spec"][1][b:]
    echo = np.stack([(mic_re - taps["err"][0]).numpy(), (mic_im - taps["err"][1]).numpy()])      # (2, n_win, F, T)
    return out.numpy().reshape(-1), taps["istft"].numpy().reshape(-1), echo


def rows():
    far, _ = read_pcm16(os.path.join(REF_ROOT, "Test_Examples", "aec", "farend_speech1.wav"))
    near, _ = read_pcm16(os.path.join(REF_ROOT, "Test_Examples", "aec", "nearend_mic1.wav"))
    far, near = far[0], near[0]
    out = [(far[o:o + L], near[o:o + L]) for o in (48000, 160000)]
    rng = np.random.default_rng(7)
    out.append(tuple(np.clip(np.round(rng.standard_normal(L) * 3000.0), -32768, 32767).astype(np.int16) for _ in range(2)))
    out.append((np.zeros(L, np.int16), near[96000:96000 + L]))                 # far end silent: echo_hat == 0 exactly
    out.append((np.zeros(L, np.int16), np.zeros(L, np.int16)))
    return [(np.ascontiguousarray(f), np.ascontiguousarray(n)) for f, n in out], far, near


def main(seed=0):
    ns = import_namespace(L)
    assert ns["MAX_SIGNAL_LENGTH"] == 126
    model, state = build(ns, seed)
    blob_tensors = nkf_aec_state_to_blob_tensors(checkpoint_names(state))
    W.save_blob(os.path.join(GOLD, f"nkf_aec_seed{seed}.adew"), blob_tensors)
    np.savez_compressed(os.path.join(GOLD, f"nkf_aec_seed{seed}_state.npz"), **checkpoint_names(state))
    rs, far_all, near_all = rows()
    io, wave, taps = {}, {}, {}
    for i, (f, n) in enumerate(rs):
        pcm, istft, echo = run(model, f, n)
        io[f"far{i}"], io[f"near{i}"], io[f"out{i}"] = f, n, pcm.astype(np.int16)
        wave[f"wave{i}"] = (istft[:L].astype(np.float64) / 32767.0).astype(np.float32)      # the waveform before the * 32767 of the PCM tail
        if i == 0:
            taps["echo_hat0"] = echo[:, 0].astype(np.float32)                                   # (re/im, F, T)
        if i == 3:
            assert not np.any(echo), "far end zero must give echo_hat == 0"
        print(f"row {i}: rms near {np.sqrt(np.mean((n / 32768.0) ** 2)):.4f} out {np.sqrt(np.mean((pcm / 32767.0) ** 2)):.4f} "
              f"rms(out - near) {np.sqrt(np.mean(((pcm.astype(np.float64) - n) / 32768.0) ** 2)):.4f}")
    np.savez_compressed(os.path.join(GOLD, f"nkf_aec_seed{seed}_io.npz"), **io)
    np.savez_compressed(os.path.join(GOLD, f"nkf_aec_seed{seed}_wave.npz"), **wave)
    np.savez_compressed(os.path.join(GOLD, f"nkf_aec_seed{seed}_taps.npz"), **taps)

    # extra cases, each one row
    extra = {}
    # (No USE_BATCH_FOLD case: the reference's folded graph is not window-separable -- KGNet's _from_grouped reshape (:106-107) assumes batch 1 and
    # interleaves the channel groups of the folded windows -- so the engine refuses use_batch_fold for this family.)
    Ls = 16000
    f, n = far_all[64000:64000 + Ls], near_all[64000:64000 + Ls]
    ns32 = import_namespace(Ls, in_dtype="F32", out_dtype="F32")
    m32, _ = build(ns32, seed)
    f32in, n32in = (f / 32768.0).astype(np.float32), (n / 32768.0).astype(np.float32)
    o32, _, _ = run(m32, f32in, n32in, dtype=torch.float32)
    extra.update(f32_far=f32in, f32_near=n32in, f32_out=o32.astype(np.float32))
    ns48 = import_namespace(Ls, out_rate=48000)
    m48, _ = build(ns48, seed)
    o48, _, _ = run(m48, f, n)
    extra.update(r48_far=f, r48_near=n, r48_out=o48.astype(np.int16))
    np.savez_compressed(os.path.join(GOLD, f"nkf_aec_seed{seed}_extra.npz"), **extra)
    for fn in sorted(os.listdir(GOLD)):
        if fn.startswith("nkf_aec"):
            print(fn, os.path.getsize(os.path.join(GOLD, fn)))


STREAM_L = 49152            # 192 hops, T = 193.  Not longer: with the seeded weights the filter is only known stable this far (at 65 536 / offset 0 and at 96 000
#                             it diverges, and two fp32 evaluations of a diverging filter disagree by the whole int16 range)


def zero_sum(x):
    """int16 signal -> the same signal with an EXACTLY zero integer sum (subtract sum // n, then one LSB from the first `sum` samples)."""
    x = x.astype(np.int64)
    x -= int(x.sum()) // len(x)
    x[:int(x.sum())] -= 1
    assert x.sum() == 0 and np.abs(x).max() < 32768
    return x.astype(np.int16)


def stream_fixture(seed=0):
    """The streaming tests' reference: NKF.forward on 49 152 samples in ONE call, on inputs whose integer sum is exactly zero -- the reference's per-call DC
    term is then exactly 0.0 and a stream (which cannot remove a whole-call mean) computes the same thing.  Writes nkf_aec_seed0_stream.npz and nothing else."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from nkf_aec_oracle import NkfAecOracle
    ns = import_namespace(STREAM_L)
    assert ns["MAX_SIGNAL_LENGTH"] == STREAM_L // 256 + 1 == 193
    model, state = build(ns, seed)
    committed = W.load_blob(os.path.join(GOLD, f"nkf_aec_seed{seed}.adew"))
    for k, v in nkf_aec_state_to_blob_tensors(checkpoint_names(state)).items():
        assert np.array_equal(v, committed[k]), f"seed-{seed} weights differ from the committed blob: {k}"
    _, far_all, near_all = rows()
    oracle = NkfAecOracle(committed, tables="exact")
    fix = {}
    for i, o in enumerate((48000, 160000)):
        f, n = zero_sum(far_all[o:o + STREAM_L]), zero_sum(near_all[o:o + STREAM_L])
        pair = torch.from_numpy(np.stack([f, n])).reshape(2, 1, -1).float()
        mean = pair.mean(dim=2)                                                                  # the reference's own DC term (:269), in fp32
        assert float(mean.abs().max()) == 0.0, f"clip {i}: the reference's fp32 mean is {mean.flatten().tolist()}, not 0"
        pcm, istft, _ = run(model, f, n)
        wave = (istft[:STREAM_L].astype(np.float64) / 32767.0).astype(np.float32)
        opcm, owave, _ = oracle.forward(f[None], n[None])
        d_pcm = int(np.abs(opcm[0].astype(np.int32) - pcm.astype(np.int32)).max())
        d_wave = float(np.abs(owave[0] - wave).max())
        print(f"clip {i} (offset {o}): max |out| {int(np.abs(pcm.astype(np.int32)).max())}  rms near {np.sqrt(np.mean((n / 32768.0) ** 2)):.4f}  "
              f"rms(out - near) {np.sqrt(np.mean(((pcm.astype(np.float64) - n) / 32768.0) ** 2)):.4f}  oracle vs reference: {d_pcm} LSB, wave {d_wave:.2e}")
        if d_pcm > 1 or d_wave > 1e-4:
            raise SystemExit("oracle and reference disagree by more than 1 LSB / 1e-4: the filter is not stable on this clip, no fixture written")
        fix[f"far{i}"], fix[f"near{i}"], fix[f"out{i}"], fix[f"wave{i}"] = f, n, pcm.astype(np.int16), wave
    path = os.path.join(GOLD, f"nkf_aec_seed{seed}_stream.npz")
    np.savez_compressed(path, **fix)
    print(os.path.basename(path), os.path.getsize(path))


if __name__ == "__main__":
    if "--stream" in sys.argv:
        stream_fixture()
    else:
        main()
