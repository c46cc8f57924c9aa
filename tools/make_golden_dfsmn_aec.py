#!/usr/bin/env python3
"""DFSMN-AEC golden vectors, produced by RUNNING THE REFERENCE (DFSMN_AEC/Export_DFSMN_AEC.py: ``DFSMN_AEC.forward`` :1268-1352 with ``NKF_Inner`` :897-1000,
``build_kaldi_fbank_conv`` :1032-1068 and the folder's own STFT_Process) in this container.

What stands in for the parts the container lacks:
  * the export script runs at module level: only its classes, functions, UPPER_CASE constants and the top-level ``if`` blocks ahead of the export are executed
    (``ast`` filter), with ``project_path_B`` overridden so that the NKF back end is selected;
  * ``torchaudio`` is absent: ``torchaudio.compliance.kaldi.get_mel_banks`` is served by audio_denoiser_onnx_amd/kaldi_mel.py, and the bank travels in the blob;
  * ``modelscope`` is absent: a seeded stand-in tree with exactly the attribute paths ``DFSMN_AEC.__init__`` / ``_uni_deep_fsmn`` read --
    ``model.linear1.linear``, ``model.relu``, ``model.sig``, ``model.linear2``, ``model.linear3``, ``model.deepfsmn[i].{linear, act, norm, project, conv1,
    skip_connect, output_dim, padding_left}``, ``preprocessor.feature.{shift, scale}``.  Its geometry (parity-unpinned, like ZipEnhancer's and DFSMN's):
    width D = 128, DEPTH = 6 layers of hidden H = 64, lorder 20, dilation 2 (the reference shares one left pad between the layers, so one dilation),
    skip_connect on every other layer.  (Nine layers of hidden 128 would put the fp32 blob over the 1 MiB a committed file may have.)
  * the NKF checkpoint is a separate download: PyTorch's default initialisation under ``torch.manual_seed``, the gain layer scaled by
    ``weightgen.NKF_GAIN_LAYER_SCALE`` (the stability rule of tools/make_golden_nkf_aec.py).

    python tools/make_golden_dfsmn_aec.py      # writes tests/golden/dfsmn_aec_seed0.adew and dfsmn_aec_seed0_*.npz
    python tools/make_golden_dfsmn_aec.py --stream        # writes tests/golden/dfsmn_aec_seed0_stream.npz only: the unfolded forward in ONE call on two clips of
                                                          # 40 960 samples, what ade_stream_* pushes + flush must equal 1344 samples later
    python tools/make_golden_dfsmn_aec.py --geometry      # writes tests/golden/aec_geom_<name>.npz only: the geometries of tests/aec_geometry_lib.py, whose
                                                          # generated weights (per-layer H / lorder / dilation / skip, distinct PReLU slopes) replace the stand-ins
"""
import ast
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from ref_import import REF_ROOT, _stub_absent_modules, import_stft_process  # noqa: E402
from audio_denoiser_onnx_amd import dfsmn_aec, kaldi_mel  # noqa: E402
from audio_denoiser_onnx_amd import weights as W  # noqa: E402
from audio_denoiser_onnx_amd.wavio import read_pcm16  # noqa: E402
from audio_denoiser_onnx_amd.weightgen import NKF_GAIN_LAYER_SCALE  # noqa: E402
from make_golden_nkf_aec import checkpoint_names, load_checkpoint  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
L = 32000
D, H, DEPTH, LORDER, DILATION = 128, 64, 6, 20, 2
SKIP = [i % 2 == 0 for i in range(DEPTH)]


def import_namespace(**over) -> dict:
    _stub_absent_modules()
    path = os.path.join(REF_ROOT, "DFSMN_AEC", "Export_DFSMN_AEC.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    over = dict(over, project_path_B="/nonexistent/NKF-AEC")
    keep = []
    for node in tree.body:
        if isinstance(node, ast.Expr) and isinstance(node.value, ast.Call) and getattr(node.value.func, "id", "") == "print":
            break                                                            # print('Export start ...'): everything from here on is the export itself
        if isinstance(node, (ast.ClassDef, ast.FunctionDef, ast.If)):
            keep.append(node)
            # An ``if`` block may re-derive an overridden setting: for the NKF back end the export sets ``INPUT_AUDIO_LENGTH = max(32000, ...)`` (:87), a
            # recommendation and not a limit of the model.  Such a name is assigned its override again right after the block.
            if isinstance(node, ast.If):
                inner = {t.id for a in ast.walk(node) if isinstance(a, ast.Assign) for t in a.targets if isinstance(t, ast.Name)}
                keep.extend(ast.parse(f"{n} = {over[n]!r}").body[0] for n in sorted(inner & set(over)))
        elif isinstance(node, ast.Assign):
            names = [t.id for t in node.targets if isinstance(t, ast.Name)]
            if names and (all(n.upper() == n and not n.startswith("_") for n in names) or names == ["project_path_B"]):
                if len(names) == 1 and names[0] in over:
                    node = ast.parse(f"{names[0]} = {over[names[0]]!r}").body[0]
                keep.append(node)
    module = ast.Module(body=keep, type_ignores=[])
    ast.fix_missing_locations(module)
    kaldi = types.ModuleType("torchaudio.compliance.kaldi")
    kaldi.get_mel_banks = lambda *a: (torch.from_numpy(kaldi_mel.get_mel_banks(*a)), None)
    ta, comp = types.ModuleType("torchaudio"), types.ModuleType("torchaudio.compliance")
    ta.compliance, comp.kaldi = comp, kaldi
    sys.modules.update({"torchaudio": ta, "torchaudio.compliance": comp, "torchaudio.compliance.kaldi": kaldi})
    ns = {"np": np, "torch": torch, "nn": nn, "F": torch.nn.functional, "STFT_Process": import_stft_process("DFSMN_AEC").STFT_Process,
          "__name__": "ref_export_dfsmn_aec"}
    exec(compile(module, path, "exec"), ns)
    assert ns["LIGHT_AEC_MODEL"] == "NKF"
    return ns


def fake_dfsmn(seed: int):
    gen = torch.Generator().manual_seed(3000 + seed)

    def lin(i, o, bias=True, gain=1.0):
        m = nn.Linear(i, o, bias=bias)
        with torch.no_grad():
            m.weight.copy_(torch.randn(o, i, generator=gen) * (gain / np.sqrt(i)))
            if bias:
                m.bias.copy_(torch.randn(o, generator=gen) * 0.1)
        return m

    class Layer(nn.Module):
        def __init__(self, skip):
            super().__init__()
            self.linear, self.act, self.norm, self.project = lin(D, H, gain=1.2), nn.ReLU(), nn.Identity(), lin(H, D, bias=False, gain=0.7)
            self.conv1 = nn.Conv2d(D, D, (LORDER, 1), dilation=(DILATION, 1), groups=D, bias=False)
            with torch.no_grad():
                self.conv1.weight.copy_(torch.randn(self.conv1.weight.shape, generator=gen) * 0.08)
            self.skip_connect, self.output_dim, self.padding_left = skip, D, DILATION * (LORDER - 1)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.linear1 = nn.Module()
            self.linear1.linear = lin(dfsmn_aec.FEAT_DIM, D, gain=0.6)
            self.relu, self.sig = nn.ReLU(), nn.Sigmoid()
            self.deepfsmn = nn.ModuleList([Layer(s) for s in SKIP])
            self.linear2, self.linear3 = lin(D, dfsmn_aec.N_BINS, gain=0.5), lin(D, 1, gain=0.5)

    net = Net().eval()
    # log-mel of int16-scale power sits around 5 .. 25: shift / scale bring it to unit range, as a trained normaliser would
    shift = -15.0 + torch.randn(dfsmn_aec.FEAT_DIM, generator=gen)
    scale = 0.2 * (1.0 + 0.1 * torch.randn(dfsmn_aec.FEAT_DIM, generator=gen))
    pipe = types.SimpleNamespace(model=net, preprocessor=types.SimpleNamespace(feature=types.SimpleNamespace(shift=shift, scale=scale)))
    state = {k: v.detach().clone().numpy() for k, v in net.state_dict().items()}
    state["feature.shift"], state["feature.scale"] = shift.numpy().copy(), scale.numpy().copy()
    return pipe, state


def dfsmn_from_state(state, skip_connect, dilation):
    """The stand-in tree of fake_dfsmn with every dimension and weight taken from a state dict (tests/aec_geometry_lib.state): per-layer hidden size, lorder,
    dilation and skip_connect.  The reference pads every layer by layer 0's ``padding_left``, so ``dilation * (lorder - 1)`` must be one number."""
    t = {k: torch.from_numpy(np.asarray(v, np.float32).copy()) for k, v in state.items()}
    width = t["linear1.linear.weight"].shape[0]

    def lin(key, bias=True):
        o, i = t[key + ".weight"].shape
        m = nn.Linear(i, o, bias=bias)
        with torch.no_grad():
            m.weight.copy_(t[key + ".weight"])
            if bias:
                m.bias.copy_(t[key + ".bias"])
        return m

    class Layer(nn.Module):
        def __init__(self, i):
            super().__init__()
            lorder = t[f"deepfsmn.{i}.conv1.weight"].shape[2]
            self.linear, self.act, self.norm, self.project = lin(f"deepfsmn.{i}.linear"), nn.ReLU(), nn.Identity(), lin(f"deepfsmn.{i}.project", bias=False)
            self.conv1 = nn.Conv2d(width, width, (lorder, 1), dilation=(dilation[i], 1), groups=width, bias=False)
            with torch.no_grad():
                self.conv1.weight.copy_(t[f"deepfsmn.{i}.conv1.weight"])
            self.skip_connect, self.output_dim, self.padding_left = bool(skip_connect[i]), width, dilation[i] * (lorder - 1)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.linear1 = nn.Module()
            self.linear1.linear = lin("linear1.linear")
            self.relu, self.sig = nn.ReLU(), nn.Sigmoid()
            self.deepfsmn = nn.ModuleList([Layer(i) for i in range(len(skip_connect))])
            self.linear2, self.linear3 = lin("linear2"), lin("linear3")

    net = Net().eval()
    assert len({l.padding_left for l in net.deepfsmn}) == 1, "the reference shares layer 0's left pad"
    got = {k: v.numpy() for k, v in net.state_dict().items()}
    assert set(got) == set(state) - {"feature.shift", "feature.scale"} and all(np.array_equal(got[k], state[k]) for k in got)
    return types.SimpleNamespace(model=net, preprocessor=types.SimpleNamespace(feature=types.SimpleNamespace(shift=t["feature.shift"], scale=t["feature.scale"])))


def build(ns, seed=0, double=False, geometry=None):
    """The construction of Export_DFSMN_AEC.py:1394-1505 for the NKF back end.  ``geometry``: ``(nkf_state, dfsmn_state, skip_connect, dilation)`` of
    tests/aec_geometry_lib.state, loaded in place of the seeded stand-ins."""
    S = ns["STFT_Process"]
    static = ns["STATIC_EXPORT"]
    assert static
    stft_a2 = S(model_type="stft_B_packed", n_fft=ns["NFFT_A2"], hop_len=ns["HOP_LENGTH_A"], win_length=ns["WINDOW_LENGTH_A"], max_frames=0,
                window_type=ns["WINDOW_TYPE"], center_pad=False, pad_mode="constant", input_scale=1.0).eval()
    istft_a2 = S(model_type="istft_B_packed", n_fft=ns["NFFT_A2"], hop_len=ns["HOP_LENGTH_A"], win_length=ns["WINDOW_LENGTH_A"], max_frames=ns["MASK_FRAMES_A2"],
                 window_type=ns["WINDOW_TYPE"], center_pad=False, pad_mode="constant", static_frames=ns["MASK_FRAMES_A2"], output_length=ns["MODEL_AUDIO_LENGTH"],
                 output_scale=1.0).eval()
    stft_b = S(model_type="stft_B_packed", n_fft=ns["NFFT_B"], hop_len=ns["HOP_LENGTH_B"], win_length=ns["WINDOW_LENGTH_B"], max_frames=0,
               window_type=ns["WINDOW_TYPE_B"], center_pad=True, pad_mode="constant", input_scale=1.0).eval()
    istft_b = S(model_type="istft_B_packed", n_fft=ns["NFFT_B"], hop_len=ns["HOP_LENGTH_B"], win_length=ns["WINDOW_LENGTH_B"], max_frames=ns["BACKEND_FRAMES_B"],
                window_type=ns["WINDOW_TYPE_B"], center_pad=True, pad_mode="constant", static_frames=ns["BACKEND_FRAMES_B"], output_length=ns["MODEL_AUDIO_LENGTH"],
                output_scale=1.0).eval()
    torch.manual_seed(seed)
    nkf = ns["NKF_Inner"](L=ns["FILTER_ORDER"], fc_dim=ns["FC_DIM"], rnn_layers=ns["RNN_LAYERS"], rnn_dim=ns["RNN_DIM"], custom_stft=stft_b, custom_istft=istft_b,
                          max_frames=ns["BACKEND_FRAMES_B"], model_batch=ns["MODEL_BATCH"]).eval()
    if geometry is not None:
        load_checkpoint(nkf, geometry[0])
    else:
        with torch.no_grad():
            for p in nkf.kg_net.fc_out_dense2.parameters():
                p.mul_(NKF_GAIN_LAYER_SCALE)
    nkf_state = checkpoint_names({k: v.detach().clone().numpy() for k, v in nkf.state_dict().items() if k.startswith("kg_net.") and "buffer" not in k})
    nkf = nkf.float().eval()
    nkf.cache_export_constants_()
    pipe, dfsmn_state = (dfsmn_from_state(*geometry[1:]), geometry[1]) if geometry is not None else fake_dfsmn(seed)
    model = ns["DFSMN_AEC"](pipe, light_aec=nkf, light_aec_type="NKF", custom_stft_A2=stft_a2, custom_istft_A2=istft_a2, custom_stft_B=None, nfft_A=ns["NFFT_A"],
                            win_length_A=ns["WINDOW_LENGTH_A"], hop_length_A=ns["HOP_LENGTH_A"], pre_emphasis=ns["PRE_EMPHASIZE"],
                            in_sample_rate=ns["IN_SAMPLE_RATE"], out_sample_rate=ns["OUT_SAMPLE_RATE"], n_mels=ns["N_MELS"], use_batch_fold=ns["USE_BATCH_FOLD"],
                            fold_window=ns["FOLD_WINDOW_LENGTH"], alpha_predictor=None, k=None, static_batch=ns["MODEL_BATCH"],
                            static_audio_length=ns["MODEL_AUDIO_LENGTH"], backend_frames=ns["BACKEND_FRAMES_B"], mask_frames=ns["MASK_FRAMES_A2"],
                            backend_input_scale_folded=False, backend_output_scale_folded=False, output_scale_folded=False,
                            output_vad_result=ns["OUTPUT_VAD_RESULT"]).eval()
    return model, nkf_state, dfsmn_state


def run(ns, model, near, far, dtype=torch.int16, taps=False):
    """-> (audio flat, vad or None, taps dict)"""
    got = {}
    F = ns["torch"].nn.functional
    orig_linear, nkf_fwd, istft_fwd, stft_fwd = F.linear, model.light_aec.forward, model.custom_istft_A2.forward, model.custom_stft_A2.forward

    def linear_spy(x, w, b=None):
        if w is model.feature_linear_weight:
            got["feat"] = x.detach().clone().numpy()
        return orig_linear(x, w, b)

    def nkf_spy(pair):
        y = nkf_fwd(pair)
        got["temp_aec"] = y.detach().clone().numpy()
        return y

    def istft_spy(x):
        got["masked"] = x.detach().clone()
        y = istft_fwd(x)
        got["wave"] = y.detach().clone().numpy()
        return y
    def stft_spy(x):
        y = stft_fwd(x)
        got["spec"] = y.detach().clone().numpy()                    # (rows, [re 321 | im 321], Tm)
        return y
    if taps:
        F.linear, model.light_aec.forward, model.custom_istft_A2.forward, model.custom_stft_A2.forward = linear_spy, nkf_spy, istft_spy, stft_spy
        sig = model.dfsmn_aec.sig.forward
        masks = []
        model.dfsmn_aec.sig.forward = lambda x: masks.append(sig(x)) or masks[-1]
    try:
        with torch.inference_mode():
            y = model(torch.from_numpy(np.ascontiguousarray(near)).reshape(1, 1, -1).to(dtype), torch.from_numpy(np.ascontiguousarray(far)).reshape(1, 1, -1).to(dtype))
    finally:
        if taps:
            F.linear, model.light_aec.forward, model.custom_istft_A2.forward, model.custom_stft_A2.forward = orig_linear, nkf_fwd, istft_fwd, stft_fwd
            model.dfsmn_aec.sig.forward = sig
    vad = None
    if isinstance(y, tuple):
        y, vad = y
        vad = vad.numpy().reshape(-1)
    if taps:
        got["mask"] = [m for m in masks if m.shape[-1] == dfsmn_aec.N_BINS][0].numpy()          # (rows, Tm, 321)
        del got["masked"]
    return y.numpy().reshape(-1), vad, got


def rows():
    far, _ = read_pcm16(os.path.join(REF_ROOT, "Test_Examples", "aec", "farend_speech1.wav"))
    near, _ = read_pcm16(os.path.join(REF_ROOT, "Test_Examples", "aec", "nearend_mic1.wav"))
    return far[0], near[0]


def vad_fixture(fix_vad):
    """The reference driver's VAD post-processing (Inference_DFSMN_ONNX_AEC.py:383-443), run on the fixture's vad_results and on seeded probability tracks."""
    path = os.path.join(REF_ROOT, "DFSMN_AEC", "Inference_DFSMN_ONNX_AEC.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    want = ("probabilities_to_silence", "vad_to_timestamps", "process_timestamps")
    module = ast.Module(body=[n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want], type_ignores=[])
    ns = {"np": np}
    exec(compile(module, path, "exec"), ns)
    rng = np.random.default_rng(21)
    tracks = [np.asarray(fix_vad, np.float32)]
    for n, smooth in ((400, 25), (150, 5), (10, 1), (0, 1), (300, 60)):
        p = rng.random(n + smooth)
        p = np.convolve(p, np.ones(smooth) / smooth, mode="valid")[:n] if n else p[:0]
        p = np.clip((p - 0.5) * (6.0 if smooth > 1 else 1.0) + 0.5, 0.0, 1.0)
        tracks.append(p.astype(np.float32))
    out = {"n_tracks": np.int64(len(tracks))}
    shift, look = dfsmn_aec.HOP_LENGTH_A / 16000.0, max(1, int(dfsmn_aec.LOOK_AHEAD / (dfsmn_aec.HOP_LENGTH_A / 16000.0)))
    for i, p in enumerate(tracks):
        times = 0.25 * i + np.arange(len(p)) * shift
        states = ns["probabilities_to_silence"](p, dfsmn_aec.SPEAKING_SCORE, dfsmn_aec.SILENCE_SCORE, look)
        raw = ns["vad_to_timestamps"](states, shift, times)
        fused = ns["process_timestamps"](raw, dfsmn_aec.FUSION_THRESHOLD, dfsmn_aec.MIN_SPEECH_DURATION)
        out[f"prob{i}"], out[f"times{i}"] = p, times
        out[f"silence{i}"] = np.asarray(states, bool)
        out[f"raw{i}"] = np.asarray(raw, np.float64).reshape(-1, 2)
        out[f"fused{i}"] = np.asarray(fused, np.float64).reshape(-1, 2)
        print(f"vad track {i}: {len(p)} frames, {len(raw)} raw / {len(fused)} fused segments")
    np.savez_compressed(os.path.join(GOLD, "dfsmn_aec_seed0_vad.npz"), **out)


def main(seed=0):
    from dfsmn_aec_oracle import DfsmnAecOracle
    far_all, near_all = rows()
    # ---- unfolded, 32000 samples
    ns = import_namespace(USE_BATCH_FOLD=False, INPUT_AUDIO_LENGTH=L)
    assert ns["MODEL_BATCH"] == 1 and ns["MASK_FRAMES_A2"] == 99 and ns["BACKEND_FRAMES_B"] == 126
    model, nkf_state, dfsmn_state = build(ns, seed)
    blob = dfsmn_aec.state_to_blob_tensors(nkf_state, dfsmn_state, SKIP, [DILATION] * DEPTH)
    for k in ("feature_linear_weight", "feature_linear_bias"):          # the folded first layer is the reference's own buffer, bit for bit
        assert np.array_equal(blob[k], getattr(model, k).numpy()), k
    assert np.array_equal(blob["mel_banks"], model.mel_banks.numpy().reshape(80, 513))
    W.save_blob(os.path.join(GOLD, f"dfsmn_aec_seed{seed}.adew"), blob)
    state = {"nkf/" + k: v for k, v in nkf_state.items()}
    state.update({"dfsmn/" + k: v for k, v in dfsmn_state.items()})
    state["config"] = np.asarray(json.dumps({"skip_connect": SKIP, "dilation": [DILATION] * DEPTH}))
    np.savez_compressed(os.path.join(GOLD, f"dfsmn_aec_seed{seed}_state.npz"), **state)

    rng = np.random.default_rng(7)
    noise = [np.clip(np.round(rng.standard_normal(L) * 3000.0), -32768, 32767).astype(np.int16) for _ in range(2)]
    cases = [(near_all[48000:48000 + L], far_all[48000:48000 + L]), (noise[0], noise[1]), (near_all[96000:96000 + L], np.zeros(L, np.int16)),
             (np.zeros(L, np.int16), np.zeros(L, np.int16))]
    io, taps0 = {}, None
    for i, (n, f) in enumerate(cases):
        pcm, _, taps = run(ns, model, n, f, taps=(i == 0))
        io[f"near{i}"], io[f"far{i}"], io[f"out{i}"] = np.ascontiguousarray(n), np.ascontiguousarray(f), pcm.astype(np.int16)
        if i == 0:
            taps0 = taps
        print(f"row {i}: rms near {np.sqrt(np.mean((n / 32768.0) ** 2)):.4f} out {np.sqrt(np.mean((pcm / 32767.0) ** 2)):.4f} "
              f"rms(out - near) {np.sqrt(np.mean(((pcm.astype(np.float64) - n) / 32768.0) ** 2)):.4f}")
    assert not np.any(io["out3"]), "all-zero input must give all-zero PCM"
    np.savez_compressed(os.path.join(GOLD, f"dfsmn_aec_seed{seed}_io.npz"), **io)

    # VAD on: the same row 0, the second output
    ns_v = import_namespace(USE_BATCH_FOLD=False, INPUT_AUDIO_LENGTH=L, OUTPUT_VAD_RESULT=True)
    model_v, _, _ = build(ns_v, seed)
    pcm_v, vad, _ = run(ns_v, model_v, *cases[0])
    assert np.array_equal(pcm_v, io["out0"]) and vad.shape == (99,)
    tap_fix = {"temp_aec": taps0["temp_aec"].reshape(-1).astype(np.float32), "feat": taps0["feat"].reshape(99, 240).astype(np.float32),
               "mask": taps0["mask"].reshape(99, 321).astype(np.float32), "vad_results": vad.astype(np.float32), "wave": taps0["wave"].reshape(-1).astype(np.float32)}

    # ---- the distance between the reference's fp32 run and a float64 evaluation of the oracle, per tap: what two correct fp32 evaluations may differ by.
    # "reference": the oracle builds the two STFT_Process DFT kernels from fp32 angles as the reference does (its arithmetic rounding alone);
    # "exact": exact trigonometry, the quantity an FFT computes -- this one includes the reference's fp32 angle error (the gates of ade_dft_tables = exact);
    # "engine": reference tables in the back end, exact trigonometry in the 640-point mask transforms -- what the engine's default computes (its gates).
    dist = {}
    for tables in ("reference", "exact", "engine"):             # "engine": the engine's default -- reference tables in the back end, exact mask transforms
        oracle = DfsmnAecOracle(blob, tables="reference", mask_tables="exact") if tables == "engine" else DfsmnAecOracle(blob, tables=tables)
        opcm, otaps = oracle.forward(cases[0][0][None], cases[0][1][None])
        d = {}
        for k in ("temp_aec", "feat", "mask", "vad_results", "wave"):
            ref = tap_fix[k].astype(np.float64).reshape(-1)
            d[k] = float(np.abs(otaps[k].reshape(-1) - ref).max())
            d[k + "_peak"] = float(np.abs(ref).max())
        d["pcm_lsb"] = int(np.abs(opcm[0].astype(np.int32) - io["out0"].astype(np.int32)).max())
        dist[tables] = d
        print(f"fp32 reference vs float64 oracle ({tables} tables): " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in d.items()))
    tap_fix["fp64_distance"] = np.asarray(json.dumps(dist))
    np.savez_compressed(os.path.join(GOLD, f"dfsmn_aec_seed{seed}_taps.npz"), **tap_fix)

    # ---- folded, the folder's default: 1.5 s windows of 24000, 32000 -> 2 windows, 48000 samples in
    ns_f = import_namespace(USE_BATCH_FOLD=True, INPUT_AUDIO_LENGTH=L)
    assert ns_f["FOLD_WINDOW_LENGTH"] == 24000 and ns_f["EXPORT_AUDIO_LENGTH"] == 48000 and ns_f["MODEL_BATCH"] == 2 and ns_f["MASK_FRAMES_A2"] == 74
    model_f, _, _ = build(ns_f, seed)
    fn, ff = near_all[48000:96000], far_all[48000:96000]
    pcm_f, _, _ = run(ns_f, model_f, fn, ff)
    fold = {"near": np.ascontiguousarray(fn), "far": np.ascontiguousarray(ff), "out": pcm_f.astype(np.int16)}
    # the fold is a batch of independent windows: 2 x 32000 folded (2 s windows) == two unfolded 32000 runs
    ns_c = import_namespace(USE_BATCH_FOLD=True, INPUT_AUDIO_LENGTH=2 * L, BATCH_WINDOW_SECONDS=2.0, OUTPUT_VAD_RESULT=True)
    assert ns_c["FOLD_WINDOW_LENGTH"] == L and ns_c["MODEL_BATCH"] == 2
    model_c, _, _ = build(ns_c, seed)
    cn, cf = near_all[48000:48000 + 2 * L], far_all[48000:48000 + 2 * L]
    pcm_c, vad_c, _ = run(ns_c, model_c, cn, cf)
    singles = [run(ns_v, model_v, cn[k * L:(k + 1) * L], cf[k * L:(k + 1) * L]) for k in range(2)]
    d_lsb = int(np.abs(pcm_c.astype(np.int32) - np.concatenate([s[0] for s in singles]).astype(np.int32)).max())
    d_vad = float(np.abs(vad_c - np.concatenate([s[1] for s in singles])).max())
    print(f"fold check: 2 x 32000 folded vs unfolded: {d_lsb} LSB, vad {d_vad:.1e}")
    assert d_lsb == 0 and d_vad <= 1e-6
    fold["fold_check"] = np.asarray(json.dumps({"pcm_lsb": d_lsb, "vad": d_vad, "window": L, "windows": 2}))
    np.savez_compressed(os.path.join(GOLD, f"dfsmn_aec_seed{seed}_fold.npz"), **fold)

    # ---- F32 in / F32 out, and 48 kHz out (unfolded: batch folding needs equal rates)
    extra = {}
    xn, xf = (cases[0][0] / 32768.0).astype(np.float32), (cases[0][1] / 32768.0).astype(np.float32)
    ns32 = import_namespace(USE_BATCH_FOLD=False, INPUT_AUDIO_LENGTH=L, IN_AUDIO_DTYPE="F32", OUT_AUDIO_DTYPE="F32")
    m32, _, _ = build(ns32, seed)
    o32, _, _ = run(ns32, m32, xn, xf, dtype=torch.float32)
    extra["f32_out"] = o32.astype(np.float32)                                   # inputs: row 0 of the io fixture / 32768
    ns48 = import_namespace(USE_BATCH_FOLD=False, INPUT_AUDIO_LENGTH=L, OUT_SAMPLE_RATE=48000)
    m48, _, _ = build(ns48, seed)
    o48, _, _ = run(ns48, m48, *cases[0])
    assert o48.size == 3 * L
    extra["r48_out"] = o48.astype(np.int16)
    # 48 kHz in: 96000 samples -> 32000 at the model rate (both inputs interpolated ahead of the back end, :1189-1207)
    ns_i = import_namespace(USE_BATCH_FOLD=False, INPUT_AUDIO_LENGTH=3 * L, IN_SAMPLE_RATE=48000)
    assert ns_i["MODEL_AUDIO_LENGTH"] == L
    m_i, _, _ = build(ns_i, seed)
    rng_i = np.random.default_rng(19)
    up = lambda x: np.clip(np.round(np.interp(np.arange(3 * L) / 3.0, np.arange(L), x.astype(np.float64)) + rng_i.standard_normal(3 * L) * 20.0), -32768, 32767).astype(np.int16)
    extra["in48_near"], extra["in48_far"] = up(cases[0][0]), up(cases[0][1])
    o_i, _, _ = run(ns_i, m_i, extra["in48_near"], extra["in48_far"])
    assert o_i.size == L
    extra["in48_out"] = o_i.astype(np.int16)
    # the manifest's key set, from the reference's own builder
    sys.path.insert(0, REF_ROOT)
    try:
        from audio_onnx_metadata import build_audio_metadata_from_globals
        g = dict(ns_f)
        g.setdefault("OPSET", 20)
        meta = build_audio_metadata_from_globals(
            g, producer="Export_DFSMN_AEC.py", model_name="DFSMN_AEC", task="aec", model_family="dfsmn_aec", max_dynamic_audio_seconds=30,
            normalize_audio_default=False, input_channels=1, output_channels=1, num_audio_inputs=2, feature_kind="kaldi_fbank_stft_aec", center_pad=False,
            pad_mode="constant", extra={k: v for k, v in dfsmn_aec.metadata(L).items() if k in (
                "light_aec_model", "n_mels", "nfft_a", "nfft_a2", "window_length_a", "hop_length_a", "nfft_b", "window_length_b", "hop_length_b", "window_type_b",
                "preemphasize", "filter_order", "output_vad_result", "num_outputs", "output_frame_shift_seconds", "output_frame_shift_samples",
                "fbank_window_length_samples", "speaking_score", "silence_score", "look_ahead_seconds", "fusion_threshold_seconds", "min_speech_duration_seconds")})
        extra["metadata_keys"] = np.asarray(json.dumps(sorted(k for k, v in meta.items() if v is not None)))
        extra["metadata_folded_default"] = np.asarray(json.dumps({k: str(v) for k, v in meta.items() if k in (
            "input_audio_length", "export_audio_length", "fold_window_length", "use_batch_fold", "model_family", "window_type", "nfft", "hop_length",
            "window_length", "center_pad", "pad_mode", "num_audio_inputs")}))
    except Exception as exc:                                                    # the key set test then skips nothing: it falls back to the listed keys
        print("reference metadata builder not importable:", exc)
    np.savez_compressed(os.path.join(GOLD, f"dfsmn_aec_seed{seed}_extra.npz"), **extra)
    vad_fixture(vad)
    for fn_ in sorted(os.listdir(GOLD)):
        if fn_.startswith("dfsmn_aec"):
            print(fn_, os.path.getsize(os.path.join(GOLD, fn_)))


STREAM_LEN, STREAM_OFFSETS = 40960, (20000, 80000)      # 160 hops, 127 mask frames; two cuts of the reference's example recordings


def stream_fixture(seed=0):
    """tests/golden/dfsmn_aec_seed0_stream.npz: the reference's unfolded DFSMN_AEC.forward in ONE call on two clips of 40 960 samples, with the committed
    seed-0 state (the construction is seeded; the state it yields is checked against tests/golden/dfsmn_aec_seed0_state.npz).  int16 near / far / out and the
    f32 waveform before the PCM tail, per clip."""
    far_all, near_all = rows()
    ns = import_namespace(USE_BATCH_FOLD=False, INPUT_AUDIO_LENGTH=STREAM_LEN)
    assert ns["MODEL_BATCH"] == 1 and ns["MASK_FRAMES_A2"] == 127 and ns["BACKEND_FRAMES_B"] == 161
    model, nkf_state, dfsmn_state = build(ns, seed)
    committed = np.load(os.path.join(GOLD, f"dfsmn_aec_seed{seed}_state.npz"))
    for prefix, state in (("nkf/", nkf_state), ("dfsmn/", dfsmn_state)):
        for k, v in state.items():
            assert np.array_equal(committed[prefix + k], v), prefix + k
    out = {}
    for i, o in enumerate(STREAM_OFFSETS):
        near, far = np.ascontiguousarray(near_all[o:o + STREAM_LEN]), np.ascontiguousarray(far_all[o:o + STREAM_LEN])
        assert near.shape == far.shape == (STREAM_LEN,)
        pcm, _, taps = run(ns, model, near, far, taps=True)
        out[f"near{i}"], out[f"far{i}"], out[f"out{i}"], out[f"wave{i}"] = near, far, pcm.astype(np.int16), taps["wave"].reshape(-1).astype(np.float32)
        print(f"clip {i}: rms near {np.sqrt(np.mean((near / 32768.0) ** 2)):.4f} out {np.sqrt(np.mean((pcm / 32767.0) ** 2)):.4f}")
    path = os.path.join(GOLD, f"dfsmn_aec_seed{seed}_stream.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


def geometry_fixtures():
    """tests/golden/aec_geom_<name>.npz for every geometry of tests/aec_geometry_lib.py: the reference's DFSMN_AEC.forward (unfolded 3200, every row; folded
    2 x 1600, two calls) and NKF.forward (3200 and 3000 samples) on the generated weights, and the recorded distances the tests' gates are read from."""
    import hashlib
    import aec_geometry_lib as G
    import make_golden_nkf_aec as nkf_tool
    from dfsmn_aec_oracle import DfsmnAecOracle
    from nkf_aec_oracle import NkfAecOracle
    WL, WF = G.W_LONG, G.W_FOLD
    ns = import_namespace(USE_BATCH_FOLD=False, INPUT_AUDIO_LENGTH=WL, OUTPUT_VAD_RESULT=True)
    ns_f = import_namespace(USE_BATCH_FOLD=True, INPUT_AUDIO_LENGTH=WL, BATCH_WINDOW_SECONDS=G.FOLD_SECONDS, OUTPUT_VAD_RESULT=True)
    Tm, Tf = dfsmn_aec.mask_frames(WL), dfsmn_aec.mask_frames(WF)
    assert ns["MODEL_BATCH"] == 1 and ns["MASK_FRAMES_A2"] == Tm == 9 and ns["BACKEND_FRAMES_B"] == 13
    assert ns_f["FOLD_WINDOW_LENGTH"] == WF and ns_f["EXPORT_AUDIO_LENGTH"] == WL and ns_f["MODEL_BATCH"] == 2 and ns_f["MASK_FRAMES_A2"] == Tf == 4
    ns_n = {L: nkf_tool.import_namespace(L) for L in G.NKF_LENGTHS}
    for name in G.GEOMETRIES:
        geometry = G.state(name)
        blob = dfsmn_aec.state_to_blob_tensors(*geometry)
        model, _, _ = build(ns, geometry=geometry)
        for k in ("feature_linear_weight", "feature_linear_bias"):          # the folded first layer is the reference's own buffer, bit for bit
            assert np.array_equal(blob[k], getattr(model, k).numpy()), k
        near, far = G.signals(name)
        fix = {"near": near, "far": far, "blob_sha256": np.asarray(hashlib.sha256(W.pack_blob(blob)).hexdigest())}
        outs, vads, row_taps = [], [], []
        for i in range(G.N_ROWS):
            pcm, vad, taps = run(ns, model, near[i], far[i], taps=True)
            outs.append(pcm.astype(np.int16))
            vads.append(vad.astype(np.float32))
            sp = taps["spec"].reshape(2, dfsmn_aec.N_BINS, Tm)
            row_taps.append({"temp_aec": taps["temp_aec"].reshape(-1), "spec": np.stack([sp[0].T, sp[1].T], axis=-1),
                             "feat": taps["feat"].reshape(Tm, dfsmn_aec.FEAT_DIM), "mask": taps["mask"].reshape(Tm, dfsmn_aec.N_BINS), "vad_results": vads[i],
                             "wave": taps["wave"].reshape(-1)})
        assert outs[0].any() and outs[1].any() and outs[3].any() and not outs[2].any(), "live rows, and all-zero input must give all-zero PCM"
        fix["out"], fix["vad"] = np.stack(outs), np.stack(vads)
        tap_fix = row_taps[0]
        for k, v in tap_fix.items():
            fix["tap_" + k] = np.ascontiguousarray(v, np.float32)
        model_f, _, _ = build(ns_f, geometry=geometry)
        folded = [run(ns_f, model_f, near[i], far[i]) for i in (0, 3)]
        fix["fold_out"], fix["fold_vad"] = np.stack([f[0].astype(np.int16) for f in folded]), np.stack([f[1].astype(np.float32) for f in folded])
        # the distance between the reference's fp32 run and the float64 oracle per tap, as dfsmn_aec_seed0_taps.npz records it (see main): row 0, which the
        # gates are read from.  ``<tap>_all_rows`` is the same distance over every row of the long shape (far end silent and all zero included): a record that
        # the reference's own fp32 run is no further from the oracle on the rows whose taps are not kept than on row 0
        dist = {}
        for tables in ("reference", "exact", "engine"):
            oracle = DfsmnAecOracle(blob, tables="reference", mask_tables="exact") if tables == "engine" else DfsmnAecOracle(blob, tables=tables)
            opcm, otaps = oracle.forward(near[:1], far[:1])
            otaps["spec"] = np.stack([otaps["spec"].real, otaps["spec"].imag], axis=-1)
            d = {}
            for k in tap_fix:
                ref = tap_fix[k].astype(np.float32).astype(np.float64).reshape(-1)
                d[k] = float(np.abs(otaps[k].reshape(-1) - ref).max())
                d[k + "_peak"] = float(np.abs(ref).max())
            d["pcm_lsb"] = int(np.abs(opcm[0].astype(np.int32) - outs[0].astype(np.int32)).max())
            _, otaps_all = oracle.forward(near, far)
            otaps_all["spec"] = np.stack([otaps_all["spec"].real, otaps_all["spec"].imag], axis=-1)
            for k in tap_fix:
                ref = np.stack([r[k] for r in row_taps]).astype(np.float32).astype(np.float64).reshape(-1)
                d[k + "_all_rows"] = float(np.abs(otaps_all[k].reshape(-1) - ref).max())
            opcm_f, _ = oracle.forward(near[[0, 3]], far[[0, 3]], fold_window=WF)
            d["fold_pcm_lsb"] = int(np.abs(opcm_f.astype(np.int32) - fix["fold_out"].astype(np.int32)).max())
            dist[tables] = d
            print(f"{name}: fp32 reference vs float64 oracle ({tables} tables): " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in d.items()))
        fix["fp64_distance"] = np.asarray(json.dumps(dist))
        # NKF.forward on the same NKF weights: rows 0, 1 (far end silent) and 3.  The engine's transforms are FFTs, so its oracle has exact tables; the recorded
        # distance of echo_hat and kg is the one between the reference-table and the exact-table oracle (the two things the existing fixtures set side by side)
        nkf_dist = {}
        for L in G.NKF_LENGTHS:
            model_n, _ = nkf_tool.build(ns_n[L], state=geometry[0])
            rows_n = (0, 1, 3)
            ref_runs = [nkf_tool.run(model_n, np.ascontiguousarray(far[i, :L]), np.ascontiguousarray(near[i, :L])) for i in rows_n]
            keep = ref_runs[0][0].size
            assert keep == 256 * (L // 256) and not np.any(ref_runs[1][2]), "far end zero must give echo_hat == 0"
            fix[f"nkf_out_{L}"] = np.stack([r[0].astype(np.int16) for r in ref_runs])
            ex = NkfAecOracle(blob, tables="exact").forward(far[rows_n, :L], near[rows_n, :L], want_taps=True, audio_len=keep)
            rf = NkfAecOracle(blob, tables="reference").forward(far[rows_n, :L], near[rows_n, :L], want_taps=True, audio_len=keep)
            ref_wave = np.stack([r[1][:keep].astype(np.float64) / 32767.0 for r in ref_runs])
            ref_echo = np.stack([r[2][0, 0] + 1j * r[2][1, 0] for r in ref_runs])                      # (rows, F, T)
            d = {"echo_hat": float(np.abs(ex[2]["echo_hat"] - rf[2]["echo_hat"]).max()), "echo_hat_peak": float(np.abs(ex[2]["echo_hat"]).max()),
                 "kg": float(np.abs(ex[2]["kg"] - rf[2]["kg"]).max()), "kg_peak": float(np.abs(ex[2]["kg"]).max()),
                 "wave": float(np.abs(ex[1] - ref_wave).max()), "wave_peak": float(np.abs(ref_wave).max()),
                 "echo_hat_fp32": float(np.abs(ex[2]["echo_hat"] - ref_echo).max()),
                 "pcm_lsb": int(np.abs(ex[0].astype(np.int32) - fix[f"nkf_out_{L}"].astype(np.int32)).max())}
            nkf_dist[str(L)] = d
            print(f"{name}: NKF {L}: " + ", ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in d.items()))
        fix["nkf_distance"] = np.asarray(json.dumps(nkf_dist))
        path = os.path.join(GOLD, f"aec_geom_{name}.npz")
        np.savez_compressed(path, **fix)
        print(os.path.basename(path), os.path.getsize(path))


if __name__ == "__main__":
    if "--geometry" in sys.argv:
        geometry_fixtures()
    elif "--stream" in sys.argv:
        stream_fixture()
    else:
        main()
