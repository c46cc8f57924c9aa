"""DFSMN-AEC without a GPU: the numpy oracle against the reference-run fixtures (tools/make_golden_dfsmn_aec.py), the manifest, the export round trip, the file
driver's slicing and VAD post-processing, and the engine's refusals (answered before any device is touched)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from dfsmn_aec_oracle import DfsmnAecOracle  # noqa: E402

GOLD = os.path.join(HERE, "golden")
L = 32000


def _blob_tensors():
    from audio_denoiser_onnx_amd.weights import load_blob
    return load_blob(os.path.join(GOLD, "dfsmn_aec_seed0.adew"))


@pytest.fixture(scope="module")
def rows():
    io = np.load(os.path.join(GOLD, "dfsmn_aec_seed0_io.npz"))
    return (np.stack([io[f"near{i}"] for i in range(4)]), np.stack([io[f"far{i}"] for i in range(4)]), np.stack([io[f"out{i}"] for i in range(4)]))


def test_oracle_matches_reference_forward(rows):
    """The float64 oracle with the reference's own DFT tables: every row within 1 LSB, the all-zero row all zero, every tap of the speech row within 1.05 x the
    distance the fixture generator recorded (the reference's fp32 rounding)."""
    near, far, out = rows
    tp = np.load(os.path.join(GOLD, "dfsmn_aec_seed0_taps.npz"))
    rec = json.loads(str(tp["fp64_distance"]))["reference"]
    pcm, taps = DfsmnAecOracle(_blob_tensors(), tables="reference").forward(near, far)
    lsb = [int(np.abs(pcm[i].astype(np.int32) - out[i]).max()) for i in range(4)]
    print("oracle vs reference, LSB per row:", lsb)
    assert max(lsb) <= 1 and not np.any(pcm[3]) and not np.any(out[3])
    got = {"temp_aec": taps["temp_aec"][0], "feat": taps["feat"][0], "mask": taps["mask"][0], "vad_results": taps["vad_results"][:99], "wave": taps["wave"][0]}
    for k, v in got.items():
        d = float(np.abs(v.reshape(-1) - tp[k].astype(np.float64).reshape(-1)).max())
        print(f"  {k}: {d:.3e} (recorded {rec[k]:.3e})")
        assert d <= 1.05 * rec[k] + 1e-12, k
    assert float(np.abs(got["wave"] - tp["wave"]).max()) <= 1e-4


def test_oracle_folded_and_float_fixtures(rows):
    near, far, _ = rows
    fx = np.load(os.path.join(GOLD, "dfsmn_aec_seed0_fold.npz"))
    oracle = DfsmnAecOracle(_blob_tensors(), tables="reference")
    pcm, taps = oracle.forward(fx["near"][None], fx["far"][None], fold_window=24000)
    assert taps["temp_aec"].shape == (2, 24000) and taps["vad_results"].shape == (148,)
    assert int(np.abs(pcm[0].astype(np.int32) - fx["out"]).max()) <= 1
    check = json.loads(str(fx["fold_check"]))          # the reference's own folded run equals its unfolded runs
    assert check["pcm_lsb"] == 0 and check["vad"] <= 1e-6
    ex = np.load(os.path.join(GOLD, "dfsmn_aec_seed0_extra.npz"))
    o32, _ = oracle.forward((near[:1] / 32768.0).astype(np.float32), (far[:1] / 32768.0).astype(np.float32), int_in=False, int_out=False)
    assert o32.dtype == np.float32 and float(np.abs(o32[0] - ex["f32_out"]).max()) <= 1e-4


def test_metadata_keys():
    from audio_denoiser_onnx_amd import dfsmn_aec
    from audio_denoiser_onnx_amd.metadata import REQUIRED_AUDIO_METADATA_KEYS
    m = dfsmn_aec.metadata(L)
    for k in REQUIRED_AUDIO_METADATA_KEYS:
        assert m.get(k), k
    want = {"light_aec_model": "NKF", "n_mels": "80", "nfft_a": "1024", "nfft_a2": "640", "window_length_a": "640", "hop_length_a": "320", "nfft_b": "1024",
            "window_length_b": "1024", "hop_length_b": "256", "window_type_b": "hann", "preemphasize": "0.97", "filter_order": "4", "output_vad_result": "0",
            "num_outputs": "1", "output_frame_shift_seconds": "0.02", "output_frame_shift_samples": "320", "fbank_window_length_samples": "640",
            "speaking_score": "0.5", "silence_score": "0.5", "look_ahead_seconds": "0.3", "fusion_threshold_seconds": "0.3", "min_speech_duration_seconds": "0.2",
            "model_family": "dfsmn_aec", "task": "aec", "num_audio_inputs": "2", "feature_kind": "kaldi_fbank_stft_aec", "center_pad": "0", "pad_mode": "constant",
            "window_type": "hamming_symmetric", "nfft": "640", "hop_length": "320", "window_length": "640", "use_batch_fold": "1", "fold_window_length": "24000",
            "export_audio_length": "48000", "input_audio_length": "32000"}
    for k, v in want.items():
        assert m[k] == v, (k, m[k], v)
    ex = np.load(os.path.join(GOLD, "dfsmn_aec_seed0_extra.npz"))
    if "metadata_keys" in ex.files:          # the key set the reference's own builder stamps for this export
        ref_keys = set(json.loads(str(ex["metadata_keys"])))
        assert ref_keys <= set(m), sorted(ref_keys - set(m))
        for k, v in json.loads(str(ex["metadata_folded_default"])).items():
            assert m[k] == {"True": "1", "False": "0"}.get(v, v), (k, m[k], v)
    mv = dfsmn_aec.metadata(L, use_batch_fold=False, output_vad_result=True, dft_tables="exact")
    assert mv["output_vad_result"] == "1" and mv["num_outputs"] == "2" and mv["export_audio_length"] == "32000" and mv["ade_dft_tables"] == "exact"


def test_export_round_trip(tmp_path):
    """state (the NKF checkpoint's key names + the DFSMN network's state dict) -> blob == the committed blob, through the function and through export_dfsmn_aec;
    the folded first layer is checked against an independent float64 evaluation."""
    from audio_denoiser_onnx_amd import dfsmn_aec
    from audio_denoiser_onnx_amd.export import export_dfsmn_aec
    from audio_denoiser_onnx_amd.metadata import read_metadata
    from audio_denoiser_onnx_amd.weights import load_blob
    st = np.load(os.path.join(GOLD, "dfsmn_aec_seed0_state.npz"))
    nkf = {k[4:]: st[k] for k in st.files if k.startswith("nkf/")}
    net = {k[6:]: st[k] for k in st.files if k.startswith("dfsmn/")}
    cfg = json.loads(str(st["config"]))
    blob = _blob_tensors()
    got = dfsmn_aec.state_to_blob_tensors(nkf, net, cfg["skip_connect"], cfg["dilation"])
    assert set(got) == set(blob)
    for k in blob:
        assert got[k].shape == blob[k].shape and np.array_equal(got[k], blob[k]), k
    w, b, sh, sc = (net[k].astype(np.float64) for k in ("linear1.linear.weight", "linear1.linear.bias", "feature.shift", "feature.scale"))
    x = np.random.default_rng(1).standard_normal(240) * 5.0 + 15.0
    assert np.allclose(blob["feature_linear_weight"].astype(np.float64) @ x + blob["feature_linear_bias"], w @ ((x + sh) * sc) + b, rtol=0, atol=1e-4)
    assert blob["fsmn_conv_weight_0"].shape == (128, 1, 20) and np.array_equal(blob["fsmn_conv_weight_2"][:, 0], net["deepfsmn.2.conv1.weight"][:, 0, :, 0])
    np.savez(tmp_path / "net.npz", config=st["config"], **net)
    np.savez(tmp_path / "nkf.npz", **nkf)
    path = export_dfsmn_aec(tmp_path / "net.npz", tmp_path / "nkf.npz", tmp_path / "model", L, output_vad_result=True)
    rt = load_blob(path)
    assert all(np.array_equal(rt[k], blob[k]) for k in blob)
    m = read_metadata(path)
    assert m["model_family"] == "dfsmn_aec" and m["export_audio_length"] == "48000" and m["output_vad_result"] == "1"
    with pytest.raises(KeyError):
        dfsmn_aec.state_to_blob_tensors(nkf, {k: v for k, v in net.items() if k != "linear3.bias"}, cfg["skip_connect"], cfg["dilation"])


def test_seeded_weightgen_is_a_valid_state():
    from audio_denoiser_onnx_amd import dfsmn_aec, weightgen
    t = dfsmn_aec.state_to_blob_tensors(*weightgen.dfsmn_aec_state(seed=3, width=96, hidden=48, depth=3, lorder=8, dilation=1))
    assert t["feature_linear_weight"].shape == (96, 240) and t["fsmn_conv_weight_2"].shape == (96, 1, 8) and t["fsmn_skip"].tolist() == [1.0, 0.0, 1.0]
    t2 = dfsmn_aec.state_to_blob_tensors(*weightgen.dfsmn_aec_state(seed=3, width=96, hidden=48, depth=3, lorder=8, dilation=1))
    assert all(np.array_equal(t[k], t2[k]) for k in t)
    rng = np.random.default_rng(0)
    x = np.clip(np.round(rng.standard_normal((2, 1, 3200)) * 3000), -32768, 32767).astype(np.int16)
    pcm, taps = DfsmnAecOracle(t, tables="exact").forward(x[0], x[1])
    assert np.all(np.isfinite(taps["wave"])) and 0.0 < float(np.abs(taps["wave"]).max()) < 4.0


class _FakeSession:
    def __init__(self, length, fold, vad=True, in_rate=16000):
        from audio_denoiser_onnx_amd import dfsmn_aec
        from audio_denoiser_onnx_amd.metadata import MetadataReader
        self.metadata = MetadataReader(dfsmn_aec.metadata(length, use_batch_fold=fold, output_vad_result=vad, in_sample_rate=in_rate))
        self.in_len = self.metadata.optional_int("export_audio_length")
        self.in_sample_rate = self.out_sample_rate = in_rate
        self._vad = vad


def test_driver_slicing():
    from audio_denoiser_onnx_amd import inference_dfsmn_aec as drv
    x = (np.arange(70000) % 2000 - 1000).astype(np.int16)
    folded, plain = _FakeSession(L, True), _FakeSession(L, False)
    assert drv.fold_window(folded) == 24000 and drv.fold_window(plain) == 0
    rf = drv.slice_signal(folded, x)
    assert rf.shape == (2, 48000) and np.array_equal(rf.reshape(-1)[:70000], x) and not np.any(rf.reshape(-1)[70000:])          # zero padding when folded
    r1, r2 = drv.slice_signal(plain, x, np.random.default_rng(5)), drv.slice_signal(plain, x, np.random.default_rng(5))
    assert r1.shape == (3, L) and np.array_equal(r1, r2) and np.array_equal(r1.reshape(-1)[:70000], x)
    tail = r1.reshape(-1)[70000:].astype(np.float64)
    ref_rms = np.sqrt(np.mean(x[-tail.size:].astype(np.float64) ** 2))
    assert tail.size == 26000 and 0.9 * ref_rms < np.sqrt(np.mean(tail ** 2)) < 1.1 * ref_rms                                    # seeded noise tail otherwise
    short = drv.slice_signal(folded, x[:1000])
    assert short.shape == (1, 48000) and not np.any(short[0, 1000:])
    # frames inside the signal: unfolded, and folded window by window
    assert [drv.valid_frames(n) for n in (0, 639, 640, 959, 960, 32000)] == [0, 0, 1, 1, 2, 99]
    assert drv.valid_frames(48000, 24000) == 148 and drv.valid_frames(24000 + 700, 24000) == 75 and drv.valid_frames(24000 + 600, 24000) == 74
    t = drv.frame_times(3.0, 24000 + 960, 24000)
    assert t.shape == (76,) and t[0] == 3.0 and abs(t[73] - (3.0 + 73 * 0.02)) < 1e-12 and abs(t[74] - 4.5) < 1e-12 and abs(t[75] - 4.52) < 1e-12
    assert np.allclose(drv.frame_times(1.0, 1000), [1.0, 1.02])


def test_vad_post_processing_matches_the_reference():
    """Hysteresis with look-ahead, segment extraction, minimum duration and fusion against the lists the reference's own functions produced (recorded by the
    fixture generator on the fixture's vad_results and on seeded probability tracks)."""
    from audio_denoiser_onnx_amd import inference_dfsmn_aec as drv
    fx = np.load(os.path.join(GOLD, "dfsmn_aec_seed0_vad.npz"))
    n = int(fx["n_tracks"])
    assert n >= 5
    seen = 0
    for i in range(n):
        prob, times = fx[f"prob{i}"], fx[f"times{i}"]
        states = drv.silence_states(prob, 0.5, 0.5, 15)
        assert states == fx[f"silence{i}"].tolist(), i
        raw = drv.segments(states, 0.02, times)
        assert np.array_equal(np.asarray(raw, np.float64).reshape(-1, 2), fx[f"raw{i}"]), i
        fused = drv.fuse_segments(raw, 0.3, 0.2)
        assert np.array_equal(np.asarray(fused, np.float64).reshape(-1, 2), fx[f"fused{i}"]), i
        seen += len(raw)
    assert seen >= 10
    assert np.array_equal(fx["prob0"], np.load(os.path.join(GOLD, "dfsmn_aec_seed0_taps.npz"))["vad_results"])
    assert drv.format_time(3661.0405) == "01:01:01.040" and drv.format_time(0.0) == "00:00:00.000"
    # through the driver's own assembly: one unfolded slice, the whole of it inside the signal
    sess = _FakeSession(L, False)
    stamps = drv.timestamps(sess, fx["prob0"][None], L)
    assert np.allclose(np.asarray(stamps).reshape(-1, 2), fx["fused0"] - fx["times0"][0])


def _create(meta_over, **kw):
    from audio_denoiser_onnx_amd import _lib, dfsmn_aec
    from audio_denoiser_onnx_amd.metadata import MetadataReader
    lib = _lib.get_library()
    m = dfsmn_aec.metadata(L, **kw)
    m.update(meta_over)
    with open(os.path.join(GOLD, "dfsmn_aec_seed0.adew"), "rb") as f:
        blob = f.read()
    h = C.c_void_p()
    st = lib.c.ade_create(MetadataReader(m).to_json().encode(), blob, len(blob), 0, C.byref(h))
    if h.value:
        lib.c.ade_destroy(h)
    err = lib.c.ade_last_error(None)
    return st, (err.decode() if err else "")


@pytest.mark.parametrize("over, kw, key", [
    ({"light_aec_model": "SDAEC"}, {}, "light_aec_model"),
    ({"light_aec_model": "Deep_Echo"}, {}, "light_aec_model"),
    ({"dynamic_axes": "1"}, {"use_batch_fold": False}, "dynamic_axes"),
    ({"nfft_a2": "512"}, {}, "nfft_a2"),
    ({"hop_length": "160"}, {}, "hop_length"),
    ({"window_type": "hann"}, {}, "window_type"),
    ({"nfft_b": "512"}, {}, "nfft_b"),
    ({"hop_length_b": "128"}, {}, "hop_length_b"),
    ({"n_mels": "64"}, {}, "n_mels"),
    ({"fold_window_length": "24100", "export_audio_length": "48200"}, {}, "fold_window_length"),
    ({"fold_window_length": "640", "export_audio_length": "32000"}, {}, "fold_window_length"),
])
def test_manifest_refusals_without_device(over, kw, key):
    """Everything but the NKF back end, static axes, the three STFT configurations, 80 mel bands and whole-hop fold windows is refused before any device is
    touched (ADE_ERR_UNSUPPORTED = 6, include/ade.h), and the message names the key."""
    st, err = _create(over, **kw)
    assert st == 6, (st, err)
    assert key in err, err
