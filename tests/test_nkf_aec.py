"""NKF-AEC on the CPU: the numpy oracle (tests/nkf_aec_oracle.py) against the reference's own outputs (tests/golden/nkf_aec_seed0*,
tools/make_golden_nkf_aec.py), the checkpoint -> blob mapping, and the manifest checks that need no device."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from nkf_aec_oracle import NkfAecOracle  # noqa: E402

GOLD = os.path.join(HERE, "golden")
N_ROWS = 5


def _blob_tensors():
    from audio_denoiser_onnx_amd.weights import load_blob
    return load_blob(os.path.join(GOLD, "nkf_aec_seed0.adew"))


def _rows():
    io = np.load(os.path.join(GOLD, "nkf_aec_seed0_io.npz"))
    return (np.stack([io[f"far{i}"] for i in range(N_ROWS)]), np.stack([io[f"near{i}"] for i in range(N_ROWS)]),
            np.stack([io[f"out{i}"] for i in range(N_ROWS)]))


@pytest.fixture(scope="module")
def oracle_runs():
    far, near, out = _rows()
    runs = {tab: NkfAecOracle(_blob_tensors(), tab).forward(far, near, want_taps=True) for tab in ("reference", "exact")}
    return far, near, out, runs


def test_oracle_matches_reference_forward(oracle_runs):
    _, _, out, runs = oracle_runs
    pcm, wave, taps = runs["reference"]
    wv = np.load(os.path.join(GOLD, "nkf_aec_seed0_wave.npz"))
    assert int(np.abs(pcm.astype(np.int32) - out).max()) <= 1
    assert max(float(np.abs(wave[i] - wv[f"wave{i}"]).max()) for i in range(N_ROWS)) <= 1e-5
    ref = np.load(os.path.join(GOLD, "nkf_aec_seed0_taps.npz"))["echo_hat0"]
    got = np.stack([taps["echo_hat"][0].real, taps["echo_hat"][0].imag])
    assert float(np.abs(got - ref).max()) <= 1e-5 * float(np.abs(ref).max())
    assert not np.any(taps["echo_hat"][3])                 # far end zero -> echo estimate exactly zero
    assert np.sqrt(np.mean(((out[0].astype(np.float64) - _rows()[1][0]) / 32768.0) ** 2)) > 0.01     # the echo path is exercised


def test_exact_tables_meet_the_contract(oracle_runs):
    """Exact trigonometry (what the engine's FFT computes) against the reference's fp32-angle DFT tables: within 1e-4 / 1 LSB."""
    _, _, out, runs = oracle_runs
    pcm, wave, _ = runs["exact"]
    wv = np.load(os.path.join(GOLD, "nkf_aec_seed0_wave.npz"))
    assert int(np.abs(pcm.astype(np.int32) - out).max()) <= 1
    assert max(float(np.abs(wave[i] - wv[f"wave{i}"]).max()) for i in range(N_ROWS)) <= 1e-4


def test_oracle_float_io_fixture():
    ex = np.load(os.path.join(GOLD, "nkf_aec_seed0_extra.npz"))
    o, _, _ = NkfAecOracle(_blob_tensors()).forward(ex["f32_far"][None], ex["f32_near"][None], int_in=False, int_out=False)
    assert float(np.abs(o[0] - ex["f32_out"]).max()) <= 1e-5


def test_export_round_trip(tmp_path):
    """checkpoint key names (load_nkf_weights, Export_NKF_AEC.py:414-455) -> blob -> the oracle reproduces the reference's output bits.
    The expected blob is assembled here from the checkpoint keys independently of nkf_aec.state_to_blob_tensors."""
    from audio_denoiser_onnx_amd import export
    from audio_denoiser_onnx_amd.metadata import metadata_path_for_model
    from audio_denoiser_onnx_amd.weights import load_blob
    sd = dict(np.load(os.path.join(GOLD, "nkf_aec_seed0_state.npz")))
    path = export.export_nkf_aec(os.path.join(GOLD, "nkf_aec_seed0_state.npz"), tmp_path)
    got = load_blob(path)

    def pair(prefix, p):
        return np.stack([sd[f"{prefix}.linear_real.{p}"], sd[f"{prefix}.linear_imag.{p}"]])
    want = {"fc_in_w": pair("kg_net.fc_in.0", "weight"), "fc_in_b": pair("kg_net.fc_in.0", "bias"), "fc_in_slope": sd["kg_net.fc_in.1.prelu.weight"].reshape(1),
            "fc_out1_w": pair("kg_net.fc_out.0", "weight"), "fc_out1_b": pair("kg_net.fc_out.0", "bias"), "fc_out_slope": sd["kg_net.fc_out.1.prelu.weight"].reshape(1),
            "fc_out2_w": pair("kg_net.fc_out.2", "weight"), "fc_out2_b": pair("kg_net.fc_out.2", "bias")}
    for ours, theirs in (("gru_w_ih", "weight_ih_l0"), ("gru_w_hh", "weight_hh_l0"), ("gru_b_ih", "bias_ih_l0"), ("gru_b_hh", "bias_hh_l0")):
        want[ours] = np.stack([sd[f"kg_net.complex_gru.gru_r.{theirs}"], sd[f"kg_net.complex_gru.gru_i.{theirs}"]])
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], want[k].astype(np.float32)), k
    far, near, out = _rows()
    pcm, _, _ = NkfAecOracle(got).forward(far[:1], near[:1])
    assert int(np.abs(pcm[0].astype(np.int32) - out[0]).max()) <= 1
    mpath = metadata_path_for_model(path)
    assert mpath.exists()
    meta = json.loads(mpath.read_text())
    assert meta["model_family"] == "nkf_aec" and meta["task"] == "aec" and meta["num_audio_inputs"] == "2"


def test_metadata_keys():
    from audio_denoiser_onnx_amd import nkf_aec
    m = nkf_aec.metadata(32000)
    assert m["task"] == "aec" and m["model_family"] == "nkf_aec" and m["num_audio_inputs"] == "2" and m["nfft"] == "1024"


def _create(meta_over):
    from audio_denoiser_onnx_amd import _lib, nkf_aec
    from audio_denoiser_onnx_amd.metadata import MetadataReader
    lib = _lib.get_library()
    m = nkf_aec.metadata(32000)
    m.update(meta_over)
    with open(os.path.join(GOLD, "nkf_aec_seed0.adew"), "rb") as f:
        blob = f.read()
    h = C.c_void_p()
    st = lib.c.ade_create(MetadataReader(m).to_json().encode(), blob, len(blob), 0, C.byref(h))
    if h.value:
        lib.c.ade_destroy(h)
    return st


def test_manifest_refusals_without_device():
    """dynamic axes, another input rate and batch folding are refused before any device is touched (ADE_ERR_UNSUPPORTED = 6, include/ade.h)"""
    assert _create({"in_sample_rate": "48000"}) == 6
    assert _create({"dynamic_axes": "1"}) == 6
    assert _create({"use_batch_fold": "1"}) == 6
