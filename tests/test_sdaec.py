"""SDAEC host side (CPU): the float64 oracle against the reference's fixtures, the checkpoint -> blob mapping and its folds, the manifest.

Fixtures: tools/make_golden_sdaec.py (the reference's own forward on seeded weights).  The 2 MB blob is not committed: the fixture records its SHA-256 and
the tests rebuild it from the sharded checkpoint-named state.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from sdaec_oracle import TAP_REF_DISTANCE, SdaecOracle, fixture_state, tap_gate  # noqa: E402

GOLD = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def blob_tensors():
    from audio_denoiser_onnx_amd import sdaec
    return sdaec.state_to_blob_tensors(*fixture_state(GOLD))


@pytest.fixture(scope="module")
def oracle(blob_tensors):
    return SdaecOracle(blob_tensors)


@pytest.fixture(scope="module")
def fixture_info():
    with open(os.path.join(GOLD, "sdaec_seed0_manifest.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def rows_result(oracle):
    io = np.load(os.path.join(GOLD, "sdaec_seed0_io.npz"))
    near, far = np.stack([io[f"near{i}"] for i in range(6)]), np.stack([io[f"far{i}"] for i in range(6)])
    return io, oracle.forward(near, far, want_taps=True)


def check(pcm, wave, ref_pcm, ref_wave):
    d_wave, d_pcm = float(np.abs(wave - ref_wave).max()), int(np.abs(pcm.astype(np.int32) - ref_pcm.astype(np.int32)).max())
    print(f"wave {d_wave:.2e} pcm {d_pcm}")
    assert d_wave <= 1e-4 and d_pcm <= 1


def test_oracle_matches_reference_rows(rows_result):
    io, (pcm, wave, _) = rows_result
    wv = np.load(os.path.join(GOLD, "sdaec_seed0_wave.npz"))
    for i in range(6):
        check(pcm[i], wave[i], io[f"out{i}"], wv[f"wave{i}"])
        if i != 5:        # the 1 LSB gate must not hide behind the clamp
            assert not np.any((io[f"out{i}"] == 32767) | (io[f"out{i}"] == -32768))
    assert np.all(np.isfinite(wave[4]))


def test_oracle_taps_within_measured_distance(rows_result):
    """The distances TAP_REF_DISTANCE records (reference fp32 tap vs the float64 oracle) still hold, and each is below its tap's gate."""
    _, (_, _, taps) = rows_result
    tp = np.load(os.path.join(GOLD, "sdaec_seed0_taps.npz"))
    fr = tp["frames"]
    d = {"alpha": float(np.abs(taps["alpha"][0] - tp["alpha"]).max())}
    for k in ("e0", "e5", "lstm_out", "d1", "spec_out"):
        d[k] = float(np.abs(taps[k][0][fr] - tp[k]).max())
    print(d)
    for k, v in d.items():
        assert v <= TAP_REF_DISTANCE[k], k
        absmax = np.abs(tp["alpha"]).max() if k == "alpha" else tp[k + "_absmax"][0]
        assert v <= tap_gate(k, absmax), k


@pytest.mark.parametrize("length", [1600, 2720, 3000])
def test_oracle_short_lengths(oracle, length):
    ex = np.load(os.path.join(GOLD, "sdaec_seed0_extra.npz"))
    pcm, wave, _ = oracle.forward(ex[f"near_{length}"][None], ex[f"far_{length}"][None])
    assert pcm.shape == (1, length)
    check(pcm[0], wave[0], ex[f"out_{length}"], ex[f"wave_{length}"])


def test_oracle_float_io_and_48k(oracle):
    ex = np.load(os.path.join(GOLD, "sdaec_seed0_extra.npz"))
    out, wave, _ = oracle.forward(ex["f32_near"][None], ex["f32_far"][None], int_in=False, int_out=False)
    assert float(np.abs(wave[0] - ex["f32_out"]).max()) <= 1e-4
    # out_sample_rate = 48000 (:429-437): * 32767 on the model-rate waveform, then linear interpolation (align_corners=False) by 3, clamp, truncate
    _, wave, _ = oracle.forward(ex["r48_near"][None], ex["r48_far"][None])
    # the interpolation itself in fp32, as torch forms it: source index fl(fl(1 / 3) * (i + 0.5) - 0.5), out = y0 * (1 - lambda) + y1 * lambda
    f32 = np.float32
    y = (wave[0] * 32767.0).astype(f32)
    src = np.maximum(f32(1.0 / 3.0) * (np.arange(3 * y.size, dtype=f32) + f32(0.5)) - f32(0.5), f32(0.0)).astype(f32)
    i0 = np.minimum(src.astype(np.int64), y.size - 1)
    i1 = np.minimum(i0 + 1, y.size - 1)
    lam = (src - i0.astype(f32)).astype(f32)
    up = ((f32(1.0) - lam) * y[i0] + lam * y[i1]).astype(f32)
    pcm = np.trunc(np.clip(up, -32768, 32767)).astype(np.int32)
    assert ex["r48_out"].shape == (48000,)
    assert int(np.abs(pcm - ex["r48_out"].astype(np.int32)).max()) <= 1


def test_oracle_fold(oracle):
    fx = np.load(os.path.join(GOLD, "sdaec_seed0_fold.npz"))
    pcm, wave, _ = oracle.forward(fx["near"][None], fx["far"][None], fold_window=24000)
    check(pcm[0], wave[0], fx["out"], fx["wave"])
    one, _, _ = oracle.forward(fx["near"][None, 24000:], fx["far"][None, 24000:])          # a window is an independent clip
    assert np.array_equal(one[0], pcm[0, 24000:])


def test_blob_round_trip(blob_tensors, fixture_info):
    from audio_denoiser_onnx_amd import weights
    blob = weights.pack_blob(blob_tensors)
    assert len(blob) == fixture_info["blob_nbytes"]
    assert hashlib.sha256(blob).hexdigest() == fixture_info["blob_sha256"]
    back = weights.unpack_blob(blob)
    assert list(back) == list(blob_tensors) and all(np.array_equal(back[k], blob_tensors[k]) for k in back)


def test_folds_bit_equal_to_reference(blob_tensors):
    fo = np.load(os.path.join(GOLD, "sdaec_seed0_folds.npz"))
    for ref, mine in (("in_fused_weight", "in_fused_w"), ("in_fused_bias", "in_fused_b"), ("out_fused_weight", "out_fused_w"), ("out_fused_bias", "out_fused_b"),
                      ("alpha_conv_kernel", "alpha_kernel")):
        assert np.array_equal(fo[ref].reshape(blob_tensors[mine].shape), blob_tensors[mine]), ref
    # the bias sums ten fp32 terms, in an order torch does not document: one ulp
    assert abs(float(fo["alpha_conv_bias"][0]) - float(blob_tensors["alpha_bias"][0])) <= float(np.spacing(np.float32(abs(fo["alpha_conv_bias"][0]))))
    for ref, mine in (("cfb_e1.LN0", "e1.ln0"), ("cfb_d1.LN0", "d1.ln0"), ("cfb_e3.ceps_unit.LN", "e3.ceps_ln"), ("ln", "ln")):
        assert np.array_equal(fo[ref + ".export_w"], blob_tensors[mine + "_w"]), ref
        assert np.array_equal(fo[ref + ".export_b"], blob_tensors[mine + "_b"]), ref
        assert np.float32(fo[ref + ".export_eps"][0]) == blob_tensors[mine + "_eps"][0], ref


def test_all_layernorm_folds_checksum(fixture_info):
    """Every LayerNorm of the reference (export_w, export_b, export_eps), by checksum."""
    from audio_denoiser_onnx_amd import sdaec
    net, _ = fixture_state(GOLD)
    order = []                                   # NET's module order: a CFB registers its cepstral unit before LN0 .. LN2; `ln` sits between the encoder and the decoder
    for n in sdaec.CFB_NAMES:
        if n == "d5":
            order.append("ln")
        order += [f"cfb_{n}.ceps_unit.LN", f"cfb_{n}.LN0", f"cfb_{n}.LN1", f"cfb_{n}.LN2"]
    assert len(order) == 41 and all(name + ".w" in net for name in order)
    sha = hashlib.sha256()
    for name in order:
        w, b, eps = sdaec.fold_layernorm(net[name + ".w"], net[name + ".b"])
        sha.update(name.encode() + w.tobytes() + b.tobytes() + np.float32(eps[0]).tobytes())
    assert sha.hexdigest() == fixture_info["layernorm_folds_sha256"]


def test_cepstral_tables_match_reference(blob_tensors):
    tp = np.load(os.path.join(GOLD, "sdaec_seed0_taps.npz"))
    assert blob_tensors["ceps_dft"].shape == (162, 160) and blob_tensors["ceps_idft"].shape == (160, 162)
    assert float(np.abs(tp["ceps_dft"] - blob_tensors["ceps_dft"]).max()) <= 1.2e-7          # one ulp at 1: fp32 cos / sin of the same fp32 angles
    assert float(np.abs(tp["ceps_idft"] - blob_tensors["ceps_idft"]).max()) <= 1e-7          # the reference's fp32 pinv against the float64 one, entries <= 1 / 80


def test_manifest_equals_reference(fixture_info):
    from audio_denoiser_onnx_amd import sdaec
    ref = fixture_info["manifest"]
    mine = sdaec.metadata(32000)
    assert ref["model_family"] == "sdaec" and ref["task"] == "aec" and ref["feature_kind"] == "stft_alpha_predictor"
    assert ref["num_audio_inputs"] == "2" and ref["alpha_k"] == "10"
    skip = {"producer", "opset", "audio_metadata_version"}
    for k, v in ref.items():
        if k not in skip:
            assert mine.get(k) == v, (k, mine.get(k), v)
    assert set(mine) - skip == set(ref) - skip


def test_named_shape_errors():
    from audio_denoiser_onnx_amd import sdaec
    net, alpha = fixture_state(GOLD)
    bad = dict(net)
    bad["cfb_e1.conv.weight"] = bad["cfb_e1.conv.weight"][:, :, :2]
    with pytest.raises(ValueError, match="cfb_e1.conv.weight"):
        sdaec.state_to_blob_tensors(bad, alpha)
    del bad["cfb_e1.conv.weight"]
    with pytest.raises(KeyError, match="cfb_e1.conv.weight"):
        sdaec.state_to_blob_tensors(bad, alpha)
    with pytest.raises(KeyError, match="linear2.weight"):
        sdaec.state_to_blob_tensors(net, {k: v for k, v in alpha.items() if k != "linear2.weight"})


def test_weightgen_state_maps():
    from audio_denoiser_onnx_amd import sdaec, weightgen
    a, b = weightgen.sdaec_state(3)
    net, _ = fixture_state(GOLD)
    assert set(a) == set(net) and all(a[k].shape == net[k].shape for k in a)
    t = sdaec.state_to_blob_tensors(a, b)
    assert t["in_fused_w"].shape == (20, 44) and t["out_fused_w"].shape == (2, 40)
