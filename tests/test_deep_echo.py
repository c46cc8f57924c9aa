"""Deep Echo AEC host side (CPU): the float64 oracle against the reference's fixtures, the checkpoint -> blob mapping and its folds, the manifest.

Fixtures: tools/make_golden_deep_echo.py (the reference's own forward on seeded weights).  The blob is not committed: the fixture records its SHA-256 and the tests
rebuild it from the checkpoint-named state.
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

from deep_echo_oracle import ORDER, TAP_REF_DISTANCE, WAVE_GATE, WAVE_REF_DISTANCE, DeepEchoOracle, fixture_state, tap_gate  # noqa: E402

GOLD = os.path.join(HERE, "golden")
N_ROWS = 4
TAPS = ("e0", "e1", "lstm_out", "d1", "path", "spec_out")


@pytest.fixture(scope="module")
def blob_tensors():
    from audio_denoiser_onnx_amd import deep_echo
    return deep_echo.state_to_blob_tensors(fixture_state(GOLD))


@pytest.fixture(scope="module")
def oracle(blob_tensors):
    return DeepEchoOracle(blob_tensors)


@pytest.fixture(scope="module")
def fixture_info():
    with open(os.path.join(GOLD, "deep_echo_seed0_manifest.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def rows_result(oracle):
    io = np.load(os.path.join(GOLD, "deep_echo_seed0_io.npz"))
    near, far = np.stack([io[f"near{i}"] for i in range(N_ROWS)]), np.stack([io[f"far{i}"] for i in range(N_ROWS)])
    return io, oracle.forward(near, far, want_taps=True)


def check(pcm, wave, ref_pcm, ref_wave):
    d_wave, d_pcm = float(np.abs(wave - ref_wave).max()), int(np.abs(pcm.astype(np.int32) - ref_pcm.astype(np.int32)).max())
    print(f"wave {d_wave:.2e} pcm {d_pcm}")
    assert d_wave <= WAVE_REF_DISTANCE          # the recorded distance holds ...
    assert d_wave <= WAVE_GATE and d_pcm <= 1   # ... and lies inside the family gate


def test_family_gate_is_the_projects():
    """The project's gate (waveform <= 1e-4, PCM <= 1 LSB) applies while the reference's own fp32 output lies within 2.5e-5 of the oracle."""
    assert WAVE_REF_DISTANCE <= 2.5e-5 and WAVE_GATE == 1e-4


def test_no_fixture_row_clamps():
    """|out| < 32767 on every row of the fixture: a clamp cannot hide a difference behind the 1 LSB gate."""
    io = np.load(os.path.join(GOLD, "deep_echo_seed0_io.npz"))
    ex = np.load(os.path.join(GOLD, "deep_echo_seed0_extra.npz"))
    fx = np.load(os.path.join(GOLD, "deep_echo_seed0_fold.npz"))
    outs = [io[f"out{i}"] for i in range(N_ROWS)] + [ex[f"out_{n}"] for n in (1600, 2720, 3000)] + [ex["r48_out"], fx["out"]]
    for o in outs:
        assert o.dtype == np.int16 and int(np.abs(o.astype(np.int32)).max()) < 32767
    assert float(np.abs(ex["f32_out"]).max()) < 1.0
    assert any(int(np.abs(io[f"out{i}"].astype(np.int32)).max()) > 4000 for i in range(N_ROWS))       # and the rows are not faint either


def test_oracle_matches_reference_rows(rows_result):
    io, (pcm, wave, _) = rows_result
    wv = np.load(os.path.join(GOLD, "deep_echo_seed0_wave.npz"))
    for i in range(N_ROWS):
        check(pcm[i], wave[i], io[f"out{i}"], wv[f"wave{i}"])
    assert np.all(np.isfinite(wave[3])) and not np.any(io["near3"]) and not np.any(io["far3"])      # both inputs zero


def test_oracle_taps_within_measured_distance(rows_result):
    """The distances TAP_REF_DISTANCE records (reference fp32 tap vs the float64 oracle) still hold, and each is below its tap's gate."""
    _, (_, _, taps) = rows_result
    tp = np.load(os.path.join(GOLD, "deep_echo_seed0_taps.npz"))
    fr = tp["frames"]
    assert list(fr) == [0, 1, 8, 9, 10, 15, 16, 49]
    d = {k: float(np.abs(taps[k][0][fr] - tp[k]).max()) for k in TAPS}
    print(d)
    for k, v in d.items():
        assert v <= TAP_REF_DISTANCE[k], k
        assert v <= tap_gate(k, tp[k + "_absmax"][0]), k


@pytest.mark.parametrize("length", [1600, 2720, 3000])
def test_oracle_short_lengths(oracle, length):
    ex = np.load(os.path.join(GOLD, "deep_echo_seed0_extra.npz"))
    pcm, wave, _ = oracle.forward(ex[f"near_{length}"][None], ex[f"far_{length}"][None])
    assert pcm.shape == (1, length)
    check(pcm[0], wave[0], ex[f"out_{length}"], ex[f"wave_{length}"])


def test_oracle_float_io_and_48k(oracle):
    ex = np.load(os.path.join(GOLD, "deep_echo_seed0_extra.npz"))
    out, wave, _ = oracle.forward(ex["f32_near"][None], ex["f32_far"][None], int_in=False, int_out=False)
    d = float(np.abs(wave[0] - ex["f32_out"]).max())
    assert d <= WAVE_REF_DISTANCE and d <= WAVE_GATE
    # out_sample_rate = 48000 (:411-419): * 32767 on the model-rate waveform, then linear interpolation (align_corners=False) by 3, clamp, truncate
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
    fx = np.load(os.path.join(GOLD, "deep_echo_seed0_fold.npz"))
    pcm, wave, _ = oracle.forward(fx["near"][None], fx["far"][None], fold_window=24000)
    check(pcm[0], wave[0], fx["out"], fx["wave"])
    one, _, _ = oracle.forward(fx["near"][None, 24000:], fx["far"][None, 24000:])          # a window is an independent clip: own mean, zero states, zero tap history
    assert np.array_equal(one[0], pcm[0, 24000:])


def test_blob_round_trip(blob_tensors, fixture_info):
    from audio_denoiser_onnx_amd import weights
    blob = weights.pack_blob(blob_tensors)
    assert len(blob) == fixture_info["blob_nbytes"]
    assert hashlib.sha256(blob).hexdigest() == fixture_info["blob_sha256"]
    back = weights.unpack_blob(blob)
    assert list(back) == list(blob_tensors) and all(np.array_equal(back[k], blob_tensors[k]) for k in back)
    assert fixture_info["out_conv_scale"] == 1.0        # the seeded state is PyTorch's initialisation as it stands


@pytest.mark.parametrize("prefix,c,f,sum_scale", [("cfb_e1.LN0", 20, 160, 1.0), ("cfb_d1.LN2", 20, 160, 1.0), ("ln", 20, 160, 1.0), ("cfb_e1.ceps_unit.LN", 40, 81, 0.25),
                                                  ("cfb_d1.ceps_unit.LN", 40, 81, 0.25)])
def test_layernorm_fold_against_unfolded_float64(prefix, c, f, sum_scale):
    """The folded (w, b, eps) triple in the kernels' form against the reference's form (:200-208 with the fused weight scale, :193-198) evaluated directly in
    float64.  The fold rounds w' and eps' to fp32 once: 2^-24 relative on the scaled term."""
    from audio_denoiser_onnx_amd import deep_echo
    state = fixture_state(GOLD)
    rng = np.random.default_rng(5)
    w = (state[prefix + ".w"].astype(np.float64) * (1.0 + 0.3 * rng.standard_normal((1, c, f, 1)))).astype(np.float32)       # the seeded w is all ones: perturb it
    b = state[prefix + ".b"]
    x = rng.standard_normal((c, f)) * 3.0 + 0.7
    n = c * f
    d = x - x.mean()
    xs, eps = d * sum_scale, 1e-8 * (n - 1) * sum_scale * sum_scale
    direct = xs / np.sqrt((xs * xs).sum() + eps) * (w[0, :, :, 0].astype(np.float64) * np.sqrt(n - 1.0)) + b[0, :, :, 0]
    fw, fb, feps = deep_echo.fold_layernorm(w, b)
    assert fw.shape == (f, c) and fb.shape == (f, c) and fw.dtype == np.float32 and feps.shape == (1,)
    folded = (d.T / np.sqrt((d * d).mean() + float(feps[0]))) * fw + fb
    scaled = np.abs(direct.T - fb)
    assert np.all(np.abs(folded - direct.T) <= 2.0 ** -23 * scaled + 1e-15)
    # near-silent planes, where eps decides: the same agreement
    xq = x * 1e-5
    dq = xq - xq.mean()
    direct_q = dq * sum_scale / np.sqrt((dq * dq).sum() * sum_scale ** 2 + eps) * (w[0, :, :, 0].astype(np.float64) * np.sqrt(n - 1.0)) + b[0, :, :, 0]
    folded_q = (dq.T / np.sqrt((dq * dq).mean() + float(feps[0]))) * fw + fb
    assert np.all(np.abs(folded_q - direct_q.T) <= 2.0 ** -22 * np.abs(direct_q.T - fb) + 1e-15)


@pytest.mark.parametrize("conv,lin,fused,n_h", [("in_conv", "in_ch_lstm.linear", "in_fused", 40), ("out_conv", "out_ch_lstm.linear", "echo", 20)])
def test_fused_linears_against_unfolded_float64(blob_tensors, conv, lin, fused, n_h):
    """conv(cat([linear(h), x])) evaluated layer by layer in float64 against the one fused Linear on cat([h, x]); the fused tensors are rounded to fp32 once."""
    state = fixture_state(GOLD)
    cw, cb = state[conv + ".weight"][:, :, 0, 0].astype(np.float64), state[conv + ".bias"].astype(np.float64)
    lw, lb = state[lin + ".weight"].astype(np.float64), state[lin + ".bias"].astype(np.float64)
    assert lw.shape[1] == n_h
    n_x = cw.shape[1] - lw.shape[0]
    rng = np.random.default_rng(9)
    h, x = rng.standard_normal((64, n_h)) * 2.0, rng.standard_normal((64, n_x)) * 2.0
    direct = np.concatenate([h @ lw.T + lb, x], axis=1) @ cw.T + cb
    fw, fb = blob_tensors[fused + "_w"].astype(np.float64), blob_tensors[fused + "_b"].astype(np.float64)
    assert fw.shape == (cw.shape[0], n_h + n_x)
    v = np.concatenate([h, x], axis=1)
    bound = 2.0 ** -24 * (np.abs(v) @ np.abs(fw).T + np.abs(fb)) * 1.01 + 1e-14
    assert np.all(np.abs(v @ fw.T + fb - direct) <= bound)


def test_echo_rows_are_re_then_im_taps(blob_tensors):
    """Row c of echo_w is out_conv's channel c: (re / im = c // 10, tap = c % 10), the reshape at :340."""
    state = fixture_state(GOLD)
    assert blob_tensors["echo_w"].shape == (2 * ORDER, 40) and blob_tensors["echo_b"].shape == (2 * ORDER,)
    assert np.array_equal(blob_tensors["echo_w"][:, 20:], state["out_conv.weight"][:, 40:, 0, 0])       # the d1 columns pass through the fold unchanged


def test_tap_order(rows_result):
    """A far end that is non-zero in one frame t0 only puts the estimated echo exactly in frames t0 .. t0 + 9, through tap 9 - d at delay d (:279, :304-306)."""
    _, (_, _, taps) = rows_result
    path = taps["path"][:1]                                        # (1, 50, 160, 20) of a real oracle run
    T, t0 = path.shape[1], 37                                      # t0 + 9 < T is not needed: the frames past the end do not exist
    rng = np.random.default_rng(2)
    fr, fi = np.zeros((1, T, 160)), np.zeros((1, T, 160))
    fr[0, t0], fi[0, t0] = rng.standard_normal(160), rng.standard_normal(160)
    er, ei = DeepEchoOracle.apply_echo_path(fr, fi, path)
    for t in range(T):
        d = t - t0
        if 0 <= d < ORDER:
            pr, pi = path[0, t, :, ORDER - 1 - d], path[0, t, :, 2 * ORDER - 1 - d]
            assert np.array_equal(er[0, t], fr[0, t0] * pr - fi[0, t0] * pi) and np.array_equal(ei[0, t], fr[0, t0] * pi + fi[0, t0] * pr), t
            assert np.any(er[0, t] != 0.0)
        else:
            assert not np.any(er[0, t]) and not np.any(ei[0, t]), t
    # and for t0 = 0: frame 0 sees tap 9 only, nothing comes from before the clip
    fr[:], fi[:] = 0.0, 0.0
    fr[0, 0] = 1.0
    er, _ = DeepEchoOracle.apply_echo_path(fr, fi, path)
    assert np.array_equal(er[0, 0], path[0, 0, :, ORDER - 1]) and np.array_equal(er[0, 9], path[0, 9, :, 0]) and not np.any(er[0, 10:])


def test_manifest_equals_reference(fixture_info):
    from audio_denoiser_onnx_amd import deep_echo
    ref = fixture_info["manifest"]
    mine = deep_echo.metadata(32000)
    assert ref["model_family"] == "deep_echo" and ref["task"] == "aec" and ref["feature_kind"] == "stft"
    assert ref["num_audio_inputs"] == "2" and ref["echo_order"] == "10" and deep_echo.frames_of(32000) == int(ref["max_signal_length"]) == 200
    skip = {"producer", "opset", "audio_metadata_version"}
    for k, v in ref.items():
        if k not in skip:
            assert mine.get(k) == v, (k, mine.get(k), v)
    assert set(mine) - skip == set(ref) - skip


def test_named_shape_errors():
    from audio_denoiser_onnx_amd import deep_echo
    net = fixture_state(GOLD)
    bad = dict(net)
    bad["out_conv.weight"] = bad["out_conv.weight"][:2]            # SDAEC's two-channel output layer is not this network's
    with pytest.raises(ValueError, match="out_conv.weight"):
        deep_echo.state_to_blob_tensors(bad)
    del bad["out_conv.weight"]
    with pytest.raises(KeyError, match="out_conv.weight"):
        deep_echo.state_to_blob_tensors(bad)


def test_checkpoint_unwrapping(blob_tensors):
    """Export_Deep_Echo.py:56-76: a nested, prefixed checkpoint maps to the same blob."""
    from audio_denoiser_onnx_amd import deep_echo, export
    net = fixture_state(GOLD)
    wrapped = {"epoch": 3, "state_dict": {"module." + k: v for k, v in net.items()}}
    t = deep_echo.state_to_blob_tensors(export.unwrap_deep_echo_checkpoint(wrapped))
    assert list(t) == list(blob_tensors) and all(np.array_equal(t[k], blob_tensors[k]) for k in t)
    with pytest.raises(TypeError):
        export.unwrap_deep_echo_checkpoint([1, 2])


def test_weightgen_state_maps():
    from audio_denoiser_onnx_amd import deep_echo, weightgen
    a = weightgen.deep_echo_state(3)
    net = fixture_state(GOLD)
    assert set(a) == set(net) and all(a[k].shape == net[k].shape for k in a)
    t = deep_echo.state_to_blob_tensors(a)
    assert t["in_fused_w"].shape == (20, 44) and t["echo_w"].shape == (20, 40)
