"""NKF-AEC on the GPU (csrc/ade_nkf_aec.hip) against the reference's own outputs (tests/golden/nkf_aec_seed0*, tools/make_golden_nkf_aec.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

GOLD = os.path.join(HERE, "golden")
N_ROWS = 5


def _blob():
    with open(os.path.join(GOLD, "nkf_aec_seed0.adew"), "rb") as f:
        return f.read()


def _session(length=32000, **kw):
    from audio_denoiser_onnx_amd import nkf_aec
    from audio_denoiser_onnx_amd.session import InferenceSession
    return InferenceSession(weights=_blob(), metadata=nkf_aec.metadata(length, **kw), device_id=0)


def _rows():
    io = np.load(os.path.join(GOLD, "nkf_aec_seed0_io.npz"))
    far = np.stack([io[f"far{i}"] for i in range(N_ROWS)])
    near = np.stack([io[f"near{i}"] for i in range(N_ROWS)])
    out = np.stack([io[f"out{i}"] for i in range(N_ROWS)])
    return far, near, out


@pytest.mark.gpu
def test_fixture_rows_through_session():
    far, near, out = _rows()
    wv = np.load(os.path.join(GOLD, "nkf_aec_seed0_wave.npz"))
    sess = _session()
    pcm, f32 = sess.run(None, {"far_end_audio": far[:, None], "near_end_audio": near[:, None]}, return_f32=True)
    assert pcm.shape == (N_ROWS, 1, 32000) and pcm.dtype == np.int16
    lsb = int(np.abs(pcm[:, 0].astype(np.int32) - out).max())
    wave = max(float(np.abs(f32[i, 0] - wv[f"wave{i}"]).max()) for i in range(N_ROWS))
    assert lsb <= 1 and wave <= 1e-4, (lsb, wave)
    # taps: the echo estimate of row 0 (mic spectrum - error spectrum)
    T, F = sess.frames, 513
    echo = sess.tap("echo_hat", N_ROWS * T * F * 2).reshape(N_ROWS, T, F, 2)
    ref = np.load(os.path.join(GOLD, "nkf_aec_seed0_taps.npz"))["echo_hat0"]        # (re/im, F, T)
    got = np.stack([echo[0, :, :, 0].T, echo[0, :, :, 1].T])
    assert float(np.abs(got - ref).max()) <= 1e-5 * float(np.abs(ref).max()), float(np.abs(got - ref).max() / np.abs(ref).max())
    # far end zero: the echo estimate is exactly zero
    assert not np.any(echo[3])
    kg = sess.tap("kg", N_ROWS * F * 4 * 2)
    assert np.all(np.isfinite(kg))


@pytest.mark.gpu
def test_float_io_and_out_rate_48k():
    ex = np.load(os.path.join(GOLD, "nkf_aec_seed0_extra.npz"))
    s32 = _session(16000, input_audio_dtype="F32", output_audio_dtype="F32")
    (o32,) = s32.run(None, {"far_end_audio": ex["f32_far"][None, None], "near_end_audio": ex["f32_near"][None, None]})
    assert o32.dtype == np.float32 and float(np.abs(o32[0, 0] - ex["f32_out"]).max()) <= 1e-4
    s16 = _session(16000, input_audio_dtype="F16", output_audio_dtype="F16")
    (o16,) = s16.run(None, {"far_end_audio": ex["f32_far"][None, None].astype(np.float16), "near_end_audio": ex["f32_near"][None, None].astype(np.float16)})
    # F16 tensors against the F32 fixture: the inputs are rounded to half precision on the way in and the output on the way out (a half's step is 2^-11
    # relative, ~5e-4 at the fixture's peak), so the gate is that rounding, not the engine's fp32 arithmetic, which the F32 case above pins
    assert o16.dtype == np.float16 and float(np.abs(o16[0, 0].astype(np.float32) - ex["f32_out"]).max()) <= 2e-3
    s48 = _session(16000, out_sample_rate=48000)
    (o48,) = s48.run(None, {"far_end_audio": ex["r48_far"][None, None], "near_end_audio": ex["r48_near"][None, None]})
    assert o48.shape == (1, 1, ex["r48_out"].size)          # 3 x the 256 (T - 1) = 15 872 samples the ISTFT keeps
    assert int(np.abs(o48[0, 0].astype(np.int32) - ex["r48_out"]).max()) <= 1


@pytest.mark.gpu
def test_batch_row_independent_and_submit():
    far, near, _ = _rows()
    sess = _session()
    rng = np.random.default_rng(3)
    B = 64
    bf = np.clip(np.round(rng.standard_normal((B, 32000)) * 2000), -32768, 32767).astype(np.int16)
    bn = np.clip(np.round(rng.standard_normal((B, 32000)) * 2000), -32768, 32767).astype(np.int16)
    bf[17], bn[17] = far[0], near[0]
    pcm = np.stack([bf, bn], axis=1).reshape(B, -1)
    out_b, f_b = sess.process(pcm, want_f32=True)
    out_1, f_1 = sess.process(pcm[17:18], want_f32=True)
    assert np.array_equal(out_b[17], out_1[0]) and np.array_equal(f_b[17], f_1[0])
    out = np.empty_like(out_b)
    t = sess.submit(pcm, out)
    sess.wait(t)
    assert np.array_equal(out, out_b)


def _drive(tmp_path, sess, far, near):
    from audio_denoiser_onnx_amd import inference_nkf_aec as drv
    from audio_denoiser_onnx_amd.wavio import read_pcm16, write_pcm16
    pf, pn, po = tmp_path / "far.wav", tmp_path / "near.wav", tmp_path / "aec.wav"
    write_pcm16(pf, far[None], 16000)
    write_pcm16(pn, near[None], 16000)
    drv.main(sess, str(pf), str(pn), str(po), rng=np.random.default_rng(5))
    y, sr = read_pcm16(po)
    return y[0], sr


@pytest.mark.gpu
@pytest.mark.parametrize("length, out_rate", [(32000, 16000), (16000, 16000), (16000, 48000)])
def test_driver(tmp_path, length, out_rate):
    """Trim to the shorter file, the reference's slice stride (the output length when the graph keeps 256 (T - 1) < L samples at equal rates),
    the output rate on the file, and every slice that lies inside the signal equal to the same slice through the session."""
    rng = np.random.default_rng(11)
    far = np.clip(np.round(rng.standard_normal(50000) * 3000), -32768, 32767).astype(np.int16)
    near = np.clip(np.round(rng.standard_normal(47000) * 3000), -32768, 32767).astype(np.int16)
    sess = _session(length, out_sample_rate=out_rate)
    y, sr = _drive(tmp_path, sess, far, near)
    assert sr == out_rate and y.shape == (47000 * out_rate // 16000,)
    stride = sess.out_len if (sess.out_len != sess.in_len and out_rate == 16000) else sess.in_len
    if length == 16000 and out_rate == 16000:
        assert stride == 15872
    k = 0
    while k * stride + sess.in_len <= 47000:
        s0 = k * stride
        (o,) = sess.run(None, {"far_end_audio": far[None, None, s0:s0 + sess.in_len], "near_end_audio": near[None, None, s0:s0 + sess.in_len]})
        assert np.array_equal(y[k * sess.out_len:(k + 1) * sess.out_len], o.reshape(-1)), k
        k += 1
    assert k >= 1


@pytest.mark.gpu
def test_session_surface_and_missing_tensor():
    from audio_denoiser_onnx_amd import nkf_aec
    from audio_denoiser_onnx_amd.session import InferenceSession
    from audio_denoiser_onnx_amd.weights import load_blob, pack_blob
    sess = _session()
    assert [(a.name, a.shape) for a in sess.get_inputs()] == [("far_end_audio", [1, 1, 32000]), ("near_end_audio", [1, 1, 32000])]
    assert [(a.name, a.shape) for a in sess.get_outputs()] == [("aec_audio", [1, 1, 32000])]
    t = load_blob(os.path.join(GOLD, "nkf_aec_seed0.adew"))
    del t["gru_w_hh"]
    from audio_denoiser_onnx_amd import _lib
    lib = _lib.get_library()
    import ctypes as C
    from audio_denoiser_onnx_amd.metadata import MetadataReader
    blob = pack_blob(t)
    h = C.c_void_p()
    st = lib.c.ade_create(MetadataReader(nkf_aec.metadata(32000)).to_json().encode(), blob, len(blob), 0, C.byref(h))
    if h.value:
        lib.c.ade_destroy(h)
    assert st == _lib.ADE_ERR_MISSING_KEY
    with pytest.raises(Exception) as ei:
        InferenceSession(weights=blob, metadata=nkf_aec.metadata(32000), device_id=0)
    assert "gru_w_hh" in str(ei.value)
