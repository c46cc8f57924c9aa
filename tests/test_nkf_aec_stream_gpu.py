"""Stateful streaming over the NKF-AEC path on the GPU (csrc/ade_nkf_aec.hip, ade_stream_*) against the reference-run fixture
tests/golden/nkf_aec_seed0_stream.npz (tools/make_golden_nkf_aec.py --stream): NKF.forward on two zero-sum clips of 49 152 samples in ONE call.

Tolerances are the family's contract against reference-run fixtures: f32 waveform <= 1e-4, PCM <= 1 LSB, over every sample.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from nkf_aec_stream_lib import DELAY, HOP, fixture, run_stream, seed0_blob  # noqa: E402

N = 49152


def _session(length=16384, **kw):
    from audio_denoiser_onnx_amd import nkf_aec
    from audio_denoiser_onnx_amd.session import InferenceSession
    return InferenceSession(weights=seed0_blob(), metadata=nkf_aec.metadata(length, **kw), device_id=0)


def _clips():
    fx = fixture()
    return (np.stack([fx["far0"], fx["far1"]]), np.stack([fx["near0"], fx["near1"]]), np.stack([fx["out0"], fx["out1"]]),
            np.stack([fx["wave0"], fx["wave1"]]))


def _stream(sess, far, near, hops):
    from audio_denoiser_onnx_amd.session import StreamingSession
    with StreamingSession(sess, far.shape[0], hops) as st:
        return run_stream(st, far, near)


@pytest.mark.gpu
def test_gpu_stream_equals_reference_one_shot_and_push_size_does_not_matter():
    """Both clips as two streams of one handle, pushes of 8 hops + flush, against the reference on the whole signal; then 1, 3, 64 and 192 hops: the same bits."""
    far, near, out, wave = _clips()
    sess = _session()
    pcm, f32 = _stream(sess, far, near, 8)
    assert pcm.shape == f32.shape == (2, N + DELAY) and pcm.dtype == np.int16
    assert not pcm[:, :DELAY].any() and not f32[:, :DELAY].any()
    d_wave = float(np.abs(f32[:, DELAY:] - wave).max())
    d_pcm = int(np.abs(pcm[:, DELAY:].astype(np.int32) - out.astype(np.int32)).max())
    print(f"8-hop pushes vs the reference's one call: wave {d_wave:.3e}, pcm {d_pcm} LSB")
    assert d_wave <= 1e-4 and d_pcm <= 1
    for hops in (1, 3, 64, 192):
        p, f = _stream(sess, far, near, hops)
        assert np.array_equal(p, pcm) and np.array_equal(f, f32), f"{hops}-hop pushes differ from 8-hop pushes"


@pytest.mark.gpu
def test_gpu_streams_are_independent_and_the_grid_scales():
    """1 500 streams built from the two clips repeated, 4 pushes of 2 hops: every row equals the 2-stream run bit for bit."""
    from audio_denoiser_onnx_amd.session import StreamingSession
    far, near, _, _ = _clips()
    P, n_push = 2 * HOP, 4
    far, near = far[:, 20000:20000 + n_push * P], near[:, 20000:20000 + n_push * P]
    sess = _session()

    def pushes(f, n):
        with StreamingSession(sess, f.shape[0], 2) as st:
            parts = [st.push_aec(f[:, i * P:(i + 1) * P], n[:, i * P:(i + 1) * P], want_f32=True) for i in range(n_push)]
        return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)
    small = pushes(far, near)
    assert small[0][:, DELAY:].any()
    big = pushes(np.concatenate([far] * 750), np.concatenate([near] * 750))
    for rows in (slice(0, 2), slice(750, 752), slice(1498, 1500)):
        assert np.array_equal(big[0][rows], small[0]) and np.array_equal(big[1][rows], small[1])


@pytest.mark.gpu
def test_gpu_push_device_on_a_caller_stream_equals_the_host_push():
    import torch
    from audio_denoiser_onnx_amd.session import StreamingSession
    far, near, _, _ = _clips()
    hops, n_push = 8, 6
    P = hops * HOP
    rows = np.stack([far, near], axis=1)[:, :, 8192:8192 + n_push * P]               # (2, 2, n)
    sess = _session()
    with StreamingSession(sess, 2, hops) as st:
        host = [st.push(rows[:, :, i * P:(i + 1) * P], want_f32=True) for i in range(n_push)]
    side = torch.cuda.Stream()
    d_in = [torch.from_numpy(np.ascontiguousarray(rows[:, :, i * P:(i + 1) * P])).cuda() for i in range(n_push)]
    d_out = [torch.empty(2, P, dtype=torch.int16, device="cuda") for _ in range(n_push)]
    d_f32 = [torch.empty(2, P, dtype=torch.float32, device="cuda") for _ in range(n_push)]
    torch.cuda.synchronize()
    with StreamingSession(sess, 2, hops) as st:
        with torch.cuda.stream(side):
            for i in range(n_push):
                st.push_device(d_in[i], d_out[i], d_f32[i], stream=side.cuda_stream)      # enqueued back to back, no synchronise in between
        side.synchronize()
        with pytest.raises(ValueError):
            st.push_device(d_in[0][:, 0], d_out[0])                                         # an AEC push is (n_streams, 2, P)
    for i in range(n_push):
        assert np.array_equal(d_out[i].cpu().numpy(), host[i][0]) and np.array_equal(d_f32[i].cpu().numpy(), host[i][1])
    assert any(h[0].any() for h in host)


@pytest.mark.gpu
def test_gpu_stream_delay_per_family():
    from ade_testlib import make_session
    from audio_denoiser_onnx_amd.session import StreamingSession
    with StreamingSession(_session(), 1, 4) as st:
        assert st.delay == 768 and st.in_channels == 2
    with StreamingSession(make_session(None, seed=0), 1, 4) as st:
        assert st.delay == 256 and st.in_channels == 1


@pytest.mark.gpu
def test_gpu_stream_refusals():
    from audio_denoiser_onnx_amd import _lib
    from audio_denoiser_onnx_amd.session import StreamingSession
    with pytest.raises(_lib.AdeUnsupportedError, match="int16"):
        StreamingSession(_session(16000, input_audio_dtype="F32", output_audio_dtype="F32"), 1, 4)      # float audio tensors
    with pytest.raises(_lib.AdeUnsupportedError, match="16000"):
        StreamingSession(_session(16000, out_sample_rate=48000), 1, 4)                                  # another output rate
    sess = _session()
    with pytest.raises(ValueError):
        StreamingSession(sess, 1, 0)                                                                    # frames_per_push < 1
    with pytest.raises(ValueError):
        StreamingSession(sess, 0, 4)
    with StreamingSession(sess, 2, 4) as st:
        with pytest.raises(ValueError):
            st.push(np.zeros((2, 4 * HOP), np.int16))                                                   # one channel short
        with pytest.raises(ValueError):
            st.push(np.zeros((2, 2, 100), np.int16))
        with pytest.raises(ValueError):
            st.push_aec(np.zeros((2, 4 * HOP), np.int16), np.zeros((1, 4 * HOP), np.int16))
        with pytest.raises(ValueError):
            st.flush()                                                                                  # nothing pushed yet
        first = st.push(np.zeros((2, 2, 4 * HOP), np.int16))
        assert not first.any()
    with StreamingSession(sess, 1, 1) as st:                   # a one-hop first push is legal: no Kalman frame yet, zeros out
        assert not st.push(np.full((1, 2, HOP), 1000, np.int16)).any()


@pytest.mark.gpu
def test_gpu_file_driver_streaming_keeps_the_echo_path_the_sliced_mode_does_not():
    """``inference_nkf_aec --stream``: the fixture clip with 62-hop pushes asked for (192 hops: not a whole number of such pushes, the driver pushes 48 hops at a
    time so that the stream ends where the clip ends) equals the reference's one call on the whole clip; the sliced ``process`` of the same clip through a
    16 384-sample handle restarts the filter twice and is a different signal."""
    from audio_denoiser_onnx_amd import inference_nkf_aec as drv
    fx = fixture()
    sess = _session(16384)
    for i in range(2):
        far, near, ref = fx[f"far{i}"], fx[f"near{i}"], fx[f"out{i}"].astype(np.int32)
        out = drv.process_streaming(sess, far, near, frames_per_push=62)
        assert out.shape == (N,) and out.dtype == np.int16
        d = int(np.abs(out.astype(np.int32) - ref).max())
        sliced = drv.process(sess, far, near, rng=np.random.default_rng(0))
        assert sliced.shape == (N,)
        rms = float(np.sqrt(np.mean((sliced.astype(np.float64) - ref) ** 2)))
        print(f"clip {i}: streamed driver vs reference {d} LSB; sliced driver vs reference {rms:.1f} LSB RMS")
        assert d <= 1
        assert rms > 100.0
