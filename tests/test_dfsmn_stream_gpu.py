"""Stateful streaming over the DFSMN path on the GPU (csrc/ade_dfsmn.hip, ade_stream_* on a model_family "dfsmn" handle).

The contract (include/ade.h): pushes of frames_per_push hops (960 samples each) plus the flush equal the reference's graph on the whole signal in ONE call, 960
samples later; the push size and the number of streams on the handle do not change a bit.  References: the reference-run fixtures
tests/golden/dfsmn_seed0_io.npz (four rows of 24 000 samples = 25 hops, 24 frames: the smallest that crosses the 19-frame memory history) and
dfsmn_seed0_stream.npz (one clip of 48 000 samples, tools/make_golden_dfsmn.py --stream), and the float64-table oracle oracle/dfsmn_oracle.py.  Gates are the
one-shot test's (tests/test_dfsmn.py): against the reference fixture <= 2 LSB in the interior and <= 24 LSB within 1920 samples of either end (the reference's
fp32-angle table error over w^2 ~ 0.0064); against the exact-table oracle f32 <= 2e-5 and PCM <= 1 LSB over every sample.
"""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from dfsmn_stream_lib import DELAY, HOP, blob_bytes, lsb, meta, run_stream, seed0_io, stream_fixture, tensors  # noqa: E402

pytestmark = pytest.mark.gpu

N = 24000            # 25 hops, 24 frames


def _session(length=N, **kw):
    from audio_denoiser_onnx_amd.session import InferenceSession
    return InferenceSession(weights=blob_bytes(), metadata=meta(length, **kw), device_id=0)


def _stream(sess, x, hops, flush=True):
    from audio_denoiser_onnx_amd.session import StreamingSession
    with StreamingSession(sess, x.shape[0], hops) as st:
        assert st.hop == HOP and st.delay == DELAY
        return run_stream(st, x, flush=flush)


@functools.lru_cache(maxsize=None)
def _five_hop_run():
    """The four fixture rows as four streams of one handle, 5-hop pushes + flush; computed once, callers do not modify it."""
    return _stream(_session(), seed0_io()[0], 5)


def _reference_gates(pcm, ref):
    d = lsb(pcm, ref)
    return int(d[..., 1920:-1920].max()), int(d.max())


def test_gpu_stream_equals_the_reference_fixture_the_oracle_and_the_one_shot_call():
    from dfsmn_oracle import DfsmnOracle
    x, out = seed0_io()
    pcm, f32 = _five_hop_run()
    assert pcm.shape == f32.shape == (4, N + DELAY) == (4, 24960) and pcm.dtype == np.int16
    assert not pcm[:, :DELAY].any() and not f32[:, :DELAY].any()
    assert not pcm[3].any() and not f32[3].any(), "an all-zero input must give an all-zero stream"
    assert np.abs(pcm[0]).max() > 1000
    inner, edge = _reference_gates(pcm[:, DELAY:], out)
    opcm, of32 = DfsmnOracle(tensors(), N, exact_dft=True).process(x)
    d_wave, d_pcm = float(np.abs(f32[:, DELAY:] - of32).max()), int(lsb(pcm[:, DELAY:], opcm).max())
    one, _ = _session().process(x)
    d_one = int(lsb(pcm[:, DELAY:], one).max())
    print(f"5-hop pushes + flush: vs the reference's one call {inner} LSB inside, {edge} LSB at the edges (gates 2, 24); vs the exact-table oracle wave {d_wave:.3e}, "
          f"pcm {d_pcm} LSB (gates 2e-5, 1); vs ade_process on the same handle family {d_one} LSB (gate 2)")
    assert inner <= 2 and edge <= 24
    assert d_wave <= 2e-5 and d_pcm <= 1
    assert d_one <= 2


@pytest.mark.parametrize("hops", [1, 25])
def test_gpu_push_size_does_not_change_a_bit(hops):
    """1-hop pushes: the first push completes no frame, every frame straddles two pushes and the 19-frame memory history crosses every push."""
    pcm, f32 = _five_hop_run()
    p, f = _stream(_session(), seed0_io()[0], hops)
    assert np.array_equal(p, pcm) and np.array_equal(f, f32), f"{hops}-hop pushes differ from 5-hop pushes"


def test_gpu_a_stream_does_not_depend_on_its_neighbours():
    pcm, f32 = _five_hop_run()
    p, f = _stream(_session(), seed0_io()[0][:1], 5)
    assert np.array_equal(p, pcm[:1]) and np.array_equal(f, f32[:1])


def test_gpu_reset_repeats_the_signal():
    from audio_denoiser_onnx_amd.session import StreamingSession
    x = seed0_io()[0]
    pcm, f32 = _five_hop_run()
    with StreamingSession(_session(), 4, 5) as st:
        run_stream(st, x[:, :15 * HOP], flush=False)                                  # abandoned mid-signal
        st.reset()
        p, f = run_stream(st, x)
        st.reset()
        again = st.push(x[:, :5 * HOP], want_f32=True)
    assert np.array_equal(p, pcm) and np.array_equal(f, f32)
    assert np.array_equal(again[0], pcm[:, :5 * HOP]) and np.array_equal(again[1], f32[:, :5 * HOP])


def test_gpu_push_device_on_a_caller_stream_equals_the_host_push():
    import torch
    from audio_denoiser_onnx_amd.session import StreamingSession
    x = seed0_io()[0]
    pcm, f32 = _five_hop_run()
    hops, n_push = 5, 5
    P = hops * HOP
    side = torch.cuda.Stream()
    d_in = [torch.from_numpy(np.ascontiguousarray(x[:, i * P:(i + 1) * P])).cuda() for i in range(n_push)]
    d_out = [torch.empty(4, P, dtype=torch.int16, device="cuda") for _ in range(n_push)]
    d_f32 = [torch.empty(4, P, dtype=torch.float32, device="cuda") for _ in range(n_push)]
    torch.cuda.synchronize()
    with StreamingSession(_session(), 4, hops) as st:
        with torch.cuda.stream(side):
            for i in range(n_push):
                st.push_device(d_in[i], d_out[i], d_f32[i], stream=side.cuda_stream)      # enqueued back to back, no synchronise in between
        side.synchronize()
    for i in range(n_push):
        assert np.array_equal(d_out[i].cpu().numpy(), pcm[:, i * P:(i + 1) * P]) and np.array_equal(d_f32[i].cpu().numpy(), f32[:, i * P:(i + 1) * P])


def test_gpu_long_reference_run():
    """48 000 samples (50 hops, 49 frames: 2.5 x the memory reach) in ten 5-hop pushes + flush against the reference's ONE call on the whole clip."""
    fx = stream_fixture()
    x, out, wave = fx["pcm_in"][None], fx["pcm_out"][None], fx["wave"][None]
    assert x.shape == (1, 48000) and x.dtype == out.dtype == np.int16 and wave.dtype == np.float32 and np.abs(out).max() > 1000
    pcm, f32 = _stream(_session(48000), x, 5)
    assert pcm.shape == (1, 48000 + DELAY) and not pcm[:, :DELAY].any()
    inner, edge = _reference_gates(pcm[:, DELAY:], out)
    d = np.abs(f32[:, DELAY:] - wave)
    print(f"5-hop pushes + flush vs the reference's one call on 48 000 samples: pcm {inner} LSB inside, {edge} LSB at the edges (gates 2, 24); wave "
          f"{float(d[:, 1920:-1920].max()):.3e} inside, {float(d.max()):.3e} at the edges (printed, not gated)")
    assert inner <= 2 and edge <= 24


def test_gpu_file_driver_streams_a_ragged_file(tmp_path):
    """``inference_dfsmn --stream 5`` on a 48 kHz file that is no whole number of hops: the pushes + flush of the zero-padded file, trimmed to the file's length."""
    import wave as wavmod
    from audio_denoiser_onnx_amd import inference_dfsmn
    from audio_denoiser_onnx_amd.inference_gtcrn import read_wav_int16
    from audio_denoiser_onnx_amd.metadata import write_metadata
    x = seed0_io()[0]
    audio = np.concatenate([x[0], x[1]])[:30001]                                      # 6.25 pushes of 4800 samples
    model = tmp_path / "DFSMN.adew"
    model.write_bytes(blob_bytes())
    write_metadata(model, meta(N))
    noisy, out_path = tmp_path / "in.wav", tmp_path / "out.wav"
    with wavmod.open(str(noisy), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(48000); w.writeframes(audio.astype("<i2").tobytes())
    assert inference_dfsmn.main([str(model), str(noisy), str(out_path), "--stream", "5"]) == 0
    got = read_wav_int16(out_path, 48000)
    padded = np.zeros((1, 7 * 5 * HOP), np.int16)
    padded[0, :len(audio)] = audio
    want, _ = _stream(_session(), padded, 5)
    assert got.shape == audio.shape and np.array_equal(got, want[0, DELAY:DELAY + len(audio)]) and np.abs(got).max() > 1000
