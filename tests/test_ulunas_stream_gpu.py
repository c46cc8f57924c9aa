"""Stateful streaming over the UL-UNAS path on the GPU (csrc/ade_ulunas.hip, ade_stream_* on a model_family "ul_unas" handle).

The contract (include/ade.h): pushes of frames_per_push hops (256 samples each) plus the flush equal the reference's graph on the whole signal in ONE call, 256
samples later; the push size and the number of streams on the handle do not change a bit.  References: the reference-run fixtures tests/golden/ulunas_seed0.npz
(three rows of 16 000 samples) and ulunas_seed0_stream.npz (one clip of 20 480 samples = 80 hops, 81 frames: past the 64-frame chunk of the time-attention kernel;
tools/make_golden_ulunas.py --stream), and the float64-table oracle oracle/ulunas_oracle.py.  Gates are the one-shot tests' (tests/test_ulunas.py): against the
reference fixture <= 1 LSB with a differing share < 0.02; against the exact-table oracle and against ade_process <= 2 LSB (share < 0.02 for the oracle).
"""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from ulunas_stream_lib import DELAY, HOP, blob_bytes, lsb, meta, oracle, run_stream, seed0, stream_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

N = 20480            # 80 hops, 81 frames


def _session(length=N, **kw):
    from audio_denoiser_onnx_amd.session import InferenceSession
    return InferenceSession(weights=blob_bytes(), metadata=meta(length, **kw), device_id=0)


def _stream(sess, x, hops, flush=True):
    from audio_denoiser_onnx_amd.session import StreamingSession
    with StreamingSession(sess, x.shape[0], hops) as st:
        assert st.hop == HOP and st.delay == DELAY
        return run_stream(st, x, flush=flush)


@functools.lru_cache(maxsize=None)
def _three():
    """Three signals of 20 480 samples: the stream fixture's clip, and the noise and silence rows of ulunas_seed0.npz continued by themselves."""
    pcm_in = seed0()[0]
    return np.ascontiguousarray(np.stack([stream_fixture()["pcm_in"], np.concatenate((pcm_in[1], pcm_in[1]))[:N], np.zeros(N, np.int16)]))


@functools.lru_cache(maxsize=None)
def _five_hop_run():
    """The three signals as three streams of one handle, 5-hop pushes + flush; computed once, callers do not modify it."""
    return _stream(_session(), _three(), 5)


def test_gpu_stream_equals_the_reference_fixture_without_a_flush():
    """The three rows of ulunas_seed0.npz cut to 15 872 samples (62 hops) in 2-hop pushes: the reference's frames 0 .. 61 are the stream's, and the output samples
    [0, 15 616) of its 16 000-sample call need no later frame."""
    pcm_in, pcm_out, _ = seed0()
    x = np.ascontiguousarray(pcm_in[:, :15872])
    pcm, f32 = _stream(_session(), x, 2, flush=False)
    assert pcm.shape == f32.shape == (3, 15872) and pcm.dtype == np.int16
    assert not pcm[:, :DELAY].any() and not f32[:, :DELAY].any()
    assert not pcm[2].any() and not f32[2].any(), "an all-zero input must give an all-zero stream"
    assert np.abs(pcm[1]).max() > 1000                                                # (the noise row carries signal, as in tests/test_ulunas.py)
    d = lsb(pcm[:, DELAY:], pcm_out[:, :15616])
    print(f"2-hop pushes vs the reference's one call on 16 000 samples, samples [0, 15616): max {int(d.max())} LSB, differing share {float((d != 0).mean()):.5f} (gates 1, 0.02)")
    assert d.max() <= 1 and (d != 0).mean() < 0.02


def test_gpu_stream_with_flush_equals_the_reference_the_oracle_and_the_one_shot_call():
    """5-hop pushes (push boundaries inside the first 64-frame time-attention chunk) + flush on the 20 480-sample clip.

    The f32 gate against the oracle's waveform is twice what ade_process measures against it on the same clip in the same test (the parent path: its paired
    transforms round differently from the one-frame ones).  Measured on an MI355X: ade_process 7.08e-08, the stream 1.12e-07 (gate 1.42e-07);
    against the reference fixture the stream's PCM is within 1 LSB, differing share 0.0036, its f32 waveform within 2.5e-06 of the reference's float output; against
    the oracle its PCM is within 1 LSB, differing share 5e-05; ade_process and the stream give the same PCM."""
    fx = stream_fixture()
    x, out, wave = fx["pcm_in"][None], fx["pcm_out"][None], fx["wave"][None]
    assert x.shape == (1, N) and x.dtype == out.dtype == np.int16 and wave.dtype == np.float32 and np.abs(out).max() > 1000
    pcm, f32 = (a[:1] for a in _five_hop_run())
    assert pcm.shape == f32.shape == (1, N + DELAY) and not pcm[:, :DELAY].any() and not f32[:, :DELAY].any()
    d = lsb(pcm[:, DELAY:], out)
    print(f"5-hop pushes + flush vs the reference's one call on 20 480 samples: max {int(d.max())} LSB, differing share {float((d != 0).mean()):.5f} (gates 1, 0.02); "
          f"f32 vs its float waveform {float(np.abs(f32[:, DELAY:] - wave).max()):.3e} (printed, not gated)")
    assert d.max() <= 1 and (d != 0).mean() < 0.02
    o = oracle(N)
    opcm = o.process(x)
    owav = o.taps["wav"]
    do = lsb(pcm[:, DELAY:], opcm)
    one, one_f32 = _session().process(x, want_f32=True)
    d_one = int(lsb(pcm[:, DELAY:], one).max())
    parent = float(np.abs(one_f32 - owav).max())
    mine = float(np.abs(f32[:, DELAY:] - owav).max())
    print(f"vs the exact-table oracle: pcm max {int(do.max())} LSB, differing share {float((do != 0).mean()):.5f} (gates 2, 0.02); vs ade_process {d_one} LSB (gate 2); "
          f"f32 vs the oracle's waveform: ade_process {parent:.3e}, the stream {mine:.3e} (gate: twice ade_process's, {2 * parent:.3e})")
    assert do.max() <= 2 and (do != 0).mean() < 0.02
    assert d_one <= 2
    assert mine <= 2 * parent


@pytest.mark.parametrize("hops", [2, 16, 80])
def test_gpu_push_size_does_not_change_a_bit(hops):
    """80 hops: ONE push crosses a 64-frame time-attention chunk; 2 hops: every push replaces a kt = 3 history whole and every frame pair straddles a boundary."""
    pcm, f32 = _five_hop_run()
    p, f = _stream(_session(), _three(), hops)
    assert np.array_equal(p, pcm) and np.array_equal(f, f32), f"{hops}-hop pushes differ from 5-hop pushes"


def test_gpu_push_size_with_the_four_wavefront_time_attention(monkeypatch):
    """ADE_ULU_TA2=0 (read when the engine is created): k_ulu_ta carries its state as k_ulu_ta2 does.  Pushes of 2, 5 and 80 hops agree bit for bit; against the
    default kernel's run the PCM stays within 1 LSB (the two kernels' sums differ by fp32 round-off)."""
    monkeypatch.setenv("ADE_ULU_TA2", "0")
    x = _three()[:1]
    sess = _session()
    runs = [_stream(sess, x, hops) for hops in (2, 5, 80)]
    for p, f in runs[1:]:
        assert np.array_equal(p, runs[0][0]) and np.array_equal(f, runs[0][1])
    assert lsb(runs[0][0], _five_hop_run()[0][:1]).max() <= 1 and np.abs(runs[0][0]).max() > 1000


def test_gpu_a_stream_does_not_depend_on_its_neighbours():
    pcm, f32 = _five_hop_run()
    p, f = _stream(_session(), _three()[:1], 5)
    assert np.array_equal(p, pcm[:1]) and np.array_equal(f, f32[:1])


def test_gpu_six_hundred_streams_equal_three():
    """600 streams x 2 hops x 4 pushes (the three signals repeated): 1200 workgroups in the one-frame-per-workgroup launches, more than the chip holds at once."""
    pcm, f32 = _five_hop_run()
    n = 8 * HOP
    p, f = _stream(_session(), np.ascontiguousarray(np.tile(_three()[:, :n], (200, 1))), 2, flush=False)
    assert p.shape == (600, n) and np.abs(p[0]).max() > 100
    for rows in (slice(0, 3), slice(597, 600)):
        assert np.array_equal(p[rows], pcm[:, :n]) and np.array_equal(f[rows], f32[:, :n])


def test_gpu_reset_repeats_the_signal():
    from audio_denoiser_onnx_amd.session import StreamingSession
    x = _three()
    pcm, f32 = _five_hop_run()
    with StreamingSession(_session(), 3, 5) as st:
        run_stream(st, x[:, :35 * HOP], flush=False)                                  # abandoned mid-signal
        st.reset()
        p, f = run_stream(st, x)
        st.reset()
        again = st.push(x[:, :5 * HOP], want_f32=True)
    assert np.array_equal(p, pcm) and np.array_equal(f, f32)
    assert np.array_equal(again[0], pcm[:, :5 * HOP]) and np.array_equal(again[1], f32[:, :5 * HOP])


def test_gpu_push_device_on_a_caller_stream_equals_the_host_push():
    import torch
    from audio_denoiser_onnx_amd.session import StreamingSession
    x = _three()
    pcm, f32 = _five_hop_run()
    hops, n_push = 5, 5
    P = hops * HOP
    side = torch.cuda.Stream()
    d_in = [torch.from_numpy(np.ascontiguousarray(x[:, i * P:(i + 1) * P])).cuda() for i in range(n_push)]
    d_out = [torch.empty(3, P, dtype=torch.int16, device="cuda") for _ in range(n_push)]
    d_f32 = [torch.empty(3, P, dtype=torch.float32, device="cuda") for _ in range(n_push)]
    torch.cuda.synchronize()
    with StreamingSession(_session(), 3, hops) as st:
        with torch.cuda.stream(side):
            for i in range(n_push):
                st.push_device(d_in[i], d_out[i], d_f32[i], stream=side.cuda_stream)      # enqueued back to back, no synchronise in between
        side.synchronize()
    for i in range(n_push):
        assert np.array_equal(d_out[i].cpu().numpy(), pcm[:, i * P:(i + 1) * P]) and np.array_equal(d_f32[i].cpu().numpy(), f32[:, i * P:(i + 1) * P])


def test_gpu_file_driver_streams_a_ragged_file(tmp_path):
    """``inference_ulunas --stream 5`` on a 16 kHz file that is no whole number of hops: the pushes + flush of the zero-padded file, trimmed to the file's length."""
    import wave as wavmod
    from audio_denoiser_onnx_amd import inference_ulunas
    from audio_denoiser_onnx_amd.inference_gtcrn import read_wav_int16
    from audio_denoiser_onnx_amd.metadata import write_metadata
    audio = _three()[0][:20001]                                                       # 15.6 pushes of 1280 samples
    model = tmp_path / "UL_UNAS.adew"
    model.write_bytes(blob_bytes())
    write_metadata(model, meta(16000))
    noisy, out_path = tmp_path / "in.wav", tmp_path / "out.wav"
    with wavmod.open(str(noisy), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(audio.astype("<i2").tobytes())
    assert inference_ulunas.main([str(model), str(noisy), str(out_path), "--stream", "5"]) == 0
    got = read_wav_int16(out_path, 16000)
    padded = np.zeros((1, 16 * 5 * HOP), np.int16)
    padded[0, :len(audio)] = audio
    want, _ = _stream(_session(), padded, 5)
    assert got.shape == audio.shape and np.array_equal(got, want[0, DELAY:DELAY + len(audio)]) and np.abs(got).max() > 1000
