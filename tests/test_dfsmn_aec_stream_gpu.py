"""Stateful streaming over the DFSMN-AEC path on the GPU (csrc/ade_dfsmn_aec.hip, csrc/ade_nkf_aec.hip, ade_stream_*).

The contract (include/ade.h): pushes of frames_per_push hops plus the flush equal the reference's unfolded graph on the whole signal in ONE call, 1344 samples
later, and the push size does not change a bit.  References: the reference-run fixtures tests/golden/dfsmn_aec_seed0_io.npz (four rows of 32 000 samples),
dfsmn_aec_seed0_taps.npz (row 0's f32 waveform) and dfsmn_aec_seed0_stream.npz (two clips of 40 960 samples, tools/make_golden_dfsmn_aec.py --stream), and
the float64 oracle tests/dfsmn_aec_oracle.py.  Gates are the family's standing ones: f32 waveform <= 1e-4, PCM <= 1 LSB, over every sample.
"""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from dfsmn_aec_stream_lib import DELAY, GOLD, HOP, run_stream, seed0_blob, seed0_io, seed0_tensors, stream_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

N = 32000            # 125 hops, 99 mask frames


def _session(length=32000, blob=None, **kw):
    from audio_denoiser_onnx_amd import dfsmn_aec
    from audio_denoiser_onnx_amd.session import InferenceSession
    kw.setdefault("use_batch_fold", False)
    return InferenceSession(weights=blob if blob is not None else seed0_blob(), metadata=dfsmn_aec.metadata(length, **kw), device_id=0)


def _stream(sess, near, far, hops, flush=True):
    from audio_denoiser_onnx_amd.session import StreamingSession
    with StreamingSession(sess, near.shape[0], hops) as st:
        return run_stream(st, near, far, flush=flush)


@functools.lru_cache(maxsize=None)
def _five_hop_run():
    """The four fixture rows as four streams of one default-mode handle, 5-hop pushes + flush; computed once, callers do not modify it."""
    near, far, _ = seed0_io()
    return _stream(_session(), near, far, 5)


def test_gpu_stream_equals_the_reference_fixture():
    _, _, out = seed0_io()
    wave = np.load(os.path.join(GOLD, "dfsmn_aec_seed0_taps.npz"))["wave"].reshape(-1)
    pcm, f32 = _five_hop_run()
    assert pcm.shape == f32.shape == (4, N + DELAY) and pcm.dtype == np.int16
    assert not pcm[:, :DELAY].any() and not f32[:, :DELAY].any()
    lsb = np.abs(pcm[:, DELAY:].astype(np.int32) - out.astype(np.int32)).max(axis=1)
    d_wave = float(np.abs(f32[0, DELAY:] - wave).max())
    print(f"5-hop pushes + flush vs the reference's one call: pcm {lsb.tolist()} LSB per row, row 0 wave {d_wave:.3e}")
    assert lsb.max() <= 1 and d_wave <= 1e-4
    assert not pcm[3].any() and not f32[3].any(), "an all-zero input must give an all-zero stream"
    assert np.abs(pcm[0]).max() > 1000


@pytest.mark.parametrize("hops", [1, 25, 125])
def test_gpu_push_size_does_not_change_a_bit(hops):
    """1-hop pushes: every fifth push completes no mask frame, every frame straddles pushes and the 38-frame memory history crosses every push."""
    near, far, _ = seed0_io()
    pcm, f32 = _five_hop_run()
    p, f = _stream(_session(), near, far, hops)
    assert np.array_equal(p, pcm) and np.array_equal(f, f32), f"{hops}-hop pushes differ from 5-hop pushes"


def test_gpu_long_reference_run():
    """Two clips of 40 960 samples (160 hops, 127 mask frames) in 8-hop pushes + flush against the reference's ONE call on the whole clip."""
    fx = stream_fixture()
    near, far = np.stack([fx["near0"], fx["near1"]]), np.stack([fx["far0"], fx["far1"]])
    out, wave = np.stack([fx["out0"], fx["out1"]]), np.stack([fx["wave0"], fx["wave1"]])
    assert near.shape == (2, 40960) and near.dtype == far.dtype == out.dtype == np.int16 and wave.dtype == np.float32 and np.abs(out).max() > 1000
    pcm, f32 = _stream(_session(), near, far, 8)
    assert not pcm[:, :DELAY].any()
    lsb = int(np.abs(pcm[:, DELAY:].astype(np.int32) - out.astype(np.int32)).max())
    d_wave = float(np.abs(f32[:, DELAY:] - wave).max())
    print(f"8-hop pushes + flush vs the reference's one call on 40 960 samples: pcm {lsb} LSB, wave {d_wave:.3e}")
    assert lsb <= 1 and d_wave <= 1e-4


def test_gpu_exact_mode_against_the_oracle():
    """ade_dft_tables = exact: the back end's FFT stream kernels.  Wave <= 1e-4 from the float64 oracle with exact tables (the existing gate of that mode); the PCM
    distance to the reference fixture is printed per row, not gated (the one-shot engine measures 1, 1, 3, 0 there: DESIGN.md section 11)."""
    from dfsmn_aec_oracle import DfsmnAecOracle
    near, far, out = seed0_io()
    opcm, taps = DfsmnAecOracle(seed0_tensors(), tables="exact", mask_tables="exact").forward(near, far)
    pcm, f32 = _stream(_session(dft_tables="exact"), near, far, 5)
    d_wave = float(np.abs(f32[:, DELAY:] - taps["wave"]).max())
    lsb_oracle = np.abs(pcm[:, DELAY:].astype(np.int32) - opcm.astype(np.int32)).max(axis=1)
    lsb_ref = np.abs(pcm[:, DELAY:].astype(np.int32) - out.astype(np.int32)).max(axis=1)
    print(f"exact mode, 5-hop pushes + flush: wave {d_wave:.3e} from the exact-table oracle; pcm {lsb_oracle.tolist()} LSB from it, {lsb_ref.tolist()} LSB from the "
          f"reference fixture")
    assert d_wave <= 1e-4


def test_gpu_streams_are_independent_and_the_grid_scales():
    """600 fresh streams (the four rows repeated; the signal is a 15-hop cut of the fixture rows from sample 8000), three 5-hop pushes: they complete 0, 4 and 4
    mask frames, so N = 600 x 4 = 2400 columns span 19 GEMM column tiles where the 4-stream run (16 columns) stays inside one."""
    near, far, _ = seed0_io()
    near, far = near[:, 8000:8000 + 15 * HOP], far[:, 8000:8000 + 15 * HOP]
    sess = _session()
    small = _stream(sess, near, far, 5, flush=False)
    assert small[0].any()
    big = _stream(sess, np.concatenate([near] * 150), np.concatenate([far] * 150), 5, flush=False)
    for rows in (slice(0, 4), slice(300, 304), slice(596, 600)):
        assert np.array_equal(big[0][rows], small[0]) and np.array_equal(big[1][rows], small[1])


def test_gpu_push_device_on_a_caller_stream_equals_the_host_push():
    import torch
    from audio_denoiser_onnx_amd.session import StreamingSession
    near, far, _ = seed0_io()
    hops, n_push = 5, 6
    P = hops * HOP
    rows = np.stack([near, far], axis=1)[:, :, 8000:8000 + n_push * P]                # (4, 2, n): near end, far end
    sess = _session()
    with StreamingSession(sess, 4, hops) as st:
        host = [st.push(rows[:, :, i * P:(i + 1) * P], want_f32=True) for i in range(n_push)]
    side = torch.cuda.Stream()
    d_in = [torch.from_numpy(np.ascontiguousarray(rows[:, :, i * P:(i + 1) * P])).cuda() for i in range(n_push)]
    d_out = [torch.empty(4, P, dtype=torch.int16, device="cuda") for _ in range(n_push)]
    d_f32 = [torch.empty(4, P, dtype=torch.float32, device="cuda") for _ in range(n_push)]
    torch.cuda.synchronize()
    with StreamingSession(sess, 4, hops) as st:
        with torch.cuda.stream(side):
            for i in range(n_push):
                st.push_device(d_in[i], d_out[i], d_f32[i], stream=side.cuda_stream)      # enqueued back to back, no synchronise in between
        side.synchronize()
    for i in range(n_push):
        assert np.array_equal(d_out[i].cpu().numpy(), host[i][0]) and np.array_equal(d_f32[i].cpu().numpy(), host[i][1])
    assert any(h[0].any() for h in host)


def test_gpu_a_geometry_off_the_seed():
    """``two_tiles`` (tests/aec_geometry_lib.py): dilation 12 >= the frames of a push, M = 130 spans two GEMM row tiles.  6400 samples against the oracle in one
    call; pushes of 1 and 5 hops are bit-identical."""
    import aec_geometry_lib as G
    from audio_denoiser_onnx_amd.weights import pack_blob
    from dfsmn_aec_oracle import DfsmnAecOracle
    near, far = G.signals("two_tiles", 25 * HOP)
    near, far = np.ascontiguousarray(near[[0, 1]]), np.ascontiguousarray(far[[0, 1]])
    tensors = G.blob_tensors("two_tiles")
    opcm, taps = DfsmnAecOracle(tensors, tables="reference", mask_tables="exact").forward(near, far)
    sess = _session(3200, blob=pack_blob(tensors))
    one, five = _stream(sess, near, far, 1), _stream(sess, near, far, 5)
    d_wave = float(np.abs(five[1][:, DELAY:] - taps["wave"]).max())
    lsb = int(np.abs(five[0][:, DELAY:].astype(np.int32) - opcm.astype(np.int32)).max())
    print(f"two_tiles, 25 hops in pushes of 5 + flush vs the one-call oracle: wave {d_wave:.3e}, pcm {lsb} LSB")
    assert d_wave <= 1e-4 and lsb <= 1 and np.abs(opcm).max() > 1000
    assert np.array_equal(one[0], five[0]) and np.array_equal(one[1], five[1]), "1-hop pushes differ from 5-hop pushes"


def test_gpu_delay_and_refusals():
    from audio_denoiser_onnx_amd import _lib
    from audio_denoiser_onnx_amd.session import StreamingSession
    with pytest.raises(_lib.AdeUnsupportedError, match="int16"):
        StreamingSession(_session(16000, input_audio_dtype="F32", output_audio_dtype="F32"), 1, 4)      # float audio tensors
    with pytest.raises(_lib.AdeUnsupportedError, match="16000"):
        StreamingSession(_session(16000, out_sample_rate=48000), 1, 4)                                  # another output rate
    sess = _session(output_vad_result=True)                                                             # accepted: a stream returns audio only
    with pytest.raises(ValueError):
        StreamingSession(sess, 1, 0)
    with pytest.raises(ValueError):
        StreamingSession(sess, 0, 4)
    with StreamingSession(sess, 2, 1) as st:
        assert st.delay == DELAY == 1344 and st.in_channels == 2
        with pytest.raises(ValueError):
            st.push(np.zeros((2, HOP), np.int16))                                                       # one channel short
        with pytest.raises(ValueError):
            st.flush()                                                                                  # nothing pushed yet
        assert not st.push(np.full((2, 2, HOP), 1000, np.int16)).any()                                  # a one-hop first push returns zeros
        for _ in range(6):
            st.push(np.full((2, 2, HOP), 1000, np.int16))
        with pytest.raises(ValueError, match="multiple of 5"):
            st.flush()                                                                                  # 7 hops: no length the static export accepts
        for _ in range(3):
            st.push(np.full((2, 2, HOP), 1000, np.int16))
        assert st.flush().shape == (2, DELAY)                                                           # 10 hops
        with pytest.raises(ValueError):
            st.push(np.zeros((2, 2, HOP), np.int16))                                                    # flushed: reset first
    with StreamingSession(_session(48000, use_batch_fold=True, batch_window_seconds=1.5), 1, 5) as st:  # a folded manifest streams alike
        assert st.delay == DELAY


def test_gpu_file_driver_streaming_keeps_the_echo_path_the_sliced_mode_does_not():
    """``inference_dfsmn_aec --stream``: a fixture clip (40 960 samples = 32 x 1280: no padding) equals the reference's one call on the whole clip within
    1 LSB; the sliced ``process`` of the same clip through a folded 1.5 s handle restarts filter and memory in every window and is outside that gate.  Its RMS
    distance is printed, not gated: nobody has measured it for this family before."""
    from audio_denoiser_onnx_amd import inference_dfsmn_aec as drv
    fx = stream_fixture()
    near, far, ref = fx["near0"], fx["far0"], fx["out0"].astype(np.int32)
    out = drv.process_streaming(_session(), near, far, frames_per_push=62)
    assert out.shape == (40960,) and out.dtype == np.int16
    d = int(np.abs(out.astype(np.int32) - ref).max())
    sliced, _ = drv.process(_session(48000, use_batch_fold=True, batch_window_seconds=1.5), near, far, rng=np.random.default_rng(0))
    assert sliced.shape == (40960,)
    diff = sliced.astype(np.float64) - ref
    d_sliced, rms = int(np.abs(diff).max()), float(np.sqrt(np.mean(diff ** 2)))
    print(f"streamed driver vs the reference's one call: {d} LSB; sliced driver (folded 1.5 s windows): max {d_sliced} LSB, {rms:.1f} LSB RMS")
    assert d <= 1
    assert d_sliced > 1
