"""Stateful streaming over the UL-UNAS path (include/ade.h, ade_stream_* on a model_family "ul_unas" handle): the kernels under the host simulator.

The contract: pushing a signal of K hops (256 samples each) in pieces and flushing equals the reference's graph on the WHOLE signal in one call, 256 samples
later, and the push size does not change a bit.  The oracle is oracle/ulunas_oracle.py with exact DFT tables in one call on the whole signal; the gate is that of
tests/test_ulunas.py::test_hipsim_short_clip_matches_oracle: PCM <= 1 LSB.  Twelve hops = thirteen frames: the 2-hop run puts a push boundary between every pair
of frames (every kt = 2 and kt = 3 history, every GRU state and the half frame cross each one), the 3-hop run renews a kt = 3 history from the middle of a push,
the 12-hop run is one push.  The 64-frame chunks of the time attention and a chip's worth of workgroups are crossed on the GPU (tests/test_ulunas_stream_gpu.py).
"""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from ulunas_stream_lib import DELAY, HOP, blob_bytes, lsb, meta, oracle, run_stream, seed0  # noqa: E402

pytestmark = pytest.mark.hipsim

N_HOPS = 12
N = N_HOPS * HOP            # 3072


@functools.lru_cache(maxsize=None)
def _simlib():
    from ade_testlib import hipsim_library
    return hipsim_library()


def _session(length=N, **kw):
    from audio_denoiser_onnx_amd.session import InferenceSession
    return InferenceSession(weights=blob_bytes(), metadata=meta(length, **kw), library=_simlib())


@functools.lru_cache(maxsize=None)
def _signal():
    return np.ascontiguousarray(seed0()[0][:2, 3000:3000 + N])


def test_stream_equals_the_one_call_oracle_and_push_size_does_not_matter():
    from audio_denoiser_onnx_amd.session import StreamingSession
    x = _signal()
    want = oracle(N).process(x)
    assert want.shape == (2, N) and np.abs(want).max() > 1000                          # (a live signal)
    sess = _session()
    outs = {}
    for hops in (2, 3, 12):
        with StreamingSession(sess, 2, hops) as st:
            assert st.delay == DELAY and st.hop == HOP and st.samples_per_push == hops * HOP and st.in_channels == 1
            pcm, f32 = run_stream(st, x)
            with pytest.raises(ValueError):
                st.push(x[:, :hops * HOP])                                           # a flushed stream must be reset first
        assert pcm.shape == f32.shape == (2, N + DELAY) and pcm.dtype == np.int16
        assert not pcm[:, :DELAY].any() and not f32[:, :DELAY].any()
        d = int(lsb(pcm[:, DELAY:], want).max())
        print(f"{N_HOPS} hops in pushes of {hops} + flush vs the one-call oracle: pcm {d} LSB (gate 1)")
        assert d <= 1
        outs[hops] = (pcm, f32)
    for hops in (3, 12):
        assert np.array_equal(outs[hops][0], outs[2][0]) and np.array_equal(outs[hops][1], outs[2][1]), f"{hops}-hop pushes differ from 2-hop pushes"


def test_refusals_and_the_stream_geometry():
    from audio_denoiser_onnx_amd import _lib
    from audio_denoiser_onnx_amd.session import StreamingSession
    sess = _session()
    with pytest.raises(ValueError, match="frames_per_push = 1"):
        StreamingSession(sess, 1, 1)                                                 # the first push could not hold the head reflection's 257 samples
    with StreamingSession(sess, 2, 2) as st:
        assert (st.hop, st.delay, st.samples_per_push) == (256, 256, 512)
        with pytest.raises(ValueError):
            st.push(_signal()[:, :HOP])                                              # a short push
    folded = _session(2 * 4096, use_batch_fold=True, batch_window_seconds=0.256)      # two windows of 4096 samples
    for bad in (folded, _session(input_audio_dtype="F32", output_audio_dtype="F32")):
        with pytest.raises(_lib.AdeUnsupportedError, match="int16") as e:
            StreamingSession(bad, 1, 2)
        assert "16000" in str(e.value)
    with StreamingSession(_session(7000, dynamic_axes=True), 1, 2) as st:            # a dynamic_axes manifest streams alike
        assert st.hop == HOP and st.delay == DELAY


def test_the_four_wavefront_time_attention_carries_its_state_too(monkeypatch):
    """ADE_ULU_TA2=0 (read when the engine is created) selects k_ulu_ta, which takes the same optional state: four hops in pushes of 2 and of 4 agree bit for bit and
    stay within 1 LSB of the oracle (its sums differ from k_ulu_ta2's by fp32 round-off, so the two kernels' bits are not compared)."""
    from audio_denoiser_onnx_amd.session import StreamingSession
    monkeypatch.setenv("ADE_ULU_TA2", "0")
    n = 4 * HOP
    x = np.ascontiguousarray(_signal()[:1, :n])
    want = oracle(n).process(x)
    sess = _session(n)
    outs = []
    for hops in (2, 4):
        with StreamingSession(sess, 1, hops) as st:
            outs.append(run_stream(st, x))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][0][:, DELAY:].any() and lsb(outs[0][0][:, DELAY:], want).max() <= 1
