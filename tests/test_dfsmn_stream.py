"""Stateful streaming over the DFSMN path (include/ade.h, ade_stream_* on a model_family "dfsmn" handle): the kernels under the host simulator.

The contract: pushing a signal of K hops (960 samples each) in pieces and flushing equals the reference's graph on the WHOLE signal in one call, 960 samples
later, and the push size does not change a bit.  The oracle is oracle/dfsmn_oracle.py with exact DFT tables in one call on the whole signal; the gates are the
family's standing ones (tests/test_dfsmn.py): f32 waveform <= 2e-5, PCM <= 1 LSB.  Six hops = five frames: under the simulator every frame costs seconds of
emulated matrix-core products, and the memory history (19 frames) is crossed on the GPU (tests/test_dfsmn_stream_gpu.py); here every push size still carries
input, history and the half frame across a push boundary, and the 1-hop run has the push that completes no frame.
"""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from dfsmn_stream_lib import DELAY, HOP, blob_bytes, lsb, meta, run_stream, seed0_io, tensors  # noqa: E402

pytestmark = pytest.mark.hipsim

N_HOPS = 6


@functools.lru_cache(maxsize=None)
def _simlib():
    from ade_testlib import hipsim_library
    return hipsim_library()


def _session(length=N_HOPS * HOP, **kw):
    from audio_denoiser_onnx_amd.session import InferenceSession
    return InferenceSession(weights=blob_bytes(), metadata=meta(length, **kw), library=_simlib())


@functools.lru_cache(maxsize=None)
def _signal():
    return np.ascontiguousarray(seed0_io()[0][:1, 5000:5000 + N_HOPS * HOP])


def test_stream_equals_the_one_call_oracle_and_push_size_does_not_matter():
    from audio_denoiser_onnx_amd.session import StreamingSession
    from dfsmn_oracle import DfsmnOracle
    x = _signal()
    opcm, of32 = DfsmnOracle(tensors(), N_HOPS * HOP, exact_dft=True).process(x)
    assert opcm.shape == (1, N_HOPS * HOP) and np.abs(opcm).max() > 1000              # (a live signal)
    sess = _session()
    outs = {}
    for hops in (1, 3, 6):
        with StreamingSession(sess, 1, hops) as st:
            assert st.delay == DELAY and st.hop == HOP and st.samples_per_push == hops * HOP and st.in_channels == 1
            pcm, f32 = run_stream(st, x)
            with pytest.raises(ValueError):
                st.push(x[:, :hops * HOP])                                           # a flushed stream must be reset first
        assert pcm.shape == f32.shape == (1, N_HOPS * HOP + DELAY) and pcm.dtype == np.int16
        assert not pcm[:, :DELAY].any() and not f32[:, :DELAY].any()
        d_wave, d_pcm = float(np.abs(f32[:, DELAY:] - of32).max()), int(lsb(pcm[:, DELAY:], opcm).max())
        print(f"{N_HOPS} hops in pushes of {hops} + flush vs the one-call oracle: wave {d_wave:.3e} (gate 2.000e-05), pcm {d_pcm} LSB (gate 1)")
        assert d_wave <= 2e-5 and d_pcm <= 1
        outs[hops] = (pcm, f32)
    for hops in (3, 6):
        assert np.array_equal(outs[hops][0], outs[1][0]) and np.array_equal(outs[hops][1], outs[1][1]), f"{hops}-hop pushes differ from 1-hop pushes"


def test_a_flush_after_one_hop_is_refused_and_the_stream_goes_on():
    from audio_denoiser_onnx_amd.session import StreamingSession
    x = _signal()
    with StreamingSession(_session(), 1, 1) as st:
        first = st.push(x[:, :HOP])
        assert first.shape == (1, HOP) and not first.any()                           # the delay hop; no frame is complete yet
        with pytest.raises(ValueError, match="at least 2"):
            st.flush()
        second = st.push(x[:, HOP:2 * HOP])                                          # still usable: the signal's first hop
        assert second.any()
        assert st.flush().shape == (1, DELAY)


def test_refusals_name_int16_and_the_model_rate():
    from audio_denoiser_onnx_amd import _lib
    from audio_denoiser_onnx_amd.session import StreamingSession
    folded = _session(2 * 2880, use_batch_fold=True, batch_window_seconds=0.06)       # two windows of 2880 samples
    for sess in (folded, _session(input_audio_dtype="F32", output_audio_dtype="F32"), _session(1920, in_rate=16000)):
        with pytest.raises(_lib.AdeUnsupportedError, match="int16") as e:
            StreamingSession(sess, 1, 2)
        assert "48000" in str(e.value)
    with StreamingSession(_session(7000, dynamic_axes=True), 1, 2) as st:            # a dynamic_axes manifest streams alike
        assert st.hop == HOP


def test_stream_hop_by_family():
    from ade_testlib import make_session
    from audio_denoiser_onnx_amd.session import StreamingSession
    with StreamingSession(_session(), 2, 3) as st:
        assert (st.hop, st.delay, st.samples_per_push) == (960, 960, 2880)
    with StreamingSession(make_session(_simlib()), 1, 2) as st:
        assert (st.hop, st.delay, st.samples_per_push) == (256, 256, 512)
