"""Stateful streaming over the NKF-AEC path (include/ade.h, ade_stream_* on a model_family "nkf_aec" handle): the fixture, and the kernels under the host simulator.

The contract: pushing a signal of n hops in pieces and flushing equals the reference's graph on the WHOLE signal in one call, 768 samples later, without the
whole-call DC removal.  The reference and the oracle remove that mean, so every test signal has an exactly zero integer sum: the mean is then exactly 0 and both
sides compute the same thing.  Tolerances are the family's contract against reference-run fixtures: f32 waveform <= 1e-4, PCM <= 1 LSB, over every sample.
"""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from nkf_aec_oracle import NkfAecOracle  # noqa: E402
from nkf_aec_stream_lib import DELAY, HOP, fixture, run_stream, seed0_blob, seed0_tensors, zero_sum  # noqa: E402

CSRC = os.path.join(REPO, "audio_denoiser_onnx_amd", "csrc")
SOURCES = ["ade_kernels.hip", "ade_fused.hip", "ade_engine.hip", "ade_stft.hip", "ade_dfsmn.hip", "ade_melband.hip", "ade_mossformer.hip", "ade_ulunas.hip",
           "ade_hgtcrn.hip", "ade_zipenhancer.hip", "ade_nkf_aec.hip"]
LIB = os.path.join(HERE, "hipsim", "_build", "libade_hipsim_nkf_stream.so")


def test_fixture_is_what_it_claims():
    """Zero integer sums (the reference's DC term is exactly 0), 192 hops, and the numpy oracle on the whole signal agrees with the stored reference output."""
    fx = fixture()
    oracle = NkfAecOracle(seed0_tensors(), tables="exact")
    for i in range(2):
        far, near, out, wave = fx[f"far{i}"], fx[f"near{i}"], fx[f"out{i}"], fx[f"wave{i}"]
        assert far.dtype == near.dtype == out.dtype == np.int16 and wave.dtype == np.float32
        assert far.shape == near.shape == out.shape == wave.shape == (192 * HOP,)
        assert int(far.astype(np.int64).sum()) == 0 and int(near.astype(np.int64).sum()) == 0
        assert far.any() and near.any() and out.any()
        opcm, owave, _ = oracle.forward(far[None], near[None])
        d_wave = float(np.abs(owave[0] - wave).max())
        d_pcm = int(np.abs(opcm[0].astype(np.int32) - out.astype(np.int32)).max())
        print(f"clip {i}: oracle vs reference fixture: wave {d_wave:.3e}, pcm {d_pcm} LSB")
        assert d_wave <= 1e-4 and d_pcm <= 1


@pytest.fixture(scope="module")
def simlib():
    """The host simulator with csrc/ade_nkf_aec.hip, built as tests/test_nkf_aec_hipsim.py builds its library, into a file of its own."""
    from audio_denoiser_onnx_amd import _lib
    deps = [os.path.join(CSRC, s) for s in SOURCES] + glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(HERE, "hipsim", "hipsim.cpp"),
                                                                                             os.path.join(HERE, "hipsim", "hip", "hip_runtime.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I",
                        os.path.join(HERE, "hipsim"), "-x", "c++"] + [os.path.join(CSRC, s) for s in SOURCES] +
                       ["-x", "c++", os.path.join(HERE, "hipsim", "hipsim.cpp"), "-o", LIB], check=True, cwd=REPO)
    return _lib.AdeLibrary(LIB)


@pytest.mark.hipsim
def test_hipsim_stream_equals_one_shot_and_push_size_does_not_matter(simlib):
    """A 24-hop cut of the fixture (zero-summed again after the cut) as pushes of 1, 3 and 8 hops + flush: the oracle's one-shot output 768 samples later,
    the same bits for every push size, the same bits after a reset, and no push after a flush."""
    from audio_denoiser_onnx_amd import nkf_aec
    from audio_denoiser_onnx_amd.session import InferenceSession, StreamingSession
    fx = fixture()
    n = 24 * HOP
    far = np.stack([zero_sum(fx["far0"][8192:8192 + n]), zero_sum(fx["far1"][20480:20480 + n])])
    near = np.stack([zero_sum(fx["near0"][8192:8192 + n]), zero_sum(fx["near1"][20480:20480 + n])])
    opcm, owave, _ = NkfAecOracle(seed0_tensors(), tables="exact").forward(far, near)
    assert np.abs(opcm).max() > 1000                                   # (a live signal: the comparison below is not between silences)
    sess = InferenceSession(weights=seed0_blob(), metadata=nkf_aec.metadata(4096), library=simlib)     # the handle's static length does not matter for streams
    outs = {}
    for hops in (1, 3, 8):
        with StreamingSession(sess, 2, hops) as st:
            assert st.delay == DELAY and st.in_channels == 2
            pcm, f32 = run_stream(st, far, near)
            with pytest.raises(ValueError):
                st.push_aec(far[:, :hops * HOP], near[:, :hops * HOP])          # a flushed stream must be reset first
            st.reset()
            again = st.push_aec(far[:, :hops * HOP], near[:, :hops * HOP], want_f32=True)
        assert np.array_equal(again[0], pcm[:, :hops * HOP]) and np.array_equal(again[1], f32[:, :hops * HOP])
        assert pcm.shape == f32.shape == (2, n + DELAY)
        assert not pcm[:, :DELAY].any() and not f32[:, :DELAY].any()
        d_wave = float(np.abs(f32[:, DELAY:] - owave).max())
        d_pcm = int(np.abs(pcm[:, DELAY:].astype(np.int32) - opcm.astype(np.int32)).max())
        print(f"{hops}-hop pushes vs the one-shot oracle: wave {d_wave:.3e}, pcm {d_pcm} LSB")
        assert d_wave <= 1e-4 and d_pcm <= 1
        outs[hops] = (pcm, f32)
    for hops in (3, 8):
        assert np.array_equal(outs[hops][0], outs[1][0]) and np.array_equal(outs[hops][1], outs[1][1]), f"{hops}-hop pushes differ from 1-hop pushes"
    with pytest.raises(ValueError):
        StreamingSession(sess, 2, 0)
    with StreamingSession(sess, 2, 3) as st:
        with pytest.raises(ValueError):
            st.push(np.zeros((2, 3 * HOP), np.int16))                   # an AEC push is (n_streams, 2, P)
        with pytest.raises(ValueError):
            st.flush()                                                  # nothing pushed yet
