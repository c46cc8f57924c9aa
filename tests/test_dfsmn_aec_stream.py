"""Stateful streaming over the DFSMN-AEC path (include/ade.h, ade_stream_* on a model_family "dfsmn_aec" handle): the kernels under the host simulator.

The contract: pushing a signal of K hops (K a multiple of 5) in pieces and flushing equals the reference's unfolded graph on the WHOLE signal in one call, 1344
samples later, and the push size does not change a bit.  The family has no whole-call DC removal, so any input serves.  The simulator library is the one
tests/test_dfsmn_aec_hipsim.py builds (its source list); the oracle is tests/dfsmn_aec_oracle.py in one call on the whole signal, with the handle's table mode.
Gates: the ones tests/test_dfsmn_aec_hipsim.py holds the one-shot call to for the waveform and the PCM in either mode -- f32 waveform <= 1e-4, PCM <= 1 LSB.

Geometries off the seed (tests/aec_geometry_lib.py): ``tails`` has three different (lorder, dilation) pairs with a memory history of 12 frames, ``no_memory``
has lorder 1: no history at all.  Signals of 6400 samples = 25 hops = 19 mask frames: more than the history, and with one-hop pushes every fifth push completes
no mask frame.
"""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import aec_geometry_lib as G  # noqa: E402
from dfsmn_aec_oracle import DfsmnAecOracle  # noqa: E402
from dfsmn_aec_stream_lib import DELAY, HOP, mask_frames_after, run_stream  # noqa: E402

pytestmark = pytest.mark.hipsim

N_HOPS = 25
ROWS = (0, 1)                     # echo + near-end noise; far end silent


def test_delay_is_the_minimum_and_is_reached():
    """320 M(k) >= 256 k - 1344 for every k, with equality at k = 9, 14, ...: 1344 samples is the smallest lag at which every push can emit its 256 F samples."""
    slack = [320 * mask_frames_after(k) - (HOP * k - DELAY) for k in range(4000)]
    assert min(slack) == 0 and [k for k in range(6, 30) if slack[k] == 0] == [9, 14, 19, 24, 29]
    assert max(s for k, s in enumerate(slack) if k >= 6) == 256
    assert mask_frames_after(N_HOPS) == 16 and (N_HOPS * HOP - 640) // 320 + 1 == 19


@functools.lru_cache(maxsize=None)
def _simlib():
    from test_dfsmn_aec_hipsim import build_simlib
    return build_simlib()


@functools.lru_cache(maxsize=None)
def _signals(name):
    near, far = G.signals(name, N_HOPS * HOP)
    return np.ascontiguousarray(near[list(ROWS)]), np.ascontiguousarray(far[list(ROWS)])


@functools.lru_cache(maxsize=None)
def _oracle(name, tables):
    """One call on the whole signal; computed once per case, callers do not modify it."""
    near, far = _signals(name)
    pcm, taps = DfsmnAecOracle(G.blob_tensors(name), tables=tables, mask_tables="exact").forward(near, far)
    return pcm, taps["wave"]


def _session(name, tables, length=3200):
    from audio_denoiser_onnx_amd import dfsmn_aec
    from audio_denoiser_onnx_amd.session import InferenceSession
    from audio_denoiser_onnx_amd.weights import pack_blob
    meta = dfsmn_aec.metadata(length, dft_tables=tables)           # the handle's static length does not matter for streams
    return InferenceSession(weights=pack_blob(G.blob_tensors(name)), metadata=meta, library=_simlib())


@pytest.mark.parametrize("name,tables", [("tails", "reference"), ("tails", "exact"), ("no_memory", "exact")])
def test_stream_equals_the_one_call_oracle_and_push_size_does_not_matter(name, tables):
    """Pushes of 1, 5 and 25 hops + flush against the oracle, bit-identical among themselves; the prefix check (a causal system: the pushes over the first 24
    hops equal the 1-hop run's pushed output) and the refused flush after 24 hops.  Under the simulator every step of the reference-table back end is two
    dense 1026 x 1024 products on simulated matrix cores, minutes per run, so that case runs the prefix check with 2-hop pushes (the dense stream loader with
    two frames per step continuing from a carry) and leaves the 3-hop prefix and the reset-and-repeat check to the FFT back end's cases: the mask stage, the
    bookkeeping and the reset are the same code in both modes."""
    from audio_denoiser_onnx_amd.session import StreamingSession
    near, far = _signals(name)
    n = N_HOPS * HOP
    opcm, owave = _oracle(name, tables)
    assert opcm.shape == (len(ROWS), n) and np.abs(opcm).max() > 1000              # (a live signal)
    sess = _session(name, tables)
    outs = {}
    for hops in (1, 5, 25):
        with StreamingSession(sess, len(ROWS), hops) as st:
            assert st.delay == DELAY and st.in_channels == 2
            pcm, f32 = run_stream(st, near, far)
            with pytest.raises(ValueError):
                st.push_aec(far[:, :hops * HOP], near[:, :hops * HOP])             # a flushed stream must be reset first
            if tables == "exact":
                st.reset()
                again = st.push_aec(far[:, :hops * HOP], near[:, :hops * HOP], want_f32=True)
                assert np.array_equal(again[0], pcm[:, :hops * HOP]) and np.array_equal(again[1], f32[:, :hops * HOP]), "a reset stream does not repeat itself"
        assert pcm.shape == f32.shape == (len(ROWS), n + DELAY)
        assert not pcm[:, :DELAY].any() and not f32[:, :DELAY].any()
        d_wave = float(np.abs(f32[:, DELAY:] - owave).max())
        lsb = int(np.abs(pcm[:, DELAY:].astype(np.int32) - opcm.astype(np.int32)).max())
        print(f"{name} ({tables} tables), {N_HOPS} hops in pushes of {hops} + flush vs the one-call oracle: wave {d_wave:.3e} (gate 1.000e-04), pcm {lsb} LSB (gate 1)")
        assert d_wave <= 1e-4 and lsb <= 1
        outs[hops] = (pcm, f32)
    for hops in (5, 25):
        assert np.array_equal(outs[hops][0], outs[1][0]) and np.array_equal(outs[hops][1], outs[1][1]), f"{hops}-hop pushes differ from 1-hop pushes"
    # a causal system: pushes of 2 and 3 hops over the first 24 hops give the 1-hop run's pushed output; 24 hops are no length the static export accepts
    for hops in (2, 3) if tables == "exact" else (2,):
        with StreamingSession(sess, len(ROWS), hops) as st:
            pcm, f32 = run_stream(st, near[:, :24 * HOP], far[:, :24 * HOP], flush=False)
            with pytest.raises(ValueError, match="multiple of 5"):
                st.flush()
        assert np.array_equal(pcm, outs[1][0][:, :24 * HOP]) and np.array_equal(f32, outs[1][1][:, :24 * HOP]), f"{hops}-hop pushes differ from 1-hop pushes"
