"""The single launch (k_gtcrn_chunk) reaches device memory through pointers it reads out of memory (ChunkFixed, SegPlan, the weight structs), the per-stage kernels
through kernel arguments.  csrc/ade_device.h (dev::gptr) gives the first the address space the second always had, and the front / back stage entries stage their tables
in one round trip (csrc/ade_stage_frontback.h, TabRegs / CopyRegs: clamped indices, guarded LDS writes).  No sum and no order of adds changes, so the single launch must
give the very bits of the per-stage kernels -- PCM, waveform and every tap -- in every geometry, at the smallest shapes where a lane's share of a table, a segment's
hand-off or the parked first hop can go wrong:

  T = 2   (264 samples: the engine takes no chunk below 258) one segment, 14 of 16 frames of a geometry-2 tile idle;
  T = 17  geometry 2 = 9 + 8 frames: two segments, one hand-off of every kind (convolution history, TRA and inter-frame GRU state, overlap-add carry, parked first hop);
  T = 33  geometry 2 = three segments of 11: the middle one both receives and hands on; geometry 1 = 17 + 16;

and a stream of two pushes of 17 frames against the one-shot call on the whole signal: the first segment of the second push continues from the slot the last segment of
the first push left (SegPlan::carry_in / carry_out), and in geometry 2 every segment with a predecessor parks its first hop behind its own exchange slot (`pend`, device
memory there, LDS in geometries 0 and 1).  The signals have an exactly zero integer sum, so the one-shot call's DC mean is exactly 0 and both sides do the same
arithmetic on the same frames: equality is bit for bit, one hop later.

Every (shape, geometry, launch form) runs once per session of the tests and is shared by the cases."""
import numpy as np
import pytest

from ade_testlib import make_session
from audio_denoiser_onnx_amd.session import StreamingSession
from audio_denoiser_onnx_amd.synth import synth_batch
from test_dpgrnn_residual import assert_same
from test_segments import run
from test_streaming import HOP, zero_sum_signal

BATCH = 3
# (length, frames, weight seed)
SHAPES = {"T2": (264, 2, 0), "T17": (4096, 17, 1), "T33": (8192, 33, 2)}
_runs = {}


def variant(shape_id, geometry, single):
    """(pcm, f32, taps) of one shape in one geometry as one launch (single = "1") or one launch per stage ("0"), full_taps = 1."""
    length, frames, seed = SHAPES[shape_id]
    if shape_id not in _runs:
        sess = make_session(None, seed=seed, length=length)
        assert sess.frames == frames
        _runs[shape_id] = (sess, synth_batch(BATCH, length), {})
    sess, x, done = _runs[shape_id]
    if (geometry, single) not in done:
        done[(geometry, single)] = run(sess, x, geometry, single=single)
    return done[(geometry, single)]


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", ["0", "1", "2"])
@pytest.mark.parametrize("shape_id", list(SHAPES))
def test_gpu_single_launch_equals_per_stage_kernels(shape_id, geometry):
    one = variant(shape_id, geometry, "1")
    frames = SHAPES[shape_id][1]
    assert_same(variant(shape_id, geometry, "0"), one, f"T = {frames}, geometry {geometry}: per-stage kernels vs the single launch")
    assert_same(variant(shape_id, "0", "0"), one, f"T = {frames}: geometry 0 per stage vs geometry {geometry} in one launch")


FRAMES_PER_PUSH = 17
_stream = {}


def stream_signals():
    if "x" not in _stream:
        rng = np.random.default_rng(5)
        _stream["x"] = np.stack([zero_sum_signal(rng, 2 * FRAMES_PER_PUSH * HOP) for _ in range(BATCH)])
        _stream["sess"] = make_session(None, seed=1, length=2 * FRAMES_PER_PUSH * HOP)
    return _stream["sess"], _stream["x"]


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", ["0", "1", "2"])
def test_gpu_two_push_stream_equals_one_shot_call(geometry):
    sess, x = stream_signals()
    assert sess.frames == 2 * FRAMES_PER_PUSH + 1
    sess.set_option("geometry", geometry)
    sess.set_option("single_launch", "1")
    sess.set_option("full_taps", "0")                       # the shipped kernel
    pcm1, f321 = sess.process(x, want_f32=True)
    P = FRAMES_PER_PUSH * HOP
    with StreamingSession(sess, BATCH, FRAMES_PER_PUSH) as st:
        parts = [st.push(x[:, i * P:(i + 1) * P], want_f32=True) for i in range(2)] + [st.flush(want_f32=True)]
    pcm = np.concatenate([p[0] for p in parts], axis=1)
    f32 = np.concatenate([p[1] for p in parts], axis=1)
    assert pcm.shape[1] == 2 * P + HOP
    assert not pcm[:, :HOP].any() and not f32[:, :HOP].any()                        # a stream's first hop is blank
    d = np.abs(f32[:, HOP:] - f321)
    print(f"geometry {geometry}: stream vs one-shot max |d f32| = {d.max():.3g}, pcm values that differ: {int((pcm[:, HOP:] != pcm1).sum())}")
    assert np.array_equal(f32[:, HOP:], f321), f"waveform differs in {int((d != 0).sum())} samples, first at {np.argwhere(d != 0)[0].tolist()}, max |d| = {d.max():.3g}"
    assert np.array_equal(pcm[:, HOP:], pcm1)
    assert sess.tap("xchg_error", 1)[0] == 0.0
