"""The DPGRNN's two residuals (csrc/ade_stage_net.h, fc_ln_rows): phase B takes x out of the LDS planes before the intra-frame GRU's outputs replace it there, phase D
asks device memory for `mid` ahead of its Linear pass.  Neither changes a sum or its order, so every geometry, in one launch or one launch per stage, must give the very
bits of geometry 0 per stage -- at the smallest shapes where the residual's ownership (16-lane row tr = tid >> 4 of frame tr, clamped past the segment) can go wrong:

  T = 2   (264 samples) one segment, 14 idle LayerNorm rows in geometry 2 (30 / 62 in geometries 1 / 0) that clamp to the last frame and emit nothing;
  T = 17  geometry 2 = 9 + 8 frames: a short last segment;
  T = 33  geometry 2 = three segments of 11, geometry 1 = 17 + 16.

Each case runs under the host simulator (CPU) and on the MI355X.  Bounds against the float64 oracle: those of test_segments.py (1e-4 on the waveform, 1 LSB)."""
import numpy as np
import pytest

from ade_testlib import golden_blob, hipsim_library, make_session
from audio_denoiser_onnx_amd.synth import synth_batch
from oracle_lib import GtcrnOracle
from test_segments import TAPS, run

# (length, batch, frames, weight seed).  T = 2 at 264 samples: the engine takes no chunk below 258 (the reflect padding of half a window), and 264 is the first
# multiple of 8 above that -- the DC mean's 16-byte path with 33 loads for 256 / 512 / 1024 lanes, every other one switched off by address.
SHAPES = [(264, 3, 2, 0), (4096, 2, 17, 1), (8192, 3, 33, 2)]
IDS = ["T2", "T17", "T33"]
_oracle = {}


def oracle(length, batch, seed):
    """The oracle's (pcm, f32) of a shape: computed once, shared by the simulator and the GPU case."""
    if length not in _oracle:
        _oracle[length] = GtcrnOracle(golden_blob(seed), length).process(synth_batch(batch, length))
    return _oracle[length]


def written(name, tap):
    """The part of a tap the kernels write: a spectrum row is 257 bins in a pitch of 260, and nobody writes (or reads) the three behind them -- they hold whatever the
    allocation held, NaN bit patterns included, which compare unequal to themselves."""
    return tap.reshape(-1, 260)[:, :257] if name == "spec" else tap


def assert_same(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"{what}: output differs, max |d f32| = {np.abs(a[1] - b[1]).max():.3g}"
    for n in TAPS:
        x, y = written(n, a[2][n]), written(n, b[2][n])
        assert np.array_equal(x, y), f"{what}: tap {n} differs in {int((x != y).sum())} of {x.size} values, first at {np.argwhere(x != y)[0].tolist()}"


_sessions = {}


def variant(lib, shape, geometry, single):
    """One run of a shape on a backend (None: the GPU), full_taps = 1: made once per session of the tests and shared by the cases that need it."""
    length, batch, frames, seed = shape
    key = (lib is None, length)
    if key not in _sessions:
        sess = make_session(lib, seed=seed, length=length)
        assert sess.frames == frames
        _sessions[key] = (sess, synth_batch(batch, length), {})
    sess, x, runs = _sessions[key]
    if (geometry, single) not in runs:
        runs[(geometry, single)] = run(sess, x, geometry, single=single)
    return runs[(geometry, single)]


def every_variant_equals_geometry0_per_stage(lib, shape):
    length, batch, frames, seed = shape
    ref = variant(lib, shape, "0", "0")
    for geometry in "012":
        for single in "01":
            if (geometry, single) != ("0", "0"):
                assert_same(ref, variant(lib, shape, geometry, single), f"T = {frames}, geometry {geometry}, single_launch {single}")
    opcm, of32 = oracle(length, batch, seed)
    err, lsb = np.abs(ref[1] - of32).max(), np.abs(ref[0].astype(np.int32) - opcm.astype(np.int32)).max()
    print(f"T = {frames}: wave max|d| vs oracle = {err:.3e}, pcm max diff = {lsb} LSB")
    assert err <= 1e-4 and lsb <= 1


def lean_taps_are_complete(lib):
    """full_taps = 0 (the shipped kernel, geometry 2, T = 17): dp0 still stores all of its output (tap dp1) although dp1 no longer reads it back, and x_e4 -- dp0's input,
    now read from LDS only -- is whole in device memory too (the decoder's skip connection).  Against the full_taps = 1 run of the same session."""
    shape = SHAPES[1]
    length, batch, frames, seed = shape
    full = variant(lib, shape, "2", "1")
    sess, x, _ = _sessions[(lib is None, length)]
    sess.set_option("geometry", "2")
    sess.set_option("single_launch", "1")
    sess.set_option("full_taps", "0")
    pcm, f32 = sess.process(x, want_f32=True)
    assert np.array_equal(pcm, full[0]) and np.array_equal(f32, full[1])
    for name in ("dp1", "x_e4"):
        assert np.array_equal(sess.tap(name, batch * frames * 65 * 16), full[2][name]), f"tap {name}"


@pytest.mark.hipsim
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_hipsim_residuals_bit_equal_every_geometry(shape):
    every_variant_equals_geometry0_per_stage(hipsim_library(), shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gpu_residuals_bit_equal_every_geometry(shape):
    every_variant_equals_geometry0_per_stage(None, shape)


@pytest.mark.hipsim
def test_hipsim_lean_stores_keep_dp1_and_x_e4():
    lean_taps_are_complete(hipsim_library())


@pytest.mark.gpu
def test_gpu_lean_stores_keep_dp1_and_x_e4():
    lean_taps_are_complete(None)
