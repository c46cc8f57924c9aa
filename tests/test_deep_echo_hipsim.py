"""Deep Echo kernels under the host-side HIP simulator vs the float64 oracle (CPU, test-only build).

tests/hipsim/build.sh and tests/test_sdaec_hipsim.py compile fixed source lists without csrc/ade_deep_echo.hip (their libraries answer ADE_ERR_UNSUPPORTED for
the family: the weak deep_echo_create).  This test builds its OWN simulator library with the g++ flags of tests/test_sdaec_hipsim.py plus that file, into a
separate file (the translation units compiled in parallel), and runs two short cases and the refused manifests.  (The address / undefined-behaviour sanitizer run of the same call is a stand-alone program,
tests/hipsim/deep_echo_sanitize.sh; it is not a test and is never loaded into Python.)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from deep_echo_oracle import WAVE_GATE, DeepEchoOracle, fixture_state  # noqa: E402

pytestmark = pytest.mark.hipsim

CSRC = os.path.join(REPO, "audio_denoiser_onnx_amd", "csrc")
SOURCES = ["ade_kernels.hip", "ade_fused.hip", "ade_engine.hip", "ade_stft.hip", "ade_dfsmn.hip", "ade_melband.hip", "ade_mossformer.hip", "ade_ulunas.hip",
           "ade_hgtcrn.hip", "ade_zipenhancer.hip", "ade_sdaec.hip", "ade_deep_echo.hip"]
LIB = os.path.join(HERE, "hipsim", "_build", "libade_hipsim_deep_echo.so")
GOLD = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def simlib():
    import glob
    from audio_denoiser_onnx_amd import _lib
    deps = [os.path.join(CSRC, s) for s in SOURCES] + glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(HERE, "hipsim", "hipsim.cpp"),
                                                                                             os.path.join(HERE, "hipsim", "hip", "hip_runtime.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        # the flags of tests/test_sdaec_hipsim.py's g++ line; one object per translation unit, compiled side by side (one serial g++ over thirteen files
        # takes minutes of the suite's time), then one link
        from concurrent.futures import ThreadPoolExecutor
        objdir = os.path.join(os.path.dirname(LIB), "deep_echo_obj")
        os.makedirs(objdir, exist_ok=True)
        flags = ["g++", "-std=c++17", "-O2", "-g", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(HERE, "hipsim")]

        def compile_one(src):
            obj = os.path.join(objdir, os.path.basename(src) + ".o")
            subprocess.run(flags + ["-x", "c++", "-c", src, "-o", obj], check=True, cwd=REPO)
            return obj
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            objs = list(pool.map(compile_one, [os.path.join(CSRC, s) for s in SOURCES] + [os.path.join(HERE, "hipsim", "hipsim.cpp")]))
        subprocess.run(["g++", "-shared", "-fPIC"] + objs + ["-o", LIB], check=True, cwd=REPO)
    return _lib.AdeLibrary(LIB)


@pytest.fixture(scope="module")
def blob():
    from audio_denoiser_onnx_amd import deep_echo, weights
    tensors = deep_echo.state_to_blob_tensors(fixture_state(GOLD))
    return weights.pack_blob(tensors), tensors


def _case(length, batch):
    io = np.load(os.path.join(GOLD, "deep_echo_seed0_io.npz"))
    near = np.stack([io[f"near{i}"][4000:4000 + length] for i in range(batch)])
    far = np.stack([io[f"far{i}"][4000:4000 + length] for i in range(batch)])
    return near, far


@pytest.mark.parametrize("length,batch", [(1600, 2), (2720, 1)])
def test_engine_matches_oracle_short_case(simlib, blob, length, batch):
    """T = 10 is one frame past the nine-frame tap history; T = 17 one frame past a 16-sequence tile."""
    from audio_denoiser_onnx_amd import deep_echo
    from audio_denoiser_onnx_amd.session import InferenceSession
    near, far = _case(length, batch)
    sess = InferenceSession(weights=blob[0], metadata=deep_echo.metadata(length), library=simlib)
    pcm, f32 = sess.run(None, {"near_end_audio": near[:, None], "far_end_audio": far[:, None]}, return_f32=True)
    opcm, owave, otaps = DeepEchoOracle(blob[1]).forward(near, far, want_taps=True)
    assert pcm.shape == (batch, 1, length)
    d_wave, d_pcm = float(np.abs(f32[:, 0] - owave).max()), int(np.abs(pcm[:, 0].astype(np.int32) - opcm.astype(np.int32)).max())
    print(f"L = {length}: wave {d_wave:.2e} pcm {d_pcm}")
    assert d_wave <= WAVE_GATE
    assert d_pcm <= 1
    T = sess.frames
    path = sess.tap("path", batch * T * 160 * 20).reshape(batch, T, 160, 20)
    assert float(np.abs(path - otaps["path"]).max()) <= 1e-5 * max(1.0, float(np.abs(otaps["path"]).max()))
    if batch == 2:      # the tap history at the clip boundary: row 1 gives the same bits alone and behind row 0
        p1, f1 = sess.run(None, {"near_end_audio": near[1:, None], "far_end_audio": far[1:, None]}, return_f32=True)
        assert np.array_equal(p1[0], pcm[1]) and np.array_equal(f1[0], f32[1])
        assert np.any(far[0, -1600:] != 0)          # row 0's last frames are not silent: a read across the boundary would have changed row 1's head


@pytest.mark.parametrize("change,named", [({"dynamic_axes": "1"}, "dynamic_axes"), ({"in_sample_rate": "48000"}, "in_sample_rate"), ({"nfft": "512"}, "nfft"),
                                          ({"window_length": "256"}, "window_length"), ({"hop_length": "128"}, "hop_length"), ({"window_type": "hann"}, "window_type"),
                                          ({"center_pad": "0"}, "center_pad"), ({"pad_mode": "reflect"}, "pad_mode"), ({"echo_order": "8"}, "echo_order")])
def test_refused_manifests(simlib, blob, change, named):
    from audio_denoiser_onnx_amd import deep_echo
    from audio_denoiser_onnx_amd._lib import AdeUnsupportedError
    from audio_denoiser_onnx_amd.session import InferenceSession
    meta = dict(deep_echo.metadata(1600))
    meta.update(change)
    with pytest.raises(AdeUnsupportedError, match=named):            # ADE_ERR_UNSUPPORTED, naming the setting
        InferenceSession(weights=blob[0], metadata=meta, library=simlib)


def test_dynamic_axes_message_says_not_built(simlib, blob):
    from audio_denoiser_onnx_amd import deep_echo
    from audio_denoiser_onnx_amd._lib import AdeUnsupportedError
    from audio_denoiser_onnx_amd.session import InferenceSession
    with pytest.raises(AdeUnsupportedError, match="dynamic_axes=1 is not built"):
        InferenceSession(weights=blob[0], metadata=dict(deep_echo.metadata(1600), dynamic_axes="1"), library=simlib)


def test_stream_refused(simlib, blob):
    from audio_denoiser_onnx_amd import deep_echo
    from audio_denoiser_onnx_amd._lib import AdeUnsupportedError
    from audio_denoiser_onnx_amd.session import InferenceSession, StreamingSession
    sess = InferenceSession(weights=blob[0], metadata=deep_echo.metadata(1600), library=simlib)
    with pytest.raises(AdeUnsupportedError, match="streaming is implemented for"):
        StreamingSession(sess, 1, 4)


def test_fixed_source_list_library_answers_unsupported(blob):
    """tests/hipsim/build.sh links without csrc/ade_deep_echo.hip: the weak deep_echo_create resolves to null and the family is refused, not crashed into."""
    from ade_testlib import hipsim_library
    from audio_denoiser_onnx_amd import deep_echo
    from audio_denoiser_onnx_amd._lib import AdeUnsupportedError
    from audio_denoiser_onnx_amd.session import InferenceSession
    with pytest.raises(AdeUnsupportedError, match="'deep_echo' is not built into this library"):
        InferenceSession(weights=blob[0], metadata=deep_echo.metadata(1600), library=hipsim_library())
