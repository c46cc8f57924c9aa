"""SDAEC kernels under the host-side HIP simulator vs the float64 oracle (CPU, test-only build).

tests/hipsim/build.sh compiles a fixed source list without csrc/ade_sdaec.hip (its library answers ADE_ERR_UNSUPPORTED for the family: the weak sdaec_create).
This test builds its OWN simulator library with the same g++ line plus that file, into a separate file, and runs two short cases and the refused manifests.
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

from sdaec_oracle import SdaecOracle, fixture_state  # noqa: E402

pytestmark = pytest.mark.hipsim

CSRC = os.path.join(REPO, "audio_denoiser_onnx_amd", "csrc")
SOURCES = ["ade_kernels.hip", "ade_fused.hip", "ade_engine.hip", "ade_stft.hip", "ade_dfsmn.hip", "ade_melband.hip", "ade_mossformer.hip", "ade_ulunas.hip",
           "ade_hgtcrn.hip", "ade_zipenhancer.hip", "ade_sdaec.hip"]
LIB = os.path.join(HERE, "hipsim", "_build", "libade_hipsim_sdaec.so")
GOLD = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def simlib():
    import glob
    from audio_denoiser_onnx_amd import _lib
    deps = [os.path.join(CSRC, s) for s in SOURCES] + glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(HERE, "hipsim", "hipsim.cpp"),
                                                                                             os.path.join(HERE, "hipsim", "hip", "hip_runtime.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I",
                        os.path.join(HERE, "hipsim"), "-x", "c++"] + [os.path.join(CSRC, s) for s in SOURCES] +
                       ["-x", "c++", os.path.join(HERE, "hipsim", "hipsim.cpp"), "-o", LIB], check=True, cwd=REPO)
    return _lib.AdeLibrary(LIB)


@pytest.fixture(scope="module")
def blob():
    from audio_denoiser_onnx_amd import sdaec, weights
    tensors = sdaec.state_to_blob_tensors(*fixture_state(GOLD))
    return weights.pack_blob(tensors), tensors


@pytest.mark.parametrize("length,batch", [(1600, 2), (2720, 1)])
def test_engine_matches_oracle_short_case(simlib, blob, length, batch):
    from audio_denoiser_onnx_amd import sdaec
    from audio_denoiser_onnx_amd.session import InferenceSession
    io = np.load(os.path.join(GOLD, "sdaec_seed0_io.npz"))
    near = np.stack([io[f"near{i}"][8000:8000 + length] for i in range(batch)])
    far = np.stack([io[f"far{i}"][8000:8000 + length] for i in range(batch)])
    sess = InferenceSession(weights=blob[0], metadata=sdaec.metadata(length), library=simlib)
    pcm, f32 = sess.run(None, {"near_end_audio": near[:, None], "far_end_audio": far[:, None]}, return_f32=True)
    opcm, owave, _ = SdaecOracle(blob[1]).forward(near, far)
    assert pcm.shape == (batch, 1, length)
    d_wave, d_pcm = float(np.abs(f32[:, 0] - owave).max()), int(np.abs(pcm[:, 0].astype(np.int32) - opcm.astype(np.int32)).max())
    print(f"L = {length}: wave {d_wave:.2e} pcm {d_pcm}")
    assert d_wave <= 1e-4
    assert d_pcm <= 1


@pytest.mark.parametrize("change,named", [({"dynamic_axes": "1"}, "dynamic_axes"), ({"in_sample_rate": "48000"}, "in_sample_rate"), ({"nfft": "512"}, "nfft"),
                                          ({"hop_length": "128"}, "hop_length"), ({"window_type": "hann"}, "window_type"), ({"center_pad": "0"}, "center_pad"),
                                          ({"pad_mode": "reflect"}, "pad_mode"), ({"alpha_k": "8"}, "alpha_k")])
def test_refused_manifests(simlib, blob, change, named):
    from audio_denoiser_onnx_amd import sdaec
    from audio_denoiser_onnx_amd._lib import AdeUnsupportedError
    from audio_denoiser_onnx_amd.session import InferenceSession
    meta = dict(sdaec.metadata(1600))
    meta.update(change)
    with pytest.raises(AdeUnsupportedError, match=named):            # ADE_ERR_UNSUPPORTED, naming the setting
        InferenceSession(weights=blob[0], metadata=meta, library=simlib)


def test_stream_refused(simlib, blob):
    from audio_denoiser_onnx_amd import sdaec
    from audio_denoiser_onnx_amd._lib import AdeUnsupportedError
    from audio_denoiser_onnx_amd.session import InferenceSession, StreamingSession
    sess = InferenceSession(weights=blob[0], metadata=sdaec.metadata(1600), library=simlib)
    with pytest.raises(AdeUnsupportedError, match="streaming is implemented for"):
        StreamingSession(sess, 1, 4)


def test_fixed_source_list_library_answers_unsupported(blob):
    """tests/hipsim/build.sh links without csrc/ade_sdaec.hip: the weak sdaec_create resolves to null and the family is refused, not crashed into."""
    from ade_testlib import hipsim_library
    from audio_denoiser_onnx_amd import sdaec
    from audio_denoiser_onnx_amd._lib import AdeUnsupportedError
    from audio_denoiser_onnx_amd.session import InferenceSession
    with pytest.raises(AdeUnsupportedError, match="'sdaec' is not built into this library"):
        InferenceSession(weights=blob[0], metadata=sdaec.metadata(1600), library=hipsim_library())
