"""NKF-AEC kernels under the host-side HIP simulator vs the numpy oracle (CPU, test-only build).

tests/hipsim/build.sh compiles a fixed source list without csrc/ade_nkf_aec.hip (its library answers ADE_ERR_UNSUPPORTED for the family: the weak
nkf_aec_create).  This test builds its OWN simulator library with the same g++ line plus that file, into a separate file, and runs a short case.
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

from nkf_aec_oracle import NkfAecOracle  # noqa: E402

pytestmark = pytest.mark.hipsim

CSRC = os.path.join(REPO, "audio_denoiser_onnx_amd", "csrc")
SOURCES = ["ade_kernels.hip", "ade_fused.hip", "ade_engine.hip", "ade_stft.hip", "ade_dfsmn.hip", "ade_melband.hip", "ade_mossformer.hip", "ade_ulunas.hip",
           "ade_hgtcrn.hip", "ade_zipenhancer.hip", "ade_nkf_aec.hip"]
LIB = os.path.join(HERE, "hipsim", "_build", "libade_hipsim_nkf.so")


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


def test_engine_matches_oracle_short_case(simlib):
    from audio_denoiser_onnx_amd import nkf_aec
    from audio_denoiser_onnx_amd.session import InferenceSession
    from audio_denoiser_onnx_amd.weights import load_blob
    gold = os.path.join(HERE, "golden")
    with open(os.path.join(gold, "nkf_aec_seed0.adew"), "rb") as f:
        blob = f.read()
    io = np.load(os.path.join(gold, "nkf_aec_seed0_io.npz"))
    L = 4096
    far = np.stack([io["far0"][:L], io["far2"][:L]])
    near = np.stack([io["near0"][:L], io["near2"][:L]])
    sess = InferenceSession(weights=blob, metadata=nkf_aec.metadata(L), library=simlib)
    pcm, f32 = sess.run(None, {"far_end_audio": far[:, None], "near_end_audio": near[:, None]}, return_f32=True)
    opcm, owave, _ = NkfAecOracle(load_blob(os.path.join(gold, "nkf_aec_seed0.adew")), tables="exact").forward(far, near)
    assert pcm.shape == (2, 1, L)
    assert float(np.abs(f32[:, 0] - owave).max()) <= 1e-4
    assert int(np.abs(pcm[:, 0].astype(np.int32) - opcm.astype(np.int32)).max()) <= 1
