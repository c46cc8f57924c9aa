"""DFSMN-AEC kernels under the host-side HIP simulator vs the numpy oracle (CPU, test-only build).

tests/hipsim/build.sh compiles a fixed source list without csrc/ade_nkf_aec.hip and csrc/ade_dfsmn_aec.hip (its library answers ADE_ERR_UNSUPPORTED for the
family: the weak dfsmn_aec_create).  This test builds its OWN simulator library with the same g++ line plus those two files, into a separate file, and runs a
short unfolded case and a two-window folded case with the default tables (the back end's dense reference-table products) and the unfolded case again with
ade_dft_tables = exact (its FFT kernels).  The oracle runs with the matching tables.  feat, mask and vad_results are held to the seed-0 gates of
tests/test_dfsmn_aec_gpu.py for the matching table mode (read from dfsmn_aec_seed0_taps.npz).
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

from dfsmn_aec_oracle import DfsmnAecOracle  # noqa: E402

pytestmark = pytest.mark.hipsim

CSRC = os.path.join(REPO, "audio_denoiser_onnx_amd", "csrc")
SOURCES = ["ade_kernels.hip", "ade_fused.hip", "ade_engine.hip", "ade_stft.hip", "ade_dfsmn.hip", "ade_melband.hip", "ade_mossformer.hip", "ade_ulunas.hip",
           "ade_hgtcrn.hip", "ade_zipenhancer.hip", "ade_nkf_aec.hip", "ade_dfsmn_aec.hip"]
LIB = os.path.join(HERE, "hipsim", "_build", "libade_hipsim_dfsmn_aec.so")
GOLD = os.path.join(HERE, "golden")


def build_simlib():
    """The simulator library with the two AEC engines, built once (tests/test_aec_geometry.py loads the same file)."""
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
def simlib():
    return build_simlib()


def _gates(dft_tables):
    """The seed-0 gates of tests/test_dfsmn_aec_gpu.py, read from the fixture's recorded distances for the matching table mode."""
    import json
    from aec_geometry_lib import gate
    dist = json.loads(str(np.load(os.path.join(GOLD, "dfsmn_aec_seed0_taps.npz"))["fp64_distance"]))["engine" if dft_tables == "reference" else "exact"]
    return {k: gate(dist, k) for k in ("feat", "mask", "vad_results")}


def _check(simlib, length, fold, window_seconds, rows, dft_tables="reference"):
    from audio_denoiser_onnx_amd import dfsmn_aec
    from audio_denoiser_onnx_amd.session import InferenceSession
    from audio_denoiser_onnx_amd.weights import load_blob
    with open(os.path.join(GOLD, "dfsmn_aec_seed0.adew"), "rb") as f:
        blob = f.read()
    io = np.load(os.path.join(GOLD, "dfsmn_aec_seed0_io.npz"))
    sess = InferenceSession(weights=blob, metadata=dfsmn_aec.metadata(length, use_batch_fold=fold, batch_window_seconds=window_seconds, output_vad_result=True,
                                                                    dft_tables=dft_tables), library=simlib)
    L = sess.in_len
    near = np.stack([io[f"near{i}"][:L] for i in rows])
    far = np.stack([io[f"far{i}"][:L] for i in rows])
    pcm, vad, f32 = None, None, None
    out = sess.run(None, {"near_end_audio": near[:, None], "far_end_audio": far[:, None]}, return_f32=True)
    pcm, f32, vad = out
    W = int(sess.metadata.optional_int("fold_window_length")) if fold else 0
    opcm, taps = DfsmnAecOracle(load_blob(os.path.join(GOLD, "dfsmn_aec_seed0.adew")), tables=dft_tables, mask_tables="exact").forward(near, far, fold_window=W)
    assert pcm.shape == (len(rows), 1, L)
    n = len(rows) * L
    d_temp = float(np.abs(sess.tap("temp_aec", n).reshape(taps["temp_aec"].shape) - taps["temp_aec"]).max())
    d_feat = float(np.abs(sess.tap("feat", taps["feat"].size).reshape(taps["feat"].shape) - taps["feat"]).max())
    d_mask = float(np.abs(sess.tap("mask", taps["mask"].size).reshape(taps["mask"].shape) - taps["mask"]).max())
    d_vad = float(np.abs(vad - taps["vad_results"]).max())
    d_wave = float(np.abs(f32[:, 0] - taps["wave"]).max())
    lsb = int(np.abs(pcm[:, 0].astype(np.int32) - opcm.astype(np.int32)).max())
    print(f"hipsim vs oracle: temp_aec {d_temp:.2e} feat {d_feat:.2e} mask {d_mask:.2e} vad {d_vad:.2e} wave {d_wave:.2e} pcm {lsb} LSB")
    assert vad.shape == (taps["vad_results"].size,)
    assert d_wave <= 1e-4 and lsb <= 1 and d_temp <= 1e-4
    g = _gates(dft_tables)
    print("gates:", " ".join(f"{k} {v:.3e}" for k, v in g.items()))
    assert d_feat <= g["feat"] and d_mask <= g["mask"] and d_vad <= g["vad_results"], (d_feat, d_mask, d_vad, g)
    return sess


def test_unfolded_short_case(simlib):
    _check(simlib, 3200, False, 1.5, (0, 1))


def test_unfolded_short_case_exact_tables(simlib):
    _check(simlib, 3200, False, 1.5, (0,), dft_tables="exact")


def test_folded_two_windows(simlib):
    sess = _check(simlib, 2500, True, 0.1, (0,))          # 0.1 s windows: W = 1600, 2 windows, 3200 samples in
    assert sess.in_len == 3200 and sess.vad_frames == 2 * sess.frames
