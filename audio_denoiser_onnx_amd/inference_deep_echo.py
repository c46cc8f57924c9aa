"""File driver for Deep Echo AEC, following Deep_Echo_AEC/Inference_Deep_Echo_ONNX.py: two 16 kHz wav files (near end, far end) -> echo-cancelled wav.

That script is SDAEC's (and so NKF-AEC's) driver with other paths: both files read as mono int16, trimmed to the shorter one, cut into static slices of the
graph's input length with the tail padded by noise, the outputs concatenated and trimmed, written at the output rate.  The slicing, padding and writing are
:mod:`inference_nkf_aec`'s; the session feeds the two inputs by name, so only the argument order (near end first) differs.
There is no ``--stream`` mode: the engine does not stream this family.

    python -m audio_denoiser_onnx_amd.inference_deep_echo <model_dir_or_.adew> [near.wav far.wav out.wav] [--normalize]
"""
from __future__ import annotations

import sys

import numpy as np

from . import inference_nkf_aec as aec


def process(sess, near: np.ndarray, far: np.ndarray, normalize: bool = False, rng=None) -> np.ndarray:
    """Whole signals -> the echo-cancelled signal at the handle's output rate (int16, or float for a float-output handle)."""
    return aec.process(sess, far, near, normalize, rng)


def main(sess, near_path=None, far_path=None, out_path: str = "aec.wav", normalize: bool = False, rng=None) -> np.ndarray:
    return aec.main(sess, far_path, near_path, out_path, normalize, rng)


if __name__ == "__main__":
    from .session import InferenceSession
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) not in (1, 4):
        print(__doc__)
        raise SystemExit(2)
    paths = args[1:] if len(args) == 4 else (None, None, "aec.wav")
    main(InferenceSession(args[0]), *paths, normalize="--normalize" in sys.argv)
    print(f"AEC done: {paths[2]}")
