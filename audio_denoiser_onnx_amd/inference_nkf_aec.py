"""File driver for NKF-AEC, following NKF_AEC/Inference_NKF_AEC_ONNX.py:268-364: two 16 kHz wav files (far end, near end) -> echo-cancelled wav.

As the reference: both files are read as mono int16, optionally RMS-normalised (before the trim, :274-275), trimmed to the shorter one, cut into static
slices of the graph's input length -- stepped by the graph's OUTPUT length when that is shorter and the rates agree (a length that is not a whole number
of hops keeps 256 (T - 1) samples per slice, :292-293) -- with the tail padded by Gaussian noise at the RMS of the signal's last samples (:299-303); the
outputs are concatenated, trimmed to ``int(n * OUT / IN)`` samples (:325, :354) and written at the OUTPUT rate (:363), PCM_16 or IEEE float.
Unlike the reference, every slice of the file runs as ONE batched call (slices are independent calls of the graph), and the tail noise can be seeded.
Float-input handles are refused: the reference driver would feed them int16-valued floats, which is not the export's normalised input.

    python -m audio_denoiser_onnx_amd.inference_nkf_aec <model_dir_or_.adew> [far.wav near.wav out.wav] [--normalize]

The default inputs are the reference's example clips, ``<ADE_TEST_EXAMPLES or ./Test_Examples>/aec/{farend_speech1,nearend_mic1}.wav``.
"""
from __future__ import annotations

import sys

import numpy as np

from .inference_gtcrn import (cut_slices, example_audio, normalise_audio, output_length, read_wav_int16, session_rates, write_wav_float32,
                              write_wav_int16)


def run_rows(sess, far_rows: np.ndarray, near_rows: np.ndarray) -> np.ndarray:
    """(n, L) int16 far / near slices -> (n, L_out): one batched call of the graph."""
    (out,) = sess.run(None, {"far_end_audio": far_rows[:, None], "near_end_audio": near_rows[:, None]})
    return out[:, 0]


def process(sess, far: np.ndarray, near: np.ndarray, normalize: bool = False, rng=None) -> np.ndarray:
    """Whole signals -> the echo-cancelled signal at the handle's output rate (int16, or float for a float-output handle)."""
    if getattr(sess, "in_dtype", np.int16) != np.int16:
        raise ValueError("inference_nkf_aec: the driver feeds int16 PCM; export the model with an INT16 input")
    in_rate, out_rate = session_rates(sess)
    far, near = normalise_audio(far, normalize), normalise_audio(near, normalize)
    n = min(len(far), len(near))
    rng = rng if rng is not None else np.random.default_rng()
    stride_out = in_rate == out_rate                            # (:292: the output-length stride only at equal rates)
    near_s, _ = cut_slices(near[:n], sess.in_len, sess.out_len, tail_pad="noise", rng=rng, out_stride=stride_out)
    far_s, _ = cut_slices(far[:n], sess.in_len, sess.out_len, tail_pad="noise", rng=rng, out_stride=stride_out)
    out = run_rows(sess, far_s, near_s)
    return np.ascontiguousarray(out.reshape(-1)[:output_length(n, in_rate, out_rate)])


def main(sess, far_path=None, near_path=None, out_path: str = "aec.wav", normalize: bool = False, rng=None) -> np.ndarray:
    in_rate, out_rate = session_rates(sess)
    far = read_wav_int16(far_path or example_audio("aec", "farend_speech1.wav"), in_rate)
    near = read_wav_int16(near_path or example_audio("aec", "nearend_mic1.wav"), in_rate)
    y = process(sess, far, near, normalize, rng)
    if y.dtype == np.int16:
        write_wav_int16(out_path, y, out_rate)
    else:
        write_wav_float32(out_path, y.astype(np.float32), out_rate)
    return y


if __name__ == "__main__":
    from .session import InferenceSession
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) not in (1, 4):
        print(__doc__)
        raise SystemExit(2)
    s = InferenceSession(args[0])
    paths = args[1:] if len(args) == 4 else (None, None, "aec.wav")
    main(s, *paths, normalize="--normalize" in sys.argv)
    print(f"AEC done: {paths[2]}")
