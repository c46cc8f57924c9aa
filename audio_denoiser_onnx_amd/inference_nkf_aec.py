"""File driver for NKF-AEC, following NKF_AEC/Inference_NKF_AEC_ONNX.py:268-364: two 16 kHz wav files (far end, near end) -> echo-cancelled wav.

As the reference: both files are read as mono int16, optionally RMS-normalised (before the trim, :274-275), trimmed to the shorter one, cut into static
slices of the graph's input length -- stepped by the graph's OUTPUT length when that is shorter and the rates agree (a length that is not a whole number
of hops keeps 256 (T - 1) samples per slice, :292-293) -- with the tail padded by Gaussian noise at the RMS of the signal's last samples (:299-303); the
outputs are concatenated, trimmed to ``int(n * OUT / IN)`` samples (:325, :354) and written at the OUTPUT rate (:363), PCM_16 or IEEE float.
Unlike the reference, every slice of the file runs as ONE batched call (slices are independent calls of the graph), and the tail noise can be seeded.
Float-input handles are refused: the reference driver would feed them int16-valued floats, which is not the export's normalised input.

``--stream N`` instead runs the whole file through ONE stateful stream (``ade_stream_*``) in pushes of N hops: the filter keeps the echo path it has learnt
over the whole file instead of converging again in every slice (:func:`process_streaming`).  The reference has no such mode.

    python -m audio_denoiser_onnx_amd.inference_nkf_aec <model_dir_or_.adew> [far.wav near.wav out.wav] [--normalize] [--stream N]

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


def process_streaming(sess, far: np.ndarray, near: np.ndarray, frames_per_push: int = 62, normalize: bool = False) -> np.ndarray:
    """Whole int16 signals -> the echo-cancelled int16 signal through ONE stateful stream (``--stream N``).

    What the mode is for: an echo canceller is an adaptive filter, and :func:`process` -- like the reference's driver -- restarts it in every slice of the graph's
    static length, so it converges to the echo path again and again.  Here the per-bin Kalman state, the far-end history and the STFT / ISTFT overlap are carried
    on the device from push to push, so the filter keeps what it has learnt over the whole file; the result is what the reference's graph would give on the whole
    file in one call, without its whole-call DC removal.  The reference has no such mode: its static export only runs on a fixed-length window.

    Both signals are trimmed to the shorter one and zero-padded to whole hops of 256 samples, and pushed in pushes of the largest number of hops that divides the
    hop count and does not exceed ``frames_per_push``: the stream then ends exactly where the signal ends.  (Padding to whole pushes of ``frames_per_push`` instead
    would add frames past the end that the one-call result does not have, and its last 256 samples would be overlap-added from four frames instead of three:
    up to 178 LSB away on the example clips.)  The stream's latency (``delay`` samples: pushes + flush, the first ``delay`` samples dropped) is removed again and
    the output cut to the input length.  The session's own static length does not matter."""
    from .session import StreamingSession
    if getattr(sess, "in_dtype", np.int16) != np.int16 or getattr(sess, "out_dtype", np.int16) != np.int16:
        raise ValueError("inference_nkf_aec: a stream takes and returns int16 PCM; export the model with INT16 audio tensors")
    far, near = normalise_audio(far, normalize), normalise_audio(near, normalize)
    n = min(len(far), len(near))
    if int(frames_per_push) < 1:
        raise ValueError("inference_nkf_aec: frames_per_push must be at least 1")
    hops = max(1, -(-n // 256))
    per_push = max(d for d in range(1, min(int(frames_per_push), hops) + 1) if hops % d == 0)
    P, n_push = per_push * 256, hops // per_push
    rows = np.zeros((1, 2, hops * 256), np.int16)
    rows[0, 0, :n], rows[0, 1, :n] = far[:n], near[:n]
    with StreamingSession(sess, 1, per_push) as st:
        parts = [st.push(rows[:, :, i * P:(i + 1) * P]) for i in range(n_push)]
        parts.append(st.flush())
        delay = st.delay
    return np.ascontiguousarray(np.concatenate(parts, axis=1)[0, delay:delay + n])


def main(sess, far_path=None, near_path=None, out_path: str = "aec.wav", normalize: bool = False, rng=None, stream_frames: int = 0) -> np.ndarray:
    in_rate, out_rate = session_rates(sess)
    far = read_wav_int16(far_path or example_audio("aec", "farend_speech1.wav"), in_rate)
    near = read_wav_int16(near_path or example_audio("aec", "nearend_mic1.wav"), in_rate)
    y = process_streaming(sess, far, near, stream_frames, normalize) if stream_frames else process(sess, far, near, normalize, rng)
    if y.dtype == np.int16:
        write_wav_int16(out_path, y, out_rate)
    else:
        write_wav_float32(out_path, y.astype(np.float32), out_rate)
    return y


if __name__ == "__main__":
    from .session import InferenceSession
    argv = sys.argv[1:]
    stream_frames = 0
    if "--stream" in argv:
        i = argv.index("--stream")
        stream_frames = int(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    args = [a for a in argv if not a.startswith("--")]
    if len(args) not in (1, 4):
        print(__doc__)
        raise SystemExit(2)
    s = InferenceSession(args[0])
    paths = args[1:] if len(args) == 4 else (None, None, "aec.wav")
    main(s, *paths, normalize="--normalize" in sys.argv, stream_frames=stream_frames)
    print(f"AEC done: {paths[2]}")
