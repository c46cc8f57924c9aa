"""File driver for DFSMN-AEC, following DFSMN_AEC/Inference_DFSMN_ONNX_AEC.py: two 16 kHz wav files (near end, far end) -> echo-cancelled wav, and with a
VAD-enabled model the speech segments as ``timestamps_second.txt`` / ``timestamps_indices.txt`` next to it.

As the reference: both files are read as mono int16, optionally RMS-normalised, trimmed to the shorter one and cut into static slices of the graph's input
length.  The last slice is padded with ZEROS when the model is a folded export (its input is whole windows, the padding lies outside the signal) and with
Gaussian noise at the RMS of the signal's last samples otherwise.  The outputs are concatenated, trimmed to ``int(n * OUT / IN)`` samples and written at the
output rate.  Unlike the reference, every slice of the file runs as ONE batched call, and the tail noise can be seeded.

The VAD post-processing works on the per-frame speech probabilities of the frames that lie inside the signal (a frame is 640 model-rate samples at a shift of
320; a folded slice restarts the count in every window):
  1. hysteresis with look-ahead (:func:`silence_states`): silence ends at a frame that reaches ``speaking_score`` if at least that share of the next
     ``look_ahead`` frames does too; speech ends at a frame at or below ``silence_score`` if more than that share of the next frames is as well.  The last
     ``look_ahead`` frames, which have no full look-ahead, switch on their own value;
  2. runs of speech become (start, end) pairs, the end one frame shift after the first silent frame (:func:`segments`);
  3. segments shorter than ``min_speech_duration`` are dropped, then neighbours at most ``fusion_threshold`` apart are merged (:func:`fuse_segments`).

    python -m audio_denoiser_onnx_amd.inference_dfsmn_aec <model_dir_or_.adew> [near.wav far.wav out.wav] [--normalize] [--stream N]

``--stream N``: one stateful stream over the whole file in pushes of at most N hops (:func:`process_streaming`) instead of independent windows; audio only.

The default inputs are the reference's example clips, ``<ADE_TEST_EXAMPLES or ./Test_Examples>/aec/{nearend_mic1,farend_speech1}.wav``.
"""
from __future__ import annotations

import sys
from pathlib import Path
from typing import List, Sequence, Tuple

import numpy as np

from .inference_gtcrn import (cut_slices, example_audio, normalise_audio, output_length, read_wav_int16, session_rates, write_wav_float32,
                              write_wav_int16)

FBANK_WINDOW, FRAME_SHIFT = 640, 320


def _meta(sess, key, kind, default):
    return sess.metadata.get(key, kind, default)


def fold_window(sess) -> int:
    """Model-rate samples per window of a folded export, 0 for an unfolded one."""
    return int(_meta(sess, "fold_window_length", "int", 0)) if _meta(sess, "use_batch_fold", "bool", False) else 0


def slice_signal(sess, audio: np.ndarray, rng=None) -> np.ndarray:
    """(n,) int16 -> (slices, in_len): zero padding when folded, seeded noise tail otherwise."""
    rows, _ = cut_slices(audio, sess.in_len, sess.in_len, tail_pad="zeros" if fold_window(sess) else "noise", rng=rng, out_stride=False)
    return rows


def valid_frames(samples: int, window: int = 0) -> int:
    """Mask frames that lie wholly inside the first ``samples`` model-rate samples of a slice; ``window`` > 0: a folded slice, counted window by window."""
    if window <= 0:
        return 0 if samples < FBANK_WINDOW else 1 + (samples - FBANK_WINDOW) // FRAME_SHIFT
    n = 0
    while samples > 0:
        n += valid_frames(min(samples, window))
        samples -= window
    return n


def frame_times(start_seconds: float, samples: int, window: int = 0, rate: int = 16000) -> np.ndarray:
    """Start time of every valid frame of a slice that begins at ``start_seconds``."""
    if window <= 0:
        return start_seconds + np.arange(valid_frames(samples)) * (FRAME_SHIFT / rate)
    out: List[float] = []
    w0 = 0
    while w0 < samples:
        n = valid_frames(min(window, samples - w0))
        out.extend(start_seconds + w0 / rate + np.arange(n) * (FRAME_SHIFT / rate))
        w0 += window
    return np.asarray(out, np.float64)


def silence_states(prob: Sequence[float], speaking_score: float, silence_score: float, look_ahead: int) -> List[bool]:
    prob = np.asarray(prob)
    silent, states = True, []
    full = max(0, len(prob) - look_ahead)
    for i in range(len(prob)):
        p = prob[i]
        if i < full:
            ahead = prob[i:i + look_ahead]
            if silent:
                silent = not (p >= speaking_score and np.mean(ahead >= speaking_score) >= speaking_score)
            elif p <= silence_score:
                silent = bool(np.mean(ahead <= silence_score) > silence_score)
            else:
                silent = False
        else:
            silent = bool(p < speaking_score) if silent else bool(p <= silence_score)
        states.append(bool(silent))
    return states


def segments(states: Sequence[bool], frame_duration: float, times=None) -> List[Tuple[float, float]]:
    times = np.arange(len(states), dtype=np.float64) * frame_duration if times is None else np.asarray(times, np.float64)
    if len(times) != len(states):
        raise ValueError(f"{len(times)} frame times for {len(states)} VAD states")
    out, start = [], None
    for i, silent in enumerate(states):
        if silent and start is not None:
            out.append((float(start), float(times[i] + frame_duration)))
            start = None
        elif not silent and start is None:
            start = times[i]
    if start is not None:
        out.append((float(start), float(times[-1] + frame_duration)))
    return out


def fuse_segments(segs: Sequence[Tuple[float, float]], fusion_threshold: float, min_duration: float) -> List[Tuple[float, float]]:
    out: List[Tuple[float, float]] = []
    for a, b in segs:
        if b - a < min_duration:
            continue
        if out and a - out[-1][1] <= fusion_threshold:
            out[-1] = (out[-1][0], b)
        else:
            out.append((a, b))
    return out


def format_time(seconds: float) -> str:
    ms = round(float(seconds) * 1000)
    s, ms = divmod(ms, 1000)
    return f"{s // 3600:02}:{(s % 3600) // 60:02}:{s % 60:02}.{ms:03}"


def timestamps(sess, vad_rows: np.ndarray, n_samples: int) -> List[Tuple[float, float]]:
    """vad_rows (slices, frames per slice) of the slices of an ``n_samples`` signal -> the fused speech segments in seconds."""
    in_rate, _ = session_rates(sess)
    in_rate = in_rate or 16000
    window = fold_window(sess)
    prob, times = [], []
    for k, row in enumerate(vad_rows):
        start = k * sess.in_len
        valid = max(0, min(sess.in_len, n_samples - start))
        model_samples = int(round(valid * 16000 / in_rate))
        n = valid_frames(model_samples, window)
        prob.extend(row[:n])
        times.extend(frame_times(start / in_rate, model_samples, window))
    shift = float(_meta(sess, "output_frame_shift_seconds", "float", FRAME_SHIFT / 16000.0))
    look = max(1, int(float(_meta(sess, "look_ahead_seconds", "float", 0.3)) / shift))
    states = silence_states(np.asarray(prob, np.float32), float(_meta(sess, "speaking_score", "float", 0.5)), float(_meta(sess, "silence_score", "float", 0.5)), look)
    return fuse_segments(segments(states, shift, np.asarray(times, np.float64)), float(_meta(sess, "fusion_threshold_seconds", "float", 0.3)),
                         float(_meta(sess, "min_speech_duration_seconds", "float", 0.2)))


def process(sess, near: np.ndarray, far: np.ndarray, normalize: bool = False, rng=None):
    """Whole signals -> (the echo-cancelled signal at the handle's output rate, the speech segments or None)."""
    if getattr(sess, "in_dtype", np.int16) != np.int16:
        raise ValueError("inference_dfsmn_aec: the driver feeds int16 PCM; export the model with an INT16 input")
    in_rate, out_rate = session_rates(sess)
    near, far = normalise_audio(near, normalize), normalise_audio(far, normalize)
    n = min(len(near), len(far))
    rng = rng if rng is not None else np.random.default_rng()
    near_s, far_s = slice_signal(sess, near[:n], rng), slice_signal(sess, far[:n], rng)
    out = sess.run(None, {"near_end_audio": near_s[:, None], "far_end_audio": far_s[:, None]})
    audio = np.ascontiguousarray(out[0][:, 0].reshape(-1)[:output_length(n, in_rate, out_rate)])
    stamps = timestamps(sess, out[1].reshape(len(near_s), -1), n) if getattr(sess, "_vad", False) else None
    return audio, stamps


def process_streaming(sess, near: np.ndarray, far: np.ndarray, frames_per_push: int = 62, normalize: bool = False) -> np.ndarray:
    """Whole int16 signals -> the echo-cancelled int16 signal through ONE stateful stream (``--stream N``).

    :func:`process` -- like the reference's driver -- restarts the Kalman filter and zeroes the mask network's memory in every window of the graph's static
    length.  Here both are carried on the device from push to push, so the canceller keeps the echo path it has learnt over the whole file; the result is what the
    reference's unfolded graph gives on the whole (padded) file in one call.  Audio only: a stream returns no speech probabilities.

    Both signals are trimmed to the shorter one and zero-padded at the end to a multiple of 1280 samples (whole hops of 256 AND a length the reference's static
    export accepts, a multiple of 320: the flush is defined only there), and pushed in pushes of the largest number of hops that divides the padded hop count and
    does not exceed ``frames_per_push``.  The stream's latency (1344 samples: the first ``delay`` samples of pushes + flush are dropped) is removed again and the
    output cut to the input length.  The session's own static length, folded or not, does not matter."""
    from .session import StreamingSession
    if getattr(sess, "in_dtype", np.int16) != np.int16 or getattr(sess, "out_dtype", np.int16) != np.int16:
        raise ValueError("inference_dfsmn_aec: a stream takes and returns int16 PCM; export the model with INT16 audio tensors")
    if int(frames_per_push) < 1:
        raise ValueError("inference_dfsmn_aec: frames_per_push must be at least 1")
    near, far = normalise_audio(near, normalize), normalise_audio(far, normalize)
    n = min(len(near), len(far))
    hops = 5 * max(1, -(-n // 1280))
    per_push = max(d for d in range(1, min(int(frames_per_push), hops) + 1) if hops % d == 0)
    P, n_push = per_push * 256, hops // per_push
    rows = np.zeros((1, 2, hops * 256), np.int16)
    rows[0, 0, :n], rows[0, 1, :n] = near[:n], far[:n]                 # this family's order: near end, far end
    with StreamingSession(sess, 1, per_push) as st:
        parts = [st.push(rows[:, :, i * P:(i + 1) * P]) for i in range(n_push)]
        parts.append(st.flush())
        delay = st.delay
    return np.ascontiguousarray(np.concatenate(parts, axis=1)[0, delay:delay + n])


def write_timestamps(stamps, directory, in_rate: int = 16000) -> None:
    directory = Path(directory)
    with open(directory / "timestamps_second.txt", "w", encoding="utf-8") as f:
        for a, b in stamps:
            f.write(f"{format_time(a)} --> {format_time(b)}\n")
    with open(directory / "timestamps_indices.txt", "w", encoding="utf-8") as f:
        for a, b in stamps:
            f.write(f"{round(a * in_rate)} --> {round(b * in_rate)}\n")


def main(sess, near_path=None, far_path=None, out_path: str = "aec.wav", normalize: bool = False, rng=None, stream: int = 0):
    in_rate, out_rate = session_rates(sess)
    near = read_wav_int16(near_path or example_audio("aec", "nearend_mic1.wav"), in_rate)
    far = read_wav_int16(far_path or example_audio("aec", "farend_speech1.wav"), in_rate)
    y, stamps = (process_streaming(sess, near, far, stream, normalize), None) if stream else process(sess, near, far, normalize, rng)
    if y.dtype == np.int16:
        write_wav_int16(out_path, y, out_rate)
    else:
        write_wav_float32(out_path, y.astype(np.float32), out_rate)
    if stamps is not None:
        write_timestamps(stamps, Path(out_path).resolve().parent, in_rate or 16000)
    return y, stamps


if __name__ == "__main__":
    from .session import InferenceSession
    argv, stream = list(sys.argv[1:]), 0
    if "--stream" in argv:                     # --stream N: one stateful stream, pushes of at most N hops (process_streaming)
        i = argv.index("--stream")
        stream = int(argv[i + 1])
        del argv[i:i + 2]
    args = [a for a in argv if not a.startswith("--")]
    if len(args) not in (1, 4):
        print(__doc__)
        raise SystemExit(2)
    s = InferenceSession(args[0])
    paths = args[1:] if len(args) == 4 else (None, None, "aec.wav")
    main(s, *paths, normalize="--normalize" in sys.argv, stream=stream)
    print(f"AEC done: {paths[2]}")
