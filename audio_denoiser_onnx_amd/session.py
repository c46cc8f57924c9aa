"""``InferenceSession`` — host-side mirror of the object the reference drives per slice.

The reference's inference scripts talk to ``onnxruntime.InferenceSession`` (GTCRN/Inference_GTCRN_ONNX.py:237,
262-267, 307-317): ``get_inputs()/get_outputs()`` metadata, pre-bound buffers, one ``run_with_iobinding`` per
slice.  This class exposes the same surface over libade's C ABI (include/ade.h); the compute is the hand-written
gfx950 path and nothing else — construction fails loudly without the built library or a GPU.

Differences from ORT that are the point of this engine: ``run`` accepts ``(B, 1, L)`` and treats the B rows as
B independent reference calls executed as one batch, and :meth:`run_device` takes device tensors.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from .metadata import MetadataReader, load_runtime_metadata, validate_audio_metadata

INPUT_NAME = "noisy_audio"       # GTCRN/Export_GTCRN.py:768
OUTPUT_NAME = "denoised_audio"   # GTCRN/Export_GTCRN.py:769
AEC_INPUT_NAMES = ("far_end_audio", "near_end_audio")   # NKF_AEC/Export_NKF_AEC.py:524-525
AEC_OUTPUT_NAME = "aec_audio"
DFSMN_AEC_INPUT_NAMES = ("near_end_audio", "far_end_audio")   # DFSMN_AEC/Export_DFSMN_AEC.py:1519, SDAEC/Export_SDAEC.py:501, Deep_Echo_AEC/Export_Deep_Echo.py:490: the near end first
VAD_OUTPUT_NAME = "vad_results"


class NodeArg:
    """What ``session.get_inputs()[i]`` looks like to the reference driver (name / shape / type)."""

    def __init__(self, name: str, shape: Sequence[int], type_: str = "tensor(int16)"):
        self.name, self.shape, self.type = name, list(shape), type_

    def __repr__(self):
        return f"NodeArg(name={self.name!r}, type={self.type!r}, shape={self.shape})"


class ModelMeta:
    def __init__(self, custom_metadata_map: Dict[str, str]):
        self.custom_metadata_map = dict(custom_metadata_map)


def resolve_model_path(path) -> Path:
    """A model directory resolves to its single ``*.adew`` blob (the reference resolves a dir to ``GTCRN.onnx``,
    Inference_GTCRN_ONNX.py:26-32)."""
    p = Path(path).expanduser()
    if p.is_dir():
        blobs = sorted(p.glob("*.adew"))
        if len(blobs) != 1:
            raise FileNotFoundError(f"expected exactly one .adew weight blob in {p}, found {len(blobs)}")
        return blobs[0]
    if not p.exists():
        raise FileNotFoundError(f"model file not found: {p}")
    return p


class InferenceSession:
    def __init__(self, model_path=None, *, weights: Optional[bytes] = None, metadata: Optional[Dict[str, str]] = None,
                 device_id: int = 0, library: Optional[_lib.AdeLibrary] = None):
        """``model_path``: ``<name>.adew`` (or its directory) with ``<name>_Metadata.json`` beside it; or pass
        ``weights`` + ``metadata`` directly.  ``library`` defaults to the in-tree gfx950 build."""
        self._lib = library or _lib.get_library()
        self._h = C.c_void_p()
        self._in_flight = {}            # ticket -> (pcm, out, f32): the buffers of submissions that have not been waited for
        if model_path is not None:
            model_path = resolve_model_path(model_path)
            reader = load_runtime_metadata(model_path)          # FileNotFoundError / KeyError like the reference
            with open(model_path, "rb") as f:
                weights = f.read()
        else:
            if weights is None or metadata is None:
                raise ValueError("pass either model_path or both weights and metadata")
            reader = MetadataReader(metadata)
        self.metadata = reader
        blob = bytes(weights)                            # libade parses and uploads it inside ade_create; nothing keeps it afterwards
        st = self._lib.c.ade_create(reader.to_json().encode(), blob, len(blob), int(device_id), C.byref(self._h))
        del blob, weights
        self._lib.check(st, None)
        io = _lib.IoDesc()
        self._lib.check(self._lib.c.ade_get_io(self._h, C.byref(io)), self._h)
        self.in_len, self.out_len, self.frames = io.in_len, io.out_len, io.frames
        self.out_channels = io.out_channels
        self.channels = io.in_channels                    # 1 (GTCRN, DFSMN) or 2 (Mel-Band-Roformer stereo)
        self.n_outputs = io.n_outputs                     # 1, or 2 for MossFormer2-SS ("separated_0", "separated_1")
        self.row_in, self.row_out = io.in_channels * io.in_len, io.n_outputs * io.out_channels * io.out_len   # one batch item, planar
        self.sample_rate = io.model_sample_rate
        self.in_sample_rate, self.out_sample_rate = io.in_sample_rate, io.out_sample_rate
        self.device_id = io.device
        in_name = "mix_audio" if reader.string("model_family", "") == "mossformer2_ss" else INPUT_NAME        # :688
        # audio tensor dtypes of the export (Export_GTCRN.py:47-48, 757-760): INT16 PCM, or normalised F32 / F16 (an F16 tensor crosses libade's ABI as IEEE half: ade_process_f16)
        self.in_dtype = {"INT16": np.int16, "F32": np.float32, "F16": np.float16}[reader.string("input_audio_dtype", "INT16")]
        self.out_dtype = {"INT16": np.int16, "F32": np.float32, "F16": np.float16}[reader.string("output_audio_dtype", "INT16")]
        tname = {np.int16: "tensor(int16)", np.float32: "tensor(float)", np.float16: "tensor(float16)"}
        family = reader.string("model_family", "")
        self._aec = family in ("nkf_aec", "dfsmn_aec", "sdaec", "deep_echo")
        self._aec_near_first = family in ("dfsmn_aec", "sdaec", "deep_echo")      # the order of the engine's two planar rows, and of a stream's
        # DFSMN-AEC's optional second output: one speech probability per mask frame of every window of the call, float32 (B * windows * frames,) (:1317-1319, :1520)
        self._vad = family == "dfsmn_aec" and bool(reader.optional_bool("output_vad_result", False))
        if self._aec:      # two graph inputs, one channel each: channels 0 and 1 of the engine's planar rows (Export_NKF_AEC.py:524-525: far end, near end; DFSMN-AEC, SDAEC and Deep Echo: near end, far end)
            self._inputs = [NodeArg(n, [1, 1, io.in_len], tname[self.in_dtype]) for n in (DFSMN_AEC_INPUT_NAMES if self._aec_near_first else AEC_INPUT_NAMES)]
        else:
            self._inputs = [NodeArg(in_name, [1, io.in_channels, io.in_len], tname[self.in_dtype])]
        out_names = ([AEC_OUTPUT_NAME] if self._aec else [OUTPUT_NAME]) if io.n_outputs == 1 else [f"separated_{i}" for i in range(io.n_outputs)]   # Export_MossFormer2_SS_16K.py:689-690
        self._outputs = [NodeArg(name, [1, io.out_channels, io.out_len], tname[self.out_dtype]) for name in out_names]
        if self._vad:
            windows = reader.optional_int("export_audio_length", io.in_len) // reader.optional_int("fold_window_length", io.in_len) if reader.optional_bool("use_batch_fold", False) else 1
            self.vad_frames = windows * io.frames                # per batch item
            self._outputs.append(NodeArg(VAD_OUTPUT_NAME, [self.vad_frames], "tensor(float)"))
        self._planar_name = "far_end_near_end_audio"            # (internal: the interleaved two-input tensor of an AEC call)
        self._inputs_meta, self._outputs_meta = self._inputs, self._outputs   # names the reference script touches
        validate_audio_metadata(reader, self)

    # -- ORT-shaped surface --------------------------------------------------------------------------------
    def get_inputs(self) -> List[NodeArg]:
        return self._inputs

    def get_outputs(self) -> List[NodeArg]:
        return self._outputs

    def get_modelmeta(self) -> ModelMeta:
        return ModelMeta(self.metadata.metadata)

    def get_providers(self) -> List[str]:
        return ["AdeMI355XExecutionProvider"]

    def run(self, output_names, input_feed: Dict[str, np.ndarray], return_f32: bool = False):
        """``session.run(None, {"noisy_audio": int16 (B,1,L)})`` -> ``[int16 (B,1,L_out)]`` (+ fp32 pre-PCM tap).
        NKF-AEC: ``{"far_end_audio": (B,1,L), "near_end_audio": (B,1,L)}`` -> ``[aec_audio (B,1,L_out)]``.
        SDAEC, Deep Echo: ``{"near_end_audio": ..., "far_end_audio": ...}`` -> ``[aec_audio]``.
        DFSMN-AEC: ``{"near_end_audio": ..., "far_end_audio": ...}`` -> ``[aec_audio]``, and with ``output_vad_result`` a last element ``vad_results`` float32 (B * frames,)."""
        out = self._run_audio(input_feed, return_f32)
        if self._vad:
            batch = int(np.asarray(input_feed[self._inputs[0].name]).shape[0])
            out.append(self.tap(VAD_OUTPUT_NAME, batch * self.vad_frames).copy())
        return out

    def _run_audio(self, input_feed: Dict[str, np.ndarray], return_f32: bool = False):
        if self._aec:
            parts = []
            for arg in self._inputs:
                if arg.name not in input_feed:
                    raise KeyError(f"missing input {arg.name!r}")
                a = np.asarray(input_feed[arg.name])
                if a.ndim != 3 or a.shape[1] != 1 or a.shape[2] != self.in_len:
                    raise ValueError(f"{arg.name} must have shape (B, 1, {self.in_len}), got {a.shape}")
                parts.append(a)
            if parts[0].shape[0] != parts[1].shape[0] or parts[0].dtype != parts[1].dtype:
                raise ValueError("far_end_audio and near_end_audio must have the same batch size and dtype")
            input_feed = {self._planar_name: np.concatenate(parts, axis=1)}      # planar (B, 2, L), in the order of the graph inputs
        name = self._planar_name if self._aec else self._inputs[0].name
        if name not in input_feed:
            raise KeyError(f"missing input {name!r}")
        x = np.asarray(input_feed[name])
        if x.dtype != self.in_dtype:
            raise ValueError(f"{INPUT_NAME} must be {np.dtype(self.in_dtype).name}, got {x.dtype}")
        if x.ndim != 3 or x.shape[1] != self.channels or x.shape[2] != self.in_len:
            raise ValueError(f"{INPUT_NAME} must have shape (B, {self.channels}, {self.in_len}), got {x.shape}")
        float_out = self.out_dtype != np.int16
        if (self.in_dtype == np.float16 or self.out_dtype == np.float16) and self.in_dtype != np.float32 and not return_f32:
            # a float16 graph tensor on either side: the half entry (the engine widens / narrows on the device)
            pcm, f16 = self.process_f16(x.reshape(x.shape[0], self.row_in), want_pcm=not float_out, want_f16=float_out)
            if float_out:
                f16 = f16.reshape(-1, self.n_outputs, self.out_channels, self.out_len)
                return [np.ascontiguousarray(f16[:, i]) for i in range(self.n_outputs)]
            pcm = pcm.reshape(-1, self.n_outputs, self.out_channels, self.out_len)
            return [np.ascontiguousarray(pcm[:, i]) for i in range(self.n_outputs)]
        if self.in_dtype == np.int16:
            pcm, f32 = self.process(x.reshape(x.shape[0], self.row_in), want_f32=return_f32 or float_out)
        else:
            pcm, f32 = self.process_f32(x.reshape(x.shape[0], self.row_in).astype(np.float32, copy=False), want_pcm=not float_out, want_f32=return_f32 or float_out)
        if float_out:        # the export's F32 / F16 output: the waveform without the PCM scale and clamp (Export_GTCRN.py:689-693)
            f32 = f32.reshape(-1, self.n_outputs, self.out_channels, self.out_len)
            return [np.ascontiguousarray(f32[:, i]).astype(self.out_dtype, copy=False) for i in range(self.n_outputs)]
        pcm = pcm.reshape(-1, self.n_outputs, self.out_channels, self.out_len)
        out = [np.ascontiguousarray(pcm[:, i]) for i in range(self.n_outputs)]               # one array per graph output
        if return_f32:
            f32 = f32.reshape(-1, self.n_outputs, self.out_channels, self.out_len)
            out += [np.ascontiguousarray(f32[:, i]) for i in range(self.n_outputs)]
        return out

    # -- batch call on host buffers ---------------------------------------------------------------------------
    def process(self, pcm: np.ndarray, want_f32: bool = False):
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        if pcm.ndim != 2 or pcm.shape[1] != self.row_in:
            raise ValueError(f"expected int16 (B, {self.row_in}), got {pcm.shape}")
        B = pcm.shape[0]
        out = np.empty((B, self.row_out), np.int16)
        f32 = np.empty((B, self.row_out), np.float32) if want_f32 else None
        st = self._lib.c.ade_process(self._h, pcm.ctypes.data, B, out.ctypes.data, f32.ctypes.data if want_f32 else None)
        self._lib.check(st, self._h)
        return out, f32

    def process_f16(self, x: np.ndarray, want_pcm: bool = True, want_f16: bool = True):
        """IEEE-half audio tensors (``ade_process_f16``): x (B, row_in) in the handle's input dtype -- float16 for a float-input manifest, int16 PCM otherwise --
        -> (int16 PCM or None, float16 waveform or None)."""
        want = np.int16 if self.in_dtype == np.int16 else np.float16
        x = np.ascontiguousarray(x, dtype=want)
        if x.ndim != 2 or x.shape[1] != self.row_in:
            raise ValueError(f"input must have shape (B, {self.row_in}), got {x.shape}")
        if not (want_pcm or want_f16):
            raise ValueError("nothing to compute")
        B = x.shape[0]
        out = np.empty((B, self.row_out), np.int16) if want_pcm else None
        f16 = np.empty((B, self.row_out), np.float16) if want_f16 else None
        st = self._lib.c.ade_process_f16(self._h, x.ctypes.data, B, out.ctypes.data if want_pcm else None, f16.ctypes.data if want_f16 else None)
        self._lib.check(st, self._h)
        return out, f16

    def process_f32(self, x: np.ndarray, want_pcm: bool = True, want_f32: bool = True):
        """fp32 audio in (input_audio_dtype F32 / F16; ``ade_process_f32``): normalised samples (B, row_in) -> (int16 PCM or None, fp32 waveform or None)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.row_in:
            raise ValueError(f"expected float32 (B, {self.row_in}), got {x.shape}")
        if not (want_pcm or want_f32):
            raise ValueError("ask for at least one output")
        B = x.shape[0]
        out = np.empty((B, self.row_out), np.int16) if want_pcm else None
        f32 = np.empty((B, self.row_out), np.float32) if want_f32 else None
        st = self._lib.c.ade_process_f32(self._h, x.ctypes.data, B, out.ctypes.data if want_pcm else None, f32.ctypes.data if want_f32 else None)
        self._lib.check(st, self._h)
        return out, f32

    # -- batch call on device buffers (torch tensors on this session's GPU) ------------------------------------
    def process_into(self, pcm: np.ndarray, out: np.ndarray, f32: Optional[np.ndarray] = None) -> None:
        """``process`` on caller-owned, re-used buffers -- the reference's io_binding pattern (Inference_GTCRN_ONNX.py:307-317): nothing is
        allocated per call.  Page-locked buffers (hipHostMalloc / a pinned torch tensor's ``.numpy()``) make both copies plain DMA."""
        B = pcm.shape[0]
        if pcm.dtype != np.int16 or out.dtype != np.int16 or pcm.shape != (B, self.row_in) or out.shape != (B, self.row_out):
            raise ValueError(f"expected int16 (B, {self.row_in}) -> int16 (B, {self.row_out})")
        if not pcm.flags.c_contiguous or not out.flags.c_contiguous or (f32 is not None and not f32.flags.c_contiguous):
            raise ValueError("buffers must be C-contiguous")
        if f32 is not None and (f32.dtype != np.float32 or f32.shape != out.shape):
            raise ValueError("f32 must be float32 with the shape of out")
        st = self._lib.c.ade_process(self._h, pcm.ctypes.data, B, out.ctypes.data, f32.ctypes.data if f32 is not None else None)
        self._lib.check(st, self._h)

    # -- the pipelined form (ade_submit / ade_wait): a file of many batches overlaps copy-in (k + 1), kernels (k) and copy-out (k - 1) -------------------------------
    def submit(self, pcm: np.ndarray, out: np.ndarray, f32: Optional[np.ndarray] = None) -> int:
        """Enqueue one ``process_into`` call without waiting; returns the ticket ``wait`` takes.  The three buffers must stay alive and untouched until that
        ``wait`` -- this object keeps references to them meanwhile.  At most ``pipe_depth`` (option, default 3) tickets between waits."""
        B = pcm.shape[0]
        if pcm.dtype != np.int16 or out.dtype != np.int16 or pcm.shape != (B, self.row_in) or out.shape != (B, self.row_out):
            raise ValueError(f"expected int16 (B, {self.row_in}) -> int16 (B, {self.row_out})")
        if not pcm.flags.c_contiguous or not out.flags.c_contiguous or (f32 is not None and (not f32.flags.c_contiguous or f32.dtype != np.float32 or f32.shape != out.shape)):
            raise ValueError("buffers must be C-contiguous (f32: float32 with the shape of out)")
        t = C.c_uint64(0)
        st = self._lib.c.ade_submit(self._h, pcm.ctypes.data, B, out.ctypes.data, f32.ctypes.data if f32 is not None else None, C.byref(t))
        self._lib.check(st, self._h)
        self._in_flight[int(t.value)] = (pcm, out, f32)
        return int(t.value)

    def wait(self, ticket: int):
        """Block until the submission is complete; returns its (out, f32) buffers.  Raises what ``process`` would have raised for that call."""
        st = self._lib.c.ade_wait(self._h, C.c_uint64(int(ticket)))
        bufs = self._in_flight.pop(int(ticket), None)
        self._lib.check(st, self._h)
        return (bufs[1], bufs[2]) if bufs else (None, None)

    def run_device(self, d_in, d_out, d_f32=None, stream: Optional[int] = None) -> None:
        """``d_in`` int16 (B, L) / ``d_out`` int16 (B, L_out) CUDA(HIP) tensors; enqueues on ``stream`` (a raw
        hipStream_t handle, e.g. ``torch.cuda.current_stream().cuda_stream``) or runs synchronously when None.
        A model whose input tensor is float (input_audio_dtype F32 / F16) takes a float32 ``d_in`` (``ade_process_device_f32``); ``d_out`` may be None when only the
        float waveform ``d_f32`` is wanted (a float OUTPUT model)."""
        B = int(d_in.shape[0])
        if tuple(d_in.shape) != (B, self.row_in) or (d_out is not None and tuple(d_out.shape) != (B, self.row_out)):
            raise ValueError("device tensors must be (B, channels * in_len) -> (B, channels * out_len)")
        if not d_in.is_contiguous() or (d_out is not None and not d_out.is_contiguous()):
            raise ValueError("device tensors must be contiguous")
        float_in = self.in_dtype != np.int16
        if str(d_in.dtype) != ("torch.float32" if float_in else "torch.int16") or (d_out is not None and str(d_out.dtype) != "torch.int16"):
            raise ValueError(f"d_in must be {'float32' if float_in else 'int16'} for this model, d_out int16")
        if d_out is None and d_f32 is None:
            raise ValueError("ask for at least one output")
        f32_ptr = None
        if d_f32 is not None:
            if tuple(d_f32.shape) != (B, self.row_out) or not d_f32.is_contiguous() or str(d_f32.dtype) != "torch.float32":
                raise ValueError("d_f32 must be a contiguous (B, channels * out_len) float32 tensor")
            f32_ptr = C.c_void_p(d_f32.data_ptr())
        fn = self._lib.c.ade_process_device_f32 if float_in else self._lib.c.ade_process_device
        st = fn(self._h, C.c_void_p(d_in.data_ptr()), B, C.c_void_p(d_out.data_ptr()) if d_out is not None else None, f32_ptr,
                C.c_void_p(stream) if stream else None)
        self._lib.check(st, self._h)

    def reserve(self, batch: int) -> None:
        self._lib.check(self._lib.c.ade_reserve(self._h, int(batch)), self._h)

    def set_option(self, key: str, value: str) -> None:
        self._lib.check(self._lib.c.ade_set_option(self._h, key.encode(), str(value).encode()), self._h)

    # -- parity / timing taps ---------------------------------------------------------------------------------
    def tap(self, name: str, count: int) -> np.ndarray:
        buf = np.empty(int(count), np.float32)
        n = C.c_size_t()
        self._lib.check(self._lib.c.ade_debug_tap(self._h, name.encode(), buf.ctypes.data, buf.size, C.byref(n)), self._h)
        return buf[: n.value]

    def profile(self, enable) -> None:
        """0/False: off; 1/True: one kernel per stage (+ phase clocks); 2: the shipped launch sequence timed as launched;
        3: the single-launch kernel's phase-clock build (tap ``phase_clock`` with 640 slots)."""
        self._lib.check(self._lib.c.ade_profile_last(self._h, int(enable)), self._h)

    def kernel_times(self) -> Dict[str, Dict[str, float]]:
        out = {}
        for i in range(self._lib.c.ade_kernel_count(self._h)):
            ms, n = C.c_float(), C.c_int()
            self._lib.check(self._lib.c.ade_kernel_ms(self._h, i, C.byref(ms), C.byref(n)), self._h)
            out[self._lib.c.ade_kernel_name(self._h, i).decode()] = {"ms": float(ms.value), "launches": int(n.value)}
        return out

    # -- STFT_Process operator on device tensors ---------------------------------------------------------------
    def stft_device(self, d_x, d_spec, stream: Optional[int] = None) -> None:
        B, L = int(d_x.shape[0]), int(d_x.shape[1])
        st = self._lib.c.ade_stft_forward(self._h, C.c_void_p(d_x.data_ptr()), B, L, C.c_void_p(d_spec.data_ptr()),
                                          C.c_void_p(stream) if stream else None)
        self._lib.check(st, self._h)

    def istft_device(self, d_spec, d_y, stream: Optional[int] = None) -> None:
        B, T = int(d_spec.shape[0]), int(d_spec.shape[2])
        st = self._lib.c.ade_istft_forward(self._h, C.c_void_p(d_spec.data_ptr()), B, T, C.c_void_p(d_y.data_ptr()),
                                           C.c_void_p(stream) if stream else None)
        self._lib.check(st, self._h)

    def close(self) -> None:
        for ref in list(getattr(self, "_streams", ())):          # child streams first: they hold device state of this engine
            child = ref()
            if child is not None:
                child.close()
        self._streams = []
        if getattr(self, "_h", None) and self._h:
            self._lib.c.ade_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class StreamingSession:
    """Stateful streaming over a GTCRN session (``ade_stream_*``, include/ade.h).

    ``n_streams`` independent audio streams advance together, ``frames_per_push`` hops (x 256 samples) at a time.  The STFT overlap,
    the causal-convolution histories and every GRU hidden state are carried on the device between pushes, so the concatenated outputs
    equal what the reference's graph computes on the whole signal in ONE call -- one hop (256 samples) later, the stream's first hop
    zero, and without the reference's whole-call DC removal (not causal).  The reference itself has no such mode: its driver calls a
    stateless graph per slice (Inference_GTCRN_ONNX.py:307-317).

    On an NKF-AEC session the stream carries the echo canceller itself -- the per-bin Kalman state, the last 768 samples of the far-end and the near-end
    signal and the ISTFT overlap -- so the filter keeps the echo path it has learnt across pushes.  ``in_channels`` is then 2 (far end, near end), ``push`` takes
    ``(n_streams, 2, samples_per_push)`` (or ``push_aec(far, near)``), and ``delay`` is 768 samples: the outputs equal the reference's graph on the whole signal
    in one call, 768 samples later.  ``delay`` is also the length of the flush; it is 256 for GTCRN.

    On a DFSMN-AEC session the stream carries both stages: the NKF back end's state as above, the near-end and ``temp_aec`` samples no mask frame has consumed yet,
    every layer's ``dilation * (lorder - 1)`` frames of memory history, the second half of the last synthesised frame and the final samples not yet due.
    ``in_channels`` is 2 in THIS family's order (near end, far end: the opposite of NKF-AEC; ``push_aec(far, near)`` stacks the two in the session's order
    either way) and ``delay`` is 1344 samples (84 ms): the outputs equal the reference's unfolded graph on the whole signal in one call, 1344 samples later,
    whatever the push size, bit for bit.  This family has no whole-call DC removal, so that holds for any input.  ``flush`` (1344 samples) ends the signal and
    needs a length the reference's static export accepts: the hops pushed a multiple of 5.  A stream returns audio only, also when the manifest has
    ``output_vad_result = 1``; folded and unfolded manifests stream alike (a stream does not use the window length).

    On a DFSMN session (48 kHz) a hop is 960 samples (``hop``, ``ade_stream_hop``), so ``samples_per_push = frames_per_push * 960``, and ``delay`` is 960 samples
    (20 ms).  The model is causal from end to end -- per-frame Kaldi mean, no centre padding, a memory that looks ``lorder - 1`` frames back -- so the stream carries
    the last 960 input samples, every layer's ``lorder - 1`` frames of memory history and the second half of the last synthesised frame, and pushes plus the flush
    equal the reference's one call on the whole signal, 960 samples later, whatever the push size, bit for bit.  ``flush`` (960 samples) needs at least two hops
    pushed.  Only unfolded int16 handles at 48 kHz in and out stream; the bits of ``process`` on the same signal are not promised (its kernels transform frames in
    pairs), both are within the family's gates of the oracle.

    On a UL-UNAS session (16 kHz) a hop is 256 samples and ``delay`` is 256 samples (16 ms), as for GTCRN: frame t is centred on sample 256 t and complete one hop
    later.  The model is causal from end to end, so the stream carries the last 257 input samples, the last ``kt - 1`` input frames of every (de)convolution with
    ``kt > 1``, the ten time-attention GRU states, the two inter-frame GRU states and the second half of the last synthesised frame, and pushes plus the flush equal
    the reference's one call on the whole signal, 256 samples later, whatever the push size, bit for bit.  ``2 <= frames_per_push <= 4096`` (the first push must
    hold the 257 samples the head reflection reads; 1 raises ValueError).  Only plain int16 handles at 16 kHz in and out stream (static or ``dynamic_axes``
    manifests; float tensors, other rates and batch-fold raise ``AdeUnsupportedError``); the bits of ``process`` on the same signal are not promised (its STFT
    transforms frames in pairs), both are within the family's gates of the oracle."""

    def __init__(self, session: InferenceSession, n_streams: int, frames_per_push: int):
        self._lib, self._session = session._lib, session
        self.n_streams, self.frames_per_push = int(n_streams), int(frames_per_push)
        self._h = C.c_void_p()
        self._lib.check(self._lib.c.ade_stream_create(session._h, self.n_streams, self.frames_per_push, C.byref(self._h)), session._h)
        delay, hop = C.c_int(0), C.c_int(0)
        self._lib.check(self._lib.c.ade_stream_delay(self._h, C.byref(delay)), session._h)
        self._lib.check(self._lib.c.ade_stream_hop(self._h, C.byref(hop)), session._h)
        self.delay, self.hop = int(delay.value), int(hop.value)
        self.samples_per_push = self.frames_per_push * self.hop
        self.in_channels = 2 if getattr(session, "_aec", False) else 1
        self._in_shape = (self.n_streams, 2, self.samples_per_push) if self.in_channels == 2 else (self.n_streams, self.samples_per_push)
        self._out_shape = (self.n_streams, self.samples_per_push)
        import weakref
        if not hasattr(session, "_streams"):
            session._streams = []
        session._streams.append(weakref.ref(self))

    def push(self, pcm: np.ndarray, want_f32: bool = False):
        """int16 (n_streams, samples_per_push) -> int16 of the same shape (+ fp32 pre-PCM waveform).
        NKF-AEC: int16 (n_streams, 2, samples_per_push), far end then near end -> int16 (n_streams, samples_per_push).
        DFSMN-AEC: the same shapes, near end then far end (the ABI's order for that family)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        if pcm.shape != self._in_shape:
            raise ValueError(f"expected int16 {self._in_shape}, got {pcm.shape}")
        out = np.empty(self._out_shape, np.int16)
        f32 = np.empty(self._out_shape, np.float32) if want_f32 else None
        st = self._lib.c.ade_stream_push(self._h, pcm.ctypes.data, out.ctypes.data, f32.ctypes.data if want_f32 else None)
        self._lib.check(st, self._session._h)
        return (out, f32) if want_f32 else out

    def push_aec(self, far: np.ndarray, near: np.ndarray, want_f32: bool = False):
        """NKF-AEC, DFSMN-AEC: two int16 (n_streams, samples_per_push) arrays, the far-end reference and the near-end microphone -> the echo-cancelled push.
        The two are stacked in the order of the session's family."""
        if self.in_channels != 2:
            raise ValueError("push_aec needs a stream of an NKF-AEC or DFSMN-AEC session")
        far, near = np.asarray(far), np.asarray(near)
        if far.shape != self._out_shape or near.shape != self._out_shape:
            raise ValueError(f"expected two int16 {self._out_shape} arrays, got {far.shape} and {near.shape}")
        rows = [near, far] if getattr(self._session, "_aec_near_first", False) else [far, near]
        return self.push(np.stack(rows, axis=1), want_f32)

    def push_device(self, d_in, d_out, d_f32=None, stream: Optional[int] = None) -> None:
        if tuple(d_in.shape) != self._in_shape or tuple(d_out.shape) != self._out_shape:
            raise ValueError(f"device tensors must be int16 {self._in_shape} in and {self._out_shape} out")
        st = self._lib.c.ade_stream_push_device(self._h, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()),
                                                C.c_void_p(d_f32.data_ptr()) if d_f32 is not None else None, C.c_void_p(stream) if stream else None)
        self._lib.check(st, self._session._h)

    def flush(self, want_f32: bool = False):
        """End of the signal: the last hop, int16 (n_streams, 256).  ``concatenate(pushes + [flush])[:, 256:]`` is then exactly the one-shot
        output of the whole signal.  ``reset()`` before pushing again.  In general the flush is ``delay`` samples long (768 for NKF-AEC, 1344 for DFSMN-AEC,
        960 for DFSMN, 256 for UL-UNAS)."""
        out = np.empty((self.n_streams, self.delay), np.int16)
        f32 = np.empty((self.n_streams, self.delay), np.float32) if want_f32 else None
        self._lib.check(self._lib.c.ade_stream_flush(self._h, out.ctypes.data, f32.ctypes.data if want_f32 else None), self._session._h)
        return (out, f32) if want_f32 else out

    def reset(self) -> None:
        self._lib.check(self._lib.c.ade_stream_reset(self._h), self._session._h)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.c.ade_stream_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
