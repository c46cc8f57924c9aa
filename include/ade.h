/*
 * ade.h — C ABI of libade, the MI355X (gfx950) engine for the reference's per-chunk denoise call.
 *
 * The reference (DakeQQ/Audio-Denoiser-ONNX) has no plugin / FFI layer: its hot-path boundary is the tensor
 * contract of the exported ONNX graph as driven by GTCRN/Inference_GTCRN_ONNX.py:307-317
 *     input  "noisy_audio"    int16 (1, 1, L)         (GTCRN/Export_GTCRN.py:768)
 *     output "denoised_audio" int16 (1, 1, L_out)     (GTCRN/Export_GTCRN.py:769)
 * with static shapes (DYNAMIC_AXES=False, Export_GTCRN.py:28), caller-owned pre-bound buffers re-used for every
 * slice (Inference_GTCRN_ONNX.py:307-311), synchronous single-threaded execution (:156), no state carried between
 * calls (zero GRU state, Export_GTCRN.py:339-352), plus the string metadata map of audio_onnx_metadata.py:8-26.
 * Each entry point below names the reference interface it replaces.  Plain pointers and sizes only.
 *
 * A batch of B rows is B INDEPENDENT reference calls (per-row DC mean, Export_GTCRN.py:647): row b of the output
 * equals what the reference's session.run returns for row b alone.
 */
#ifndef ADE_H
#define ADE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADE_ABI_VERSION 1

/* Status codes map 1:1 onto the exception classes the reference raises at this boundary
 * (audio_onnx_metadata.py:251-256 KeyError, :281-287 / :325-351 ValueError, :293-297 FileNotFoundError). */
typedef enum ade_status {
    ADE_OK = 0,
    ADE_ERR_NOT_FOUND = 1,      /* FileNotFoundError: weights / manifest carrier missing            */
    ADE_ERR_MISSING_KEY = 2,    /* KeyError: required metadata key or weight tensor absent          */
    ADE_ERR_SHAPE_MISMATCH = 3, /* ValueError: length / channel / tensor-shape disagreement         */
    ADE_ERR_BAD_VALUE = 4,      /* ValueError: malformed value (bad bool, bad blob, bad argument)   */
    ADE_ERR_DEVICE = 5,         /* no usable gfx950 device / HIP runtime failure (no CPU fallback)  */
    ADE_ERR_UNSUPPORTED = 6     /* model family or configuration this build does not implement      */
} ade_status;

typedef struct ade_engine* ade_handle;

/* What session.get_inputs()/get_outputs() report for the bound tensors (Inference_GTCRN_ONNX.py:262-267,276-277). */
typedef struct ade_io_desc {
    int32_t abi_version;
    int32_t in_channels;       /* 1; 2 for Mel-Band-Roformer stereo (Export_MelBandRoformer.py:714); 2 = (far end, near end) for nkf_aec, (near end, far end) for dfsmn_aec, sdaec and deep_echo */
    int32_t out_channels;      /* = in_channels, except H-GTCRN: 2 in, 1 out (Export_H_GTCRN.py:1181-1182)             */
    int32_t n_outputs;         /* 1 ("denoised_audio"); 2 for MossFormer2-SS ("separated_0/1", Export_MossFormer2_SS_16K.py:689) */
    int32_t in_len;            /* L: static input length in samples                      */
    int32_t out_len;           /* L_out = 256 * (L / 256): 15872 for L = 16000           */
    int32_t in_sample_rate;
    int32_t out_sample_rate;
    int32_t model_sample_rate;
    int32_t frames;            /* T = L / hop + 1 (Export_GTCRN.py:45)                    */
    int32_t max_batch;         /* rows the current workspace holds without re-allocation */
    int32_t device;            /* HIP device ordinal                                      */
} ade_io_desc;

/* Replaces onnxruntime.InferenceSession(model) + load_runtime_metadata/validate_audio_metadata
 * (Inference_GTCRN_ONNX.py:237-239).  `manifest_json`: flat JSON object of string values carrying the reference's
 * metadata key set (audio_onnx_metadata.py:161-203); `weights`: ADEWGT01 blob of the BN-folded tensors under the
 * reference's state_dict names.  `device` must be a gfx950 HIP device ordinal (there is no CPU mode).
 * The manifest key `model_family` selects the engine: "gtcrn" (GTCRN/Export_GTCRN.py), "dfsmn" (DFSMN/Export_DFSMN.py),
 * "mel_band_roformer" (Mel_Band_Roformer/Stereo/Export_MelBandRoformer.py), "mossformer2_ss"
 * (MossFormer2_SS_16K/Export_MossFormer2_SS_16K.py), "zipenhancer" (ZipEnhancer/Export_ZipEnhancer.py), "ul_unas"
 * (UL-UNAS/Export_UL_UNAS.py), "h_gtcrn" (H-GTCRN/Export_H_GTCRN.py: two microphones in, one channel out) or "nkf_aec"
 * (NKF_AEC/Export_NKF_AEC.py: far-end reference and near-end microphone in, the echo-cancelled microphone out) or "dfsmn_aec"
 * (DFSMN_AEC/Export_DFSMN_AEC.py with light_aec_model = NKF: near-end microphone FIRST, far-end reference second -- the opposite of
 * nkf_aec -- one channel out; a use_batch_fold manifest takes whole windows of fold_window_length samples per channel row; the per-frame
 * speech probability of output_vad_result is read with ade_debug_tap(h, "vad_results", ...), one float per mask frame of every window of
 * the last call; the optional key ade_dft_tables = "reference" (default) | "exact" selects the back end's transforms) or "sdaec"
 * (SDAEC/Export_SDAEC.py: near-end microphone first, far-end reference second, one channel out; static axes, 16 kHz in, any
 * input_audio_length >= 320, use_batch_fold windows of fold_window_length samples; no streams) or "deep_echo"
 * (Deep_Echo_AEC/Export_Deep_Echo.py: the same inputs, output and accepted manifests as sdaec, with echo_order = 10 in place of alpha_k;
 * the reference's dynamic_axes export is not built; no streams); the blob then
 * carries that export's fused buffers. */
ade_status ade_create(const char* manifest_json, const void* weights, size_t weights_nbytes, int device,
                      ade_handle* out);

/* Replaces session.get_inputs()/get_outputs() shape queries. */
ade_status ade_get_io(ade_handle h, ade_io_desc* desc);

/* Replaces one (or B) `_update_ortvalue + run_with_iobinding + output copy` rounds
 * (Inference_GTCRN_ONNX.py:314-317) on caller-owned HOST buffers.  Synchronous.
 *   in        [B][in_channels][in_len] int16 ;  out_pcm [B][n_outputs][out_channels][out_len] int16 (channel-planar) ;
 *   out_f32   optional, same layout as out_pcm, float: the waveform before the PCM tail (scale / clamp / truncate; parity tap). */
ade_status ade_process(ade_handle h, const int16_t* in, int batch, int16_t* out_pcm, float* out_f32);

/* Same call on DEVICE buffers (what a GPU execution provider's io-binding does, Inference_GTCRN_ONNX.py:69-92,
 * 193-198): enqueues on `hip_stream` (a hipStream_t, NULL = the engine's own stream) and returns without
 * synchronising when a stream is given. */
ade_status ade_process_device(ade_handle h, const int16_t* d_in, int batch, int16_t* d_out_pcm, float* d_out_f32,
                              void* hip_stream);

/* The same call PIPELINED: what the reference's driver does around its session is a LOOP of runs over the slices of a file (Inference_GTCRN_ONNX.py:314-333,
 * timed as a whole, :323-343).  ade_submit enqueues one ade_process call -- copy-in, kernels, copy-out on three streams tied by events -- and returns a ticket
 * without waiting; ade_wait(ticket) blocks until that call's output is in the caller's buffers and returns ITS status (a time-out of its launch included).
 * Up to `pipe_depth` (option, 2..4, default 3) submissions are in flight: the copy engines move call k + 1 in and call k - 1 out under call k's kernels, so a
 * file of many batches runs at max(kernel, copies) per batch instead of their sum.  Rules: `in`, `out_pcm`, `out_f32` stay the caller's and must stay valid and
 * untouched from ade_submit until ade_wait of the same ticket (page-locked buffers are DMA'd directly, pageable ones go through the slot's page-locked staging);
 * tickets may be waited for in any order, each exactly once; submitting into a full ring completes its oldest submission first (its status still waits for
 * ade_wait).  Results are bit-identical to ade_process on the same rows.  int16 handles of every model family (float-input manifests: ade_process_f32). */
ade_status ade_submit(ade_handle h, const int16_t* in, int batch, int16_t* out_pcm, float* out_f32, uint64_t* ticket);
ade_status ade_wait(ade_handle h, uint64_t ticket);

/* fp32 audio IN (manifest input_audio_dtype "F32" or "F16": normalised samples, no 2^-15 scale -- GTCRN/Export_GTCRN.py:645-646; an F16 tensor crosses this ABI as
 * fp32, the graph computes in fp32 either way).  Every family: the sub-engine families run such handles through their resampling-edge kernels with the family's input gain
 * (each export script's own IN_AUDIO_DTYPE branch).  The outputs are the same pair as above: out_f32 is the export's F32 / F16 output
 * (no * 32767, no clamp, :680-693), out_pcm its INT16 output; either may be NULL. */
ade_status ade_process_f32(ade_handle h, const float* in, int batch, int16_t* out_pcm, float* out_f32);
ade_status ade_process_device_f32(ade_handle h, const float* d_in, int batch, int16_t* d_out_pcm, float* d_out_f32, void* hip_stream);

/* IEEE-half audio tensors at the boundary (manifest input_audio_dtype and / or output_audio_dtype "F16": `noisy_audio` / `denoised_audio` are float16 graph tensors,
 * GTCRN/Export_GTCRN.py:47-48, 645-646, 691-693; the graph itself computes in fp32 either way).  `in`: the input tensor in the handle's INPUT dtype -- half for an F16 / F32
 * input manifest (normalised samples, widened exactly), int16 PCM otherwise; out_f16: the export's float output rounded to half (`audio_out.to(torch.float16)`,
 * round to nearest even), out_pcm its INT16 output; either may be NULL.  Layouts as above. */
ade_status ade_process_f16(ade_handle h, const void* in, int batch, int16_t* out_pcm, uint16_t* out_f16);
ade_status ade_process_device_f16(ade_handle h, const void* d_in, int batch, int16_t* d_out_pcm, uint16_t* d_out_f16, void* hip_stream);

/* The stitch step of a multi-GPU job (chunks are dealt to the ranks in contiguous blocks, the only exchange is the final concatenation,
 * Inference_GTCRN_ONNX.py:326-332): all-gather this rank's `rows` output rows, d_local [rows][n_outputs * out_channels * out_len] int16, into
 * d_all [world * rows][...] on every rank over the CALLER's RCCL communicator (`nccl_comm` = its ncclComm_t), enqueued on `hip_stream` behind the
 * ade_process_device call that filled d_local -- one ncclAllGather of bytes (RCCL has no int16 type).  librccl is opened on first use; ADE_ERR_UNSUPPORTED when
 * it is not installed.  Ranks with fewer rows pad their block (the gathered array is then trimmed by the caller). */
ade_status ade_stitch_device(ade_handle h, const int16_t* d_local, int rows, int16_t* d_all, void* nccl_comm, void* hip_stream);

/* Grow the workspace so `batch` rows run without allocation inside the timed path. */
ade_status ade_reserve(ade_handle h, int batch);

/* Options: "graph" = "0"/"1" replay the launch sequence from a captured hipGraph (default 1); "fused" / "single_launch" = "0"/"1" GTCRN's per-chunk LDS-resident path,
 * as one launch; "geometry" = "auto"/"0"/"1"/"2" its workgroup geometry (0: one 1024-thread workgroup per chunk; 1: 512-thread workgroups that each own a run of at most 32
 * frames, two per CU; 2: 256-thread workgroups of at most 16 frames, four per CU -- the default where the frame count allows; identical bits in all three);
 * "stagger_us" (geometry 0), "seg_prio" = "0".."4" (base wave priority by segment; the recurrences always run at priority 3), "wave_swap": measurement knobs, see DESIGN.md.
 * "xwait_ms" = bound of one inter-workgroup wait of the segmented fused path in milliseconds (default 200).  When a wait gives up, the CALL fails with ADE_ERR_DEVICE
 * (message: chunk, segment and the hand-off that did not arrive), no PCM is handed out, every hand-off flag is cleared and the next call starts clean; a launch on a
 * caller-provided stream is not synchronised by the engine, so its failure is reported by the NEXT call on the handle (or by the debug tap "xchg_error").
 * "xwait_retry" = "1" (default) / "0": ade_process (synchronous, host buffers) re-runs a call whose launch timed out ONCE on the path without hand-offs (whole chunks per
 * workgroup: the same bits) and returns ADE_OK -- a pre-empted or profiled GPU must not fail a valid call; ade_last_error then names the retry, the tap "xwait_retries" counts
 * them.  The device-pointer entries and "0" keep the failure.
 * "full_taps" = "0"/"1": 1 launches the debug build of the single-launch kernel, which stores every inter-stage tensor whole (the shipped kernel keeps channels 0-7 of
 * x_d0 / x_d1 / dp2 in LDS -- their only reader is the next block); set it before a call whose ade_debug_tap results are compared channel by channel.
 * "host_stream" = "0".."8": row groups ade_process streams a host batch THROUGH ONE LAUNCH in (GTCRN's fused path): every group's copy-in is followed by a 64 KB copy carrying
 * the call's epoch, the group's workgroups wait for it before their first PCM read, the group's last workgroup tells the host thread, which starts the group's copy-out -- the
 * copies of the other groups run under the launch's arithmetic (0 = per call: four groups from 128 rows; 1 = off; same bits as the device-resident launch).
 * "host_split" = "0".."8": with "host_stream" = "1": sub-batches ade_process cuts a host batch into instead, each with its own launch on its own stream (0 = per call: two
 * for 128 rows or more; 1 = never).  DESIGN.md section 6 has the measurements of both.
 * "xchg_withhold" = "0"/"1": TEST HOOK, makes the first workgroup of the next launches raise its hand-off flags where nobody polls (forces the time-out path). */
ade_status ade_set_option(ade_handle h, const char* key, const char* value);

/* Parity taps: copy a named intermediate of the LAST processed batch to host (engine-native layout, see
 * DESIGN.md "Data layout").  `count` = capacity of `out` in floats; `*written` = floats copied. */
ade_status ade_debug_tap(ade_handle h, const char* name, float* out, size_t count, size_t* written);

/* Timing tap: device time (ms) of the kernels launched by the last ade_process_device/ade_process call, measured with
 * hipEvents on the stream the kernels ran on.  ade_profile_last(h, 2): time the shipped launch sequence as launched
 * (one "gtcrn_chunk" kernel on the fused path); (h, 1): one kernel per network stage + in-kernel phase clocks;
 * (h, 3): the single-launch kernel's phase-clock build (debug tap "phase_clock", 640 slots); (h, 0): off.
 * Index results by ade_kernel_name(i). */
int ade_kernel_count(ade_handle h);
const char* ade_kernel_name(ade_handle h, int index);
ade_status ade_profile_last(ade_handle h, int enable);
ade_status ade_kernel_ms(ade_handle h, int index, float* total_ms, int* launches);

/* Message of the last failing call on this handle (or of ade_create when h == NULL). */
const char* ade_last_error(ade_handle h);

void ade_destroy(ade_handle h);

/* ---- STFT_Process operator (GTCRN/STFT_Process.py:129-341), FFT-based, on device buffers -----------------
 * stft_B packed:  x [B][L] float -> spec [B][2*(n_fft/2+1)][T]   (reference layout, re rows then im rows)
 * istft_B packed: spec [B][2F][T] -> y [B][hop*(T-1)] (center_pad=True, static_norm=True).
 * This build implements n_fft = 512, hop = 256, window "hann_sqrt", center pad, reflect. */
ade_status ade_stft_forward(ade_handle h, const float* d_x, int batch, int length, float* d_spec, void* hip_stream);
ade_status ade_istft_forward(ade_handle h, const float* d_spec, int batch, int frames, float* d_y, void* hip_stream);

/* ---- stateful streaming over the GTCRN path -----------------------------------------------------
 * The reference resets every state at each slice (zero GRU state, zero causal padding, reflected STFT edges:
 * Inference_GTCRN_ONNX.py:307-317 calls a stateless graph), so slice edges are audible and a slice cannot be shorter than the
 * network's memory.  A stream carries, per independent audio stream: the last 256 input samples (STFT overlap), each GTConvBlock's
 * last 2 * dilation frames of depthwise input, the six TRA GRU and two inter-frame GRU hidden states, and the ISTFT overlap.
 * Pushing a long signal in pieces of frames_per_push * 256 samples then produces EXACTLY what the reference's graph would produce
 * on the whole signal in one call (every op of the network is causal in time), with two stated differences: the output is one
 * hop (256 samples, 16 ms) behind the input -- a frame is complete one hop after its centre -- with the stream's first hop zero;
 * and the per-call DC removal of GTCRN_CUSTOM.forward (Export_GTCRN.py:647, a mean over the WHOLE call, not computable causally)
 * is not applied.  Plain GTCRN handles (not batch-fold; of the other model families NKF-AEC, DFSMN-AEC, DFSMN and UL-UNAS stream, see below).  All streams of a handle advance
 * together.  A push is frames_per_push HOPS of ade_stream_hop samples: 256 at 16 kHz for GTCRN, NKF-AEC, DFSMN-AEC and UL-UNAS, 960 at 48 kHz for DFSMN.  A handle that cannot
 * stream answers ADE_ERR_UNSUPPORTED with a message that names what its family's streams take: int16 PCM in and out at the handle's own model rate (16000 or 48000 Hz).
 * A push of up to 512 frames is ONE kernel launch (the fused chunk kernel continuing from the state its previous launch left); longer pushes, or a
 * stream created while the option "fused" is 0, take the multi-kernel sequence. */
typedef struct ade_stream* ade_stream_handle;
ade_status ade_stream_create(ade_handle h, int n_streams, int frames_per_push, ade_stream_handle* out);
/* in / out: [n_streams][frames_per_push * hop] int16 (out_f32 optional float, pre-PCM-tail), caller-owned HOST buffers; synchronous.  hop = ade_stream_hop: 256, or 960
 * for a DFSMN stream. */
ade_status ade_stream_push(ade_stream_handle s, const int16_t* in, int16_t* out_pcm, float* out_f32);
/* the same on DEVICE buffers; enqueues on `hip_stream` (NULL = the engine's stream, then synchronous). */
ade_status ade_stream_push_device(ade_stream_handle s, const int16_t* d_in, int16_t* d_out_pcm, float* d_out_f32, void* hip_stream);
/* End of the signal: the last hop (out: [n_streams][256]), computed from the one frame the reference's graph evaluates past the end
 * (its second half is the reflection of the last 257 samples).  Pushes + flush then reproduce the one-shot output sample for sample,
 * shifted by one hop.  The stream must be reset before it is pushed again. */
ade_status ade_stream_flush(ade_stream_handle s, int16_t* out_pcm, float* out_f32);
ade_status ade_stream_reset(ade_stream_handle s);      /* back to a fresh stream (zero state, next push reflects its head) */
void ade_stream_destroy(ade_stream_handle s);           /* before ade_destroy of its engine */
/* Samples the stream's output lags its input, which is also the flush length per stream: 256 for a GTCRN or a UL-UNAS stream, 768 for an NKF-AEC stream, 1344 for a
 * DFSMN-AEC stream, 960 for a DFSMN stream. */
ade_status ade_stream_delay(ade_stream_handle s, int* samples);
/* Samples of one hop, the unit of frames_per_push: 256 for a GTCRN, NKF-AEC, DFSMN-AEC or UL-UNAS stream (16 kHz), 960 for a DFSMN stream (48 kHz). */
ade_status ade_stream_hop(ade_stream_handle s, int* samples);

/* ---- stateful streaming over the NKF-AEC path (model_family "nkf_aec"; the same entry points) -------------------------------
 * An echo canceller is an adaptive filter: it is useful while it keeps the echo path it has learnt.  The one-shot call, like the
 * reference's file driver, restarts every state at each slice, so the filter converges again every input_audio_length samples.
 * A stream carries, per independent call: the last 768 input samples of each of the two channels, the Kalman state of each of the
 * 513 bins (h_prior, h_post, the last 4 far-end frames, the four GRU hidden vectors: 96 floats) and the ISTFT overlap (the last
 * three windowed frames).  Pushing a signal of n hops (n * 256 samples per channel) in pieces of frames_per_push * 256 samples and
 * then flushing produces what the reference's graph (NKF.forward, Export_NKF_AEC.py:246-411, exported with
 * INPUT_AUDIO_LENGTH = n * 256) produces on the whole signal in ONE call, with two stated differences:
 *  1. The output is 768 samples (three hops, 48 ms) behind the input, and the stream's first 768 output samples are zero.  Frame t
 *     covers the samples [256 t - 512, 256 t + 512), so after k hops of input the frames 0 .. k - 2 exist; output sample m sums the
 *     frames up to m / 256 + 2, so 256 (k - 3) output samples are final.  The first push of F hops therefore runs F - 1 Kalman
 *     frames, every later push F, and the flush the last two (frames n - 1 and n, zero-padded past the end as the reference's
 *     constant centre pad does).
 *  2. The per-call DC removal (:269, a mean over the whole call, not computable causally) is not applied -- as for GTCRN.
 * Buffers: in [n_streams][2][frames_per_push * 256] int16 (far end, near end: the channel order of ade_process), out
 * [n_streams][frames_per_push * 256] int16, out_f32 optional float of the same shape (the waveform before the PCM tail).
 * ade_stream_flush returns the last 768 samples per stream (out [n_streams][768]), each divided by the window-square sum of the
 * frames that cover it with T = n + 1 frames in all, i.e. the end-of-signal norm of the reference's static ISTFT (the engine sums
 * the squared window over the covering frames in the order the one-shot table is built, so head, steady state -- 1.5 -- and tail
 * are the same rule).  After a flush the stream must be reset before it is pushed again; ade_stream_reset returns to zero state.
 * All streams of a handle advance together.  frames_per_push >= 1: the STFT pads with zeros, not a reflection, so a one-hop first
 * push is legal (it runs no Kalman frame and returns zeros).  The result does not depend on the push size, bit for bit: every
 * transform holds one frame index only (the far-end and near-end frame of index t in the analysis, one frame in the synthesis).
 * Scope: int16 PCM in and out at 16 kHz; a handle with float audio tensors or another output rate answers ADE_ERR_UNSUPPORTED.
 * ade_stream_push_device enqueues four kernels on the caller's stream and does not synchronise. */

/* ---- stateful streaming over the DFSMN-AEC path (model_family "dfsmn_aec"; the same entry points) ----------------------------
 * The one-shot call, and every folded 1.5 s window of it, restarts the Kalman filter of the NKF back end and zeroes the memory of the
 * mask network.  A stream carries both stages.  Every operation of the second stage is causal and frame-local (DFSMN_AEC.forward,
 * Export_DFSMN_AEC.py:1268-1352: the Kaldi frames remove a per-frame mean, the depthwise memory is causal, the 640 / 320 mask STFT
 * has no centre pad) and this family has no whole-call DC removal, so for ANY input pushes plus the flush equal the reference's
 * unfolded graph on the whole signal in ONE call, 1344 samples later, within the family's gates (waveform 1e-4, PCM 1 LSB).
 * Eligible handles: int16 audio at 16 kHz on both sides (F32 / F16 audio tensors or another sample rate: ADE_ERR_UNSUPPORTED, the
 * message names int16 / 16000); a folded or an unfolded manifest (a stream does not use the window length); either ade_dft_tables
 * mode, which the stream follows (reference: the back end's transforms are dense products with the reference's tables; exact: its
 * FFT stream kernels).  A handle with output_vad_result = 1 is accepted; a stream returns AUDIO ONLY.
 * Buffers: in [n_streams][2][frames_per_push * 256] int16, channel 0 the NEAR end, channel 1 the FAR end (this family's order in
 * ade_process, the opposite of nkf_aec); out [n_streams][frames_per_push * 256] int16, out_f32 optional float of the same shape (the
 * waveform before the PCM tail).  1 <= frames_per_push <= 4096.  All streams of a handle advance together.  ade_stream_push_device
 * enqueues on the caller's stream and does not synchronise.
 * Delay: 1344 samples (84 ms), the minimum, and exact.  After k hops of input
 *   - the back end (768 samples behind, see above) has nt = 256 max(0, k - 3) final temp_aec samples;
 *   - mask frame m needs temp_aec and near-end samples [320 m, 320 m + 640), so M = 0 frames are complete if nt < 640, else
 *     M = (nt - 640) / 320 + 1 (integer division);
 *   - an output sample is final once both frames that cover it are complete: 320 M samples;
 *   - nt - 640 - 320 (M - 1) <= 319 and is a multiple of 64 (gcd(256, 320)), hence <= 256, so 320 M >= nt - 576 = 256 k - 1344, with
 *     equality at k = 9, 14, 19, ...: a push of F hops can always emit its 256 F samples at a lag of 1344, and at no smaller lag.
 *     (Also checked by enumeration for k < 4000.)  At most 256 final samples wait for the next push.
 * The stream's first 1344 output samples are zero; output sample j of the stream is sample j - 1344 of the one-call result.  A push
 * that completes no mask frame (with one-hop pushes every fifth) runs the back end only and still emits its samples.
 * ade_stream_flush returns the last 1344 samples per stream (out [n_streams][1344]) and ends the signal of L = 256 K samples after
 * K hops: the back end's last two frames, the remaining three mask frames, the end-of-signal entries of the static window-square
 * table.  Signal indices below zero come out as zeros (K = 5 only).  It is defined only where the reference's static export accepts
 * the length, L % 320 == 0: K a multiple of 5, at least 5; otherwise ADE_ERR_BAD_VALUE with a message that says so (the stream
 * stays usable).  After a flush the stream must be reset before it is pushed again.
 * The result does not depend on frames_per_push, bit for bit, PCM and f32: every transform holds one frame (the mask synthesis runs
 * one frame per FFT; the one-shot kernel's pairs would make a frame's rounding depend on where the push ends), the memory sums its
 * taps in the one-shot order from a per-layer history of dilation * (lorder - 1) frames, and the overlap-add adds at most two frames
 * in ascending order and reads the one-shot's 1 / window-square table. */

/* ---- stateful streaming over the DFSMN path (model_family "dfsmn", 48 kHz; the same entry points) ------------------------------
 * DFSMN.forward (Export_DFSMN.py:176-246) is causal from end to end: the Kaldi mean is taken per frame (no whole-call DC removal),
 * there is no centre padding (frame t covers the samples [960 t, 960 t + 1920)), every layer of the mask network is frame-local
 * except the depthwise memory, which looks lorder - 1 frames back over a zero pad, and the synthesis is a two-frame overlap-add.  So
 * pushes plus the flush equal the reference's ONE call on the whole signal, one hop (960 samples, 20 ms) later, within the family's
 * gates (waveform 2e-5, PCM 1 LSB from the exact-table oracle), where the per-slice driver restarts the nine memories and divides
 * its one-frame edges by w^2 ~ 0.0064.  A stream carries, per independent stream: the last 960 input samples, per layer the last
 * lorder - 1 frames of the projection output, and the second half of the last synthesised frame.
 * Eligible handles: int16 audio at 48 kHz on both sides, not folded (F32 / F16 audio tensors, another input or output rate, or
 * use_batch_fold = 1 -- a folded call treats its windows as independent clips, which is not what a stream computes --:
 * ADE_ERR_UNSUPPORTED, the message names int16 / 48000).  Static and dynamic_axes manifests both stream; a stream does not use the
 * window length.
 * Buffers: in [n_streams][960 F] int16, F = frames_per_push hops (ade_stream_hop = 960); out the same shape; out_f32 optional float
 * of the same shape (the waveform before the PCM tail).  1 <= F <= 4096.  All streams of a handle advance together.
 * ade_stream_push_device enqueues on the caller's stream and does not synchronise.
 * Output timing: the stream's first 960 output samples are zero; output sample j of the stream is sample j - 960 of the one-call
 * result.  A fresh stream's first push completes F - 1 frames, every later push F.  With F = 1 the first push completes none: it
 * returns 960 zeros and runs no network kernel (it only stores the carried samples).
 * ade_stream_flush returns the last 960 samples per stream (out [n_streams][960]): the second half of the last frame over
 * w^2[960 + n].  It ends a signal of 960 K samples after K hops, equal to the static export with input_audio_length = 960 K.  It
 * needs K >= 2, one whole frame; otherwise ADE_ERR_BAD_VALUE with a message that says so (the stream stays usable).  After a flush
 * the stream must be reset before it is pushed again.
 * The push size does not change a bit of the output, PCM and f32, and a stream's bits do not depend on how many other streams share
 * the handle: every transform holds ONE frame (each real transform is a half-length complex FFT plus a split pass), the memory sums
 * its taps in one order from history or push alike, the overlap-add adds at most two frames in ascending order.
 * NOT promised: the bits of ade_process on the same signal.  The one-shot kernels transform frames in pairs, which a stream must not
 * (a frame's rounding would depend on where a push ends); both are held to the same gates against the oracle. */

/* ---- stateful streaming over the UL-UNAS path (model_family "ul_unas", 16 kHz; the same entry points) ----------------------------
 * ULUNAS_CUSTOM.forward (Export_UL_UNAS.py:848-913) is causal from end to end: every (de)convolution is causal in time (:229-240,
 * :266-269), the time attention of each cTFA is a forward GRU over frames, its frequency attention and the intra-frame GRU run along
 * frequency inside one frame, the inter-frame GRU is GTCRN's, and the wrapper removes no DC (REMOVE_DC_OFFSET = False).  So pushes
 * plus the flush equal the reference's ONE call on the whole signal, one hop (256 samples, 16 ms) later, within the family's gates
 * (PCM 1 LSB from the exact-table oracle under the host simulator, 2 LSB on the GPU), where the per-slice driver restarts ten
 * time-attention GRUs, two inter-frame GRUs and every convolution history at each slice.  A stream carries, per independent stream:
 * the last 257 input samples; the last kt - 1 INPUT frames of every (de)convolution with kt > 1 (for a decoder block the frame of
 * x + skip, already summed): kt = 3 in the first encoder and the last decoder block, kt = 2 in the two (2, 3) blocks of either side;
 * the ten time-attention hidden states (2 C floats each); the two inter-frame GRU states (33 x 16 each); the synthesis overlap (the
 * second half of the last synthesised frame, 256 samples).  The state is one allocation; a reset is one memset.
 * Eligible handles: plain ul_unas handles with int16 audio at 16 kHz on both sides, from a static or a dynamic_axes manifest (a stream
 * does not use the window length).  F32 / F16 audio tensors, another input or output rate, or use_batch_fold = 1: ADE_ERR_UNSUPPORTED,
 * the message names int16 / 16000.  (The engine applies no DC removal for this family, so there is no remove_dc_offset to refuse.)
 * Buffers: in [n_streams][256 F] int16, F = frames_per_push hops (ade_stream_hop = 256); out the same shape; out_f32 optional float
 * of the same shape (the waveform before the PCM tail).  2 <= F <= 4096: the first push must hold the 257 samples the head reflection
 * reads, which is GTCRN's rule; F = 1 answers ADE_ERR_BAD_VALUE with a message that says so.  All streams of a handle advance together.
 * Output timing: ade_stream_hop and ade_stream_delay are 256.  Frame t is centred on sample 256 t and complete one hop later, as for
 * GTCRN.  The stream's first 256 output samples are zero; output sample j of the stream is sample j - 256 of the reference's ONE call
 * on the whole signal of 256 K samples (T = K + 1 frames, 256 K output samples).  A fresh stream's first push of F hops completes the
 * frames 0 .. F - 1 (the head reflected), every later push F more.
 * ade_stream_flush returns the last 256 samples per stream (out [n_streams][256]), computed from frame K, whose second half is the
 * reflection of the last 257 samples -- which is why the input carry reaches back 257 samples and not 256.  After a flush the stream
 * must be reset before it is pushed again; ade_stream_reset and ade_stream_destroy behave as for the other families.
 * The push size does not change a bit of the output, PCM and f32, and a stream's bits do not depend on how many other streams share
 * the handle: every transform holds ONE frame (a 512-point real transform as a 256-point complex FFT plus a split pass, and the
 * Hermitian inverse of one frame), a convolution sums its taps in one order from history or push alike, the time attention's 64-frame
 * chunks only decide when a frame's input projections are formed, and the overlap-add adds the two frames of a sample in ascending
 * order over the one-shot's window-square sum (Hann^2 at half overlap is not constant: a 256-entry table; every sample of the trimmed
 * one-shot output has both of its frames, so the same table serves the signal's first and last hop).
 * NOT promised: the bits of ade_process on the same signal.  The one-shot path's generic STFT transforms frames in pairs, paired by
 * the frame's parity inside the call, which a stream must not (a frame's rounding would depend on where a push ends); both are held
 * to the same gates against the oracle.
 * ade_stream_push_device enqueues on the caller's ONE stream and does not synchronise (65 launches per push; the row groups that
 * ade_process runs on side streams, ADE_ULU_GROUPS, are not used by a stream). */

/* ---- generic STFT_Process operator: any n_fft / win_length / hop / window, for the other model families -------
 * Replaces the reference's STFT_Process module in its 'stft_B' (packed) and 'istft_B' (packed, static_norm=True) forms
 * as instantiated by GTCRN (512/512/256 hann_sqrt, GTCRN/Export_GTCRN.py:719-741), ZipEnhancer (400/400/100 hann,
 * ZipEnhancer/Export_ZipEnhancer.py:947-948), Mel-Band-Roformer (2048/2048/441 hann,
 * Mel_Band_Roformer/Stereo/Export_MelBandRoformer.py:695-696) and DFSMN (1920/1920/960 symmetric hamming analysis,
 * periodic hamming synthesis, no centre pad, DFSMN/Export_DFSMN.py:273-274); class at GTCRN/STFT_Process.py:129-341.
 * Window names: "hann", "hann_sqrt", "hamming" (torch periodic=True), with a "_sym" suffix for periodic=False;
 * "hamming_periodic" is accepted as an alias of "hamming".  Layouts are the reference's: x [B][L] float ->
 * spec [B][2*(n_fft/2+1)][T] (re rows, then im rows) -> y [B][out_len].  5-smooth transform sizes (every folder's: 512, 400, 2048, 1920) run as mixed-radix
 * Stockham FFTs in LDS; other sizes as the reference's own dense windowed DFT on the fp32 matrix cores. */
typedef struct ade_stft_plan* ade_stft_handle;
typedef struct ade_stft_config {
    int n_fft, win_length, hop;
    const char* window;             /* analysis window */
    const char* synthesis_window;   /* NULL: same as the analysis window */
    int center_pad;                 /* 1: pad n_fft/2 on both sides (pad_mode), ISTFT trims them again */
    const char* pad_mode;           /* "reflect" | "constant" (NULL = "reflect") */
} ade_stft_config;
ade_status ade_stft_create(const ade_stft_config* cfg, int device, ade_stft_handle* out);
ade_status ade_stft_frames(ade_stft_handle h, int length, int* frames);             /* T for an input of `length` samples */
ade_status ade_stft_output_length(ade_stft_handle h, int frames, int* out_len);     /* ISTFT output length for T frames */
/* The dynamic-length trim of a DYNAMIC_AXES export: the reference's ISTFT slices [n_fft/2 : out_end(max_frames)] and is fed fewer frames than max_frames
 * (UL-UNAS/STFT_Process.py:170-177, :317-326; Mel_Band_Roformer/Stereo/STFT_Process.py:296-306), so the output keeps the second half of the last frame:
 * hop (T - 1) + n_fft / 2 samples, each divided by the squared-window sum of the frames that cover it.  keep_tail = 0 (default) is the static trim hop (T - 1). */
ade_status ade_stft_keep_tail(ade_stft_handle h, int keep_tail);
ade_status ade_stft_analyze(ade_stft_handle h, const float* d_x, int batch, int length, float* d_spec, void* hip_stream);
ade_status ade_stft_synthesize(ade_stft_handle h, const float* d_spec, int batch, int frames, float* d_y, void* hip_stream);
/* The polar form (model_type "istft_A", STFT_Process.py:343-361): magnitude and phase, each [batch][F][T]; real = mag cos(phase),
 * imag = mag sin(phase) are formed inside the GEMM's operand loader. */
ade_status ade_stft_synthesize_polar(ade_stft_handle h, const float* d_mag, const float* d_phase, int batch, int frames, float* d_y, void* hip_stream);
const char* ade_stft_last_error(ade_stft_handle h);   /* h == NULL: the last failing ade_stft_create of this thread */
void ade_stft_destroy(ade_stft_handle h);

#ifdef __cplusplus
}
#endif
#endif /* ADE_H */
