// ade_dfsmn_aec.hip — DFSMN-AEC on the MI355X: the NKF linear echo canceller followed by a DFSMN residual-echo mask (and a per-frame speech probability).
//
// Reference: DFSMN_AEC.forward, DFSMN_AEC/Export_DFSMN_AEC.py:1268-1352, with light_aec_model = "NKF" (NKF_Inner :897-1000), build_kaldi_fbank_conv (:1032-1068) and
// the folder's STFT_Process.  Two inputs per call -- channel 0 the near-end microphone, channel 1 the far-end reference (the export's input order, :1519; the opposite
// of nkf_aec) -- and one output.  A call is n_win windows of W samples back to back (USE_BATCH_FOLD, :1271-1273): every window is an independent clip.
//
//   NKF back end      the four launches of csrc/ade_nkf_aec.hip through nkf_backend_create (ade_internal.h): analysis, the per-bin Kalman kernel, synthesis and the
//                     overlap-add that keeps [512, 512 + W) -> temp_aec, a float waveform of W samples per window.  ade_dft_tables = "reference" (the default): its two
//                     transforms are dense products with the reference's fp32-angle tables (the logarithm of the echo band amplifies that angle error to 3 LSB of
//                     the output); "exact": the FFT kernels nkf_aec uses
//   k_dfa_features    one workgroup per group of kGroup mask frames; per frame, in LDS: the Kaldi frames of near and temp_aec (mean removal, 0.97 pre-emphasis,
//                     symmetric hamming, zero pad to 1024) as the real and the imaginary part of ONE complex 1024-point FFT, split into the two spectra, the echo
//                     spectrum near - 1.15 temp, the three powers * 2^30 (LDS only), the banded 80-band mel sum, max(., eps), log -> the 240-wide feature row;
//                     then the 640-point mask transform of temp_aec (symmetric hamming, no centre pad; 640 = 4^3 x 2 x 5) -> 321 complex bins
//   mask network      matrix-core GEMMs (csrc/ade_gemm.h) with bias / ReLU / sigmoid in the store; activations channels-first (C, N), N = windows x frames
//   k_dfa_memory      the causal depthwise memory with dilation, the optional skip and the outer residual
//   k_dfa_synthesis   mask * spectrum -> Hermitian inverse 640-point FFT (two frames per transform) -> * symmetric hamming / 640
//   k_dfa_ola         overlap-add at hop 320 as a gather (at most two frames per sample), * 1 / window-square sum -> the f32 waveform; * 32767, clamp, truncate -> int16
// Every network dimension (width, hidden sizes, lorder, dilation, depth) is read from the blob.
//
// Streams (ade_stream_* on a dfsmn_aec handle, include/ade.h; DESIGN.md section 11, "Streaming"): a push of F hops continues the signal, 1344 samples behind the input --
//   back end             NkfBackend::stream_step: the stream kernels of csrc/ade_nkf_aec.hip, the float temp_aec of the step left in device memory
//   k_dfa_stream_stage   the push's near-end samples and the step's temp_aec samples into two rings addressed by the signal's sample index
//   k_dfa_features       the same kernel, its 640 samples per frame read from the rings (RingSrc)
//   mask network         the same GEMMs, N = streams x the frames the push completes
//   k_dfa_stream_memory  the memory with the frames before the push taken from the layer's history, which it also renews
//   k_dfa_stream_synthesis  ONE frame per transform (a pair would make a frame's bits depend on where the push ends)
//   k_dfa_stream_out     overlap-add gather, the one-shot's 1 / window-square table, the samples that are final but not yet due, the PCM tail
// Every count is a function of the hops pushed and is computed on the host.
#include "ade_fft.h"
#include "ade_gemm.h"
#include "ade_internal.h"
#include "../../include/ade.h"

#include <cmath>
#include <cstring>
#include <memory>

namespace ade {

namespace {

using namespace dev;

constexpr int kNA = 640, kHA = 320, kFA = kNA / 2 + 1;          // mask STFT
constexpr int kNK = 1024, kFK = kNK / 2 + 1;                    // Kaldi fbank transform
constexpr int kMelN = 80, kFeat = 3 * kMelN;
constexpr int kGroup = 4;                                       // mask frames per workgroup of k_dfa_features
constexpr float kEchoFactor = 1.15f;                            // (:1187)
constexpr float kLogFloor = 1.1920928955078125e-07f;            // torch.finfo(float32).eps (:1186)

struct FeatFrameB {            // B(k, j) = feature k of frame j (frame-major rows of 240, written by k_dfa_features)
    static constexpr bool kAlongN = false;
    const float* p;
    __device__ float operator()(int k, int j) const { return p[(size_t)j * kFeat + k]; }
};
struct MaskTStore {            // mask[j][f] = sigmoid(v + bias[f]): linear2, stored frame-major for the per-frame synthesis kernel (:1320)
    static constexpr bool kCtx = true;
    float* out;
    const float* bias;
    __device__ float row(int f) const { return bias[f]; }
    __device__ gemm::None col(int) const { return gemm::None{}; }
    __device__ gemm::None pre(int, int, float) const { return gemm::None{}; }
    __device__ void operator()(int f, int j, float v, float b, gemm::None, gemm::None) const { out[(size_t)j * kFA + f] = 1.0f / (1.0f + expf(-(v + b))); }
};

// Where k_dfa_features takes the 640 (near, temp_aec) samples of mask frame fr from.
// One-shot: frame fr = row * Tm + t of window row = call * n_win + w: the near end is channel 0 of the caller's [call][2][n_win * W] rows, temp_aec is [row][W].
struct CallSrc {
    const int16_t* pcm;
    const float* fpcm;
    const float* temp;
    int W, Tm, n_win;
    struct Frame { const int16_t* pcm; const float* fpcm; const float* temp; size_t at_near, at_temp; };
    __device__ Frame frame(int fr) const {
        const int row = fr / Tm, t = fr - row * Tm, call = row / n_win, w = row - call * n_win;
        return Frame{pcm, fpcm, temp, ((size_t)call * 2 * n_win + w) * W + (size_t)t * kHA, (size_t)row * W + (size_t)t * kHA};
    }
    static __device__ float near(const Frame& f, int n) { return (f.fpcm ? f.fpcm[f.at_near + n] : (float)f.pcm[f.at_near + n]) * (1.0f / 32768.0f); }
    static __device__ float temp_aec(const Frame& f, int n) { return f.temp[f.at_temp + n]; }
};
// Streams: frame fr = stream * Mp + i is the i-th frame the push completes; sample n of it sits in the stream's rings at (offset of the push's first frame + 320 i + n)
// modulo the ring length (the rings are addressed by the signal's sample index; the offsets come from the host).
struct RingSrc {
    const int16_t* near_ring;
    const float* temp_ring;
    int Mp, RN, RT, near_off, temp_off;
    struct Frame { const int16_t* nr; const float* tr; int RN, RT, n0, t0; };
    __device__ Frame frame(int fr) const {
        const int st = fr / Mp, i = fr - st * Mp;
        return Frame{near_ring + (size_t)st * RN, temp_ring + (size_t)st * RT, RN, RT, (near_off + i * kHA) % RN, (temp_off + i * kHA) % RT};
    }
    static __device__ float near(const Frame& f, int n) { int p = f.n0 + n; if (p >= f.RN) p -= f.RN; return (float)f.nr[p] * (1.0f / 32768.0f); }
    static __device__ float temp_aec(const Frame& f, int n) { int p = f.t0 + n; if (p >= f.RT) p -= f.RT; return f.tr[p]; }
};

template <class Src>
__global__ __launch_bounds__(256) void k_dfa_features(Src src, int nframes, fft::Plan p1024, fft::Plan p640, const float2* __restrict__ tw1024, const float2* __restrict__ tw640,
                                                      const float* __restrict__ win_k, const float* __restrict__ win_a, BandTab mel, float2* __restrict__ spec,
                                                      float* __restrict__ feat) {
    __shared__ float2 A[kNK];
    __shared__ float2 B[kNK];
    __shared__ float2 xs[kNA];                   // (near, temp_aec) samples of the frame
    __shared__ float P[3][kFK + 3];              // near, temp, echo power
    __shared__ double red[2][256];
    const int tid = threadIdx.x;
    for (int g = 0; g < kGroup; ++g) {
        const int fr = (int)blockIdx.x * kGroup + g;
        if (fr >= nframes) break;                // uniform over the workgroup
        const auto frame = src.frame(fr);
        double part[2] = {0.0, 0.0};
        for (int n = tid; n < kNA; n += 256) {
            const float a = Src::near(frame, n), b = Src::temp_aec(frame, n);
            xs[n] = make_float2(a, b);
            part[0] += (double)a;
            part[1] += (double)b;
        }
        red[0][tid] = part[0];
        red[1][tid] = part[1];
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
            __syncthreads();
        }
        const float m0 = (float)(red[0][0] / (double)kNA), m1 = (float)(red[1][0] / (double)kNA);
        // Kaldi's order: mean removal, pre-emphasis (the first sample is its own predecessor), window, zero pad (:1057-1064)
        for (int n = tid; n < kNK; n += 256) {
            float2 v = make_float2(0.0f, 0.0f);
            if (n < kNA) {
                const float2 c = xs[n], p = xs[n > 0 ? n - 1 : 0];
                const float wk = win_k[n];
                v = make_float2(((c.x - m0) - 0.97f * (p.x - m0)) * wk, ((c.y - m1) - 0.97f * (p.y - m1)) * wk);
            }
            A[n] = v;
        }
        const float2* r = fft::forward(A, B, p1024, tw1024, tid, 256);
        for (int f = tid; f < kFK; f += 256) {
            const float2 z = r[f], zc = r[f == 0 ? 0 : kNK - f];
            const float re0 = 0.5f * (z.x + zc.x), im0 = 0.5f * (z.y - zc.y), re1 = 0.5f * (z.y + zc.y), im1 = 0.5f * (zc.x - z.x);
            const float ree = re0 - kEchoFactor * re1, ime = im0 - kEchoFactor * im1;              // echo estimate (:1304)
            P[0][f] = (re0 * re0 + im0 * im0) * (32768.0f * 32768.0f);
            P[1][f] = (re1 * re1 + im1 * im1) * (32768.0f * 32768.0f);
            P[2][f] = (ree * ree + ime * ime) * (32768.0f * 32768.0f);
        }
        __syncthreads();
        if (tid < kFeat) {                                                                       // feature row [near 80 | temp 80 | echo 80] (:1310-1311)
            const int s = tid / kMelN, b = tid - s * kMelN, st = mel.start[b];
            float acc = 0.0f;
            for (int j = 0; j < mel.count; ++j) acc += mel.w[j * kMelN + b] * P[s][st + j];
            feat[(size_t)fr * kFeat + tid] = logf(acc > kLogFloor ? acc : kLogFloor);
        }
        // the mask transform of temp_aec (:1288)
        for (int n = tid; n < kNA; n += 256) A[n] = make_float2(xs[n].y * win_a[n], 0.0f);
        r = fft::forward(A, B, p640, tw640, tid, 256);
        for (int f = tid; f < kFA; f += 256) spec[(size_t)fr * kFA + f] = r[f];
        __syncthreads();                                                                         // the next frame overwrites xs, A, B, P, red
    }
}

// causal depthwise memory, optional skip, outer residual (:1253-1266): x[c][j] += sum_k w[c][k] * h[c][j - dil (lo - 1 - k)] (+ h[c][j]), zero before the window's first frame
__global__ __launch_bounds__(256) void k_dfa_memory(const float* __restrict__ h, const float* __restrict__ w, float* __restrict__ x, int N, int T, int lo, int dil, int skip,
                                                    long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i / N), j = (int)(i - (long long)c * N);
    const int t = j % T;
    float s = 0.0f;
    const float* row = h + (size_t)c * N + j;
    for (int k = 0; k < lo; ++k) {                   // unconditional loads from clamped frames, masked afterwards (as k_fsmn_memory)
        const int dt = (k - (lo - 1)) * dil;
        const bool ok = t + dt >= 0;
        const float v = row[ok ? dt : 0];
        s += ok ? w[c * lo + k] * v : 0.0f;
    }
    if (skip) s += row[0];
    x[i] += s;
}

// One workgroup per PAIR of frames of one window: W = H(Z0) + i H(Z1) stored conjugated, x0 + i x1 = conj(DFT(conj W)) / N, Z = mask * spectrum (:1324-1327); the sine
// rows of the DC and Nyquist bins of the reference's inverse table are zero, so those imaginary parts are dropped.
__global__ __launch_bounds__(256) void k_dfa_synthesis(const float2* __restrict__ spec, const float* __restrict__ mask, int T, fft::Plan p640, const float2* __restrict__ tw640,
                                                       const float* __restrict__ win, float* __restrict__ frames) {
    __shared__ float2 A[kNA];
    __shared__ float2 B[kNA];
    const int tid = threadIdx.x, ppr = (T + 1) / 2, b = (int)blockIdx.x / ppr, t0 = 2 * ((int)blockIdx.x - b * ppr);
    const int f0 = b * T + t0;
    const bool two = t0 + 1 < T;
    const int f1 = two ? f0 + 1 : f0;
    for (int f = tid; f < kFA; f += 256) {
        const bool edge = f == 0 || f == kFA - 1;
        const float m0 = mask[(size_t)f0 * kFA + f], m1 = two ? mask[(size_t)f1 * kFA + f] : 0.0f;
        const float2 s0 = spec[(size_t)f0 * kFA + f], s1 = spec[(size_t)f1 * kFA + f];
        const float2 z0 = make_float2(s0.x * m0, edge ? 0.0f : s0.y * m0), z1 = make_float2(s1.x * m1, edge ? 0.0f : s1.y * m1);
        A[f] = make_float2(z0.x - z1.y, -(z0.y + z1.x));
        if (!edge) A[kNA - f] = make_float2(z0.x + z1.y, z0.y - z1.x);
    }
    const float2* r = fft::forward(A, B, p640, tw640, tid, 256);
    for (int n = tid; n < kNA; n += 256) {
        const float w = win[n];
        frames[(size_t)f0 * kNA + n] = (r[n].x * (1.0f / (float)kNA)) * w;
        if (two) frames[(size_t)(f0 + 1) * kNA + n] = (-r[n].y * (1.0f / (float)kNA)) * w;
    }
}

// conv_transpose overlap-add as a gather (raw length 640 + 320 (T - 1) == W), * the static 1 / window-square sum, then the PCM tail (:1335-1347)
__global__ __launch_bounds__(256) void k_dfa_ola(const float* __restrict__ frames, const float* __restrict__ inv_ws, int T, int W, float* __restrict__ wave,
                                                 int16_t* __restrict__ pcm, float* __restrict__ f32, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int b = (int)(i / W), m = (int)(i - (long long)b * W);
    int t_hi = m / kHA;
    if (t_hi > T - 1) t_hi = T - 1;
    const int t_lo = m < kNA ? 0 : (m - kNA) / kHA + 1;
    float s = 0.0f;
    for (int t = t_lo; t <= t_hi; ++t) s += frames[((size_t)b * T + t) * kNA + (m - t * kHA)];
    const float y = s * inv_ws[m];
    wave[i] = y;
    if (f32) f32[i] = y;
    if (pcm) pcm[i] = (int16_t)(int)fminf(fmaxf(y * 32767.0f, -32768.0f), 32767.0f);          // .to(torch.int16): truncation
}

// ---- streams ----------------------------------------------------------------------------------------------------------------------------------------------------
// After k hops of input the back end has nt = 256 max(0, k - 3) final temp_aec samples, M(k) = 0 if nt < 640, else (nt - 640) / 320 + 1 mask frames are complete and
// 320 M(k) output samples are final; 320 M(k) >= 256 k - 1344 (include/ade.h has the derivation).
constexpr int kDelay = 1344, kPend = 256;       // output lag in samples; the most final samples a push can leave for the next one (320 M(k) - (256 k - 1344) <= 256)
constexpr int kNearLag = 1408, kTempLag = 640;  // samples a ring holds beyond one step: 256 k - 320 M(k) < 1408, nt(k) - 320 M(k) < 640

// The step's new samples into the rings: near-end sample q of the push (channel 0 of the caller's [stream][2][P] rows; null in the flush) at (near_off + q) % RN,
// temp_aec sample q of the back end's step ([stream][Pt]) at (temp_off + q) % RT for q >= t_min (the samples before the signal's first are skipped).
__global__ __launch_bounds__(256) void k_dfa_stream_stage(const int16_t* __restrict__ pcm, const float* __restrict__ temp, int P, int Pt, int t_min, int16_t* __restrict__ near_ring,
                                                          float* __restrict__ temp_ring, int RN, int RT, int near_off, int temp_off, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int span = P + Pt, st = (int)(i / span), q = (int)(i - (long long)st * span);
    if (q < P) near_ring[(size_t)st * RN + (near_off + q) % RN] = pcm[(size_t)st * 2 * P + q];
    else if (q - P >= t_min) temp_ring[(size_t)st * RT + (temp_off + (q - P)) % RT] = temp[(size_t)st * Pt + (q - P)];
}

// k_dfa_memory over the Mp frames a push completes, column j = stream * Mp + i.  A tap that reaches before the push reads the layer's history, hist_in [c][stream][Hl]:
// the Hl = dil (lo - 1) frames before the push, oldest first, zeros before the stream's first frame (the reset's memset).  The taps are summed in k_dfa_memory's order.
// The threads from `total` on write the next history into hist_out: the last Hl frames of [history | push].
// Not promised: the one-shot call's bits.  k_dfa_memory adds a literal 0 for a tap before the window's first frame, this kernel w * (a history value, zero before the
// stream's first frame), and the compiler may contract the two forms differently; the contract is the family's gates (1e-4, 1 LSB) against the one call on the whole
// signal, and bit identity between push sizes, which only needs this kernel to agree with itself.
__global__ __launch_bounds__(256) void k_dfa_stream_memory(const float* __restrict__ h, const float* __restrict__ w, float* __restrict__ x, const float* __restrict__ hist_in,
                                                           float* __restrict__ hist_out, int S, int Mp, int Hl, int lo, int dil, int skip, long long total, long long total_all) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total_all) return;
    const int N = S * Mp;
    if (i < total) {
        const int c = (int)(i / N), j = (int)(i - (long long)c * N), st = j / Mp, t = j - st * Mp;
        const float* row = h + (size_t)c * N + j;
        const float* old = hist_in + ((size_t)c * S + st) * Hl + Hl + t;          // old[dt]: frame t + dt of the push, t + dt < 0
        float s = 0.0f;
        for (int k = 0; k < lo; ++k) {
            const int dt = (k - (lo - 1)) * dil;
            const float v = t + dt >= 0 ? row[dt] : old[dt];
            s += w[c * lo + k] * v;
        }
        if (skip) s += row[0];
        x[i] += s;
        return;
    }
    const long long e = i - total;                                                // (c, stream, slot): slot q holds frame Mp - Hl + q of the push
    const int q = (int)(e % Hl), cs = (int)(e / Hl), c = cs / S, st = cs - c * S, t = Mp - Hl + q;
    hist_out[e] = t >= 0 ? h[(size_t)c * N + (size_t)st * Mp + t] : hist_in[(size_t)cs * Hl + (Hl + t)];
}

// One workgroup per frame: mask * spectrum -> the Hermitian inverse 640-point transform of ONE frame -> * symmetric hamming / 640.  The last frame of a stream's push
// also leaves its second half in half_out [stream][320], which the next push's overlap-add starts from.
__global__ __launch_bounds__(256) void k_dfa_stream_synthesis(const float2* __restrict__ spec, const float* __restrict__ mask, int Mp, fft::Plan p640, const float2* __restrict__ tw640,
                                                              const float* __restrict__ win, float* __restrict__ frames, float* __restrict__ half_out) {
    __shared__ float2 A[kNA];
    __shared__ float2 B[kNA];
    const int tid = threadIdx.x, fr = (int)blockIdx.x, st = fr / Mp, i = fr - st * Mp;
    for (int f = tid; f < kFA; f += 256) {
        const bool edge = f == 0 || f == kFA - 1;
        const float m = mask[(size_t)fr * kFA + f];
        const float2 sp = spec[(size_t)fr * kFA + f];
        const float re = sp.x * m, im = edge ? 0.0f : sp.y * m;
        A[f] = make_float2(re, -im);
        if (!edge) A[kNA - f] = make_float2(re, im);
    }
    const float2* r = fft::forward(A, B, p640, tw640, tid, 256);
    for (int n = tid; n < kNA; n += 256) {
        const float v = (r[n].x * (1.0f / (float)kNA)) * win[n];
        frames[(size_t)fr * kNA + n] = v;
        if (i == Mp - 1 && n >= kHA) half_out[(size_t)st * kHA + (n - kHA)] = v;
    }
}

// Output of a step.  Positions are counted from the first sample of the push's first frame (signal sample 320 M0): output sample q of the step is position e_rel + q.
//   position < 0     final since an earlier push: pend_in[stream][q] for q < n_pend, else before the signal's first sample, zero
//   position r >= 0  frame r / 320 of the push and the frame before it, added in ascending frame order (k_dfa_ola's); the frame before the push's first is half_in
//                    (has_prev), and nothing at the signal's first frame
// times the one-shot's 1 / window-square table: its head entries for the signal's first 320 samples (head), its tail entries from position tail_from on (the flush:
// the signal's last 320 samples), its steady entries 320 .. 639 otherwise.  The threads q >= Pout write the kPend samples behind the step into pend_out, zero where
// they are not final yet (pend_out null: the flush).
__global__ __launch_bounds__(256) void k_dfa_stream_out(const float* __restrict__ frames, const float* __restrict__ half_in, const float* __restrict__ pend_in, float* __restrict__ pend_out,
                                                        const float* __restrict__ inv_ws, int W, int Mp, int Pout, int e_rel, int n_pend, int has_prev, int head, int tail_from,
                                                        int16_t* __restrict__ pcm, float* __restrict__ f32, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int span = Pout + (pend_out ? kPend : 0), st = (int)(i / span), q = (int)(i - (long long)st * span), r = e_rel + q;
    float y = 0.0f;
    if (r < 0) {
        if (q < n_pend) y = pend_in[(size_t)st * kPend + q];
    } else if (r < kHA * Mp + (q < Pout ? kHA : 0)) {                     // (an emitted sample is always final; one kept for later only inside the completed frames)
        const int fi = r / kHA, n = r - fi * kHA;
        float s = 0.0f;
        if (fi > 0) s += frames[((size_t)st * Mp + fi - 1) * kNA + kHA + n];
        else if (has_prev) s += half_in[(size_t)st * kHA + n];
        if (fi < Mp) s += frames[((size_t)st * Mp + fi) * kNA + n];
        const int at = head && r < kHA ? r : (r >= tail_from ? W - kHA + n : kHA + n);
        y = s * inv_ws[at];
    }
    if (q >= Pout) {
        pend_out[(size_t)st * kPend + (q - Pout)] = y;
        return;
    }
    const size_t o = (size_t)st * Pout + q;
    if (f32) f32[o] = y;
    if (pcm) pcm[o] = (int16_t)(int)fminf(fmaxf(y * 32767.0f, -32768.0f), 32767.0f);          // .to(torch.int16): truncation
}

void hamming_symmetric_f32(int n, std::vector<float>& w) {      // torch.hamming_window(n, periodic=False) as evaluated in fp32
    w.resize((size_t)n);
    const float step = (float)(2.0 * M_PI / (double)(n - 1));
    for (int k = 0; k < n; ++k) w[k] = cosf((float)k * step) * (-0.46f) + 0.54f;
}

int afail(std::string& err, int st, const std::string& msg) { err = msg; return st; }
#define DA_HIP(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) return afail(err, ADE_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

}  // namespace

struct DfsmnAecEngine : SubEngine {
    int device = 0, W = 0, n_win = 1, Tm = 0, D = 0, Hmax = 0, depth = 0;
    std::unique_ptr<NkfBackend> nkf;
    float* d_w = nullptr;      // one arena: tables + weights
    const float *win_k = nullptr, *win_a = nullptr, *inv_ws = nullptr, *lin1_w = nullptr, *lin1_b = nullptr, *lin2_w = nullptr, *lin2_b = nullptr, *lin3_w = nullptr,
                *lin3_b = nullptr;
    const float2 *tw1024 = nullptr, *tw640 = nullptr;
    BandTab mel{nullptr, nullptr, 0, 0};
    fft::Plan p1024, p640;
    struct Layer { const float *lin_w, *lin_b, *proj_w, *conv_w; int H, lorder, dilation, skip; };
    std::vector<Layer> layers;
    int capacity = 0;
    float* ws = nullptr;
    float *temp = nullptr, *feat = nullptr, *x = nullptr, *f1 = nullptr, *p1 = nullptr, *mask = nullptr, *vad = nullptr, *frames_buf = nullptr, *wave = nullptr;
    float2* spec = nullptr;

    ~DfsmnAecEngine() override {
        (void)hipSetDevice(device);
        if (d_w) (void)hipFree(d_w);
        if (ws) (void)hipFree(ws);
    }
    int frames() const override { return Tm; }
    int in_len() const override { return W * n_win; }
    int out_len() const override { return W * n_win; }          // the mask ISTFT's raw overlap-add length is exactly W per window
    int channels() const override { return 2; }                 // near end, far end (:1519)
    int out_channels() const override { return 1; }
    bool accepts_float_input() const override { return true; }
    int reserve(int batch, std::string& err) override;
    int run(hipStream_t s, const int16_t* d_in, int batch, int16_t* d_out, float* d_f32, std::string& err) override;
    int tap(hipStream_t s, const char* name, int batch, float* out, size_t count, size_t* written, std::string& err) override;
    // streams (ade_stream_*): state per stream object, see DfaStream below.  Audio only: the speech-probability head is not evaluated.
    int stream_delay() const override { return kDelay; }
    int stream_create(int n_streams, int frames_per_push, void** state, std::string& err) override;
    int stream_reset(void* state, hipStream_t s, std::string& err) override;
    int stream_push(void* state, hipStream_t s, const int16_t* d_in, int16_t* d_out, float* d_f32, std::string& err) override;
    int stream_flush(void* state, hipStream_t s, int16_t* d_out, float* d_f32, std::string& err) override;
    void stream_destroy(void* state) override;
    int stream_step(struct DfaStream* st, hipStream_t s, const int16_t* d_in, int16_t* d_out, float* d_f32, std::string& err);
};

// What a stream carries between pushes, for S streams that advance together: one allocation, its leading part cleared by a reset.
struct DfaStream {
    int S = 0, F = 0, Mmax = 0;                 // streams, hops per push, the most mask frames one step completes
    long long hops = 0;                         // hops pushed since the last reset
    void* nkf = nullptr;                        // the back end's own stream state
    int RN = 0, RT = 0;
    int16_t* near_ring = nullptr;               // [S][RN] near-end samples not yet consumed by a mask frame, sample a at a % RN
    float* temp_ring = nullptr;                 // [S][RT] temp_aec samples not yet consumed, sample a at a % RT
    float* hist[2] = {};                        // per layer [D][S][dilation (lorder - 1)]: the last frames of the projection output, ping-ponged
    std::vector<size_t> hist_off;               // a layer's offset inside hist[.]
    float* half[2] = {};                        // [S][320] the second half of the last synthesised frame, ping-ponged with hist (cur)
    float* pend[2] = {};                        // [S][256] final output samples not yet emitted, ping-ponged every step (pcur)
    int cur = 0, pcur = 0;
    float *temp = nullptr, *feat = nullptr, *x = nullptr, *f1 = nullptr, *p1 = nullptr, *mask = nullptr, *frames = nullptr;     // one step's workspace
    float2* spec = nullptr;
    void* block = nullptr;
    size_t reset_bytes = 0;
};

int dfsmn_aec_create(const std::map<std::string, Tensor>& tensors, int window_len, int n_win, bool exact_dft, int device, SubEngine** out, std::string& err) {
    *out = nullptr;
    if (!nkf_backend_create) return afail(err, ADE_ERR_UNSUPPORTED, "dfsmn_aec: the NKF back end is not built into this library");
    if (window_len < kNK || window_len % kHA)
        return afail(err, ADE_ERR_SHAPE_MISMATCH, "dfsmn_aec: the window (input_audio_length, or fold_window_length) must be a multiple of the 320-sample hop, at least 1024");
    bool missing = false;
    auto get = [&](const std::string& name, std::vector<int> dims, const float** p) -> bool {
        auto it = tensors.find(name);
        if (it == tensors.end()) { err = "weights: tensor missing: " + name; missing = true; return false; }
        if (it->second.dims != dims) { err = "weights: tensor has the wrong shape: " + name; return false; }
        *p = it->second.data;
        return true;
    };
    auto bad = [&]() { return missing ? ADE_ERR_MISSING_KEY : ADE_ERR_SHAPE_MISMATCH; };
    auto itw = tensors.find("feature_linear_weight");
    if (itw == tensors.end()) return afail(err, ADE_ERR_MISSING_KEY, "weights: tensor missing: feature_linear_weight");
    if (itw->second.dims.size() != 2 || itw->second.dims[1] != kFeat || itw->second.dims[0] < 1)
        return afail(err, ADE_ERR_SHAPE_MISMATCH, "weights: feature_linear_weight must be (width, 240)");
    const int D = itw->second.dims[0];
    auto its = tensors.find("fsmn_skip");
    if (its == tensors.end()) return afail(err, ADE_ERR_MISSING_KEY, "weights: tensor missing: fsmn_skip");
    const int depth = (int)its->second.count;
    const float *l1w, *l1b, *l2w, *l2b, *l3w, *l3b, *melp, *skipp, *dilp;
    if (!get("feature_linear_weight", {D, kFeat}, &l1w) || !get("feature_linear_bias", {D}, &l1b) || !get("linear2.weight", {kFA, D}, &l2w) ||
        !get("linear2.bias", {kFA}, &l2b) || !get("linear3.weight", {1, D}, &l3w) || !get("linear3.bias", {1}, &l3b) || !get("mel_banks", {kMelN, kFK}, &melp) ||
        !get("fsmn_skip", {depth}, &skipp) || !get("fsmn_dilation", {depth}, &dilp))
        return bad();
    struct HostLayer { const float *lw, *lb, *pw, *cw; int H, lo, dil, skip; };
    std::vector<HostLayer> hl((size_t)depth);
    int Hmax = 1;
    for (int i = 0; i < depth; ++i) {
        const std::string p = "deepfsmn." + std::to_string(i);
        auto itl = tensors.find(p + ".linear.weight");
        auto itc = tensors.find("fsmn_conv_weight_" + std::to_string(i));
        if (itl == tensors.end()) return afail(err, ADE_ERR_MISSING_KEY, "weights: tensor missing: " + p + ".linear.weight");
        if (itc == tensors.end()) return afail(err, ADE_ERR_MISSING_KEY, "weights: tensor missing: fsmn_conv_weight_" + std::to_string(i));
        if (itl->second.dims.size() != 2 || itl->second.dims[1] != D || itl->second.dims[0] < 1)
            return afail(err, ADE_ERR_SHAPE_MISMATCH, "weights: " + p + ".linear.weight must be (hidden, width)");
        if (itc->second.dims.size() != 3 || itc->second.dims[0] != D || itc->second.dims[1] != 1 || itc->second.dims[2] < 1)
            return afail(err, ADE_ERR_SHAPE_MISMATCH, "weights: fsmn_conv_weight_" + std::to_string(i) + " must be (width, 1, lorder)");
        HostLayer& h = hl[i];
        h.H = itl->second.dims[0];
        h.lo = itc->second.dims[2];
        h.dil = (int)dilp[i];
        h.skip = skipp[i] != 0.0f;
        if (h.dil < 1 || (float)h.dil != dilp[i]) return afail(err, ADE_ERR_BAD_VALUE, "weights: fsmn_dilation must hold positive integers");
        if (!get(p + ".linear.weight", {h.H, D}, &h.lw) || !get(p + ".linear.bias", {h.H}, &h.lb) || !get(p + ".project.weight", {D, h.H}, &h.pw) ||
            !get("fsmn_conv_weight_" + std::to_string(i), {D, 1, h.lo}, &h.cw))
            return bad();
        if (h.H > Hmax) Hmax = h.H;
    }
    std::unique_ptr<DfsmnAecEngine> d(new DfsmnAecEngine());
    d->device = device;
    d->W = window_len;
    d->n_win = n_win;
    d->Tm = (window_len - kNA) / kHA + 1;                      // MASK_FRAMES_A2 (:174); 640 + 320 (Tm - 1) == W
    d->D = D;
    d->Hmax = Hmax;
    d->depth = depth;
    NkfBackend* nb = nullptr;
    const int nst = nkf_backend_create(tensors, window_len, !exact_dft, device, &nb, err);
    if (nst != ADE_OK) return nst;
    d->nkf.reset(nb);

    std::vector<float> arena;
    auto push = [&](const float* src, size_t n) { const size_t off = arena.size(); arena.resize(off + ((n + 63) & ~(size_t)63), 0.0f); if (src) memcpy(&arena[off], src, n * sizeof(float)); return off; };
    std::vector<float> wk((size_t)kNA), wa;
    for (int n = 0; n < kNA; ++n) wk[n] = (float)(0.54 - 0.46 * cos(2.0 * M_PI * n / (double)(kNA - 1)));     // the fbank's float64 symmetric hamming, rounded once (:1051)
    hamming_symmetric_f32(kNA, wa);                                                                          // WINDOW_TYPE 'hamming_symmetric' for both mask transforms (:55)
    const size_t o_wk = push(wk.data(), wk.size()), o_wa = push(wa.data(), wa.size());
    auto twiddles = [&](int n) {
        std::vector<float> tw((size_t)2 * n);
        for (int m = 0; m < n; ++m) { const double a = -2.0 * M_PI * (double)m / (double)n; tw[2 * m] = (float)cos(a); tw[2 * m + 1] = (float)sin(a); }
        return push(tw.data(), tw.size());
    };
    const size_t o_tw1024 = twiddles(kNK), o_tw640 = twiddles(kNA);
    if (!fft::make_plan(kNK, &d->p1024) || !fft::make_plan(kNA, &d->p640)) return afail(err, ADE_ERR_UNSUPPORTED, "dfsmn_aec: FFT plan");
    const size_t o_iws = push(nullptr, (size_t)window_len);
    {
        std::vector<float> wsum((size_t)window_len, 0.0f);     // conv_transpose1d(ones, window^2, stride 320) in fp32 (STFT_Process.py:257-266)
        for (int t = 0; t < d->Tm; ++t)
            for (int n = 0; n < kNA; ++n) wsum[(size_t)t * kHA + n] += wa[n] * wa[n];
        for (int m = 0; m < window_len; ++m) arena[o_iws + m] = 1.0f / wsum[m];
    }
    // the mel bank as a band table: band b sums `count` consecutive bins from start[b] (zero-padded weights, so the sum is the dense row's term for term)
    std::vector<int> start(kMelN, 0);
    int count = 1;
    for (int b = 0; b < kMelN; ++b) {
        int lo = kFK, hi = -1;
        for (int f = 0; f < kFK; ++f)
            if (melp[(size_t)b * kFK + f] != 0.0f) { if (f < lo) lo = f; hi = f; }
        if (hi < 0) { lo = 0; hi = 0; }
        start[b] = lo;
        if (hi - lo + 1 > count) count = hi - lo + 1;
    }
    for (int b = 0; b < kMelN; ++b)
        if (start[b] + count > kFK) start[b] = kFK - count;
    std::vector<float> bw((size_t)count * kMelN, 0.0f);
    for (int b = 0; b < kMelN; ++b)
        for (int j = 0; j < count; ++j) bw[(size_t)j * kMelN + b] = melp[(size_t)b * kFK + start[b] + j];
    const size_t o_ms = push(nullptr, kMelN), o_mw = push(bw.data(), bw.size());
    memcpy(&arena[o_ms], start.data(), sizeof(int) * kMelN);
    const size_t o_l1w = push(l1w, (size_t)D * kFeat), o_l1b = push(l1b, D), o_l2w = push(l2w, (size_t)kFA * D), o_l2b = push(l2b, kFA), o_l3w = push(l3w, D),
                 o_l3b = push(l3b, 1);
    std::vector<size_t> o_h((size_t)4 * depth);
    for (int i = 0; i < depth; ++i) {
        o_h[4 * i] = push(hl[i].lw, (size_t)hl[i].H * D);
        o_h[4 * i + 1] = push(hl[i].lb, hl[i].H);
        o_h[4 * i + 2] = push(hl[i].pw, (size_t)D * hl[i].H);
        o_h[4 * i + 3] = push(hl[i].cw, (size_t)D * hl[i].lo);
    }
    if (hipSetDevice(device) != hipSuccess) return afail(err, ADE_ERR_DEVICE, "hipSetDevice failed");
    if (hipMalloc((void**)&d->d_w, arena.size() * sizeof(float)) != hipSuccess) return afail(err, ADE_ERR_DEVICE, "hipMalloc of the DFSMN-AEC weights failed");
    if (hipMemcpy(d->d_w, arena.data(), arena.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return afail(err, ADE_ERR_DEVICE, "upload of the DFSMN-AEC weights failed");
    float* w = d->d_w;
    d->win_k = w + o_wk; d->win_a = w + o_wa; d->inv_ws = w + o_iws;
    d->tw1024 = reinterpret_cast<const float2*>(w + o_tw1024); d->tw640 = reinterpret_cast<const float2*>(w + o_tw640);
    d->mel = BandTab{reinterpret_cast<const int*>(w + o_ms), w + o_mw, count, kMelN};
    d->lin1_w = w + o_l1w; d->lin1_b = w + o_l1b; d->lin2_w = w + o_l2w; d->lin2_b = w + o_l2b; d->lin3_w = w + o_l3w; d->lin3_b = w + o_l3b;
    for (int i = 0; i < depth; ++i)
        d->layers.push_back(DfsmnAecEngine::Layer{w + o_h[4 * i], w + o_h[4 * i + 1], w + o_h[4 * i + 2], w + o_h[4 * i + 3], hl[i].H, hl[i].lo, hl[i].dil, hl[i].skip});
    *out = d.release();
    return ADE_OK;
}

int DfsmnAecEngine::reserve(int calls, std::string& err) {
    if (calls <= capacity) return ADE_OK;
    const size_t rows = (size_t)calls * n_win, N = rows * Tm;
    if (N * kNA > 0x7fffffffULL || rows * (size_t)W > 0x7fffffffULL) return afail(err, ADE_ERR_BAD_VALUE, "dfsmn_aec: batch too large for one call");
    int st = nkf->reserve((int)rows, err);
    if (st != ADE_OK) return st;
    DA_HIP(hipSetDevice(device));
    DA_HIP(hipDeviceSynchronize());
    if (ws) (void)hipFree(ws);
    ws = nullptr;
    capacity = 0;
    const size_t sizes[10] = {rows * W, N * kFA * 2, N * kFeat, (size_t)D * N, (size_t)Hmax * N, (size_t)D * N, N * kFA, N, N * kNA, rows * W};
    size_t total = 0;
    for (size_t s : sizes) total += (s + 63) & ~(size_t)63;
    DA_HIP(hipMalloc((void**)&ws, total * sizeof(float)));
    float* p[10];
    size_t off = 0;
    for (int i = 0; i < 10; ++i) { p[i] = ws + off; off += (sizes[i] + 63) & ~(size_t)63; }
    temp = p[0]; spec = reinterpret_cast<float2*>(p[1]); feat = p[2]; x = p[3]; f1 = p[4]; p1 = p[5]; mask = p[6]; vad = p[7]; frames_buf = p[8]; wave = p[9];
    capacity = calls;
    return ADE_OK;
}

int DfsmnAecEngine::run(hipStream_t s, const int16_t* d_in, int batch, int16_t* d_out, float* d_f32, std::string& err) {
    if (batch == 0) return ADE_OK;
    int st = reserve(batch, err);
    if (st != ADE_OK) return st;
    using namespace gemm;
    const int rows = batch * n_win, N = rows * Tm;
    // 1. the linear canceller: temp_aec                                                                   (:1277-1282)
    st = nkf->run(s, d_in, float_in, batch, n_win, temp, err);
    if (st != ADE_OK) return st;
    // 2. Kaldi features of near / temp_aec / echo estimate and the mask transform of temp_aec               (:1288-1311)
    hipLaunchKernelGGL(k_dfa_features<CallSrc>, dim3((unsigned)((N + kGroup - 1) / kGroup)), dim3(256), 0, s, CallSrc{d_in, float_in, temp, W, Tm, n_win}, N, p1024, p640,
                       tw1024, tw640, win_k, win_a, mel, spec, feat);
    // 3. the mask network                                                                                  (:1312-1320)
    launch(s, RowMajorA{lin1_w, kFeat}, FeatFrameB{feat}, BiasActStore<kActRelu>{x, N, lin1_b, 0.0f}, D, N, kFeat);
    for (const Layer& l : layers) {
        launch(s, RowMajorA{l.lin_w, D}, RowMajorB{x, N}, BiasActStore<kActRelu>{f1, N, l.lin_b, 0.0f}, l.H, N, D);
        launch(s, RowMajorA{l.proj_w, l.H}, RowMajorB{f1, N}, BiasActStore<kActNone>{p1, N, nullptr, 0.0f}, D, N, l.H);
        const long long total = (long long)D * N;
        hipLaunchKernelGGL(k_dfa_memory, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)p1, l.conv_w, x, N, Tm, l.lorder, l.dilation, l.skip, total);
    }
    launch(s, RowMajorA{lin3_w, D}, RowMajorB{x, N}, BiasActStore<kActSigmoid>{vad, N, lin3_b, 0.0f}, 1, N, D);
    launch(s, RowMajorA{lin2_w, D}, RowMajorB{x, N}, MaskTStore{mask, lin2_b}, kFA, N, D);
    // 4. masked spectrum -> ISTFT frames, overlap-add, PCM tail                                             (:1323-1347)
    hipLaunchKernelGGL(k_dfa_synthesis, dim3((unsigned)(rows * ((Tm + 1) / 2))), dim3(256), 0, s, (const float2*)spec, (const float*)mask, Tm, p640, tw640, win_a, frames_buf);
    const long long total = (long long)rows * W;
    hipLaunchKernelGGL(k_dfa_ola, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)frames_buf, inv_ws, Tm, W, wave, d_out, d_f32, total);
    DA_HIP(hipGetLastError());
    return ADE_OK;
}

int DfsmnAecEngine::tap(hipStream_t s, const char* name, int batch, float* out, size_t count, size_t* written, std::string& err) {
    if (!ws || batch <= 0 || batch > capacity) return afail(err, ADE_ERR_NOT_FOUND, "tap has no data yet");
    const size_t rows = (size_t)batch * n_win, N = rows * Tm;
    const float* src = nullptr;
    size_t n = 0;
    if (strcmp(name, "temp_aec") == 0) { src = temp; n = rows * W; }                              // [window][W]
    else if (strcmp(name, "feat") == 0) { src = feat; n = N * kFeat; }                            // [frame][240]
    else if (strcmp(name, "spec") == 0) { src = reinterpret_cast<const float*>(spec); n = N * kFA * 2; }     // [frame][321] (re, im)
    else if (strcmp(name, "mask") == 0) { src = mask; n = N * kFA; }                              // [frame][321]
    else if (strcmp(name, "vad_results") == 0) { src = vad; n = N; }                              // [frame]
    else if (strcmp(name, "wave") == 0) { src = wave; n = rows * W; }                             // [call][n_win * W]
    else return afail(err, ADE_ERR_NOT_FOUND, std::string("unknown tap: ") + name);
    if (count < n) return afail(err, ADE_ERR_SHAPE_MISMATCH, "tap buffer too small");
    DA_HIP(hipStreamSynchronize(s));
    DA_HIP(hipMemcpy(out, src, n * sizeof(float), hipMemcpyDeviceToHost));
    *written = n;
    return ADE_OK;
}

// ---- streams ----------------------------------------------------------------------------------------------------------------------------------------------------
namespace {
long long mask_frames_after(long long hops) {           // M(k): the mask frames complete after k hops of input
    const long long nt = hops > 3 ? (hops - 3) * 256 : 0;
    return nt < kNA ? 0 : (nt - kNA) / kHA + 1;
}
}  // namespace

int DfsmnAecEngine::stream_create(int n_streams, int frames_per_push, void** state, std::string& err) {
    *state = nullptr;
    if (n_streams < 1 || frames_per_push < 1 || frames_per_push > 4096)
        return afail(err, ADE_ERR_BAD_VALUE, "ade_stream_create: dfsmn_aec needs n_streams >= 1 and 1 <= frames_per_push <= 4096");
    const int P = frames_per_push * 256, Pmax = P > 768 ? P : 768;                    // the flush is a step of the back end's last 768 samples
    const int Mmax = P / kHA + 1 > 3 ? P / kHA + 1 : 3;                               // the flush completes at most three frames
    const size_t S = (size_t)n_streams, N = S * Mmax;
    if (N * kNA > 0x7fffffffULL || S * (size_t)(Pmax + kNearLag) > 0x7fffffffULL)
        return afail(err, ADE_ERR_BAD_VALUE, "ade_stream_create: dfsmn_aec: n_streams * frames_per_push exceeds the launch grid");
    std::unique_ptr<DfaStream> st(new DfaStream());
    st->S = n_streams; st->F = frames_per_push; st->Mmax = Mmax;
    st->RN = Pmax + kNearLag; st->RT = Pmax + kTempLag;
    int rc = nkf->stream_create(n_streams, frames_per_push, &st->nkf, err);
    if (rc != ADE_OK) return rc;
    auto up = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    size_t hist_floats = 0;
    for (const Layer& l : layers) { st->hist_off.push_back(hist_floats); hist_floats += (size_t)D * S * l.dilation * (l.lorder - 1); }
    const size_t b_near = up(S * st->RN * sizeof(int16_t)), b_temp = up(S * st->RT * sizeof(float)), b_hist = up(hist_floats * sizeof(float)), b_half = up(S * kHA * sizeof(float)),
                 b_pend = up(S * kPend * sizeof(float));
    const size_t work[8] = {up(S * Pmax * sizeof(float)), up(N * kFA * sizeof(float2)), up(N * kFeat * sizeof(float)), up((size_t)D * N * sizeof(float)),
                            up((size_t)Hmax * N * sizeof(float)), up((size_t)D * N * sizeof(float)), up(N * kFA * sizeof(float)), up(N * kNA * sizeof(float))};
    size_t total = b_near + b_temp + 2 * b_hist + 2 * b_half + 2 * b_pend;
    st->reset_bytes = total;
    for (size_t b : work) total += b;
    if (hipSetDevice(device) != hipSuccess || hipMalloc(&st->block, total) != hipSuccess) {
        nkf->stream_destroy(st->nkf);
        return afail(err, ADE_ERR_DEVICE, "ade_stream_create: hipMalloc of the DFSMN-AEC stream state failed");
    }
    char* p = (char*)st->block;
    st->near_ring = (int16_t*)p; p += b_near;
    st->temp_ring = (float*)p; p += b_temp;
    for (int i = 0; i < 2; ++i) { st->hist[i] = (float*)p; p += b_hist; }
    for (int i = 0; i < 2; ++i) { st->half[i] = (float*)p; p += b_half; }
    for (int i = 0; i < 2; ++i) { st->pend[i] = (float*)p; p += b_pend; }
    st->temp = (float*)p; p += work[0];
    st->spec = (float2*)p; p += work[1];
    st->feat = (float*)p; p += work[2];
    st->x = (float*)p; p += work[3];
    st->f1 = (float*)p; p += work[4];
    st->p1 = (float*)p; p += work[5];
    st->mask = (float*)p; p += work[6];
    st->frames = (float*)p;
    *state = st.release();
    return ADE_OK;
}

int DfsmnAecEngine::stream_reset(void* state, hipStream_t s, std::string& err) {
    DfaStream* st = (DfaStream*)state;
    const int rc = nkf->stream_reset(st->nkf, s, err);
    if (rc != ADE_OK) return rc;
    DA_HIP(hipMemsetAsync(st->block, 0, st->reset_bytes, s));
    st->hops = 0;
    st->cur = 0;
    st->pcur = 0;
    return ADE_OK;
}

// One step: a push of F hops (d_in set), or the flush (d_in null: the back end's last 768 temp_aec samples, the remaining mask frames, 1344 output samples).
int DfsmnAecEngine::stream_step(DfaStream* st, hipStream_t s, const int16_t* d_in, int16_t* d_out, float* d_f32, std::string& err) {
    using namespace gemm;
    const bool flush = d_in == nullptr;
    const int S = st->S, P = flush ? 0 : st->F * 256, Pt = flush ? 768 : P, Pout = flush ? kDelay : P;
    const long long k0 = st->hops, k1 = k0 + (flush ? 0 : st->F);
    const long long M0 = mask_frames_after(k0), M1 = flush ? (k0 * 256 - kNA) / kHA + 1 : mask_frames_after(k1);
    const int Mp = (int)(M1 - M0), N = S * Mp;
    // 1. the linear canceller: the step's temp_aec samples, signal samples 256 k0 - 768 onwards
    int rc = flush ? nkf->stream_flush(st->nkf, s, st->temp, err) : nkf->stream_step(st->nkf, s, d_in, st->temp, err);
    if (rc != ADE_OK) return rc;
    // 2. into the rings, addressed by the signal's sample index
    const long long t_first = k0 * 256 - 768;                                             // signal index of the step's first temp_aec sample (negative: not a sample)
    const int t_min = t_first < 0 ? (int)-t_first : 0;
    {
        const long long total = (long long)S * (P + Pt);
        hipLaunchKernelGGL(k_dfa_stream_stage, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_in, (const float*)st->temp, P, Pt, t_min, st->near_ring, st->temp_ring,
                           st->RN, st->RT, (int)((k0 * 256) % st->RN), (int)(((t_first % st->RT) + st->RT) % st->RT), total);
    }
    const int nxt = st->cur ^ 1;
    if (Mp > 0) {
        // 3. features and the mask transform of the frames this step completes
        const RingSrc src{st->near_ring, st->temp_ring, Mp, st->RN, st->RT, (int)((M0 * kHA) % st->RN), (int)((M0 * kHA) % st->RT)};
        hipLaunchKernelGGL(k_dfa_features<RingSrc>, dim3((unsigned)((N + kGroup - 1) / kGroup)), dim3(256), 0, s, src, N, p1024, p640, tw1024, tw640, win_k, win_a, mel, st->spec,
                           st->feat);
        // 4. the mask network, the memory continued from each layer's history
        launch(s, RowMajorA{lin1_w, kFeat}, FeatFrameB{st->feat}, BiasActStore<kActRelu>{st->x, N, lin1_b, 0.0f}, D, N, kFeat);
        for (size_t li = 0; li < layers.size(); ++li) {
            const Layer& l = layers[li];
            launch(s, RowMajorA{l.lin_w, D}, RowMajorB{st->x, N}, BiasActStore<kActRelu>{st->f1, N, l.lin_b, 0.0f}, l.H, N, D);
            launch(s, RowMajorA{l.proj_w, l.H}, RowMajorB{st->f1, N}, BiasActStore<kActNone>{st->p1, N, nullptr, 0.0f}, D, N, l.H);
            const int Hl = l.dilation * (l.lorder - 1);
            const long long total = (long long)D * N, total_all = total + (long long)D * S * Hl;
            hipLaunchKernelGGL(k_dfa_stream_memory, dim3((unsigned)((total_all + 255) / 256)), dim3(256), 0, s, (const float*)st->p1, l.conv_w, st->x,
                               (const float*)(st->hist[st->cur] + st->hist_off[li]), st->hist[nxt] + st->hist_off[li], S, Mp, Hl, l.lorder, l.dilation, l.skip, total, total_all);
        }
        launch(s, RowMajorA{lin2_w, D}, RowMajorB{st->x, N}, MaskTStore{st->mask, lin2_b}, kFA, N, D);
        // 5. one inverse transform per frame
        hipLaunchKernelGGL(k_dfa_stream_synthesis, dim3((unsigned)N), dim3(256), 0, s, (const float2*)st->spec, (const float*)st->mask, Mp, p640, tw640, win_a, st->frames,
                           st->half[nxt]);
    }
    // 6. overlap-add, norm, the samples kept for the next step, PCM tail
    {
        const long long e_first = k0 * 256 - kDelay;                                      // signal index of the step's first output sample
        const int e_rel = (int)(e_first - M0 * kHA), n_pend = M0 > 0 ? -e_rel : 0;
        const long long total = (long long)S * (Pout + (flush ? 0 : kPend));
        hipLaunchKernelGGL(k_dfa_stream_out, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)st->frames, (const float*)st->half[st->cur],
                           (const float*)st->pend[st->pcur], flush ? (float*)nullptr : st->pend[st->pcur ^ 1], inv_ws, W, Mp, Pout, e_rel, n_pend, M0 > 0 ? 1 : 0, M0 == 0 ? 1 : 0,
                           flush ? Mp * kHA : 0x7fffffff, d_out, d_f32, total);
    }
    DA_HIP(hipGetLastError());
    if (Mp > 0) st->cur = nxt;
    st->pcur ^= 1;
    st->hops = k1;
    return ADE_OK;
}

int DfsmnAecEngine::stream_push(void* state, hipStream_t s, const int16_t* d_in, int16_t* d_out, float* d_f32, std::string& err) {
    return stream_step((DfaStream*)state, s, d_in, d_out, d_f32, err);
}

int DfsmnAecEngine::stream_flush(void* state, hipStream_t s, int16_t* d_out, float* d_f32, std::string& err) {
    DfaStream* st = (DfaStream*)state;
    if (st->hops < 5 || st->hops % 5)
        return afail(err, ADE_ERR_BAD_VALUE, "ade_stream_flush: dfsmn_aec ends a signal only where the reference's static export accepts its length, a multiple of 320 samples: "
                                             "the hops pushed must be a multiple of 5, at least 5 (pushed: " + std::to_string(st->hops) + ")");
    return stream_step(st, s, nullptr, d_out, d_f32, err);
}

void DfsmnAecEngine::stream_destroy(void* state) {
    DfaStream* st = (DfaStream*)state;
    if (!st) return;
    (void)hipSetDevice(device);
    if (st->nkf) nkf->stream_destroy(st->nkf);
    if (st->block) (void)hipFree(st->block);
    delete st;
}

}  // namespace ade
