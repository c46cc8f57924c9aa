// ade_dfsmn.hip — DFSMN (48 kHz acoustic noise suppression) on the MI355X: SURVEY.md section 8 row a19.
//
// Reference: DFSMN.forward, DFSMN/Export_DFSMN.py:180-246, and the buffers its constructor builds (:86-178):
//   int16 -> * 2^-15 -> ONE strided analysis convolution [Kaldi fbank (DC removal + 0.97 pre-emphasis + symmetric hamming
//   + 2048-pt DFT, folded into a (2050, 1920) matrix) | 1920-pt mask STFT] -> power -> mel(120) -> log ->
//   Linear(120,256)+ReLU -> 9 x [Linear+ReLU, Linear (no bias), causal depthwise memory (lorder 20) with the inner
//   residual folded into the current tap, outer residual] -> Linear(256,961)+Sigmoid -> mask * spectrum ->
//   ISTFT (periodic hamming, no centre pad, static COLA) -> * 32768, clamp, truncate -> int16.
// The two analysis transforms and the synthesis are FFTs (csrc/ade_fft.h: one workgroup per frame, mixed-radix Stockham passes in LDS -- 2048 = 4^5 x 2 for the
// Kaldi filter bank, 1920 = 4^3 x 2 x 3 x 5 for the mask STFT and its inverse): 0.3 MFLOP per frame instead of the 22.9 MFLOP of the reference's dense
// (3972 + 1922) x 1920 windowed-DFT products, which used to be 67 % of this model's step as matrix-core GEMMs.  The steps the reference folds into its
// analysis matrix -- DC removal, 0.97 pre-emphasis, symmetric hamming (:97-120) -- are applied to the frame explicitly before the 2048-point transform.
// The mask network is matrix products and stays on the generic matrix-core GEMM of csrc/ade_gemm.h (activations channels-first (C, N), N = batch * frames):
//   analysis   P(N, 1025) = |FFT_2048(hamming * preemph(frame - mean))|^2 * 2^30 ;  S(N, 2 x 961) = FFT_1920(hamming * frame)         k_dfsmn_analysis
//   log-mel    F(120, N)  = mel(120, 1025) x P^T                         store = log(max(., eps))
//   layers     X(256, N)  = relu(W x + b) ...                            store = bias + ReLU / none ; the last one bias + sigmoid, transposed to (N, 961)
//   synthesis  frames(N, 1920) = hamming_periodic * Re IFFT_1920(hermitian(mask * S))                                                   k_dfsmn_synthesis
// followed by a gather overlap-add with the PCM tail fused.  Twiddles are exact (double-precision angles), like the dense tables they replace.
//
// Streams (ade_stream_* on a dfsmn handle, include/ade.h): the model is causal from end to end -- per-frame Kaldi mean, no centre
// pad, a memory that looks lorder - 1 frames back -- so a push of F hops (960 samples each) continues the signal, one hop behind the input:
//   k_dfsmn_stream_analysis   rows [960 carried | 960 F new]; ONE frame per transform, each real transform as a half-length complex FFT plus a split pass
//   mask network              the same GEMMs, N = streams x the frames the push completes
//   k_dfsmn_stream_memory     the memory with the frames before the push taken from the layer's history, which it also renews
//   k_dfsmn_stream_synthesis  the Hermitian inverse of one frame as a 960-point complex transform
//   k_dfsmn_stream_out        two-frame overlap-add from the carried half frame, / the window-square sum, the PCM tail, the next carried half
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

constexpr int kKaldiNfft = 2048, kFrame = 1920, kHopD = 960, kNfftD = 1920;
constexpr int kFbBins = kKaldiNfft / 2 + 1;      // 1025
constexpr int kStBins = kNfftD / 2 + 1;          // 961
constexpr int kMel = 120, kHid = 256;

struct PowerFrameB {           // B(f, j) = power bin f of frame j (frame-major P, written by k_dfsmn_analysis)   (:216)
    static constexpr bool kAlongN = false;
    const float* p;
    __device__ float operator()(int f, int j) const { return p[(size_t)j * kFbBins + f]; }
};
struct SigmoidTStore {         // mask[j][f] = sigmoid(v + bias[f]): the last Linear, stored frame-major for the per-frame synthesis kernel   (:230)
    static constexpr bool kCtx = true;
    float* out;
    const float* bias;
    __device__ float row(int f) const { return bias[f]; }
    __device__ gemm::None col(int) const { return gemm::None{}; }
    __device__ gemm::None pre(int, int, float) const { return gemm::None{}; }
    __device__ void operator()(int f, int j, float v, float b, gemm::None, gemm::None) const { out[(size_t)j * kStBins + f] = 1.0f / (1.0f + expf(-(v + b))); }
};

// One workgroup per PAIR of frames: [Kaldi filter-bank power | mask STFT] of each frame's 1920 samples.  Both transforms take real input, so the two frames ride one
// complex FFT as real and imaginary part: Z = FFT(x0 + i x1), X0[f] = (Z[f] + conj Z[N - f]) / 2, X1[f] = (Z[f] - conj Z[N - f]) / (2 i) -- half the butterflies.
//   x = samples * 2^-15 (:186-190); fbank branch: y = x - mean(x); z[n] = y[n] - 0.97 y[n - 1] (z[0] = 0.03 y[0]); * symmetric hamming; zero-pad to 2048;
//   FFT; power = (re^2 + im^2) * 2^30 -- the steps Export_DFSMN.py:97-120 folds into its analysis matrix, in Kaldi's order.  STFT branch: x * hamming; FFT_1920.
__global__ __launch_bounds__(256) void k_dfsmn_analysis(const int16_t* __restrict__ pcm, const float* __restrict__ fpcm, int L, int T, fft::Plan p2048, fft::Plan p1920,
                                                        const float2* __restrict__ tw2048, const float2* __restrict__ tw1920, const float* __restrict__ win_fb,
                                                        const float* __restrict__ win_st, float* __restrict__ power, float* __restrict__ spec) {
    __shared__ float2 A[kKaldiNfft];
    __shared__ float2 B[kKaldiNfft];
    __shared__ double red[2][256];
    const int tid = threadIdx.x;
    int frame[2];
    size_t at[2];
    bool live[2];
    const int ppr = (T + 1) / 2, b = (int)blockIdx.x / ppr, t0 = 2 * ((int)blockIdx.x - b * ppr);      // pairs never straddle two calls: a row's result must not depend
#pragma unroll                                                                                          // on which row shares its transform (batch rows are independent calls)
    for (int u = 0; u < 2; ++u) {
        live[u] = t0 + u < T;
        const int t = live[u] ? t0 + u : t0;
        frame[u] = b * T + t;
        at[u] = (size_t)b * L + (size_t)t * kHopD;
    }
    auto sample = [&](int u, int n) { return (fpcm ? fpcm[at[u] + n] : (float)pcm[at[u] + n]) * (1.0f / 32768.0f); };
    double part[2] = {0.0, 0.0};
    for (int n = tid; n < kFrame; n += 256) { part[0] += (double)sample(0, n); part[1] += (double)sample(1, n); }
    red[0][tid] = part[0];
    red[1][tid] = part[1];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
        __syncthreads();
    }
    const float mean[2] = {(float)(red[0][0] / (double)kFrame), (float)(red[1][0] / (double)kFrame)};
    for (int n = tid; n < kKaldiNfft; n += 256) {
        float v[2] = {0.0f, 0.0f};
        if (n < kFrame) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float y = sample(u, n) - mean[u], yp = sample(u, n > 0 ? n - 1 : 0) - mean[u];
                v[u] = live[u] ? (y - 0.97f * yp) * win_fb[n] : 0.0f;          // an odd row's last frame is paired with zeros
            }
        }
        A[n] = make_float2(v[0], v[1]);
    }
    float2* r = fft::forward(A, B, p2048, tw2048, tid, 256);
    for (int f = tid; f < kFbBins; f += 256) {
        const float2 z = r[f], zc = r[f == 0 ? 0 : kKaldiNfft - f];
        const float re0 = 0.5f * (z.x + zc.x), im0 = 0.5f * (z.y - zc.y), re1 = 0.5f * (z.y + zc.y), im1 = 0.5f * (zc.x - z.x);
        if (live[0]) power[(size_t)frame[0] * kFbBins + f] = (re0 * re0 + im0 * im0) * (32768.0f * 32768.0f);
        if (live[1]) power[(size_t)frame[1] * kFbBins + f] = (re1 * re1 + im1 * im1) * (32768.0f * 32768.0f);
    }
    __syncthreads();
    for (int n = tid; n < kNfftD; n += 256) { const float w = win_st[n]; A[n] = make_float2(sample(0, n) * w, live[1] ? sample(1, n) * w : 0.0f); }
    r = fft::forward(A, B, p1920, tw1920, tid, 256);
    for (int f = tid; f < kStBins; f += 256) {
        const float2 z = r[f], zc = r[f == 0 ? 0 : kNfftD - f];
        if (live[0]) {
            spec[(size_t)frame[0] * 2 * kStBins + f] = 0.5f * (z.x + zc.x);
            spec[(size_t)frame[0] * 2 * kStBins + kStBins + f] = 0.5f * (z.y - zc.y);
        }
        if (live[1]) {
            spec[(size_t)frame[1] * 2 * kStBins + f] = 0.5f * (z.y + zc.y);
            spec[(size_t)frame[1] * 2 * kStBins + kStBins + f] = 0.5f * (zc.x - z.x);
        }
    }
}

// One workgroup per PAIR of frames: mask * spectrum (:236-237) -> Hermitian extension -> inverse FFT_1920 -> * periodic hamming / N = the reference's inverse table applied
// to the masked half spectrum (its sine rows of the DC and Nyquist bins are zero, so their imaginary parts do not contribute: set to zero here).
// x N = sum_f Z[f] e^{+i theta} = conj(DFT(conj Z)) with Z Hermitian; two frames share one transform as W = H(Z0) + i H(Z1): x0 + i x1 = conj(DFT(conj W)) / N.
__global__ __launch_bounds__(256) void k_dfsmn_synthesis(const float* __restrict__ spec, const float* __restrict__ mask, int T, fft::Plan p1920, const float2* __restrict__ tw1920,
                                                         const float* __restrict__ win_syn, float* __restrict__ frames) {
    __shared__ float2 A[kNfftD];
    __shared__ float2 B[kNfftD];
    const int tid = threadIdx.x, ppr = (T + 1) / 2, b = (int)blockIdx.x / ppr, t0 = 2 * ((int)blockIdx.x - b * ppr);   // pairs inside one call's row, as in the analysis
    const int f0 = b * T + t0, f1 = f0 + 1;
    const bool two = t0 + 1 < T;
    const float *sp0 = spec + (size_t)f0 * 2 * kStBins, *mk0 = mask + (size_t)f0 * kStBins;
    const float *sp1 = spec + (size_t)(two ? f1 : f0) * 2 * kStBins, *mk1 = mask + (size_t)(two ? f1 : f0) * kStBins;
    for (int f = tid; f < kStBins; f += 256) {
        const bool edge = f == 0 || f == kStBins - 1;
        const float m0 = mk0[f], m1 = two ? mk1[f] : 0.0f;
        const float2 z0 = make_float2(sp0[f] * m0, edge ? 0.0f : sp0[kStBins + f] * m0), z1 = make_float2(sp1[f] * m1, edge ? 0.0f : sp1[kStBins + f] * m1);
        // W[f] = z0 + i z1 = (z0.x - z1.y, z0.y + z1.x); W[N - f] = conj z0 + i conj z1 = (z0.x + z1.y, z1.x - z0.y); both stored conjugated
        A[f] = make_float2(z0.x - z1.y, -(z0.y + z1.x));
        if (!edge) A[kNfftD - f] = make_float2(z0.x + z1.y, z0.y - z1.x);
    }
    const float2* r = fft::forward(A, B, p1920, tw1920, tid, 256);
    for (int n = tid; n < kNfftD; n += 256) {
        const float w = win_syn[n];
        frames[(size_t)f0 * kNfftD + n] = (r[n].x * (1.0f / (float)kNfftD)) * w;
        if (two) frames[(size_t)f1 * kNfftD + n] = (-r[n].y * (1.0f / (float)kNfftD)) * w;
    }
}

// causal depthwise memory + outer residual: x[c][j] += sum_k w[c][k] * p1[c][j - (lo-1) + k], zero before the row's first frame (:228-229)
__global__ __launch_bounds__(256) void k_fsmn_memory(const float* __restrict__ p1, const float* __restrict__ w, float* __restrict__ x, int N, int T,
                                                     int lo, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i / N), j = (int)(i - (long long)c * N);
    const int t = j % T;
    float s = 0.0f;
    const float* row = p1 + (size_t)c * N + j;
    for (int k = 0; k < lo; ++k) {                   // unconditional loads from clamped frames, masked afterwards: a branch around each load would serialise the taps
        const int dt = k - (lo - 1);
        const bool ok = t + dt >= 0;
        const float v = row[ok ? dt : 0];
        s += ok ? w[c * lo + k] * v : 0.0f;
    }
    x[i] += s;
}

// conv_transpose overlap-add as a gather, / static COLA sum, then the PCM tail (:238-244)
__global__ __launch_bounds__(256) void k_dfsmn_ola_pcm(const float* __restrict__ frames, const float* __restrict__ wsum, int16_t* __restrict__ pcm,
                                                       float* __restrict__ f32, int T, int out_len, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int b = (int)(i / out_len), m = (int)(i - (long long)b * out_len);
    int t_hi = m / kHopD;
    if (t_hi > T - 1) t_hi = T - 1;
    const int t_lo = m - kNfftD + 1 <= 0 ? 0 : (m - kNfftD + kHopD) / kHopD;
    float s = 0.0f;
    for (int t = t_lo; t <= t_hi; ++t) s += frames[((size_t)b * T + t) * kNfftD + (m - t * kHopD)];
    const float y = s / wsum[m];
    if (f32) f32[i] = y;
    if (pcm) pcm[i] = (short)(int)fminf(fmaxf(y * 32768.0f, -32768.0f), 32767.0f);
}

// ---- streams ----------------------------------------------------------------------------------------------------------------------------------------------------
constexpr int kHalfK = kKaldiNfft / 2, kHalfS = kNfftD / 2;      // 1024, 960: the complex lengths of the two real transforms

using fft::split_bin;      // a real transform as a half-length complex one plus a split pass (ade_fft.h)

// One workgroup per frame the push completes, plus one per stream that renews the carried input.  A stream's row is [960 carried samples | the push's 960 F samples];
// completed frame i of stream s (column s * Mp + i) covers row samples [off + 960 i, off + 960 i + 1920): off = 0, or 960 on a fresh stream, whose carried samples are
// no signal.  ONE frame per transform: k_dfsmn_analysis rides two frames on one complex FFT and the partner's rounding leaks into a frame, which would make a frame's
// bits depend on where a push ends.  Each real transform is instead a half-length complex one (2048 real -> 1024 complex, 1920 real -> 960 complex: even samples the
// real part, odd the imaginary) and a split pass; the butterflies per frame stay what the paired kernel spends, the LDS per workgroup halves.
// The Kaldi branch keeps k_dfsmn_analysis's order: mean in double, subtract, 0.97 pre-emphasis, symmetric hamming, zero pad.
__global__ __launch_bounds__(256) void k_dfsmn_stream_analysis(const int16_t* __restrict__ in, const int16_t* __restrict__ carry_in, int16_t* __restrict__ carry_out, int P, int Mp, int N,
                                                               int off, fft::Plan p1024, fft::Plan p960, const float2* __restrict__ tw1024, const float2* __restrict__ tw960,
                                                               const float2* __restrict__ tw2048, const float2* __restrict__ tw1920, const float* __restrict__ win_fb,
                                                               const float* __restrict__ win_st, float* __restrict__ power, float* __restrict__ spec) {
    __shared__ float2 A[kHalfK];
    __shared__ float2 B[kHalfK];
    __shared__ double red[256];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= N) {                   // the row's last 960 samples (always of this push: F >= 1) are what the next push's first frame starts with
        const int s = (int)blockIdx.x - N;
        for (int n = tid; n < kHopD; n += 256) carry_out[(size_t)s * kHopD + n] = in[(size_t)s * P + (P - kHopD) + n];
        return;
    }
    const int fr = (int)blockIdx.x, s = fr / Mp, i = fr - s * Mp, r0 = off + i * kHopD;
    const int16_t *old = carry_in + (size_t)s * kHopD, *row = in + (size_t)s * P;               // row position r: old[r] below 960, row[r - 960] from there on
    auto sample = [&](int n) { const int r = r0 + n; return (float)(r < kHopD ? old[r] : row[r - kHopD]) * (1.0f / 32768.0f); };
    double part = 0.0;
    for (int n = tid; n < kFrame; n += 256) part += (double)sample(n);
    red[tid] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const float mean = (float)(red[0] / (double)kFrame);
    for (int m = tid; m < kHalfK; m += 256) {
        float v[2] = {0.0f, 0.0f};
        if (2 * m < kFrame) {
            const float yp = sample(m > 0 ? 2 * m - 1 : 0) - mean, y0 = sample(2 * m) - mean, y1 = sample(2 * m + 1) - mean;
            v[0] = (y0 - 0.97f * yp) * win_fb[2 * m];
            v[1] = (y1 - 0.97f * y0) * win_fb[2 * m + 1];
        }
        A[m] = make_float2(v[0], v[1]);
    }
    float2* r = fft::forward(A, B, p1024, tw1024, tid, 256);
    for (int f = tid; f < kFbBins; f += 256) {
        const float2 x = split_bin(r, f, kHalfK, tw2048);
        power[(size_t)fr * kFbBins + f] = (x.x * x.x + x.y * x.y) * (32768.0f * 32768.0f);
    }
    __syncthreads();
    for (int m = tid; m < kHalfS; m += 256) A[m] = make_float2(sample(2 * m) * win_st[2 * m], sample(2 * m + 1) * win_st[2 * m + 1]);
    r = fft::forward(A, B, p960, tw960, tid, 256);
    for (int f = tid; f < kStBins; f += 256) {
        const float2 x = split_bin(r, f, kHalfS, tw1920);
        spec[(size_t)fr * 2 * kStBins + f] = x.x;
        spec[(size_t)fr * 2 * kStBins + kStBins + f] = x.y;
    }
}

// k_fsmn_memory over the Mp frames a push completes, column j = stream * Mp + i.  A tap that reaches before the push reads the layer's history, hist_in [c][stream][Hl]:
// the Hl = lo - 1 frames of p1 before the push, oldest first, zeros before the stream's first frame (the reset's memset).  The taps are summed in k_fsmn_memory's
// order.  The threads from `total` on write the next history into hist_out: the last Hl frames of [history | push].
__global__ __launch_bounds__(256) void k_dfsmn_stream_memory(const float* __restrict__ p1, const float* __restrict__ w, float* __restrict__ x, const float* __restrict__ hist_in,
                                                             float* __restrict__ hist_out, int S, int Mp, int Hl, int lo, long long total, long long total_all) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total_all) return;
    const int N = S * Mp;
    if (i < total) {
        const int c = (int)(i / N), j = (int)(i - (long long)c * N), st = j / Mp, t = j - st * Mp;
        const float* row = p1 + (size_t)c * N + j;
        const float* old = hist_in + ((size_t)c * S + st) * Hl + Hl + t;          // old[dt]: frame t + dt of the push, t + dt < 0
        float s = 0.0f;
        for (int k = 0; k < lo; ++k) {
            const int dt = k - (lo - 1);
            const float v = t + dt >= 0 ? row[dt] : old[dt];
            s += w[c * lo + k] * v;
        }
        x[i] += s;
        return;
    }
    const long long e = i - total;                                                // (c, stream, slot): slot q holds frame Mp - Hl + q of the push
    const int q = (int)(e % Hl), cs = (int)(e / Hl), c = cs / S, st = cs - c * S, t = Mp - Hl + q;
    hist_out[e] = t >= 0 ? p1[(size_t)c * N + (size_t)st * Mp + t] : hist_in[(size_t)cs * Hl + (Hl + t)];
}

// One workgroup per frame: mask * spectrum (:236-237) -> the Hermitian inverse 1920-point transform of ONE frame as a 960-point complex one -> * periodic hamming / N.
// With X the masked half spectrum (imaginary parts of the DC and Nyquist bins zero, as in k_dfsmn_synthesis) and h = 960:
//   W[f] = (X[f] + conj X[h - f]) + i (X[f] - conj X[h - f]) e^{+2 pi i f / N},  f < h;   x[2 m] + i x[2 m + 1] = (1 / N) sum_f W[f] e^{+2 pi i f m / h} = conj(DFT_h(conj W))[m] / N
__global__ __launch_bounds__(256) void k_dfsmn_stream_synthesis(const float* __restrict__ spec, const float* __restrict__ mask, fft::Plan p960, const float2* __restrict__ tw960,
                                                                const float2* __restrict__ tw1920, const float* __restrict__ win_syn, float* __restrict__ frames) {
    __shared__ float2 A[kHalfS];
    __shared__ float2 B[kHalfS];
    const int tid = threadIdx.x, fr = (int)blockIdx.x;
    const float *sp = spec + (size_t)fr * 2 * kStBins, *mk = mask + (size_t)fr * kStBins;
    auto bin = [&](int f) { const float m = mk[f]; return make_float2(sp[f] * m, f == 0 || f == kStBins - 1 ? 0.0f : sp[kStBins + f] * m); };
    for (int f = tid; f < kHalfS; f += 256) {
        const float2 a = bin(f), b = bin(kHalfS - f), t = tw1920[f];          // conj X[h - f] = (b.x, -b.y); e^{+2 pi i f / N} = conj t
        const float2 sm = make_float2(a.x + b.x, a.y - b.y), d = make_float2(a.x - b.x, a.y + b.y);
        const float2 dt = make_float2(d.x * t.x + d.y * t.y, d.y * t.x - d.x * t.y);
        A[f] = make_float2(sm.x - dt.y, -(sm.y + dt.x));                        // conj(sm + i dt)
    }
    const float2* r = fft::forward(A, B, p960, tw960, tid, 256);
    float2* out = reinterpret_cast<float2*>(frames + (size_t)fr * kNfftD);
    for (int m = tid; m < kHalfS; m += 256)
        out[m] = make_float2((r[m].x * (1.0f / (float)kNfftD)) * win_syn[2 * m], (-r[m].y * (1.0f / (float)kNfftD)) * win_syn[2 * m + 1]);
}

// Output of a push (or of the flush) and the next carried half frame.  Output hop k of stream s is the second half of the frame before local frame i = k - lead plus the
// first half of frame i, added in ascending frame order as k_dfsmn_ola_pcm does, over the matching sum of squared windows wsq [head | steady | tail][960]:
//   i < 0           the delay hop of a fresh stream (lead = 1): zero
//   i == 0          the frame before is the carried half (has_prev), or there is none: the signal's first hop, first-half term and the head sum only
//   i == Mp         the flush (Mp = 0, has_prev): the second-half term and the tail sum only
// The threads from `total` on copy the second half of the push's last frame into half_out [stream][960] (none when Mp = 0).
__global__ __launch_bounds__(256) void k_dfsmn_stream_out(const float* __restrict__ frames, const float* __restrict__ half_in, float* __restrict__ half_out,
                                                          const float* __restrict__ wsq, int Mp, int Pout, int lead, int has_prev, int16_t* __restrict__ pcm,
                                                          float* __restrict__ f32, long long total, long long total_all) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total_all) return;
    if (g >= total) {
        const long long e = g - total;
        const int st = (int)(e / kHopD), n = (int)(e - (long long)st * kHopD);
        half_out[e] = frames[((size_t)st * Mp + (Mp - 1)) * kNfftD + kHopD + n];
        return;
    }
    const int st = (int)(g / Pout), q = (int)(g - (long long)st * Pout), k = q / kHopD, n = q - k * kHopD, i = k - lead;
    float y = 0.0f;
    if (i >= 0) {
        float s = 0.0f;
        const bool prev = i > 0 || has_prev, cur = i < Mp;
        if (i > 0) s += frames[((size_t)st * Mp + i - 1) * kNfftD + kHopD + n];
        else if (has_prev) s += half_in[(size_t)st * kHopD + n];
        if (cur) s += frames[((size_t)st * Mp + i) * kNfftD + n];
        y = s / wsq[(prev ? (cur ? kHopD : 2 * kHopD) : 0) + n];
    }
    if (f32) f32[g] = y;
    if (pcm) pcm[g] = (short)(int)fminf(fmaxf(y * 32768.0f, -32768.0f), 32767.0f);
}

void hamming(int n, bool periodic, std::vector<double>& w) {   // torch.hamming_window(alpha 0.54, beta 0.46)
    w.resize((size_t)n);
    const double denom = periodic ? n : n - 1;
    for (int k = 0; k < n; ++k) w[k] = 0.54 - 0.46 * cos(2.0 * M_PI * k / denom);
}
void hamming_f32(int n, bool periodic, std::vector<float>& w) {   // the fp32 evaluation STFT_Process uses
    w.resize((size_t)n);
    const float step = (float)(2.0 * M_PI / (double)(periodic ? n : n - 1));
    for (int k = 0; k < n; ++k) w[k] = cosf((float)k * step) * (-0.46f) + 0.54f;
}

}  // namespace

struct DfsmnEngine : SubEngine {
    int device = 0, in_len_ = 0 /* one window */, n_win = 1, T = 0, out_len_ = 0, depth = 0, lorder = 0;
    float* d_w = nullptr;      // one arena: tables + weights
    const float *win_fb = nullptr, *win_st = nullptr, *win_syn = nullptr, *wsum = nullptr, *mel = nullptr, *lin1_w = nullptr, *lin1_b = nullptr, *lin2_w = nullptr,
                *lin2_b = nullptr;
    const float2 *tw2048 = nullptr, *tw1920 = nullptr, *tw1024 = nullptr, *tw960 = nullptr;      // (the half-length tables and plans: streams)
    const float* wsq = nullptr;     // [3][960] sum of squared synthesis windows over a hop: the signal's first hop | two frames | its last hop (streams)
    fft::Plan p2048, p1920, p1024, p960;
    std::vector<const float*> uf_lin_w, uf_lin_b, uf_proj_w, uf_conv_w;
    int capacity = 0;
    float* ws = nullptr;
    float *power = nullptr, *spec = nullptr, *feat = nullptr, *x = nullptr, *f1 = nullptr, *p1 = nullptr, *mask = nullptr, *frames_buf = nullptr;

    ~DfsmnEngine() override {
        (void)hipSetDevice(device);
        if (d_w) (void)hipFree(d_w);
        if (ws) (void)hipFree(ws);
    }
    int frames() const override { return T; }
    // batch-fold (:194-198, :231-232): a call is n_win windows back to back, each an independent clip whose raw overlap-add length equals the window
    int in_len() const override { return in_len_ * n_win; }
    int out_len() const override { return out_len_ * n_win; }
    bool accepts_float_input() const override { return true; }
    int reserve(int batch, std::string& err) override;
    int run(hipStream_t s, const int16_t* d_in, int batch, int16_t* d_out, float* d_f32, std::string& err) override;
    int tap(hipStream_t s, const char* name, int batch, float* out, size_t count, size_t* written, std::string& err) override;
    // streams (ade_stream_*): state per stream object, see DfsmnStream below
    int stream_delay() const override { return kHopD; }
    int stream_hop() const override { return kHopD; }
    int stream_windows() const override { return n_win; }
    int stream_channels() const override { return 1; }
    int stream_create(int n_streams, int frames_per_push, void** state, std::string& err) override;
    int stream_reset(void* state, hipStream_t s, std::string& err) override;
    int stream_push(void* state, hipStream_t s, const int16_t* d_in, int16_t* d_out, float* d_f32, std::string& err) override;
    int stream_flush(void* state, hipStream_t s, int16_t* d_out, float* d_f32, std::string& err) override;
    void stream_destroy(void* state) override;
};

// What a stream carries between pushes, for S streams that advance together: one allocation, its leading part cleared by a reset.
struct DfsmnStream {
    int S = 0, F = 0;                           // streams, hops per push
    long long hops = 0;                         // hops pushed since the last reset
    int16_t* carry[2] = {};                     // [S][960] the last 960 input samples, ping-ponged every push (ccur)
    float* hist[2] = {};                        // per layer [256][S][lorder - 1]: the last frames of the projection output p1, ping-ponged with half (cur)
    float* half[2] = {};                        // [S][960] the second half of the last synthesised frame
    int ccur = 0, cur = 0;
    float *power = nullptr, *spec = nullptr, *feat = nullptr, *x = nullptr, *f1 = nullptr, *p1 = nullptr, *mask = nullptr, *frames = nullptr;     // one push's workspace, S * F frames
    void* block = nullptr;
    size_t reset_bytes = 0;
};

namespace {
int dfail(std::string& err, int st, const std::string& msg) { err = msg; return st; }
#define DF_HIP(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) return dfail(err, ADE_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)
}  // namespace

int dfsmn_create(const std::map<std::string, Tensor>& tensors, int in_len, int n_win, int device, SubEngine** out, std::string& err) {
    *out = nullptr;
    if (in_len < kFrame) return dfail(err, ADE_ERR_SHAPE_MISMATCH, "dfsmn: input_audio_length shorter than one 1920-sample frame");
    auto get = [&](const std::string& name, std::vector<int> dims, const float** p) -> bool {
        auto it = tensors.find(name);
        if (it == tensors.end()) { err = "weights: tensor missing: " + name; return false; }
        if (!dims.empty() && it->second.dims != dims) { err = "weights: tensor has the wrong shape: " + name; return false; }
        *p = it->second.data;
        return true;
    };
    int depth = 0;
    while (tensors.count("uf_lin_w_" + std::to_string(depth))) ++depth;
    if (depth < 1) return dfail(err, ADE_ERR_MISSING_KEY, "weights: tensor missing: uf_lin_w_0");
    const float *mel, *l1w, *l1b, *l2w, *l2b;
    if (!get("mel_banks", {kMel, kFbBins}, &mel) || !get("lin1_w", {kHid, kMel}, &l1w) || !get("lin1_b", {kHid}, &l1b) ||
        !get("lin2_w", {kStBins, kHid}, &l2w) || !get("lin2_b", {kStBins}, &l2b))
        return err.find("missing") != std::string::npos ? ADE_ERR_MISSING_KEY : ADE_ERR_SHAPE_MISMATCH;
    auto itc = tensors.find("uf_conv_w_0");
    if (itc == tensors.end() || itc->second.dims.size() != 2 || itc->second.dims[0] != kHid)
        return dfail(err, ADE_ERR_SHAPE_MISMATCH, "weights: uf_conv_w_0 must be (256, lorder)");
    const int lo = itc->second.dims[1];
    std::vector<const float*> hw(4 * depth);
    for (int i = 0; i < depth; ++i) {
        const std::string s = std::to_string(i);
        if (!get("uf_lin_w_" + s, {kHid, kHid}, &hw[4 * i]) || !get("uf_lin_b_" + s, {kHid}, &hw[4 * i + 1]) ||
            !get("uf_proj_w_" + s, {kHid, kHid}, &hw[4 * i + 2]) || !get("uf_conv_w_" + s, {kHid, lo}, &hw[4 * i + 3]))
            return err.find("missing") != std::string::npos ? ADE_ERR_MISSING_KEY : ADE_ERR_SHAPE_MISMATCH;
    }
    DfsmnEngine* d = new DfsmnEngine();
    d->device = device;
    d->in_len_ = in_len;
    d->n_win = n_win;
    d->T = (in_len - kFrame) / kHopD + 1;                       // STFT_SIGNAL_LENGTH (Export_DFSMN.py:66)
    d->out_len_ = kNfftD + kHopD * (d->T - 1);                   // raw conv_transpose length, no centre trim
    d->depth = depth;
    d->lorder = lo;

    // ---- host tables
    std::vector<float> arena;
    auto push = [&](const float* src, size_t n) { const size_t off = arena.size(); arena.resize(off + ((n + 63) & ~(size_t)63)); if (src) memcpy(&arena[off], src, n * sizeof(float)); return off; };
    // ---- windows and twiddles
    std::vector<float> wa, wsyn, wfb((size_t)kFrame);
    {
        std::vector<double> win;
        hamming(kFrame, false, win);        // the Kaldi filter bank's symmetric hamming, float64 rounded once like the folded matrix it replaces (Export_DFSMN.py:97-120)
        for (int n = 0; n < kFrame; ++n) wfb[n] = (float)win[n];
    }
    hamming_f32(kNfftD, false, wa);     // analysis: symmetric hamming (DFSMN/STFT_Process.py:92)
    hamming_f32(kNfftD, true, wsyn);    // synthesis: periodic hamming (:93)
    const size_t o_wfb = push(wfb.data(), wfb.size()), o_wst = push(wa.data(), wa.size()), o_wsyn = push(wsyn.data(), wsyn.size());
    auto twiddles = [&](int n) {
        std::vector<float> tw((size_t)2 * n);
        for (int m = 0; m < n; ++m) { const double a = -2.0 * M_PI * (double)m / (double)n; tw[2 * m] = (float)cos(a); tw[2 * m + 1] = (float)sin(a); }
        return push(tw.data(), tw.size());
    };
    const size_t o_tw2048 = twiddles(kKaldiNfft), o_tw1920 = twiddles(kNfftD), o_tw1024 = twiddles(kHalfK), o_tw960 = twiddles(kHalfS);
    if (!fft::make_plan(kKaldiNfft, &d->p2048) || !fft::make_plan(kNfftD, &d->p1920) || !fft::make_plan(kHalfK, &d->p1024) || !fft::make_plan(kHalfS, &d->p960)) {
        delete d;
        return dfail(err, ADE_ERR_UNSUPPORTED, "dfsmn: FFT plan");
    }
    const size_t o_wsq = push(nullptr, (size_t)3 * kHopD);        // summed like the static table below: frame t - 1's second half first, then frame t's first half
    for (int n = 0; n < kHopD; ++n) {
        const float lo2 = wsyn[n] * wsyn[n], hi2 = wsyn[kHopD + n] * wsyn[kHopD + n];
        arena[o_wsq + n] = 0.0f + lo2;
        arena[o_wsq + kHopD + n] = (0.0f + hi2) + lo2;
        arena[o_wsq + 2 * kHopD + n] = 0.0f + hi2;
    }
    const size_t o_ws = push(nullptr, (size_t)d->out_len_);
    for (int t = 0; t < d->T; ++t)
        for (int n = 0; n < kNfftD; ++n) arena[o_ws + (size_t)t * kHopD + n] += wsyn[n] * wsyn[n];
    const size_t o_mel = push(mel, (size_t)kMel * kFbBins), o_l1w = push(l1w, (size_t)kHid * kMel), o_l1b = push(l1b, kHid),
                 o_l2w = push(l2w, (size_t)kStBins * kHid), o_l2b = push(l2b, kStBins);
    std::vector<size_t> o_h(4 * depth);
    for (int i = 0; i < depth; ++i) {
        o_h[4 * i] = push(hw[4 * i], (size_t)kHid * kHid);
        o_h[4 * i + 1] = push(hw[4 * i + 1], kHid);
        o_h[4 * i + 2] = push(hw[4 * i + 2], (size_t)kHid * kHid);
        o_h[4 * i + 3] = push(hw[4 * i + 3], (size_t)kHid * lo);
    }
    auto bail = [&](int st) { delete d; return st; };
    if (hipSetDevice(device) != hipSuccess) return bail(dfail(err, ADE_ERR_DEVICE, "hipSetDevice failed"));
    if (hipMalloc((void**)&d->d_w, arena.size() * sizeof(float)) != hipSuccess) return bail(dfail(err, ADE_ERR_DEVICE, "hipMalloc of the DFSMN weights failed"));
    if (hipMemcpy(d->d_w, arena.data(), arena.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return bail(dfail(err, ADE_ERR_DEVICE, "upload of the DFSMN weights failed"));
    d->win_fb = d->d_w + o_wfb; d->win_st = d->d_w + o_wst; d->win_syn = d->d_w + o_wsyn; d->wsum = d->d_w + o_ws; d->mel = d->d_w + o_mel;
    d->tw2048 = reinterpret_cast<const float2*>(d->d_w + o_tw2048); d->tw1920 = reinterpret_cast<const float2*>(d->d_w + o_tw1920);
    d->tw1024 = reinterpret_cast<const float2*>(d->d_w + o_tw1024); d->tw960 = reinterpret_cast<const float2*>(d->d_w + o_tw960); d->wsq = d->d_w + o_wsq;
    d->lin1_w = d->d_w + o_l1w; d->lin1_b = d->d_w + o_l1b; d->lin2_w = d->d_w + o_l2w; d->lin2_b = d->d_w + o_l2b;
    for (int i = 0; i < depth; ++i) {
        d->uf_lin_w.push_back(d->d_w + o_h[4 * i]);
        d->uf_lin_b.push_back(d->d_w + o_h[4 * i + 1]);
        d->uf_proj_w.push_back(d->d_w + o_h[4 * i + 2]);
        d->uf_conv_w.push_back(d->d_w + o_h[4 * i + 3]);
    }
    *out = d;
    return ADE_OK;
}

int DfsmnEngine::reserve(int calls, std::string& err) {
    DfsmnEngine* d = this;
    if (calls <= d->capacity) return ADE_OK;
    const int batch = calls * n_win;
    DF_HIP(hipSetDevice(d->device));
    DF_HIP(hipDeviceSynchronize());
    if (d->ws) (void)hipFree(d->ws);
    d->ws = nullptr;
    d->capacity = 0;
    const size_t N = (size_t)batch * d->T;
    const size_t sizes[8] = {(size_t)kFbBins * N, (size_t)2 * kStBins * N, (size_t)kMel * N, (size_t)kHid * N, (size_t)kHid * N, (size_t)kHid * N, (size_t)kStBins * N,
                             N * kNfftD};
    size_t total = 0;
    for (size_t s : sizes) total += (s + 63) & ~(size_t)63;
    DF_HIP(hipMalloc((void**)&d->ws, total * sizeof(float)));
    float** ptrs[8] = {&d->power, &d->spec, &d->feat, &d->x, &d->f1, &d->p1, &d->mask, &d->frames_buf};
    size_t off = 0;
    for (int i = 0; i < 8; ++i) { *ptrs[i] = d->ws + off; off += (sizes[i] + 63) & ~(size_t)63; }
    d->capacity = calls;
    return ADE_OK;
}

int DfsmnEngine::run(hipStream_t s, const int16_t* d_in, int batch, int16_t* d_out, float* d_f32, std::string& err) {
    DfsmnEngine* d = this;
    if (batch == 0) return ADE_OK;
    int st = reserve(batch, err);
    if (st != ADE_OK) return st;
    batch *= n_win;
    using namespace gemm;
    const int N = batch * d->T;
    // analysis: Kaldi filter-bank power and the mask STFT of every frame as FFTs                              (Export_DFSMN.py:205-209, 216)
    hipLaunchKernelGGL(k_dfsmn_analysis, dim3((unsigned)(batch * ((d->T + 1) / 2))), dim3(256), 0, s, d_in, float_in, d->in_len_, d->T, d->p2048, d->p1920, d->tw2048, d->tw1920, d->win_fb, d->win_st,
                       d->power, d->spec);
    // Kaldi log-mel: mel_banks x power, clamp(eps), log                                                  (:216-217)
    launch(s, RowMajorA{d->mel, kFbBins}, PowerFrameB{d->power}, BiasActStore<kActLogFloor>{d->feat, N, nullptr, 1.1920928955078125e-07f}, kMel, N, kFbBins);
    // mask network                                                                                          (:224-230)
    launch(s, RowMajorA{d->lin1_w, kMel}, RowMajorB{d->feat, N}, BiasActStore<kActRelu>{d->x, N, d->lin1_b, 0.0f}, kHid, N, kMel);
    for (int i = 0; i < d->depth; ++i) {
        launch(s, RowMajorA{d->uf_lin_w[i], kHid}, RowMajorB{d->x, N}, BiasActStore<kActRelu>{d->f1, N, d->uf_lin_b[i], 0.0f}, kHid, N, kHid);
        launch(s, RowMajorA{d->uf_proj_w[i], kHid}, RowMajorB{d->f1, N}, BiasActStore<kActNone>{d->p1, N, nullptr, 0.0f}, kHid, N, kHid);
        const long long total = (long long)kHid * N;
        hipLaunchKernelGGL(k_fsmn_memory, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)d->p1, d->uf_conv_w[i], d->x, N, d->T,
                           d->lorder, total);
    }
    launch(s, RowMajorA{d->lin2_w, kHid}, RowMajorB{d->x, N}, SigmoidTStore{d->mask, d->lin2_b}, kStBins, N, kHid);
    // masked spectrum -> ISTFT frames, then overlap-add + PCM tail                                        (:236-244)
    hipLaunchKernelGGL(k_dfsmn_synthesis, dim3((unsigned)(batch * ((d->T + 1) / 2))), dim3(256), 0, s, (const float*)d->spec, (const float*)d->mask, d->T, d->p1920, d->tw1920, d->win_syn, d->frames_buf);
    const long long total = (long long)batch * d->out_len_;
    hipLaunchKernelGGL(k_dfsmn_ola_pcm, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)d->frames_buf, d->wsum, d_out, d_f32, d->T,
                       d->out_len_, total);
    DF_HIP(hipGetLastError());
    return ADE_OK;
}

int DfsmnEngine::tap(hipStream_t s, const char* name, int batch, float* out, size_t count, size_t* written, std::string& err) {
    DfsmnEngine* d = this;
    const size_t N = (size_t)batch * n_win * d->T;
    const float* src = nullptr;
    size_t n = 0;
    if (strcmp(name, "logmel") == 0) { src = d->feat; n = kMel * N; }
    else if (strcmp(name, "mask") == 0) { src = d->mask; n = kStBins * N; }          // frame-major (frames, 961)
    else return dfail(err, ADE_ERR_NOT_FOUND, std::string("unknown tap: ") + name);
    if (!src || batch <= 0) return dfail(err, ADE_ERR_NOT_FOUND, "tap has no data yet");
    if (count < n) return dfail(err, ADE_ERR_SHAPE_MISMATCH, "tap buffer too small");
    DF_HIP(hipStreamSynchronize(s));
    DF_HIP(hipMemcpy(out, src, n * sizeof(float), hipMemcpyDeviceToHost));
    *written = n;
    return ADE_OK;
}

// ---- streams ----------------------------------------------------------------------------------------------------------------------------------------------------
int DfsmnEngine::stream_create(int n_streams, int frames_per_push, void** state, std::string& err) {
    *state = nullptr;
    if (n_streams < 1 || frames_per_push < 1 || frames_per_push > 4096)
        return dfail(err, ADE_ERR_BAD_VALUE, "ade_stream_create: dfsmn needs n_streams >= 1 and 1 <= frames_per_push <= 4096");
    const size_t S = (size_t)n_streams, N = S * frames_per_push, Hl = (size_t)(lorder - 1);
    if (N * kNfftD > 0x7fffffffULL || (size_t)kHid * S * (Hl > (size_t)frames_per_push ? Hl : (size_t)frames_per_push) > 0x7fffffffULL)
        return dfail(err, ADE_ERR_BAD_VALUE, "ade_stream_create: dfsmn: n_streams * frames_per_push exceeds the launch grid");
    std::unique_ptr<DfsmnStream> st(new DfsmnStream());
    st->S = n_streams; st->F = frames_per_push;
    auto up = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    const size_t b_carry = up(S * kHopD * sizeof(int16_t)), b_hist = up((size_t)depth * kHid * S * Hl * sizeof(float)), b_half = up(S * kHopD * sizeof(float));
    const size_t work[8] = {up(N * kFbBins * sizeof(float)), up(N * 2 * kStBins * sizeof(float)), up(N * kMel * sizeof(float)), up(N * kHid * sizeof(float)),
                            up(N * kHid * sizeof(float)), up(N * kHid * sizeof(float)), up(N * kStBins * sizeof(float)), up(N * kNfftD * sizeof(float))};
    size_t total = 2 * b_carry + 2 * b_hist + 2 * b_half;
    st->reset_bytes = total;
    for (size_t b : work) total += b;
    if (hipSetDevice(device) != hipSuccess || hipMalloc(&st->block, total) != hipSuccess) {
        (void)hipGetLastError();
        return dfail(err, ADE_ERR_DEVICE, "ade_stream_create: hipMalloc of the DFSMN stream state failed");
    }
    char* p = (char*)st->block;
    for (int i = 0; i < 2; ++i) { st->carry[i] = (int16_t*)p; p += b_carry; }
    for (int i = 0; i < 2; ++i) { st->hist[i] = (float*)p; p += b_hist; }
    for (int i = 0; i < 2; ++i) { st->half[i] = (float*)p; p += b_half; }
    float** ptrs[8] = {&st->power, &st->spec, &st->feat, &st->x, &st->f1, &st->p1, &st->mask, &st->frames};
    for (int i = 0; i < 8; ++i) { *ptrs[i] = (float*)p; p += work[i]; }
    *state = st.release();
    return ADE_OK;
}

int DfsmnEngine::stream_reset(void* state, hipStream_t s, std::string& err) {
    DfsmnStream* st = (DfsmnStream*)state;
    DF_HIP(hipMemsetAsync(st->block, 0, st->reset_bytes, s));
    st->hops = 0;
    st->ccur = 0;
    st->cur = 0;
    return ADE_OK;
}

// A push of F hops.  A fresh stream's first push completes F - 1 frames (its carried samples are no signal), every later push F.
int DfsmnEngine::stream_push(void* state, hipStream_t s, const int16_t* d_in, int16_t* d_out, float* d_f32, std::string& err) {
    using namespace gemm;
    DfsmnStream* st = (DfsmnStream*)state;
    const bool fresh = st->hops == 0;
    const int S = st->S, P = st->F * kHopD, Mp = fresh ? st->F - 1 : st->F, N = S * Mp, Hl = lorder - 1;
    const int nxt = st->cur ^ 1;
    // 1. analysis of the frames this push completes (none: a one-hop first push), and the next carried input -- N + S >= 1 workgroups
    hipLaunchKernelGGL(k_dfsmn_stream_analysis, dim3((unsigned)(N + S)), dim3(256), 0, s, d_in, (const int16_t*)st->carry[st->ccur], st->carry[st->ccur ^ 1], P, Mp, N,
                       fresh ? kHopD : 0, p1024, p960, tw1024, tw960, tw2048, tw1920, win_fb, win_st, st->power, st->spec);
    if (Mp > 0) {
        // 2. Kaldi log-mel and the mask network, the memory continued from each layer's history
        launch(s, RowMajorA{mel, kFbBins}, PowerFrameB{st->power}, BiasActStore<kActLogFloor>{st->feat, N, nullptr, 1.1920928955078125e-07f}, kMel, N, kFbBins);
        launch(s, RowMajorA{lin1_w, kMel}, RowMajorB{st->feat, N}, BiasActStore<kActRelu>{st->x, N, lin1_b, 0.0f}, kHid, N, kMel);
        for (int i = 0; i < depth; ++i) {
            launch(s, RowMajorA{uf_lin_w[i], kHid}, RowMajorB{st->x, N}, BiasActStore<kActRelu>{st->f1, N, uf_lin_b[i], 0.0f}, kHid, N, kHid);
            launch(s, RowMajorA{uf_proj_w[i], kHid}, RowMajorB{st->f1, N}, BiasActStore<kActNone>{st->p1, N, nullptr, 0.0f}, kHid, N, kHid);
            const size_t at = (size_t)i * kHid * S * Hl;
            const long long total = (long long)kHid * N, total_all = total + (long long)kHid * S * Hl;
            hipLaunchKernelGGL(k_dfsmn_stream_memory, dim3((unsigned)((total_all + 255) / 256)), dim3(256), 0, s, (const float*)st->p1, uf_conv_w[i], st->x,
                               (const float*)(st->hist[st->cur] + at), st->hist[nxt] + at, S, Mp, Hl, lorder, total, total_all);
        }
        launch(s, RowMajorA{lin2_w, kHid}, RowMajorB{st->x, N}, SigmoidTStore{st->mask, lin2_b}, kStBins, N, kHid);
        // 3. one inverse transform per frame
        hipLaunchKernelGGL(k_dfsmn_stream_synthesis, dim3((unsigned)N), dim3(256), 0, s, (const float*)st->spec, (const float*)st->mask, p960, tw960, tw1920, win_syn, st->frames);
    }
    // 4. overlap-add, window-square sum, PCM tail, the next carried half
    {
        const long long total = (long long)S * P, total_all = total + (Mp > 0 ? (long long)S * kHopD : 0);
        hipLaunchKernelGGL(k_dfsmn_stream_out, dim3((unsigned)((total_all + 255) / 256)), dim3(256), 0, s, (const float*)st->frames, (const float*)st->half[st->cur], st->half[nxt],
                           wsq, Mp, P, fresh ? 1 : 0, st->hops >= 2 ? 1 : 0, d_out, d_f32, total, total_all);
    }
    DF_HIP(hipGetLastError());
    if (Mp > 0) st->cur = nxt;
    st->ccur ^= 1;
    st->hops += st->F;
    return ADE_OK;
}

// The last hop: the second half of the last frame over its own window squares.  It ends a signal of 960 K samples, K >= 2 (one frame at least).
int DfsmnEngine::stream_flush(void* state, hipStream_t s, int16_t* d_out, float* d_f32, std::string& err) {
    DfsmnStream* st = (DfsmnStream*)state;
    if (st->hops < 2)
        return dfail(err, ADE_ERR_BAD_VALUE, "ade_stream_flush: dfsmn ends a signal of at least one 1920-sample frame: the hops pushed must be at least 2 (pushed: " +
                                             std::to_string(st->hops) + ")");
    const long long total = (long long)st->S * kHopD;
    hipLaunchKernelGGL(k_dfsmn_stream_out, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)st->frames, (const float*)st->half[st->cur], (float*)nullptr, wsq, 0,
                       kHopD, 0, 1, d_out, d_f32, total, total);
    DF_HIP(hipGetLastError());
    return ADE_OK;
}

void DfsmnEngine::stream_destroy(void* state) {
    DfsmnStream* st = (DfsmnStream*)state;
    if (!st) return;
    (void)hipSetDevice(device);
    if (st->block) (void)hipFree(st->block);
    delete st;
}

}  // namespace ade
