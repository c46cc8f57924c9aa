// ade_nkf_aec.hip — NKF-AEC (neural Kalman filter, acoustic echo cancellation) on the MI355X.
//
// Reference: NKF.forward, NKF_AEC/Export_NKF_AEC.py:246-411, with KGNet_Real (:150-197) and the folder's STFT_Process (stft_B / istft_B, 1024 / 1024 / 256,
// periodic hann, constant centre pad, static window-square norm).  Two inputs per call -- channel 0 the far-end reference, channel 1 the near-end microphone
// (the export's input order, :524) -- and one output.
//
//   k_nkf_mean      per (call, channel): the DC mean of the call's samples in int16 units (:259-269; the 2^-15 of an int16 input is folded into the window)
//   k_nkf_analysis  per (call, channel, frame pair): framing with zero centre pad, * hann * 2^-15, two real frames as one complex 1024-point FFT
//                   (csrc/ade_fft.h) -> spectra stored bin-contiguous [call][channel][frame][bin] (float2)
//   k_nkf_kalman    THE HOT KERNEL: one lane per (call, bin) runs the whole recurrence over all frames (:302-373) with every state in registers:
//                   h_prior / h_post (4 complex taps each), the last 4 reference frames, the four GRU hidden vectors of 18.  The weights (~4.4 k floats) are
//                   read at wave-uniform addresses only, so they stream through the scalar cache and every multiply-add takes its weight as an SGPR operand.
//                   Every product is a (re, im) pair: gru_r / gru_i act on the real and the imaginary input with the SAME weights (one broadcast weight
//                   per packed FMA), the ComplexDense layers apply their real and imaginary weight sets to the real and imaginary halves (weights stored
//                   interleaved (w_re, w_im), one 64-bit scalar operand per packed FMA).  No matrix cores: the exact-fp32 MFMA has the vector pipe's rate on
//                   gfx950 and K = 18 would pad to 20.  Output: the error spectrum mic - echo_hat, [call][frame][bin].
//   k_nkf_synthesis per (call, frame pair): the Hermitian inverse transform of two frames as one complex FFT, * hann / 1024 (istft_B's inverse kernel; the
//                   sine rows of DC and Nyquist are zero with exact trigonometry)
//   k_nkf_ola       overlap-add as a gather, trim [512 : 512 + 256 (T - 1)], * 1 / window-square sum (the f32 waveform) and * 32767 / sum -> .to(int16)
//                   (:383-408); the [:audio_len] trim keeps min(L, 256 (T - 1)) samples.
// The frame-0 branch of the reference (:309-335) is the general step with zero state, so one loop body serves every frame.
//
// Streams (ade_stream_* on an nkf_aec handle, include/ade.h): a push of F hops continues where the previous one stopped, four launches and no mean kernel --
//   k_nkf_stream_analysis   rows [768 carried | P new]; the far-end and the near-end frame of the SAME index as one complex FFT; keeps the next carry
//   k_nkf_kalman<true>      the same kernel, the 96 state floats of each lane loaded at entry and stored at exit ([96][streams * 513])
//   k_nkf_stream_synthesis  one frame per transform, appended to the stream's last three windowed frames
//   k_nkf_stream_ola        the gather over the covering frames with the window-square sum formed alongside, 768 samples behind the input
// so that the result does not depend on the push size, bit for bit ("Streaming").
#include "ade_fft.h"
#include "ade_gemm.h"
#include "ade_internal.h"
#include "../../include/ade.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace ade {

namespace {

using namespace dev;

constexpr int kN = 1024, kHopN = 256, kF = kN / 2 + 1, kTaps = 4, kIn = 2 * kTaps + 1, kFc = 18, kHid = 18, kG3 = 3 * kHid;
constexpr int kKalmanThreads = 64;

#ifdef HIPSIM            // the host simulator (tests/hipsim, g++): a plain pair with the element-wise operators clang's vector type has
struct f2v { float x, y; };
inline f2v operator+(f2v a, f2v b) { return f2v{a.x + b.x, a.y + b.y}; }
inline f2v operator-(f2v a, f2v b) { return f2v{a.x - b.x, a.y - b.y}; }
inline f2v operator*(f2v a, f2v b) { return f2v{a.x * b.x, a.y * b.y}; }
inline f2v& operator+=(f2v& a, f2v b) { return a = a + b; }
inline f2v& operator-=(f2v& a, f2v b) { return a = a - b; }
#else
typedef float f2v __attribute__((ext_vector_type(2)));
#endif

// the weight arena, in floats; the ComplexDense layers interleaved (w_re, w_im) per (out, in) element, the GRUs plain PyTorch layout
constexpr int oFcInW = 0;                                    // [18][9] x 2
constexpr int oFcInB = oFcInW + kFc * kIn * 2;               // [18] x 2
constexpr int oGru = oFcInB + kFc * 2;                       // per GRU g: w_ih [54][18], w_hh [54][18], b_ih [54], b_hh [54]
constexpr int kGruSize = kG3 * kFc + kG3 * kHid + 2 * kG3;
constexpr int oFc1W = oGru + 2 * kGruSize;                   // [18][18] x 2
constexpr int oFc1B = oFc1W + kFc * kHid * 2;
constexpr int oFc2W = oFc1B + kFc * 2;                       // [4][18] x 2
constexpr int oFc2B = oFc2W + kTaps * kFc * 2;
constexpr int oSlope = oFc2B + kTaps * 2;                    // fc_in slope, fc_out slope
constexpr int kWeights = oSlope + 2;

// The weights are read through the constant address space at wave-uniform addresses: scalar loads, each FMA takes its weight as an SGPR operand.
#ifdef HIPSIM
typedef const float CFloat;
typedef const f2v CF2;
__device__ __forceinline__ CFloat* frame_weights(const float* w) { return w; }
#else
typedef __attribute__((address_space(4))) const float CFloat;
typedef __attribute__((address_space(4))) const f2v CF2;
__device__ __forceinline__ CFloat* frame_weights(unsigned long long a) {
    // laundered through an empty asm every frame: otherwise the compiler hoists all ~4.4 k loop-invariant weights out of the frame loop into SGPRs,
    // spills them into VGPR lanes (1191 spills) and reads each back with v_readlane; this way the scalar loads are issued again each frame
    __asm__ volatile("" : "+s"(a));
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32));
    return (CFloat*)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ CFloat* frame_weights(const float* w) { return frame_weights((unsigned long long)w); }
#endif
// Column j of a stream's Kalman state, [kStateFloats][lanes].  The base is pinned to scalar registers at every use: left to itself the compiler forms the 96 per-lane
// 64-bit addresses of the loads at kernel entry in vector registers and keeps every one of them alive, in 174 accumulator registers, for the stores at exit --
// 430 registers, one wave per SIMD instead of two.
#ifdef HIPSIM
__device__ __forceinline__ float* state_column(float* state, size_t off) { return state + off; }
#else
__device__ __forceinline__ float* state_column(float* state, size_t off) {
    unsigned long long a = (unsigned long long)(state + off);
    __asm__ volatile("" : "+s"(a));
    return (float*)a;
}
#endif
__device__ __forceinline__ f2v ld2(CFloat* p) { return *reinterpret_cast<CF2*>(p); }
__device__ __forceinline__ f2v splat(float w) { return f2v{w, w}; }
__device__ __forceinline__ f2v cmulv(f2v a, f2v b) { return f2v{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ f2v leaky(f2v v, float s) { return f2v{v.x > 0.0f ? v.x : v.x * s, v.y > 0.0f ? v.y : v.y * s}; }
__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// one GRU cell (PyTorch nn.GRU, gates r, z, n: :68-69) on a PAIR of (input, hidden) sequences sharing its weights -- .x the real input's, .y the imaginary's
__device__ __forceinline__ void gru_pair(CFloat* g, const f2v (&u)[kFc], f2v (&h)[kHid]) {
    f2v hn[kHid];
#pragma unroll
    for (int j = 0; j < kHid; ++j) {
        CFloat *wih = g, *bih = wih + kG3 * kFc + kG3 * kHid, *bhh = bih + kG3;
        f2v ar = splat(bih[j]), az = splat(bih[kHid + j]), an = splat(bih[2 * kHid + j]);
        f2v br = splat(bhh[j]), bz = splat(bhh[kHid + j]), bn = splat(bhh[2 * kHid + j]);
#pragma unroll
        for (int k = 0; k < kFc; ++k) {
            ar += splat(wih[j * kFc + k]) * u[k];
            az += splat(wih[(kHid + j) * kFc + k]) * u[k];
            an += splat(wih[(2 * kHid + j) * kFc + k]) * u[k];
        }
        CFloat* whh = g + kG3 * kFc;
#pragma unroll
        for (int k = 0; k < kHid; ++k) {
            br += splat(whh[j * kHid + k]) * h[k];
            bz += splat(whh[(kHid + j) * kHid + k]) * h[k];
            bn += splat(whh[(2 * kHid + j) * kHid + k]) * h[k];
        }
        const float rx = sigm(ar.x + br.x), ry = sigm(ar.y + br.y), zx = sigm(az.x + bz.x), zy = sigm(az.y + bz.y);
        const float nx = tanhf(an.x + rx * bn.x), ny = tanhf(an.y + ry * bn.y);
        hn[j] = f2v{(1.0f - zx) * nx + zx * h[j].x, (1.0f - zy) * ny + zy * h[j].y};
    }
#pragma unroll
    for (int j = 0; j < kHid; ++j) h[j] = hn[j];
}

__global__ __launch_bounds__(256) void k_nkf_mean(const int16_t* __restrict__ pcm, const float* __restrict__ fpcm, int L, float* __restrict__ mean) {
    __shared__ double red[256];
    const int row = blockIdx.x, tid = threadIdx.x;                  // row = call * 2 + channel
    double s = 0.0;
    for (int n = tid; n < L; n += 256) s += fpcm ? (double)fpcm[(size_t)row * L + n] : (double)pcm[(size_t)row * L + n];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) mean[row] = (float)(red[0] / (double)L);
}

// one workgroup per (call, channel, frame pair): Z = FFT(a + i b), A[f] = (Z[f] + conj Z[N - f]) / 2, B[f] = (Z[f] - conj Z[N - f]) / (2 i)
// n_win / swap (the back end of dfsmn_aec, nkf_backend_create): the source rows are [call][channel][n_win windows of L]; row = (call * n_win + window) * 2 + channel
// reads source channel 1 - channel when swap is set (that family's channel 0 is the near end).  mean null: no DC removal.
__global__ __launch_bounds__(256) void k_nkf_analysis(const int16_t* __restrict__ pcm, const float* __restrict__ fpcm, const float* __restrict__ mean, int L, int T,
                                                      fft::Plan plan, const float2* __restrict__ tw, const float* __restrict__ win, float2* __restrict__ spec,
                                                      int n_win, int swap) {
    __shared__ float2 A[kN];
    __shared__ float2 Bf[kN];
    const int tid = threadIdx.x, ppr = (T + 1) / 2, row = (int)blockIdx.x / ppr, t0 = 2 * ((int)blockIdx.x - row * ppr);
    const bool two = t0 + 1 < T;
    const float m = mean ? mean[row] : 0.0f;
    const int wrow = row >> 1, ch = swap ? 1 - (row & 1) : (row & 1), call = wrow / n_win;
    const size_t base = (((size_t)call * 2 + ch) * n_win + (wrow - call * n_win)) * L;
    auto sample = [&](int t, int n) {
        const int p = t * kHopN + n - kN / 2;
        if (p < 0 || p >= L) return 0.0f;                               // centre pad with zeros, after the mean is removed (:269, :278)
        return ((fpcm ? fpcm[base + p] : (float)pcm[base + p]) - m) * win[n];
    };
    for (int n = tid; n < kN; n += 256) A[n] = make_float2(sample(t0, n), two ? sample(t0 + 1, n) : 0.0f);
    const float2* r = fft::forward(A, Bf, plan, tw, tid, 256);
    float2* out0 = spec + ((size_t)row * T + t0) * kF;
    for (int f = tid; f < kF; f += 256) {
        const float2 z = r[f], zc = r[f == 0 ? 0 : kN - f];
        out0[f] = make_float2(0.5f * (z.x + zc.x), 0.5f * (z.y - zc.y));
        if (two) out0[kF + f] = make_float2(0.5f * (z.y + zc.y), 0.5f * (zc.x - z.x));
    }
}

// one lane per (call, bin): the whole Kalman recurrence of the call (:302-373).  CARRY (streams): the lane's state -- xt, h_prior, h_post, the four GRU hidden vectors,
// kStateFloats floats -- is loaded from `state` at entry and stored back at exit, laid out [kStateFloats][rows * kF] so that a wave's loads and stores of one
// float are contiguous; T = 0 (a stream's first one-hop push) runs no frame and leaves the state as it was.  kg is an output of every frame and is not carried.
constexpr int kStateFloats = 2 * (3 * kTaps + 2 * kHid);
template <bool CARRY>
__global__ __launch_bounds__(kKalmanThreads) void k_nkf_kalman(const float2* __restrict__ spec, const float* __restrict__ W0, int T, int rows,
                                                              float2* __restrict__ err, float2* __restrict__ kg_last, float* __restrict__ state) {
    const int i = (int)blockIdx.x * kKalmanThreads + (int)threadIdx.x;
    if (i >= rows * kF) return;
    const int call = i / kF, f = i - call * kF;
    const float2* ref = spec + (size_t)call * 2 * T * kF + f;
    const float2* mic = ref + (size_t)T * kF;
    float2* out = err + (size_t)call * T * kF + f;
    const float s_in = W0[oSlope], s_out = W0[oSlope + 1];
    f2v xt[kTaps], hp[kTaps], hq[kTaps], kg[kTaps];
    f2v hr[kHid], hi[kHid];                       // gru_r: (h_rr, h_ir); gru_i: (h_ri, h_ii)
#pragma unroll
    for (int k = 0; k < kTaps; ++k) { xt[k] = f2v{0.0f, 0.0f}; hp[k] = xt[k]; hq[k] = xt[k]; kg[k] = xt[k]; }
#pragma unroll
    for (int k = 0; k < kHid; ++k) { hr[k] = f2v{0.0f, 0.0f}; hi[k] = hr[k]; }
    // state float j of this lane: a wave-uniform column base (state_column: a scalar register pair) plus the lane's 32-bit index
    const size_t sn = (size_t)rows * kF;
    auto col = [&](int j) -> float* { return state_column(state, (size_t)j * sn); };
    const unsigned lane = (unsigned)i;
    if constexpr (CARRY) {
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            xt[k] = f2v{col(2 * k)[lane], col(2 * k + 1)[lane]};
            hp[k] = f2v{col(2 * (kTaps + k))[lane], col(2 * (kTaps + k) + 1)[lane]};
            hq[k] = f2v{col(2 * (2 * kTaps + k))[lane], col(2 * (2 * kTaps + k) + 1)[lane]};
        }
#pragma unroll
        for (int k = 0; k < kHid; ++k) {
            hr[k] = f2v{col(2 * (3 * kTaps + k))[lane], col(2 * (3 * kTaps + k) + 1)[lane]};
            hi[k] = f2v{col(2 * (3 * kTaps + kHid + k))[lane], col(2 * (3 * kTaps + kHid + k) + 1)[lane]};
        }
    }
    for (int t = 0; t < T; ++t) {
        // the weight pointer laundered through an empty asm each frame: without it the compiler hoists all ~4.4 k uniform weights out of the frame loop into
        // SGPRs, spills them into VGPR lanes (1191 spills) and reads each back with v_readlane; this way they are re-fetched by scalar loads every frame
        const CFloat* W = frame_weights(W0);
        const float2 rt = ref[(size_t)t * kF], mt = mic[(size_t)t * kF];
#pragma unroll
        for (int k = 0; k < kTaps - 1; ++k) xt[k] = xt[k + 1];          // ref_padded[t : t + 4], oldest first (:339)
        xt[kTaps - 1] = f2v{rt.x, rt.y};
        f2v feat[kIn];
        f2v e = f2v{mt.x, mt.y};
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            feat[kTaps + 1 + k] = hq[k] - hp[k];                          // dh = h_post - h_prior (:345-346)
            hp[k] = hq[k];                                                // h_prior <- h_post (:347-348)
            e -= cmulv(xt[k], hp[k]);                                     // e = mic - <xt, h_prior> (:351-352)
            feat[k] = xt[k];
        }
        feat[kTaps] = e;
        // fc_in (:184-188): [xt, e, dh] -> 18, leaky ReLU with the cached PReLU slope
        f2v u[kFc];
#pragma unroll
        for (int j = 0; j < kFc; ++j) {
            f2v a = ld2(W + oFcInB + 2 * j);
#pragma unroll
            for (int k = 0; k < kIn; ++k) a += ld2(W + oFcInW + 2 * (j * kIn + k)) * feat[k];
            u[j] = leaky(a, s_in);
        }
        // gru_r -> (h_rr, h_ir) (:75-76), then gru_i -> (h_ri, h_ii) (:77-78): one copy of the cell's code, the two state sets swapped between the passes
#pragma unroll 1
        for (int gi = 0; gi < 2; ++gi) {
            gru_pair(W + oGru + gi * kGruSize, u, hr);
#pragma unroll
            for (int k = 0; k < kHid; ++k) { const f2v tmp = hr[k]; hr[k] = hi[k]; hi[k] = tmp; }
        }
        f2v g[kHid];
#pragma unroll
        for (int k = 0; k < kHid; ++k) g[k] = f2v{hr[k].x - hi[k].y, hi[k].x + hr[k].y};     // (h_rr - h_ii, h_ri + h_ir) (:79)
        f2v v[kFc];
#pragma unroll
        for (int j = 0; j < kFc; ++j) {
            f2v a = ld2(W + oFc1B + 2 * j);
#pragma unroll
            for (int k = 0; k < kHid; ++k) a += ld2(W + oFc1W + 2 * (j * kHid + k)) * g[k];
            v[j] = leaky(a, s_out);
        }
        f2v echo = f2v{0.0f, 0.0f};
#pragma unroll
        for (int l = 0; l < kTaps; ++l) {
            f2v a = ld2(W + oFc2B + 2 * l);
#pragma unroll
            for (int k = 0; k < kFc; ++k) a += ld2(W + oFc2W + 2 * (l * kFc + k)) * v[k];
            kg[l] = a;
            hq[l] = hp[l] + cmulv(a, e);                                  // h_post = h_prior + kg e (:368-369)
            echo += cmulv(xt[l], hq[l]);                                  // echo_hat = <xt, h_post> (:372-373)
        }
        out[(size_t)t * kF] = make_float2(mt.x - echo.x, mt.y - echo.y);  // mic - echo_hat (:380-381)
    }
    if (kg_last) {
#pragma unroll
        for (int l = 0; l < kTaps; ++l) kg_last[(size_t)i * kTaps + l] = make_float2(kg[l].x, kg[l].y);
    }
    if constexpr (CARRY) {
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            col(2 * k)[lane] = xt[k].x; col(2 * k + 1)[lane] = xt[k].y;
            col(2 * (kTaps + k))[lane] = hp[k].x; col(2 * (kTaps + k) + 1)[lane] = hp[k].y;
            col(2 * (2 * kTaps + k))[lane] = hq[k].x; col(2 * (2 * kTaps + k) + 1)[lane] = hq[k].y;
        }
#pragma unroll
        for (int k = 0; k < kHid; ++k) {
            col(2 * (3 * kTaps + k))[lane] = hr[k].x; col(2 * (3 * kTaps + k) + 1)[lane] = hr[k].y;
            col(2 * (3 * kTaps + kHid + k))[lane] = hi[k].x; col(2 * (3 * kTaps + kHid + k) + 1)[lane] = hi[k].y;
        }
    }
}

// ---- streams: a push of F hops continues the signal where the previous push stopped (include/ade.h, ade_stream_*) ---------------------------------------------
// Frame t covers the samples [256 t - 512, 256 t + 512), so after k hops of input the frames 0 .. k - 2 exist.  A push reads rows [768 carried | P new] samples,
// which start at sample 256 k - 768 (k = hops before the push): its first frame, t = k - 1, starts at row offset 0 (the stream's first push has no frame -1 and
// starts with frame 0 at offset 256, its carry being the zeros of the constant centre pad).
constexpr int kCarry = 3 * kHopN;

// one workgroup per (stream, frame): the far-end and the near-end frame OF THE SAME INDEX as one complex transform.  Pairing frames (t, t + 1) as the one-shot
// kernel does would make a frame's rounding depend on where the push boundary falls (the two halves of a packed transform share rounding cross-talk); the two
// channels of a frame always arrive together.  The last workgroup of a stream (frame index T) moves the rows' last 768 samples into the OTHER carry buffer.
// pcm null (flush): the new samples are zeros, no carry is kept.  swap (the back end of dfsmn_aec): the caller's channel 0 is the near end, so the far-end frame is
// read from source channel 1; the carries keep the caller's order.  T = 0 with a carry_out: only the carry moves (the dense-table back end frames its rows itself).
__global__ __launch_bounds__(256) void k_nkf_stream_analysis(const int16_t* __restrict__ pcm, const int16_t* __restrict__ carry_in, int16_t* __restrict__ carry_out, int P, int T,
                                                             int off0, fft::Plan plan, const float2* __restrict__ tw, const float* __restrict__ win, float2* __restrict__ spec,
                                                             int swap) {
    __shared__ float2 A[kN];
    __shared__ float2 Bf[kN];
    const int tid = threadIdx.x, per = T + (carry_out ? 1 : 0), st = (int)blockIdx.x / per, j = (int)blockIdx.x - st * per;
    auto row = [&](int ch, int p) -> int {                                  // sample p of the row [768 carried | P new] of channel ch
        if (p < kCarry) return carry_in[((size_t)st * 2 + ch) * kCarry + p];
        return pcm && p - kCarry < P ? pcm[((size_t)st * 2 + ch) * P + (p - kCarry)] : 0;
    };
    if (j == T) {
        for (int n = tid; n < 2 * kCarry; n += 256) {
            const int ch = n / kCarry, p = n - ch * kCarry;
            carry_out[((size_t)st * 2 + ch) * kCarry + p] = (int16_t)row(ch, P + p);
        }
        return;
    }
    const int o = off0 + j * kHopN;
    for (int n = tid; n < kN; n += 256) A[n] = make_float2((float)row(swap, o + n) * win[n], (float)row(1 - swap, o + n) * win[n]);
    const float2* r = fft::forward(A, Bf, plan, tw, tid, 256);
    float2* far = spec + ((size_t)st * 2 * T + j) * kF;
    float2* near = far + (size_t)T * kF;
    for (int f = tid; f < kF; f += 256) {
        const float2 z = r[f], zc = r[f == 0 ? 0 : kN - f];
        far[f] = make_float2(0.5f * (z.x + zc.x), 0.5f * (z.y - zc.y));
        near[f] = make_float2(0.5f * (z.y + zc.y), 0.5f * (zc.x - z.x));
    }
}

// The windowed frames of a stream live in rows of `slots` frames: [the last frames before this push | the push's frames from slot `base` on].  One workgroup per
// (stream, slot): slots below `base` are copied from the OTHER buffer (slot prev_off + j there; zeros on the first push), the others are the inverse transform of
// ONE error frame each -- no pairing, so a frame's bits do not depend on its neighbours in the push.
__global__ __launch_bounds__(256) void k_nkf_stream_synthesis(const float2* __restrict__ err, int T, int base, int slots, const float* __restrict__ prev, int prev_off,
                                                              fft::Plan plan, const float2* __restrict__ tw, const float* __restrict__ win, float* __restrict__ frames) {
    __shared__ float2 A[kN];
    __shared__ float2 Bf[kN];
    const int tid = threadIdx.x, per = base + T, st = (int)blockIdx.x / per, j = (int)blockIdx.x - st * per;
    float* dst = frames + ((size_t)st * slots + j) * kN;
    if (j < base) {
        const float* src = prev ? prev + ((size_t)st * slots + prev_off + j) * kN : nullptr;
        for (int n = tid; n < kN; n += 256) dst[n] = src ? src[n] : 0.0f;
        return;
    }
    const float2* s0 = err + ((size_t)st * T + (j - base)) * kF;
    for (int f = tid; f < kF; f += 256) {
        const bool edge = f == 0 || f == kF - 1;
        const float2 a = s0[f];
        const float im = edge ? 0.0f : a.y;
        A[f] = make_float2(a.x, -im);
        if (!edge) A[kN - f] = make_float2(a.x, im);
    }
    const float2* r = fft::forward(A, Bf, plan, tw, tid, 256);
    for (int n = tid; n < kN; n += 256) dst[n] = r[n].x * (win[n] * (1.0f / (float)kN));
}

// Overlap-add of a push as a gather: output sample q of the push lies 768 samples behind the push's first input sample; slot j of the stream's frame row covers it at
// n = q + 768 - 256 j.  The sum runs over the covering slots in [jmin, jmax] in ascending order (the order of k_nkf_ola) -- jmin: the slot of frame 0 while the
// stream is younger than four hops, jmax: the last frame of the push, which only the flush reaches (the end of the signal) -- and so does the sum of the squared
// window (win2 = fp32 hann^2, added in the same order as the one-shot table is built), so head, steady state and tail need no tables.  q < qmin: before the
// stream's first sample, zero.
__global__ __launch_bounds__(256) void k_nkf_stream_ola(const float* __restrict__ frames, const float* __restrict__ win2, int slots, int jmin, int jmax, int qmin, int P,
                                                        int16_t* __restrict__ pcm, float* __restrict__ f32, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long st = i / P;
    const int q = (int)(i - st * P);
    float s = 0.0f, ws = 0.0f;
    if (q >= qmin) {
        int lo = q / kHopN, hi = lo + 3;
        if (lo < jmin) lo = jmin;
        if (hi > jmax) hi = jmax;
        for (int j = lo; j <= hi; ++j) {
            const int n = q + kCarry - j * kHopN;
            s += frames[((size_t)st * slots + j) * kN + n];
            ws += win2[n];
        }
    }
    const bool live = ws > 0.0f;
    if (f32) f32[i] = live ? s * (1.0f / ws) : 0.0f;
    if (pcm) pcm[i] = live ? (int16_t)(int)fminf(fmaxf(s * (32767.0f / ws), -32768.0f), 32767.0f) : (int16_t)0;
}

// one workgroup per (call, frame pair): W = H(Z0) + i H(Z1) stored conjugated, x0 + i x1 = conj(DFT(conj W)) / N
__global__ __launch_bounds__(256) void k_nkf_synthesis(const float2* __restrict__ err, int T, fft::Plan plan, const float2* __restrict__ tw, const float* __restrict__ win,
                                                       float* __restrict__ frames) {
    __shared__ float2 A[kN];
    __shared__ float2 Bf[kN];
    const int tid = threadIdx.x, ppr = (T + 1) / 2, call = (int)blockIdx.x / ppr, t0 = 2 * ((int)blockIdx.x - call * ppr);
    const bool two = t0 + 1 < T;
    const size_t f0 = (size_t)call * T + t0;
    const float2* s0 = err + f0 * kF;
    const float2* s1 = two ? s0 + kF : s0;
    for (int f = tid; f < kF; f += 256) {
        const bool edge = f == 0 || f == kF - 1;
        const float2 a = s0[f], b = s1[f];
        const float2 z0 = make_float2(a.x, edge ? 0.0f : a.y), z1 = two ? make_float2(b.x, edge ? 0.0f : b.y) : make_float2(0.0f, 0.0f);
        A[f] = make_float2(z0.x - z1.y, -(z0.y + z1.x));
        if (!edge) A[kN - f] = make_float2(z0.x + z1.y, z0.y - z1.x);
    }
    const float2* r = fft::forward(A, Bf, plan, tw, tid, 256);
    for (int n = tid; n < kN; n += 256) {
        const float w = win[n] * (1.0f / (float)kN);
        frames[f0 * kN + n] = r[n].x * w;
        if (two) frames[(f0 + 1) * kN + n] = -r[n].y * w;
    }
}

__global__ __launch_bounds__(256) void k_nkf_ola(const float* __restrict__ frames, const float* __restrict__ inv_ws, const float* __restrict__ inv_ws_pcm, int T, int keep,
                                                 int16_t* __restrict__ pcm, float* __restrict__ f32, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long call = i / keep;
    const int m = (int)(i - call * keep), p = m + kN / 2;
    int t_hi = p / kHopN;
    if (t_hi > T - 1) t_hi = T - 1;
    const int t_lo = p < kN ? 0 : (p - kN) / kHopN + 1;
    float s = 0.0f;
    for (int t = t_lo; t <= t_hi; ++t) s += frames[((size_t)call * T + t) * kN + (p - t * kHopN)];
    if (f32) f32[i] = s * inv_ws[m];
    if (pcm) pcm[i] = (int16_t)(int)fminf(fmaxf(s * inv_ws_pcm[m], -32768.0f), 32767.0f);     // .to(torch.int16): truncation (:407-408)
}

// ---- the back end's transforms with the REFERENCE's tables (nkf_backend_create, reference_tables): STFT_Process builds its windowed DFT kernels from fp32 angles
// fl(fl(2 pi / N * f) * t) (DFSMN_AEC/STFT_Process.py:212-251), up to 3200 rad where half an ulp is 1.2e-4 rad.  A consumer that takes the logarithm of a difference
// of spectra (dfsmn_aec's echo band) amplifies that angle error beyond 1 LSB of its output, so there the two transforms are dense products with tables built the same way,
// on the matrix cores (csrc/ade_gemm.h); the Kalman kernel between them is the same launch either way.
struct DenseFrameB {           // B(k, n): sample k of frame n = row * T + t, zero in the constant centre pad, * 2^-15
    static constexpr bool kAlongN = false;
    const int16_t* pcm;
    const float* fpcm;
    int L, T, n_win, swap;
    __device__ float operator()(int k, int n) const {
        const int row = n / T, t = n - row * T, p = t * kHopN + k - kN / 2;
        if (p < 0 || p >= L) return 0.0f;
        const int wrow = row >> 1, ch = swap ? 1 - (row & 1) : (row & 1), call = wrow / n_win;
        const size_t at = (((size_t)call * 2 + ch) * n_win + (wrow - call * n_win)) * L + p;
        return (fpcm ? fpcm[at] : (float)pcm[at]) * (1.0f / 32768.0f);
    }
};
struct DenseSpecStore {        // rows 0 .. 512 the real parts, 513 .. 1025 the imaginary parts -> [frame][bin] (re, im)
    float* spec;
    __device__ void operator()(int m, int n, float v) const { spec[((size_t)n * kF + (m < kF ? m : m - kF)) * 2 + (m >= kF ? 1 : 0)] = v; }
};
struct DenseInvA {             // A(j, k) = inverse table row k (packed re | im bins), sample j
    static constexpr bool kAlongK = false;
    const float* p;
    __device__ float operator()(int m, int k) const { return p[(size_t)k * kN + m]; }
};
struct DenseErrB {             // B(k, n) = packed [re bins | im bins] of error frame n
    static constexpr bool kAlongN = false;
    const float* e;
    __device__ float operator()(int k, int n) const { return e[((size_t)n * kF + (k < kF ? k : k - kF)) * 2 + (k >= kF ? 1 : 0)]; }
};
struct DenseFrameStore {
    float* p;
    __device__ void operator()(int m, int n, float v) const { p[(size_t)n * kN + m] = v; }
};
// The same two products over a stream's step: column n = (stream * 2 + channel) * T + j is frame j of the step, read from the rows [768 carried | P new] as
// k_nkf_stream_analysis reads them (pcm null: the flush's zeros; swap: channel 0 of the spectra, the far end, is source channel 1) ...
struct DenseStreamFrameB {
    static constexpr bool kAlongN = false;
    const int16_t* pcm;
    const int16_t* carry;
    int P, T, off0, swap;
    __device__ float operator()(int k, int n) const {
        const int row = n / T, j = n - row * T, st = row >> 1, ch = swap ? 1 - (row & 1) : (row & 1), p = off0 + j * kHopN + k;
        int v = 0;
        if (p < kCarry) v = carry[((size_t)st * 2 + ch) * kCarry + p];
        else if (pcm && p - kCarry < P) v = pcm[((size_t)st * 2 + ch) * P + (p - kCarry)];
        return (float)v * (1.0f / 32768.0f);
    }
};
// ... and error frame n = stream * T + j stored into slot base + j of the stream's frame row (k_nkf_stream_synthesis's layout)
struct DenseStreamFrameStore {
    float* p;
    int T, base, slots;
    __device__ void operator()(int m, int n, float v) const {
        const int st = n / T, j = n - st * T;
        p[((size_t)st * slots + base + j) * kN + m] = v;
    }
};

}  // namespace

struct NkfAecEngine : SubEngine {
    int device = 0, L = 0, T = 0, keep = 0;
    float* d_w = nullptr;                       // one arena: weights, window, twiddles, norms
    const float *wts = nullptr, *win = nullptr, *syn_win = nullptr, *inv_ws = nullptr, *inv_ws_pcm = nullptr;
    const float2* tw = nullptr;
    fft::Plan plan;
    int capacity = 0;
    float* ws = nullptr;
    float* mean = nullptr;
    float2 *spec = nullptr, *errs = nullptr, *kg = nullptr;
    float* frames_buf = nullptr;
    int last_batch = 0;

    ~NkfAecEngine() override {
        (void)hipSetDevice(device);
        if (d_w) (void)hipFree(d_w);
        if (ws) (void)hipFree(ws);
    }
    int frames() const override { return T; }
    int in_len() const override { return L; }
    int out_len() const override { return keep; }
    int channels() const override { return 2; }          // far end, near end (Export_NKF_AEC.py:524)
    int out_channels() const override { return 1; }
    bool accepts_float_input() const override { return true; }
    int reserve(int batch, std::string& err) override;
    int run(hipStream_t s, const int16_t* d_in, int batch, int16_t* d_out, float* d_f32, std::string& err) override;
    int tap(hipStream_t s, const char* name, int batch, float* out, size_t count, size_t* written, std::string& err) override;
    // streams (ade_stream_*): state per stream object, see NkfStream below
    const float* win2 = nullptr;                // fp32 hann^2, the terms of the window-square sum
    int stream_delay() const override { return kCarry; }
    int stream_create(int n_streams, int frames_per_push, void** state, std::string& err) override;
    int stream_reset(void* state, hipStream_t s, std::string& err) override;
    int stream_push(void* state, hipStream_t s, const int16_t* d_in, int16_t* d_out, float* d_f32, std::string& err) override;
    int stream_flush(void* state, hipStream_t s, int16_t* d_out, float* d_f32, std::string& err) override;
    void stream_destroy(void* state) override;
    int stream_step(struct NkfStream* st, hipStream_t s, const int16_t* d_in, int hops, int16_t* d_out, float* d_f32, std::string& err);
    bool near_first = false;                    // the back end of dfsmn_aec: the caller's rows are (near end, far end)
    const float *dense_fwd = nullptr, *dense_inv = nullptr;      // [1026][1024] each, the reference's fp32-angle tables (back end with reference_tables only)
    int run_backend(hipStream_t s, const int16_t* pcm, const float* fpcm, int calls, int n_win, float* wave, std::string& err);
};

// What a stream carries between pushes, for S streams that advance together.
struct NkfStream {
    int S = 0, F = 0, slots = 0;                // streams, hops per push, frame slots per stream row (3 carried + the frames of the longest step)
    long long hops = 0;                         // hops pushed since the last reset
    int16_t* carry[2] = {};                     // [S][2][768] the last input samples of both channels, ping-ponged
    int cur = 0;                                // carry[cur] / frames[cur] hold what the last step left
    float* kalman = nullptr;                    // [kStateFloats][S * 513]
    float* frames[2] = {};                      // [S][slots][1024] windowed frames, ping-ponged: the last three of a step are the head of the next one
    int prev_off = 0;                           // slot of frames[cur] that becomes slot 0 of the next step
    float2 *spec = nullptr, *errs = nullptr;    // one step's spectra [S][2][T][513] and error spectra [S][T][513]
    void* block = nullptr;                      // the one allocation behind all of the above
    size_t reset_bytes = 0;                     // its leading part that a reset clears (carries and Kalman state)
};

namespace {
int nfail(std::string& err, int st, const std::string& msg) { err = msg; return st; }
#define NK_HIP(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) return nfail(err, ADE_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)
}  // namespace

// backend: the linear canceller of another family (nkf_backend_create) -- the ISTFT keeps the raw overlap-add samples [512, 512 + in_len) and the matching slice of
// the static window-square table (the folder's istft_B_packed with output_length, DFSMN_AEC/STFT_Process.py:174-176, :256-266)
static int nkf_build(const std::map<std::string, Tensor>& tensors, int in_len, int device, bool backend, bool reference_tables, NkfAecEngine** out, std::string& err) {
    *out = nullptr;
    if (in_len < kHopN) return nfail(err, ADE_ERR_SHAPE_MISMATCH, "nkf_aec: input_audio_length shorter than one 256-sample hop");
    struct Want { const char* name; std::vector<int> dims; const float* p; };
    Want want[] = {{"fc_in_w", {2, kFc, kIn}, nullptr}, {"fc_in_b", {2, kFc}, nullptr}, {"fc_in_slope", {1}, nullptr},
                   {"gru_w_ih", {2, kG3, kFc}, nullptr}, {"gru_w_hh", {2, kG3, kHid}, nullptr}, {"gru_b_ih", {2, kG3}, nullptr}, {"gru_b_hh", {2, kG3}, nullptr},
                   {"fc_out1_w", {2, kFc, kHid}, nullptr}, {"fc_out1_b", {2, kFc}, nullptr}, {"fc_out_slope", {1}, nullptr},
                   {"fc_out2_w", {2, kTaps, kFc}, nullptr}, {"fc_out2_b", {2, kTaps}, nullptr}};
    for (auto& w : want) {
        auto it = tensors.find(w.name);
        if (it == tensors.end()) return nfail(err, ADE_ERR_MISSING_KEY, std::string("weights: tensor missing: ") + w.name);
        if (it->second.dims != w.dims) return nfail(err, ADE_ERR_SHAPE_MISMATCH, std::string("weights: tensor has the wrong shape: ") + w.name);
        w.p = it->second.data;
    }
    const float *fin_w = want[0].p, *fin_b = want[1].p, *gw_ih = want[3].p, *gw_hh = want[4].p, *gb_ih = want[5].p, *gb_hh = want[6].p, *f1w = want[7].p,
                *f1b = want[8].p, *f2w = want[10].p, *f2b = want[11].p;
    std::vector<float> arena;
    auto push = [&](size_t n) { const size_t off = arena.size(); arena.resize(off + ((n + 63) & ~(size_t)63), 0.0f); return off; };
    const size_t o_w = push(kWeights);
    float* w = &arena[o_w];
    auto interleave = [&](int off, const float* src, int n) { for (int e = 0; e < n; ++e) { w[off + 2 * e] = src[e]; w[off + 2 * e + 1] = src[n + e]; } };
    interleave(oFcInW, fin_w, kFc * kIn);
    interleave(oFcInB, fin_b, kFc);
    for (int g = 0; g < 2; ++g) {
        float* d = w + oGru + g * kGruSize;
        memcpy(d, gw_ih + (size_t)g * kG3 * kFc, sizeof(float) * kG3 * kFc);
        memcpy(d + kG3 * kFc, gw_hh + (size_t)g * kG3 * kHid, sizeof(float) * kG3 * kHid);
        memcpy(d + kG3 * kFc + kG3 * kHid, gb_ih + (size_t)g * kG3, sizeof(float) * kG3);
        memcpy(d + kG3 * kFc + kG3 * kHid + kG3, gb_hh + (size_t)g * kG3, sizeof(float) * kG3);
    }
    interleave(oFc1W, f1w, kFc * kHid);
    interleave(oFc1B, f1b, kFc);
    interleave(oFc2W, f2w, kTaps * kFc);
    interleave(oFc2B, f2b, kTaps);
    w[oSlope] = want[2].p[0];
    w[oSlope + 1] = want[9].p[0];

    NkfAecEngine* d = new NkfAecEngine();
    d->device = device;
    d->L = in_len;
    d->T = in_len / kHopN + 1;                                       // MAX_SIGNAL_LENGTH (:35)
    d->keep = kHopN * (d->T - 1) < in_len ? kHopN * (d->T - 1) : in_len;     // the ISTFT's trimmed length, then [:audio_len] (:389)
    d->near_first = backend;
    if (backend) d->keep = in_len;                                   // 512 + in_len <= 1024 + 256 (T - 1): inside the raw overlap-add
    // periodic hann as torch.hann_window builds it in fp32; the 2^-15 input scale of an int16 export folded into the analysis window (:485)
    std::vector<float> hann(kN);
    for (int n = 0; n < kN; ++n) hann[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * n / kN));
    const size_t o_wa = push(kN), o_win = push(kN), o_tw = push(2 * kN), o_iws = push(d->keep), o_iwp = push(d->keep), o_w2 = push(kN);
    for (int n = 0; n < kN; ++n) { arena[o_wa + n] = hann[n] * (1.0f / 32768.0f); arena[o_win + n] = hann[n]; arena[o_w2 + n] = hann[n] * hann[n]; }
    for (int m = 0; m < kN; ++m) { const double a = -2.0 * M_PI * (double)m / (double)kN; arena[o_tw + 2 * m] = (float)cos(a); arena[o_tw + 2 * m + 1] = (float)sin(a); }
    {
        std::vector<float> wsum((size_t)kN + (size_t)kHopN * (d->T - 1), 0.0f);     // conv_transpose1d(ones, window^2) in fp32 (STFT_Process.py:242-249)
        for (int t = 0; t < d->T; ++t)
            for (int n = 0; n < kN; ++n) wsum[(size_t)t * kHopN + n] += hann[n] * hann[n];
        for (int m = 0; m < d->keep; ++m) {
            arena[o_iws + m] = 1.0f / wsum[kN / 2 + m];
            arena[o_iwp + m] = 32767.0f / wsum[kN / 2 + m];
        }
    }
    size_t o_df = 0, o_di = 0;
    if (backend && reference_tables) {
        o_df = push((size_t)2 * kF * kN);
        o_di = push((size_t)2 * kF * kN);
        const float c32 = (float)(2.0 * M_PI / kN);
        for (int f = 0; f < kF; ++f) {
            const float cf = c32 * (float)f, sc = (f == 0 || f == kF - 1) ? 1.0f : 2.0f;
            for (int t = 0; t < kN; ++t) {
                const float om = cf * (float)t, c = cosf(om), sn = sinf(om);
                arena[o_df + (size_t)f * kN + t] = c * hann[t];
                arena[o_df + (size_t)(kF + f) * kN + t] = -sn * hann[t];
                arena[o_di + (size_t)f * kN + t] = (sc * c * (1.0f / (float)kN)) * hann[t];
                arena[o_di + (size_t)(kF + f) * kN + t] = (sc * -sn * (1.0f / (float)kN)) * hann[t];
            }
        }
    }
    if (!fft::make_plan(kN, &d->plan)) { delete d; return nfail(err, ADE_ERR_UNSUPPORTED, "nkf_aec: FFT plan"); }
    auto bail = [&](int st) { delete d; return st; };
    if (hipSetDevice(device) != hipSuccess) return bail(nfail(err, ADE_ERR_DEVICE, "hipSetDevice failed"));
    if (hipMalloc((void**)&d->d_w, arena.size() * sizeof(float)) != hipSuccess) return bail(nfail(err, ADE_ERR_DEVICE, "hipMalloc of the NKF-AEC weights failed"));
    if (hipMemcpy(d->d_w, arena.data(), arena.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return bail(nfail(err, ADE_ERR_DEVICE, "upload of the NKF-AEC weights failed"));
    d->wts = d->d_w + o_w;
    d->win = d->d_w + o_wa;
    d->tw = reinterpret_cast<const float2*>(d->d_w + o_tw);
    d->inv_ws = d->d_w + o_iws;
    d->inv_ws_pcm = d->d_w + o_iwp;
    d->syn_win = d->d_w + o_win;
    d->win2 = d->d_w + o_w2;
    if (backend && reference_tables) { d->dense_fwd = d->d_w + o_df; d->dense_inv = d->d_w + o_di; }
    *out = d;
    return ADE_OK;
}

int nkf_aec_create(const std::map<std::string, Tensor>& tensors, int in_len, int device, SubEngine** out, std::string& err) {
    NkfAecEngine* d = nullptr;
    const int st = nkf_build(tensors, in_len, device, false, false, &d, err);
    *out = d;
    return st;
}

namespace {
struct NkfBackendImpl : NkfBackend {
    NkfAecEngine* e = nullptr;
    ~NkfBackendImpl() override { delete e; }
    int frames() const override { return e->T; }
    int reserve(int windows, std::string& err) override { return e->reserve(windows, err); }
    int run(hipStream_t s, const int16_t* pcm, const float* fpcm, int calls, int n_win, float* wave, std::string& err) override {
        return e->run_backend(s, pcm, fpcm, calls, n_win, wave, err);
    }
    int stream_create(int n_streams, int frames_per_push, void** state, std::string& err) override { return e->stream_create(n_streams, frames_per_push, state, err); }
    int stream_reset(void* state, hipStream_t s, std::string& err) override { return e->stream_reset(state, s, err); }
    int stream_step(void* state, hipStream_t s, const int16_t* pcm, float* wave, std::string& err) override { return e->stream_push(state, s, pcm, nullptr, wave, err); }
    int stream_flush(void* state, hipStream_t s, float* wave, std::string& err) override { return e->stream_flush(state, s, nullptr, wave, err); }
    void stream_destroy(void* state) override { e->stream_destroy(state); }
};
}  // namespace

int nkf_backend_create(const std::map<std::string, Tensor>& tensors, int window_len, bool reference_tables, int device, NkfBackend** out, std::string& err) {
    *out = nullptr;
    NkfAecEngine* d = nullptr;
    const int st = nkf_build(tensors, window_len, device, true, reference_tables, &d, err);
    if (st != ADE_OK) return st;
    NkfBackendImpl* b = new NkfBackendImpl();
    b->e = d;
    *out = b;
    return ADE_OK;
}

int NkfAecEngine::reserve(int calls, std::string& err) {
    if (calls <= capacity) return ADE_OK;
    NK_HIP(hipSetDevice(device));
    NK_HIP(hipDeviceSynchronize());
    if (ws) (void)hipFree(ws);
    ws = nullptr;
    capacity = 0;
    const size_t B = calls, nsp = (size_t)T * kF;
    const size_t sizes[5] = {B * 2, B * 2 * nsp * 2, B * nsp * 2, B * kF * kTaps * 2, B * T * kN};
    size_t total = 0;
    for (size_t s : sizes) total += (s + 63) & ~(size_t)63;
    NK_HIP(hipMalloc((void**)&ws, total * sizeof(float)));
    float* p[5];
    size_t off = 0;
    for (int i = 0; i < 5; ++i) { p[i] = ws + off; off += (sizes[i] + 63) & ~(size_t)63; }
    mean = p[0];
    spec = reinterpret_cast<float2*>(p[1]);
    errs = reinterpret_cast<float2*>(p[2]);
    kg = reinterpret_cast<float2*>(p[3]);
    frames_buf = p[4];
    capacity = calls;
    return ADE_OK;
}

int NkfAecEngine::run(hipStream_t s, const int16_t* d_in, int batch, int16_t* d_out, float* d_f32, std::string& err) {
    if (batch == 0) return ADE_OK;
    int st = reserve(batch, err);
    if (st != ADE_OK) return st;
    const int ppr = (T + 1) / 2;
    hipLaunchKernelGGL(k_nkf_mean, dim3((unsigned)(batch * 2)), dim3(256), 0, s, d_in, float_in, L, mean);
    hipLaunchKernelGGL(k_nkf_analysis, dim3((unsigned)(batch * 2 * ppr)), dim3(256), 0, s, d_in, float_in, (const float*)mean, L, T, plan, tw, win, spec, 1, 0);
    hipLaunchKernelGGL(k_nkf_kalman<false>, dim3((unsigned)((batch * kF + kKalmanThreads - 1) / kKalmanThreads)), dim3(kKalmanThreads), 0, s, (const float2*)spec, wts, T,
                       batch, errs, kg, (float*)nullptr);
    hipLaunchKernelGGL(k_nkf_synthesis, dim3((unsigned)(batch * ppr)), dim3(256), 0, s, (const float2*)errs, T, plan, tw, syn_win, frames_buf);
    const long long total = (long long)batch * keep;
    hipLaunchKernelGGL(k_nkf_ola, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)frames_buf, inv_ws, inv_ws_pcm, T, keep, d_out, d_f32, total);
    NK_HIP(hipGetLastError());
    last_batch = batch;
    return ADE_OK;
}

// The back end form: no mean kernel, the caller's [call][near, far][n_win windows] rows, every window an independent filter, a float waveform of L samples per window.
int NkfAecEngine::run_backend(hipStream_t s, const int16_t* pcm, const float* fpcm, int calls, int n_win, float* wave, std::string& err) {
    const int rows = calls * n_win;
    if (rows == 0) return ADE_OK;
    int st = reserve(rows, err);
    if (st != ADE_OK) return st;
    const int ppr = (T + 1) / 2;
    if (dense_fwd)
        gemm::launch(s, gemm::RowMajorA{dense_fwd, kN}, DenseFrameB{pcm, fpcm, L, T, n_win, 1}, DenseSpecStore{reinterpret_cast<float*>(spec)}, 2 * kF, rows * 2 * T, kN);
    else
        hipLaunchKernelGGL(k_nkf_analysis, dim3((unsigned)(rows * 2 * ppr)), dim3(256), 0, s, pcm, fpcm, (const float*)nullptr, L, T, plan, tw, win, spec, n_win, 1);
    hipLaunchKernelGGL(k_nkf_kalman<false>, dim3((unsigned)((rows * kF + kKalmanThreads - 1) / kKalmanThreads)), dim3(kKalmanThreads), 0, s, (const float2*)spec, wts, T,
                       rows, errs, kg, (float*)nullptr);
    if (dense_inv)
        gemm::launch(s, DenseInvA{dense_inv}, DenseErrB{reinterpret_cast<const float*>(errs)}, DenseFrameStore{frames_buf}, kN, rows * T, 2 * kF);
    else
        hipLaunchKernelGGL(k_nkf_synthesis, dim3((unsigned)(rows * ppr)), dim3(256), 0, s, (const float2*)errs, T, plan, tw, syn_win, frames_buf);
    const long long total = (long long)rows * keep;
    hipLaunchKernelGGL(k_nkf_ola, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)frames_buf, inv_ws, (const float*)nullptr, T, keep,
                       (int16_t*)nullptr, wave, total);
    NK_HIP(hipGetLastError());
    last_batch = rows;
    return ADE_OK;
}

int NkfAecEngine::tap(hipStream_t s, const char* name, int batch, float* out, size_t count, size_t* written, std::string& err) {
    const size_t nsp = (size_t)T * kF;
    if (!spec || batch <= 0 || batch > capacity) return nfail(err, ADE_ERR_NOT_FOUND, "tap has no data yet");
    size_t n = 0;
    if (strcmp(name, "spec") == 0) n = (size_t)batch * 2 * nsp * 2;               // [call][far, near][frame][bin] (re, im)
    else if (strcmp(name, "echo_hat") == 0) n = (size_t)batch * nsp * 2;          // [call][frame][bin] (re, im)
    else if (strcmp(name, "kg") == 0) n = (size_t)batch * kF * kTaps * 2;         // [call][bin][tap] (re, im), the last frame's Kalman gain
    else return nfail(err, ADE_ERR_NOT_FOUND, std::string("unknown tap: ") + name);
    if (count < n) return nfail(err, ADE_ERR_SHAPE_MISMATCH, "tap buffer too small");
    NK_HIP(hipStreamSynchronize(s));
    if (strcmp(name, "echo_hat") == 0) {                                           // mic - (mic - echo_hat)
        std::vector<float> sp((size_t)batch * 2 * nsp * 2);
        NK_HIP(hipMemcpy(sp.data(), spec, sp.size() * sizeof(float), hipMemcpyDeviceToHost));
        NK_HIP(hipMemcpy(out, errs, n * sizeof(float), hipMemcpyDeviceToHost));
        for (int b = 0; b < batch; ++b) {
            const float* mic = sp.data() + ((size_t)b * 2 + 1) * nsp * 2;
            float* o = out + (size_t)b * nsp * 2;
            for (size_t k = 0; k < nsp * 2; ++k) o[k] = mic[k] - o[k];
        }
    } else {
        NK_HIP(hipMemcpy(out, strcmp(name, "spec") == 0 ? (const void*)spec : (const void*)kg, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    *written = n;
    return ADE_OK;
}

// ---- streams ----------------------------------------------------------------------------------------------------------------------------------------------------
int NkfAecEngine::stream_create(int n_streams, int frames_per_push, void** state, std::string& err) {
    *state = nullptr;
    if (n_streams < 1 || frames_per_push < 1 || frames_per_push > 4096)
        return nfail(err, ADE_ERR_BAD_VALUE, "ade_stream_create: nkf_aec needs n_streams >= 1 and 1 <= frames_per_push <= 4096");
    if ((long long)n_streams * kF > 0x7fffffffLL / 2 || (long long)n_streams * (frames_per_push + 1) * 2 > 0x7fffffffLL)
        return nfail(err, ADE_ERR_BAD_VALUE, "ade_stream_create: nkf_aec: n_streams * frames_per_push exceeds the launch grid");
    NK_HIP(hipSetDevice(device));
    NkfStream* st = new NkfStream();
    st->S = n_streams;
    st->F = frames_per_push;
    const size_t S = (size_t)n_streams, Tm = (size_t)(frames_per_push > 2 ? frames_per_push : 2);      // the flush runs two frames
    st->slots = (int)Tm + 3;
    auto up = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    const size_t b_carry = up(S * 2 * kCarry * sizeof(int16_t)), b_kal = up((size_t)kStateFloats * S * kF * sizeof(float)), b_fr = up(S * st->slots * kN * sizeof(float)),
                 b_spec = up(S * 2 * Tm * kF * sizeof(float2)), b_err = up(S * Tm * kF * sizeof(float2));
    if (hipMalloc(&st->block, 2 * b_carry + b_kal + 2 * b_fr + b_spec + b_err) != hipSuccess) {
        delete st;
        return nfail(err, ADE_ERR_DEVICE, "ade_stream_create: hipMalloc of the NKF-AEC stream state failed");
    }
    char* p = (char*)st->block;
    st->carry[0] = (int16_t*)p; p += b_carry;
    st->carry[1] = (int16_t*)p; p += b_carry;
    st->kalman = (float*)p; p += b_kal;
    st->reset_bytes = 2 * b_carry + b_kal;
    st->frames[0] = (float*)p; p += b_fr;
    st->frames[1] = (float*)p; p += b_fr;
    st->spec = (float2*)p; p += b_spec;
    st->errs = (float2*)p;
    *state = st;
    return ADE_OK;
}

int NkfAecEngine::stream_reset(void* state, hipStream_t s, std::string& err) {
    NkfStream* st = (NkfStream*)state;
    NK_HIP(hipMemsetAsync(st->block, 0, st->reset_bytes, s));     // the frame rows need no clearing: the first step writes its carried slots as zeros
    st->hops = 0;
    st->cur = 0;
    st->prev_off = 0;
    return ADE_OK;
}

// One step: `hops` new hops of input (d_in null: zeros past the end of the signal, the flush).  Analysis, Kalman, synthesis, overlap-add: four launches (six with the
// reference's tables, the back end of dfsmn_aec in its default mode: each transform is a dense product plus the kernel that moves what is carried).
int NkfAecEngine::stream_step(NkfStream* st, hipStream_t s, const int16_t* d_in, int hops, int16_t* d_out, float* d_f32, std::string& err) {
    const bool first = st->hops == 0, flush = d_in == nullptr;
    const int S = st->S, P = hops * kHopN, T = first ? hops - 1 : hops, base = first ? 4 : 3, nxt = st->cur ^ 1;
    const int out = flush ? kCarry : P;                                                  // the flush emits the 768 samples still owed
    const int young = st->hops < 4 ? (int)st->hops : 4;                                  // slot j holds frame hops - 4 + j
    const int swap = near_first ? 1 : 0;
    const int16_t* carry = st->carry[st->cur];
    int16_t* carry_next = flush ? (int16_t*)nullptr : st->carry[nxt];
    const float* prev = first ? (const float*)nullptr : (const float*)st->frames[st->cur];
    if (dense_fwd) {          // the reference's tables: the frames of the step as one dense product, the carry moved by the analysis kernel run without frames
        if (T > 0)
            gemm::launch(s, gemm::RowMajorA{dense_fwd, kN}, DenseStreamFrameB{d_in, carry, P, T, first ? kHopN : 0, swap}, DenseSpecStore{reinterpret_cast<float*>(st->spec)},
                         2 * kF, S * 2 * T, kN);
        if (!flush)
            hipLaunchKernelGGL(k_nkf_stream_analysis, dim3((unsigned)S), dim3(256), 0, s, d_in, carry, carry_next, P, 0, 0, plan, tw, win, st->spec, swap);
    } else {
        hipLaunchKernelGGL(k_nkf_stream_analysis, dim3((unsigned)(S * (T + (flush ? 0 : 1)))), dim3(256), 0, s, d_in, carry, carry_next, P, T, first ? kHopN : 0, plan, tw,
                           win, st->spec, swap);
    }
    hipLaunchKernelGGL(k_nkf_kalman<true>, dim3((unsigned)((S * kF + kKalmanThreads - 1) / kKalmanThreads)), dim3(kKalmanThreads), 0, s, (const float2*)st->spec, wts, T, S,
                       st->errs, (float2*)nullptr, st->kalman);
    if (dense_inv) {          // the carried slots copied by the synthesis kernel run without frames, the new ones stored by the product
        hipLaunchKernelGGL(k_nkf_stream_synthesis, dim3((unsigned)(S * base)), dim3(256), 0, s, (const float2*)st->errs, 0, base, st->slots, prev, st->prev_off, plan, tw,
                           syn_win, st->frames[nxt]);
        if (T > 0)
            gemm::launch(s, DenseInvA{dense_inv}, DenseErrB{reinterpret_cast<const float*>(st->errs)}, DenseStreamFrameStore{st->frames[nxt], T, base, st->slots}, kN, S * T,
                         2 * kF);
    } else {
        hipLaunchKernelGGL(k_nkf_stream_synthesis, dim3((unsigned)(S * (base + T))), dim3(256), 0, s, (const float2*)st->errs, T, base, st->slots, prev, st->prev_off, plan,
                           tw, syn_win, st->frames[nxt]);
    }
    const long long total = (long long)S * out;
    hipLaunchKernelGGL(k_nkf_stream_ola, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)st->frames[nxt], win2, st->slots, 4 - young, base + T - 1,
                       kCarry - young * kHopN > 0 ? kCarry - young * kHopN : 0, out, d_out, d_f32, total);
    NK_HIP(hipGetLastError());
    st->prev_off = base + T - 3;
    st->cur = nxt;
    st->hops += hops;
    return ADE_OK;
}

int NkfAecEngine::stream_push(void* state, hipStream_t s, const int16_t* d_in, int16_t* d_out, float* d_f32, std::string& err) {
    NkfStream* st = (NkfStream*)state;
    return stream_step(st, s, d_in, st->F, d_out, d_f32, err);
}

// the last two frames (n - 1 and n after n hops), their samples past the end the zeros of the reference's constant centre pad
int NkfAecEngine::stream_flush(void* state, hipStream_t s, int16_t* d_out, float* d_f32, std::string& err) {
    NkfStream* st = (NkfStream*)state;
    if (st->hops == 0) return nfail(err, ADE_ERR_BAD_VALUE, "ade_stream_flush: nothing to flush");
    return stream_step(st, s, nullptr, 2, d_out, d_f32, err);
}

void NkfAecEngine::stream_destroy(void* state) {
    NkfStream* st = (NkfStream*)state;
    if (!st) return;
    (void)hipSetDevice(device);
    if (st->block) (void)hipFree(st->block);
    delete st;
}

}  // namespace ade
