// ade_ulunas.hip — UL-UNAS (ultra-lightweight 16 kHz speech enhancement) on the MI355X: SURVEY.md section 8 row f2.
//
// Reference: ULUNAS_CUSTOM.forward (UL-UNAS/Export_UL_UNAS.py:848-913) around ULUNAS.forward and its blocks (:111-739), over the
// tensors audio_denoiser_onnx_amd/ulunas.py::fold_state_dict produces (BatchNorm folded into the convolutions, AffinePReLU as
// positive / negative slope tables per (channel, bin), the two half-width GRUs of every grouped GRU):
//   int16 -> * 2^-15 -> STFT(512, hop 256, periodic hann, reflect) -> log(max(|X|^2, 1e-24)) -> ERB merge (65 + 64 bands) ->
//   5 encoder blocks (XConvBlock / XMBBlocks / XDWSBlock: grouped, depthwise and pointwise convolutions causal in time, stride on
//   frequency, AffinePReLU, channel shuffle, each ending in a causal time-frequency attention cTFA = time GRU gate x frequency
//   bi-GRU gate) -> 2 x DPGRNN (the same grouped dual-path GRU as GTCRN's) -> 5 decoder blocks on x + skip (transposed
//   convolutions) -> sigmoid -> ERB split -> real mask x spectrum -> ISTFT -> * 32767, clamp, truncate -> int16.
// A first, correctness-first implementation: activations are channels-last (batch, frame, bin, channel) tensors in HBM and every
// operator is its own bandwidth-bound kernel (one generic convolution kernel covers all 23 convolutions through a descriptor).
// The DPGRNN blocks ARE GTCRN's (same widths: 33 bins x 16 channels) and reuse its multi-kernel path (ade_kernels.hip); the STFT
// pair is the generic operator of ade_stft.hip (dense windowed DFT on the matrix cores, exact-angle tables).
#include "ade_device.h"
#include "ade_fft.h"
#include "ade_internal.h"
#include "../../include/ade.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <type_traits>

namespace ade {

namespace {

using dev::mk2;
using dev::v2f;

constexpr int kUNfft = 512, kUHop = 256, kUBins = 257, kULow = 65, kUBands = 64, kUHigh = 192, kUErb = kULow + kUBands;   // 129

__device__ __forceinline__ float usig(float x) { return ade::dev::sigmoid_f(x); }      // (round 5: hardware exp2 / rcp; libm expf + the IEEE division were ~27 instructions per gate of the cTFA GRUs)

struct ConvDesc {              // one (de)convolution + bias [+ AffinePReLU] [+ channel shuffle] over (B, T, F, C) tensors
    const float *w, *b, *pos, *neg, *abias;     // w in torch layout: Conv2d (Cout, Cin/g, kt, kf); ConvTranspose2d (Cin, Cout/g, kt, kf)
    int Cin, Cout, Fi, Fo, kt, kf, stride, groups, deconv, shuffle;
};

__device__ __forceinline__ int shuffled(int j, int C) { return (j & 1) ? (j >> 1) + (C >> 1) : (j >> 1); }   // Shuffle.indices (:200-203)

// One output of one (de)convolution of a frame: position o = fo * Cout + co of the output frame, from the kt staged input frames xin[a][Fi * Cin] (tap a = frame
// t - (KT - 1) + a, or t - a for a transposed convolution) and the weights wl in their torch layout, both in LDS.  Bias, AffinePReLU and the channel shuffle included.
template <int KT, int KF, int STRIDE, bool DECONV>      // the five kernel shapes of ULUNAS() (:667) as compile-time constants: the tap loops unroll
__device__ __forceinline__ float conv_out(const float* __restrict__ xin, int row, const float* __restrict__ wl, const ConvDesc& d, int o, int cog, int cig) {
    constexpr int pf = KF / 2;
    const int fo = o / d.Cout, co = o - fo * d.Cout;
    const int cc = d.shuffle ? shuffled(co, d.Cout) : co;       // output position co holds convolution channel cc
    const int g = cc / cog;
    float acc = d.b[cc];
    if (KT == 1 && KF == 1 && !DECONV && STRIDE == 1 && !(cig & 3) && !(d.Cin & 3)) {
        // pointwise convolution (twelve per call, 28 % of the step as launches of their own): the channel run of the position and the weight row are both contiguous -- four
        // channels per ds_read_b128 pair instead of two scalar LDS reads per multiply-add; four partial sums, added in a fixed order
        const float4* xr4 = reinterpret_cast<const float4*>(xin + fo * d.Cin + g * cig);
        const float4* wr4 = reinterpret_cast<const float4*>(wl + cc * cig);
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        for (int q = 0; q < (cig >> 2); ++q) {
            const float4 xv = xr4[q], wv = wr4[q];
            a0 = fmaf(xv.x, wv.x, a0); a1 = fmaf(xv.y, wv.y, a1); a2 = fmaf(xv.z, wv.z, a2); a3 = fmaf(xv.w, wv.w, a3);
        }
        acc += (a0 + a1) + (a2 + a3);
    } else
#pragma unroll
    for (int a = 0; a < KT; ++a)
#pragma unroll
        for (int bb = 0; bb < KF; ++bb) {
            int fi;
            if (DECONV) {
                const int num = fo + pf - bb;
                if (num < 0 || num % STRIDE) continue;
                fi = num / STRIDE;
            } else {
                fi = fo * STRIDE - pf + bb;
            }
            if (fi < 0 || fi >= d.Fi) continue;
            const float* xr = xin + a * row + fi * d.Cin + g * cig;
            for (int ci = 0; ci < cig; ++ci) {
                const float wv = DECONV ? wl[(((g * cig + ci) * cog + (cc - g * cog)) * KT + a) * KF + bb] : wl[((cc * cig + ci) * KT + a) * KF + bb];
                acc += xr[ci] * wv;
            }
        }
    if (d.pos) acc = (acc > 0.0f ? d.pos[cc * d.Fo + fo] : d.neg[cc * d.Fo + fo]) * acc + d.abias[cc * d.Fo + fo];   // AffinePReLU (:128-130)
    return acc;
}

// A whole output frame of one (de)convolution by the workgroup: emit(o, value) for every position o = fo * Cout + co.  (Round 5.)  conv_out() per output spends its
// time on index arithmetic -- two integer divisions, the shuffle, the group, three table addresses -- not on multiply-adds: a launch ran at ~13 % of the vector rate.
// Here a thread KEEPS its output channel (co = tid % Cout, one division per thread and frame) and walks the positions fo0, fo0 + 256 / Cout, ...: channel, group, bias,
// AffinePReLU rows and -- for the pointwise and the one-input-channel shapes, all but the last deconvolution -- its weight row in registers are per-thread constants.
template <int CIG>
__device__ __forceinline__ float pw_dot(const float* __restrict__ xr, const float (&w)[CIG]) {
    if constexpr (CIG % 4 == 0) {      // four partial sums, added in a fixed order (the order of the float4 path of conv_out)
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
        for (int q = 0; q < CIG / 4; ++q) {
            const float4 xv = reinterpret_cast<const float4*>(xr)[q];
            a0 = fmaf(xv.x, w[4 * q], a0); a1 = fmaf(xv.y, w[4 * q + 1], a1); a2 = fmaf(xv.z, w[4 * q + 2], a2); a3 = fmaf(xv.w, w[4 * q + 3], a3);
        }
        return (a0 + a1) + (a2 + a3);
    } else {
        float a = 0.0f;
#pragma unroll
        for (int q = 0; q < CIG / 2; ++q) {
            const float2 xv = reinterpret_cast<const float2*>(xr)[q];
            a += xv.x * w[2 * q]; a += xv.y * w[2 * q + 1];
        }
        return a;
    }
}
template <int KT, int KF, int STRIDE, bool DECONV, class Emit>
__device__ __forceinline__ void conv_frame(const float* __restrict__ xin, int row, const float* __restrict__ wl, const ConvDesc& d, Emit&& emit) {
    const int Cout = d.Cout, cog = Cout / d.groups, cig = d.Cin / d.groups, Fo = d.Fo;
    constexpr bool kPw = KT == 1 && KF == 1 && !DECONV && STRIDE == 1;
    const bool fast = kPw ? (cig == 6 && !(d.Cin & 1)) || ((cig == 8 || cig == 12 || cig == 16) && !(d.Cin & 3)) : cig == 1;      // (vector LDS reads of a position's channel run)
    if (!fast || Cout > 256) {         // (the last deconvolution: 12 -> 1 channels, 3 x 3 taps)
        for (int o = threadIdx.x; o < Fo * Cout; o += 256) emit(o, conv_out<KT, KF, STRIDE, DECONV>(xin, row, wl, d, o, cog, cig));
        return;
    }
    const int nper = 256 / Cout, fo0 = (int)threadIdx.x / Cout, co = (int)threadIdx.x - fo0 * Cout;
    if (fo0 >= nper) return;
    const int cc = d.shuffle ? shuffled(co, Cout) : co, g = cc / cog;
    const float bias = d.b[cc];
    const float *pos = d.pos ? d.pos + cc * Fo : nullptr, *neg = d.pos ? d.neg + cc * Fo : nullptr, *ab = d.pos ? d.abias + cc * Fo : nullptr;
    auto act = [&](float acc, int fo) { return pos ? (acc > 0.0f ? pos[fo] : neg[fo]) * acc + ab[fo] : acc; };      // AffinePReLU (:128-130)
    if constexpr (kPw) {
        const float* xg = xin + g * cig;
        auto run = [&](auto cig_c) {
            constexpr int CIG = decltype(cig_c)::value;
            float w[CIG];
#pragma unroll
            for (int q = 0; q < CIG; ++q) w[q] = wl[cc * CIG + q];
            for (int fo = fo0; fo < Fo; fo += nper) emit(fo * Cout + co, act(bias + pw_dot<CIG>(xg + fo * d.Cin, w), fo));
        };
        if (cig == 6) run(std::integral_constant<int, 6>{});
        else if (cig == 8) run(std::integral_constant<int, 8>{});
        else if (cig == 12) run(std::integral_constant<int, 12>{});
        else run(std::integral_constant<int, 16>{});
    } else {                           // one input channel per output channel (depthwise, and the first block's 1 -> 12): KT x KF weights
        constexpr int pf = KF / 2;
        float w[KT][KF];
#pragma unroll
        for (int a = 0; a < KT; ++a)
#pragma unroll
            for (int bb = 0; bb < KF; ++bb) w[a][bb] = wl[(cc * KT + a) * KF + bb];      // (both layouts: Conv2d (Cout, 1, kt, kf); ConvTranspose2d (Cin, cog, kt, kf) at cig == 1)
        const float* xg = xin + g;
        for (int fo = fo0; fo < Fo; fo += nper) {
            float acc = bias;
#pragma unroll
            for (int a = 0; a < KT; ++a)
#pragma unroll
                for (int bb = 0; bb < KF; ++bb) {
                    int fi;
                    if (DECONV) {
                        const int num = fo + pf - bb;
                        if (num < 0 || num % STRIDE) continue;
                        fi = num / STRIDE;
                    } else {
                        fi = fo * STRIDE - pf + bb;
                    }
                    if (fi < 0 || fi >= d.Fi) continue;
                    acc += xg[a * row + fi * d.Cin] * w[a][bb];
                }
            emit(fo * Cout + co, act(acc, fo));
        }
    }
}

// The cTFA statistics of a block's last convolution (:181-182, :150): zt[c] = mean_f y^2, pfreq[f] = mean_c y^2 of the frame this workgroup has just written to orow.
// sq: Fo * Cout floats of LDS nobody reads any more (the caller has synchronised).
__device__ __forceinline__ void frame_stats(const float* __restrict__ orow, float* __restrict__ sq, int Fo, int Cout, long long frame, float* __restrict__ zt,
                                            float* __restrict__ pfreq) {
    for (int o = threadIdx.x; o < Fo * Cout; o += 256) { const float v = orow[o]; sq[o] = v * v; }   // own writes: visible to this thread
    __syncthreads();
    for (int c = threadIdx.x; c < Cout; c += 256) {
        float a = 0.0f;
        for (int f = 0; f < Fo; ++f) a += sq[f * Cout + c];
        zt[frame * Cout + c] = a / (float)Fo;
    }
    for (int f = threadIdx.x; f < Fo; f += 256) {
        float a = 0.0f;
        for (int c = 0; c < Cout; ++c) a += sq[f * Cout + c];
        pfreq[frame * Fo + f] = a / (float)Cout;
    }
}

// Where k_ulu_conv takes its input frames from.  stage(): tap frame tt of row b into dst (tt < 0: before the row's first frame); keep(): called with the staged
// frame t itself, already summed with the second input.
struct ClipFrames {            // a whole clip per row: nothing precedes frame 0
    const float *x, *x2;
    __device__ __forceinline__ void stage(float* __restrict__ dst, long long b, int tt, int T, int row) const {
        const size_t at = ((size_t)b * T + (tt < 0 ? 0 : tt)) * row;
        for (int i = threadIdx.x; i < row; i += 256) dst[i] = tt < 0 ? 0.0f : (x2 ? x[at + i] + x2[at + i] : x[at + i]);
    }
    __device__ __forceinline__ void keep(const float*, long long, int, int, int) const {}
};
// A push of T frames per stream (row b = stream): the Hk = kt - 1 frames before it come from the stream's history hist_in [stream][Hk][row], oldest first -- zeros on a
// fresh stream, the reset's memset -- and the push's last Hk staged frames become hist_out (the OTHER buffer of a ping-pong pair: workgroups of this launch still read
// hist_in).  T >= Hk, so the next history is always whole frames of this push; hist_out null: the flush, after which the stream is reset.
struct PushFrames {
    const float *x, *x2, *hist_in;
    float* hist_out;
    int Hk;
    __device__ __forceinline__ void stage(float* __restrict__ dst, long long b, int tt, int T, int row) const {
        if (tt < 0) {
            const float* h = hist_in + ((size_t)b * Hk + (Hk + tt)) * row;
            for (int i = threadIdx.x; i < row; i += 256) dst[i] = h[i];
            return;
        }
        const size_t at = ((size_t)b * T + tt) * row;
        for (int i = threadIdx.x; i < row; i += 256) dst[i] = x2 ? x[at + i] + x2[at + i] : x[at + i];
    }
    __device__ __forceinline__ void keep(const float* __restrict__ cur, long long b, int t, int T, int row) const {
        const int q = t - (T - Hk);
        if (!hist_out || q < 0) return;
        float* h = hist_out + ((size_t)b * Hk + q) * row;
        for (int i = threadIdx.x; i < row; i += 256) h[i] = cur[i];       // (elements this thread staged itself: no barrier needed)
    }
};

// out[b][t][fo][co] = act(bias + sum over taps / group channels), causal in t (:222-238, :264-267); optional second input added first (:648).
// One workgroup per frame: the kt input frames it needs (already summed with the skip tensor) and the whole weight tensor are staged in LDS
// once, so HBM / L2 sees every input element kt times instead of once per tap, channel and output.
template <int KT, int KF, int STRIDE, bool DECONV, class Src>
__global__ __launch_bounds__(256) void k_ulu_conv(Src src, ConvDesc d, float* __restrict__ out, int T, int wsize, float* __restrict__ zt, float* __restrict__ pfreq) {
    HIP_DYNAMIC_SHARED(float, lds)
    const long long frame = blockIdx.x;
    const long long b = frame / T;
    const int t = (int)(frame - b * T), row = d.Fi * d.Cin;
    float* xin = lds;                      // [kt][Fi * Cin]
    float* wl = lds + KT * row;          // the weights in their torch layout
    for (int a = 0; a < KT; ++a) src.stage(xin + a * row, b, DECONV ? t - a : t - (KT - 1) + a, T, row);
    if constexpr (KT > 1) src.keep(xin + (DECONV ? 0 : KT - 1) * row, b, t, T, row);
    for (int i = threadIdx.x; i < wsize; i += 256) wl[i] = d.w[i];
    __syncthreads();
    float* orow = out + (size_t)frame * d.Fo * d.Cout;
    conv_frame<KT, KF, STRIDE, DECONV>(xin, row, wl, d, [&](int o, float v) { orow[o] = v; });
    if (!zt) return;
    __syncthreads();                       // every thread is done with the staged inputs: the region is reused for the squares (Fo * Cout <= the staged size is NOT guaranteed -> sized by the launcher)
    frame_stats(orow, lds, d.Fo, d.Cout, frame, zt, pfreq);
}

// time attention (:183-186): GRU(C -> 2C) over frames, Linear(2C -> C), sigmoid.  The recurrence is a chain of T dependent steps, so
// everything it touches lives in LDS (weights once per workgroup, the clip's inputs 64 frames at a time) and one step is spread over four
// wavefronts: wavefront p accumulates a quarter of the C + 2C contraction for every hidden unit (lane = unit), wavefront 0 adds the
// four partial sums, applies the gates and the output Linear.
// wih_t [C][3][2C], whh_t [2C][3][2C] (transposed so that lanes read consecutive floats), fc_t [2C][C].
template <int C>               // compile-time channel count: the k loops unroll and their LDS reads pipeline
__global__ __launch_bounds__(256) void k_ulu_ta(const float* __restrict__ zt, const float* __restrict__ wih_t, const float* __restrict__ whh_t,
                                                const float* __restrict__ bih, const float* __restrict__ bhh, const float* __restrict__ fc_t,
                                                const float* __restrict__ fc_b, float* __restrict__ at, int T, float* __restrict__ state) {
    HIP_DYNAMIC_SHARED(float, lds)
    __shared__ float hs[64];
    __shared__ float part[4][6][64];
    constexpr int H = 2 * C, KI = (C + 3) / 4, KH = (H + 3) / 4;       // per-wavefront slices of the two contractions
    const int b = blockIdx.x, tid = threadIdx.x, j = tid & 63, p = tid >> 6;
    float* s_wih = lds;                       // C * 3 * H
    float* s_whh = s_wih + C * 3 * H;         // H * 3 * H
    float* s_fc = s_whh + H * 3 * H;          // H * C
    float* s_z = s_fc + H * C;                // 64 frames of the clip's zt rows
    for (int i = tid; i < C * 3 * H; i += 256) s_wih[i] = wih_t[i];
    for (int i = tid; i < H * 3 * H; i += 256) s_whh[i] = whh_t[i];
    for (int i = tid; i < H * C; i += 256) s_fc[i] = fc_t[i];
    const bool unit = j < H;
    float bi[3] = {0.0f, 0.0f, 0.0f}, bh[3] = {0.0f, 0.0f, 0.0f};
    if (unit && p == 0)
        for (int g = 0; g < 3; ++g) { bi[g] = bih[g * H + j]; bh[g] = bhh[g * H + j]; }
    const float fb = (p == 0 && j < C) ? fc_b[j] : 0.0f;
    float h = (state && unit && p == 0) ? state[(size_t)b * H + j] : 0.0f;       // streams: the hidden state the previous push left ([clip][2C]; null: a whole clip)
    if (tid < 64) hs[tid] = (state && tid < H) ? state[(size_t)b * H + tid] : 0.0f;
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        if ((t & 63) == 0) {
            __syncthreads();
            const int n = min(64, T - t) * C;
            for (int i = tid; i < n; i += 256) s_z[i] = zt[((size_t)b * T + t) * C + i];
            __syncthreads();
        }
        const float* z = s_z + (t & 63) * C;
        float gi[3] = {0.0f, 0.0f, 0.0f}, gh[3] = {0.0f, 0.0f, 0.0f};
        if (unit) {
#pragma unroll
            for (int kk = 0; kk < KI; ++kk) {
                const int k = p * KI + kk;
                if (k < C) {
                    const float zk = z[k];
#pragma unroll
                    for (int g = 0; g < 3; ++g) gi[g] += s_wih[(k * 3 + g) * H + j] * zk;
                }
            }
#pragma unroll
            for (int kk = 0; kk < KH; ++kk) {
                const int k = p * KH + kk;
                if (k < H) {
                    const float hk = hs[k];
#pragma unroll
                    for (int g = 0; g < 3; ++g) gh[g] += s_whh[(k * 3 + g) * H + j] * hk;
                }
            }
#pragma unroll
            for (int g = 0; g < 3; ++g) { part[p][g][j] = gi[g]; part[p][3 + g][j] = gh[g]; }
        }
        __syncthreads();
        if (p == 0 && unit) {
            float si[3], sh[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                si[g] = bi[g] + ((part[0][g][j] + part[1][g][j]) + (part[2][g][j] + part[3][g][j]));
                sh[g] = bh[g] + ((part[0][3 + g][j] + part[1][3 + g][j]) + (part[2][3 + g][j] + part[3][3 + g][j]));
            }
            const float r = usig(si[0] + sh[0]), zg = usig(si[1] + sh[1]), n = ade::dev::tanh_f(si[2] + r * sh[2]);
            h = (1.0f - zg) * n + zg * h;
            hs[j] = h;
        }
        __syncthreads();
        if (p == 0 && j < C) {
            float a = fb;
#pragma unroll
            for (int k = 0; k < H; ++k) a += s_fc[k * C + j] * hs[k];
            at[((size_t)b * T + t) * C + j] = usig(a);
        }
    }
    if (state && p == 0 && unit) state[(size_t)b * H + j] = h;
}

// The same time attention with the recurrence on ONE wavefront and nothing but the recurrence inside it (round 5).  k_ulu_ta spreads every step's contraction over four
// wavefronts and pays three workgroup barriers per step: 2.5 us per step, 105 - 160 us per launch, a quarter of the model's time.  Here a workgroup (one clip, 64 frames at
// a time) runs three phases: (1) all four wavefronts form the input projections b_ih + W_ih z_t of the whole chunk (no dependence between frames) into LDS; (2) wavefront 0
// alone walks the chunk: lane j = hidden unit j, h_{t-1} broadcast lane by lane into scalar registers (v_readlane), the unit's 3 x H recurrent weights held in REGISTERS (a
// 256-thread workgroup that fills a CU's LDS is one wavefront per SIMD: 512 registers each; reading them from LDS -- 144 to 192 ds_read_b32 per step -- made the step as slow
// as the four-wavefront form, 1.6 us), r | z gates as one packed accumulator, h_t into LDS -- no barrier, no other wavefront involved; (3) all four wavefronts apply the output Linear + sigmoid to the chunk's hidden
// states.  Sums run k ascending (k_ulu_ta adds four partial sums: the results differ by fp32 round-off, 1e-7).
template <int C>
__global__ __launch_bounds__(256) void k_ulu_ta2(const float* __restrict__ zt, const float* __restrict__ wih_t, const float* __restrict__ whh_t,
                                                 const float* __restrict__ bih, const float* __restrict__ bhh, const float* __restrict__ fc_t,
                                                 const float* __restrict__ fc_b, float* __restrict__ at, int T, float* __restrict__ state) {
    HIP_DYNAMIC_SHARED(float, lds)
    constexpr int H = 2 * C, G = 3 * H;
    const int b = blockIdx.x, tid = threadIdx.x, j = tid & 63;
    constexpr bool kNLds = C >= 32;           // 3 x 64 weights + the loop's working set pass the 256 architected registers: the n-gate row stays in LDS there (measured: 185 us with
                                              // all three rows in registers, 141 us with all three in LDS)
    float* s_gi = lds;                        // [64 frames][3][H]
    float* s_h = s_gi + 64 * G;               // [64 frames][H]
    float* s_z = s_h + 64 * H;                // [64 frames][C]
    float* s_wn = s_z + 64 * C;               // [H][H]: W_hn^T (kNLds only)
    const int u = j < H ? j : H - 1;          // (lanes beyond H compute unit H - 1 again and store nothing)
    v2f wrz[H];                               // this unit's recurrent rows: (W_hr, W_hz)[u][k] and W_hn[u][k]
    float wn[kNLds ? 1 : H];
    if (kNLds)
        for (int i = tid; i < H * H; i += 256) s_wn[i] = whh_t[((i / H) * 3 + 2) * H + (i % H)];
    float bh[3] = {0.0f, 0.0f, 0.0f};
    if (tid < 64) {
#pragma unroll
        for (int k = 0; k < H; ++k) { wrz[k] = mk2(whh_t[(k * 3 + 0) * H + u], whh_t[(k * 3 + 1) * H + u]); if (!kNLds) wn[k] = whh_t[(k * 3 + 2) * H + u]; }
#pragma unroll
        for (int g = 0; g < 3; ++g) bh[g] = bhh[g * H + u];
    } else {
#pragma unroll
        for (int k = 0; k < H; ++k) { wrz[k] = mk2(0.0f, 0.0f); if (!kNLds) wn[k] = 0.0f; }
    }
    // streams: h continues from the state the previous push left ([clip][2C]; null: a whole clip).  The chunks below only decide WHEN a frame's projections are formed, every
    // frame's sums are its own and the recurrence is one chain: where a push ends relative to a chunk changes no bit.
    float h = (state && tid < 64) ? state[(size_t)b * H + u] : 0.0f;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int nt = min(64, T - t0);
        __syncthreads();                      // (the previous chunk's phase 3 is done with s_h; first pass: the weights are staged)
        for (int i = tid; i < nt * C; i += 256) s_z[i] = zt[((size_t)b * T + t0) * C + i];
        __syncthreads();
        // (1) input projections of the chunk: output (t, g, u) = b_ih[g][u] + sum_k W_ih^T[k][g][u] z_t[k]; consecutive threads = consecutive u (coalesced weight rows)
        for (int o = tid; o < nt * G; o += 256) {
            const int t = o / G, gu = o - t * G;
            float a = bih[gu];
#pragma unroll 4
            for (int k = 0; k < C; ++k) a = fmaf(wih_t[k * G + gu], s_z[t * C + k], a);
            s_gi[o] = a;
        }
        __syncthreads();
        // (2) the recurrence: wavefront 0, lane j = hidden unit
        if (tid < 64) {
            for (int t = 0; t < nt; ++t) {
                v2f grz = mk2(bh[0], bh[1]);
                float gn = bh[2];
#pragma unroll
                for (int k = 0; k < H; ++k) {
                    const float hk = __shfl(h, k, 64);               // constant lane: v_readlane into a scalar register
                    grz += wrz[k] * hk;
                    gn = fmaf(kNLds ? s_wn[k * H + u] : wn[k], hk, gn);
                }
                const float* gi = s_gi + t * G;
                const float r = usig(gi[u] + grz[0]), zg = usig(gi[H + u] + grz[1]), n = ade::dev::tanh_f(gi[2 * H + u] + r * gn);
                h = (1.0f - zg) * n + zg * h;
                if (j < H) s_h[t * H + j] = h;
            }
        }
        __syncthreads();
        // (3) at[t][c] = sigmoid(fc_b[c] + sum_k fc^T[k][c] h_t[k])
        for (int o = tid; o < nt * C; o += 256) {
            const int t = o / C, c = o - t * C;
            float a = fc_b[c];
#pragma unroll 4
            for (int k = 0; k < H; ++k) a = fmaf(fc_t[k * C + c], s_h[t * H + k], a);
            at[((size_t)b * T + t0) * C + o] = usig(a);
        }
    }
    if (state && tid < H) state[(size_t)b * H + tid] = h;       // (H <= 64: wavefront 0, lane = unit)
}

// frequency attention GRUs (:151-153): per frame, the zero-padded bin powers in groups of 4 are a sequence of H steps through a
// bidirectional GRU(4 -> 4).  One thread per (frame, direction); weights [12][4] | [12][4] | [12] | [12] per direction.
__global__ __launch_bounds__(256) void k_ulu_fa_gru(const float* __restrict__ pfreq, const float* __restrict__ wf, const float* __restrict__ wb,
                                                    float* __restrict__ fah, int F, int H, long long frames) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= frames * 2) return;
    const long long frame = i >> 1;
    const int dir = (int)(i & 1);
    const float* w = dir ? wb : wf;
    float wih[12][4], whh[12][4], bi[12], bh[12];
    for (int r = 0; r < 12; ++r) {
        for (int k = 0; k < 4; ++k) { wih[r][k] = w[r * 4 + k]; whh[r][k] = w[48 + r * 4 + k]; }
        bi[r] = w[96 + r];
        bh[r] = w[108 + r];
    }
    float h[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = 0; s < H; ++s) {
        const int step = dir ? H - 1 - s : s;
        float x[4];
        for (int k = 0; k < 4; ++k) { const int f = 4 * step + k; x[k] = f < F ? pfreq[frame * F + f] : 0.0f; }
        float hn[4];
        for (int u = 0; u < 4; ++u) {
            float gi[3], gh[3];
            for (int g = 0; g < 3; ++g) {
                gi[g] = bi[g * 4 + u];
                gh[g] = bh[g * 4 + u];
                for (int k = 0; k < 4; ++k) { gi[g] += wih[g * 4 + u][k] * x[k]; gh[g] += whh[g * 4 + u][k] * h[k]; }
            }
            const float r = usig(gi[0] + gh[0]), z = usig(gi[1] + gh[1]), n = ade::dev::tanh_f(gi[2] + r * gh[2]);
            hn[u] = (1.0f - z) * n + z * h[u];
        }
        for (int u = 0; u < 4; ++u) { h[u] = hn[u]; fah[((size_t)frame * H + step) * 8 + dir * 4 + u] = hn[u]; }
    }
}

// cTFA output (:154, :188-194) with the block's tail: out[.., co] = at[c] * x[c] * sigmoid(fc(fa)[f]) (+ residual[c]) with c = shuffle(co)
__global__ __launch_bounds__(256) void k_ulu_apply(const float* __restrict__ x, const float* __restrict__ at, const float* __restrict__ fah,
                                                   const float* __restrict__ fa_fc_w, const float* __restrict__ fa_fc_b, const float* __restrict__ res,
                                                   float* __restrict__ out, int F, int C, int H, int shuffle, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int co = (int)(i % C);
    const long long r = i / C;
    const int f = (int)(r % F);
    const long long frame = r / F;
    const int c = shuffle ? shuffled(co, C) : co, u = f & 3;
    const float* hrow = fah + ((size_t)frame * H + (f >> 2)) * 8;
    float a = fa_fc_b[u];
    for (int k = 0; k < 8; ++k) a += fa_fc_w[u * 8 + k] * hrow[k];
    const size_t src = ((size_t)frame * F + f) * C + c;
    float v = (at[(size_t)frame * C + c] * x[src]) * usig(a);
    if (res) v += res[src];
    out[i] = v;
}

__global__ __launch_bounds__(256) void k_ulu_pcm2f(const int16_t* __restrict__ pcm, float* __restrict__ x, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) x[i] = (float)pcm[i] * (1.0f / 32768.0f);
}
// the resampled entry (:851-867): fp32 samples in PCM units (audio.float() interpolated by the engine); the * INV_INT16 before or after the interpolation is the
// same number either way (a power of two commutes with every rounding of the interpolation)
__global__ __launch_bounds__(256) void k_ulu_f2f(const float* __restrict__ in, float* __restrict__ x, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) x[i] = in[i] * (1.0f / 32768.0f);
}
// log-power + ERB merge (:725-727, :97-100): feat[frame][j], j < 129; spec is [b][re 257 | im 257][T].  band_lo / band_hi: the non-zero
// run of every ERB filter row (the filters are triangles: contiguous support).
__global__ __launch_bounds__(256) void k_ulu_feat(const float* __restrict__ spec, const float* __restrict__ erb, const int* __restrict__ band_lo,
                                                  const int* __restrict__ band_hi, float* __restrict__ feat, int T, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i % kUErb);
    const long long frame = i / kUErb;
    const long long b = frame / T;
    const int t = (int)(frame - b * T);
    const float* s = spec + (size_t)b * 2 * kUBins * T + t;
    auto logp = [&](int f) { const float re = s[(size_t)f * T], im = s[(size_t)(kUBins + f) * T]; return logf(fmaxf(re * re + im * im, 1e-24f)); };
    float v;
    if (j < kULow) v = logp(j);
    else {
        v = 0.0f;
        const float* row = erb + (size_t)(j - kULow) * kUHigh;
        for (int k = band_lo[j - kULow]; k < band_hi[j - kULow]; ++k) v += row[k] * logp(kULow + k);     // ascending k: the dense matmul's order, zeros dropped
    }
    feat[i] = v;
}
// sigmoid + ERB split (:649, :102-105) + real mask on both spectrum halves (:880), in place on spec.  bin_lo / bin_hi: the bands whose
// filter covers high bin k (contiguous, at most a few).
__global__ __launch_bounds__(256) void k_ulu_mask(const float* __restrict__ m129, const float* __restrict__ erb, const int* __restrict__ bin_lo,
                                                  const int* __restrict__ bin_hi, float* __restrict__ spec, float* __restrict__ mask_tap, int T, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int f = (int)(i % kUBins);
    const long long frame = i / kUBins;
    const long long b = frame / T;
    const int t = (int)(frame - b * T);
    const float* m = m129 + (size_t)frame * kUErb;
    float v;
    if (f < kULow) v = usig(m[f]);
    else {
        v = 0.0f;
        for (int e = bin_lo[f - kULow]; e < bin_hi[f - kULow]; ++e) v += usig(m[kULow + e]) * erb[(size_t)e * kUHigh + (f - kULow)];
    }
    float* s = spec + (size_t)b * 2 * kUBins * T + t;
    s[(size_t)f * T] *= v;
    s[(size_t)(kUBins + f) * T] *= v;
    if (mask_tap) mask_tap[i] = v;
}
// rows of `stride` synthesised samples -> the first `keep` of each (the static trim: keep == stride; a dynamic export slices audio[..., :audio_len], :888-889)
__global__ __launch_bounds__(256) void k_ulu_f2pcm(const float* __restrict__ y, int16_t* __restrict__ pcm, float* __restrict__ f32, int stride, int keep, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long r = i / keep;
    const float v = y[r * stride + (i - r * keep)];
    if (f32) f32[i] = v;
    if (pcm) pcm[i] = (int16_t)(int)fminf(fmaxf(v * 32767.0f, -32768.0f), 32767.0f);
}

// ---- streams (ade_stream_* on a ul_unas handle, include/ade.h) ---------------------------------------------------------------------------------
// The model is causal from end to end, so a push of F hops continues the signal one hop behind the input: frame g is centred on sample 256 g and complete when
// 256 (g + 1) samples have arrived.  A push completes F frames (a fresh stream's first push: frames 0 .. F - 1, the head reflected), the flush frame K of a signal of
// 256 K samples (the tail reflected).  Per push, all on the caller's ONE stream:
//   k_ulu_stream_analysis   [257 carried | 256 F new] -> spectrum in the (stream, 2 x 257, F) layout k_ulu_feat / k_ulu_mask read; renews the carried samples
//   the network             run_net() with T = F: k_ulu_conv<.., PushFrames> for the kt > 1 convolutions, the time attention from its state, k_ulu_stream_inter_gru
//   k_ulu_stream_synthesis  the Hermitian inverse of ONE frame as a 256-point complex transform, windowed
//   k_ulu_stream_out        overlap-add with the carried half frame / the steady window-square sum, the PCM tail of k_ulu_f2pcm, the next carried half
// ONE frame per transform (a 512-point real transform = a 256-point complex one plus a split pass, ade_fft.h): the one-shot path's generic STFT rides two frames on one
// complex transform, paired by the frame's parity inside the call, so its bits would move with the push size.
constexpr int kUHalf = kUNfft / 2, kUCarry = kUHop + 1;      // 256 complex points; 257 carried samples: the tail reflection of the flush reaches sample L - 257

// mode 0: a push that continues a signal; 1: a fresh stream's first push (the head reflection instead of the carried samples); 2: the flush (F = 1, the carried samples
// and their reflection, `in` unused).  Workgroups from N on (modes 0, 1) copy the push's last 257 samples into carry_out (the other buffer of the ping-pong pair).
__global__ __launch_bounds__(256) void k_ulu_stream_analysis(const int16_t* __restrict__ in, const int16_t* __restrict__ carry_in, int16_t* __restrict__ carry_out, int P, int F, int N,
                                                             int mode, fft::Plan p256, const float2* __restrict__ tw256, const float2* __restrict__ tw512,
                                                             const float* __restrict__ win, float* __restrict__ spec) {
    __shared__ float2 A[kUHalf];
    __shared__ float2 B[kUHalf];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= N) {
        const int s = (int)blockIdx.x - N;
        for (int n = tid; n < kUCarry; n += 256) carry_out[(size_t)s * kUCarry + n] = in[(size_t)s * P + (P - kUCarry) + n];
        return;
    }
    const int fr = (int)blockIdx.x, s = fr / F, i = fr - s * F;
    const int16_t *old = carry_in + (size_t)s * kUCarry, *row = in + (size_t)s * P;
    // sample n of the frame, signal position p0 + 256 i - 256 + n with p0 the push's first sample: the carried samples are positions p0 - 257 .. p0 - 1
    auto sample = [&](int n) {
        int16_t v;
        if (mode == 2) v = old[n < kUHop ? n + 1 : 2 * kUHop - 1 - n];           // second half: position L + q reflects to L - 2 - q = carried sample 255 - q
        else if (mode == 1) { const int idx = kUHop * i - kUHop + n; v = row[idx < 0 ? -idx : idx]; }
        else { const int r = kUHop * i + 1 + n; v = r < kUCarry ? old[r] : row[r - kUCarry]; }
        return ((float)v * (1.0f / 32768.0f)) * win[n];
    };
    A[tid] = make_float2(sample(2 * tid), sample(2 * tid + 1));
    const float2* r = fft::forward(A, B, p256, tw256, tid, 256);
    float* sp = spec + (size_t)s * 2 * kUBins * F + i;
    for (int f = tid; f < kUBins; f += 256) {
        const float2 x = fft::split_bin(r, f, kUHalf, tw512);
        sp[(size_t)f * F] = x.x;
        sp[(size_t)(kUBins + f) * F] = x.y;
    }
}

// The inter-frame GRU of a push: k_inter_gru's recurrence (ade_kernels.hip: per (stream, bin) column two groups of GRU(8 -> 8) along the frames, 16 lanes per column, lane =
// group * 8 + unit, `gru` in its lane format [3 x 8 ih | 3 x 8 hh | 3 b_ih | 3 b_hh]) from the stream's state [stream][33][16], which it updates in place.  Not
// k_inter_gru itself: that kernel walks four frames per trip and the compiler contracts h' = (1 - z) n + z h into one fused multiply-add in the first of the four and into
// two products and a sum in the other three (gfx950 code of the build at hand), so a frame's last bit there depends on its index inside the launch modulo 4 -- nothing a
// whole clip notices, but a stream's frames change that index with the push size.  Here: one frame per trip, and every rounding of a step spelled out.
__global__ __launch_bounds__(256) void k_ulu_stream_inter_gru(const float* __restrict__ x, const float* __restrict__ gru, float* __restrict__ rnn, int B, int T,
                                                              float* __restrict__ state) {
    const int site = blockIdx.x * 16 + (threadIdx.x >> 4), q = threadIdx.x & 15, grp = q >> 3;
    const bool live = site < B * kFw;
    const int sc = live ? site : B * kFw - 1;            // (lanes past the last column repeat it and store nothing)
    const int b = sc / kFw, f = sc - b * kFw;
    const float* pk = gru + q * 54;
    float wi[3][8], wh[3][8], bi[3], bh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { wi[g][k] = pk[g * 8 + k]; wh[g][k] = pk[24 + g * 8 + k]; }
        bi[g] = pk[48 + g];
        bh[g] = pk[51 + g];
    }
    float h = state[(size_t)sc * kCh + q];
    const float* xb = x + ((size_t)b * T * kFw + f) * kCh + grp * 8;      // frame t at xb + t * kFw * kCh
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        const float4 x0 = *reinterpret_cast<const float4*>(xb + (size_t)t * kFw * kCh), x1 = *reinterpret_cast<const float4*>(xb + (size_t)t * kFw * kCh + 4);
        const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
        float gi[3] = {bi[0], bi[1], bi[2]}, gh[3] = {bh[0], bh[1], bh[2]};
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int g = 0; g < 3; ++g) gi[g] = fmaf(wi[g][k], xv[k], gi[g]);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float hk = __shfl(h, k, 8);
#pragma unroll
            for (int g = 0; g < 3; ++g) gh[g] = fmaf(wh[g][k], hk, gh[g]);
        }
        const float r = usig(__fadd_rn(gi[0], gh[0])), z = usig(__fadd_rn(gi[1], gh[1])), n = ade::dev::tanh_f(fmaf(r, gh[2], gi[2]));
        h = fmaf(z, h, __fmul_rn(1.0f - z, n));
        if (live) rnn[(((size_t)b * T + t) * kFw + f) * kCh + q] = h;
    }
    if (live) state[(size_t)sc * kCh + q] = h;
}

// One workgroup per frame: the masked half spectrum (imaginary parts of the DC and Nyquist bins dropped, as the generic synthesis does) -> 512 windowed samples.
__global__ __launch_bounds__(256) void k_ulu_stream_synthesis(const float* __restrict__ spec, int F, fft::Plan p256, const float2* __restrict__ tw256,
                                                              const float2* __restrict__ tw512, const float* __restrict__ win, float* __restrict__ frames) {
    __shared__ float2 A[kUHalf];
    __shared__ float2 B[kUHalf];
    const int tid = threadIdx.x, fr = (int)blockIdx.x, s = fr / F, i = fr - s * F;
    const float* sp = spec + (size_t)s * 2 * kUBins * F + i;
    auto bin = [&](int f) { return make_float2(sp[(size_t)f * F], f == 0 || f == kUHalf ? 0.0f : sp[(size_t)(kUBins + f) * F]); };
    A[tid] = fft::merge_bin_conj(bin(tid), bin(kUHalf - tid), tw512[tid]);
    const float2* r = fft::forward(A, B, p256, tw256, tid, 256);
    float2* out = reinterpret_cast<float2*>(frames + (size_t)fr * kUNfft);
    constexpr float inv = 1.0f / (float)kUNfft;
    out[tid] = make_float2(__fmul_rn(r[tid].x * inv, win[2 * tid]), __fmul_rn(-r[tid].y * inv, win[2 * tid + 1]));
}

// Output hop i of a push = the second half of the frame before local frame i (the carried half for i = 0) + the first half of frame i, in that order, over den[256] =
// the two window squares summed in the same order; a fresh stream's hop 0 is the delay: zero.  Then the PCM tail of k_ulu_f2pcm.  The threads from `total` on copy the
// second half of the push's last frame into half_out (null: the flush).
__global__ __launch_bounds__(256) void k_ulu_stream_out(const float* __restrict__ frames, const float* __restrict__ half_in, float* __restrict__ half_out,
                                                        const float* __restrict__ den, int F, int fresh, int16_t* __restrict__ pcm, float* __restrict__ f32, long long total,
                                                        long long total_all) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total_all) return;
    if (g >= total) {
        const long long e = g - total;
        const long long st = e / kUHop;
        half_out[e] = frames[((size_t)st * F + (F - 1)) * kUNfft + kUHop + (int)(e - st * kUHop)];
        return;
    }
    const long long fr = g / kUHop;                 // = stream * F + i: the output row of a stream is its F hops
    const int n = (int)(g - fr * kUHop), i = (int)(fr % F);
    float y = 0.0f;
    if (!(fresh && i == 0)) {
        const float prev = i > 0 ? frames[(size_t)(fr - 1) * kUNfft + kUHop + n] : half_in[(size_t)(fr / F) * kUHop + n];
        y = (prev + frames[(size_t)fr * kUNfft + n]) / den[n];
    }
    if (f32) f32[g] = y;
    if (pcm) pcm[g] = (int16_t)(int)fminf(fmaxf(y * 32767.0f, -32768.0f), 32767.0f);
}

int ufail(std::string& err, int st, const std::string& msg) { err = msg; return st; }
#define UL_HIP(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) return ufail(err, ADE_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

struct CtfaW { const float *ta_wih_t, *ta_whh_t, *ta_bih, *ta_bhh, *ta_fc_t, *ta_fc_b, *fa_f, *fa_b, *fa_fc_w, *fa_fc_b; };
struct Block {
    int type, cin, cout, width, in_width, kt, kf, stride, groups, deconv, last;
    ConvDesc conv[3];          // type 0: conv ; type 1: pconv, dconv ; type 2: pconv1, dconv, pconv2
    CtfaW ctfa;
};
struct DpPacked { const float *intra_gru, *inter_gru, *fc[2], *fc_b[2], *ln_w[2], *ln_b[2]; };

// PyTorch GRU rows of hidden unit j -> [3x8 ih | 3xH hh | 3 b_ih | 3 b_hh]: the lane format of k_intra_gru / k_inter_gru (ade_kernels.hip)
void pack_gru_lane(float* dst, const float* wih, const float* whh, const float* bih, const float* bhh, int H, int j) {
    for (int g = 0; g < 3; ++g)
        for (int k = 0; k < 8; ++k) dst[g * 8 + k] = wih[(g * H + j) * 8 + k];
    for (int g = 0; g < 3; ++g)
        for (int k = 0; k < H; ++k) dst[24 + g * H + k] = whh[(g * H + j) * H + k];
    for (int g = 0; g < 3; ++g) { dst[24 + 3 * H + g] = bih[g * H + j]; dst[24 + 3 * H + 3 + g] = bhh[g * H + j]; }
}

}  // namespace

// The buffers of one pass through the network and its frame count per row: the engine's own (one call, reserve()) or, for the length of a push, a stream's.
struct UlunasWork {
    int T = 0;
    float *xf = nullptr, *spec = nullptr, *yf = nullptr, *bufA = nullptr, *bufB = nullptr, *bufC = nullptr, *bufD = nullptr, *dpa = nullptr, *dpb = nullptr, *skip[5] = {}, *zt = nullptr, *pfreq = nullptr, *at = nullptr,
          *fah = nullptr, *rnn = nullptr, *dpm = nullptr, *mask_tap = nullptr;
};
struct UlunasStream;

struct UlunasEngine : SubEngine, UlunasWork {
    int device = 0, L = 0 /* one window */, n_win = 1, out_len_ = 0;
    int syn_len = 0;                   // samples per row the ISTFT writes: out_len_ for a static export, 256 T (the kept tail) for a dynamic one
    bool ta2 = !(getenv("ADE_ULU_TA2") && atoi(getenv("ADE_ULU_TA2")) == 0);     // the single-wavefront time-attention kernel (k_ulu_ta2; ADE_ULU_TA2=0: the four-wavefront form)
    ade_stft_handle plan = nullptr;
    float* d_w = nullptr;
    const float* erb = nullptr;
    int* d_tab = nullptr;              // band_lo[64] | band_hi[64] | bin_lo[192] | bin_hi[192]
    Block blocks[10];
    DpPacked dp[2];
    int capacity = 0;
    float* ws = nullptr;
    // streams: the one-frame transforms' tables (the window make_window() gives the generic operator; den[256] = its squares summed over the two frames of a sample) and,
    // while a push is being enqueued, the stream whose state the network continues (null: a whole clip per row)
    const float *swin = nullptr, *sden = nullptr, *stw512 = nullptr, *stw256 = nullptr;
    fft::Plan p256;
    const UlunasStream* live = nullptr;

    // Row groups on side streams (round 5): the network between the two STFTs runs per group of rows, group k > 0 on its own stream between a fork and a join event, so that
    // one group's latency-bound launches (the time-attention recurrences: one workgroup per clip, 63 dependent steps, 20 % of the call with the chip nearly idle) run under
    // another group's bandwidth-bound ones.  Same kernels on the same rows: the same bits.  ADE_ULU_GROUPS = 1 .. 4 (1: one stream).
    int groups_ = getenv("ADE_ULU_GROUPS") ? std::min(4, std::max(1, atoi(getenv("ADE_ULU_GROUPS")))) : 2;
    hipStream_t side[3] = {};
    hipEvent_t ev_fork = nullptr, ev_join[3] = {};
    void shift_rows(long long rows);
    void run_net(hipStream_t s, int B);

    ~UlunasEngine() override {
        (void)hipSetDevice(device);
        for (int k = 0; k < 3; ++k) { if (side[k]) (void)hipStreamDestroy(side[k]); if (ev_join[k]) (void)hipEventDestroy(ev_join[k]); }
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (plan) ade_stft_destroy(plan);
        if (d_w) (void)hipFree(d_w);
        if (d_tab) (void)hipFree(d_tab);
        if (ws) (void)hipFree(ws);
    }
    int frames() const override { return T; }
    // batch-fold (:866-871, :886-887): a call is n_win whole windows back to back; each is an independent clip and the outputs are
    // stitched in place, so folding is only a reinterpretation of the rows (W is a multiple of the hop: every window returns W samples)
    int in_len() const override { return L * n_win; }
    int out_len() const override { return out_len_ * n_win; }
    bool accepts_float_input() const override { return true; }
    int reserve(int batch, std::string& err) override;
    int run(hipStream_t s, const int16_t* d_in, int batch, int16_t* d_out, float* d_f32, std::string& err) override;
    int tap(hipStream_t s, const char* name, int batch, float* out, size_t count, size_t* written, std::string& err) override;
    void ctfa(hipStream_t s, const Block& bk, const float* x, const float* res, float* out, int B, int shuffle);
    float* run_block(hipStream_t s, const Block& bk, const float* x, const float* x2, float* t0, float* t1, float* dst, int B);
    // streams (ade_stream_*): state per stream object, see UlunasStream below
    int stream_delay() const override { return kUHop; }
    int stream_hop() const override { return kUHop; }
    int stream_windows() const override { return n_win; }
    int stream_channels() const override { return 1; }
    int stream_create(int n_streams, int frames_per_push, void** state, std::string& err) override;
    int stream_reset(void* state, hipStream_t s, std::string& err) override;
    int stream_push(void* state, hipStream_t s, const int16_t* d_in, int16_t* d_out, float* d_f32, std::string& err) override;
    int stream_flush(void* state, hipStream_t s, int16_t* d_out, float* d_f32, std::string& err) override;
    void stream_destroy(void* state) override;
    int stream_step(UlunasStream* st, hipStream_t s, const int16_t* d_in, int16_t* d_out, float* d_f32, std::string& err);
};

// What a stream carries between pushes, for S streams that advance together: one allocation, its leading part cleared by a reset.
struct UlunasStream {
    int S = 0, F = 0;                           // streams, hops per push
    long long hops = 0;                         // hops pushed since the last reset
    int cur = 0;                                // which buffer of every ping-pong pair holds the state
    bool flushing = false;
    int16_t* carry[2] = {};                     // [S][257] the last 257 input samples
    float* hist[2] = {};                        // per convolution with kt > 1, at hist_off[block]: [S][kt - 1][Fi * Cin] its last input frames (x + skip already summed)
    float* half[2] = {};                        // [S][256] the second half of the last synthesised frame
    float* ta = nullptr;                        // per block, at ta_off[block]: [S][2 C] the time-attention GRU's hidden state (updated in place: one workgroup per stream)
    float* inter[2] = {};                       // [S][33][16] the two inter-frame GRU states (in place)
    size_t hist_off[10] = {}, ta_off[10] = {};
    UlunasWork work;                            // one push's workspace, S * F frames
    float* frames = nullptr;                    // [S * F][512] windowed synthesis frames
    void* block = nullptr;
    size_t reset_bytes = 0;
};

int ulunas_create(const std::map<std::string, Tensor>& tensors, int in_len, int n_win, int dynamic_keep, int device, SubEngine** out, std::string& err) {
    *out = nullptr;
    if (dynamic_keep > 0 && n_win != 1) return ufail(err, ADE_ERR_BAD_VALUE, "ul_unas: batch folding requires a static shape (Export_UL_UNAS.py:39)");
    if (in_len < kUNfft) return ufail(err, ADE_ERR_SHAPE_MISMATCH, "ul_unas: input_audio_length shorter than one 512-sample frame");
    if (n_win < 1 || (n_win > 1 && in_len % kUHop)) return ufail(err, ADE_ERR_BAD_VALUE, "ul_unas: fold windows must be whole hops");
    // ULUNAS() defaults (:655-668)
    static const int types[5] = {0, 2, 1, 2, 1}, strides[5] = {2, 2, 1, 1, 1}, groups[5] = {1, 2, 2, 2, 2}, channels[5] = {12, 24, 24, 32, 16},
                     kts[5] = {3, 2, 2, 1, 1}, kfs[5] = {3, 3, 3, 5, 5}, widths[5] = {65, 33, 33, 33, 33};
    std::vector<float> arena;
    auto put = [&](const float* src, size_t n) { const size_t at = arena.size(); arena.resize(at + ((n + 63) & ~(size_t)63), 0.0f); if (src) memcpy(&arena[at], src, n * sizeof(float)); return at; };
    bool ok = true;
    auto get = [&](const std::string& name, std::vector<int> dims) -> const float* {
        auto it = tensors.find(name);
        if (it == tensors.end()) { if (ok) err = "weights: tensor missing: " + name; ok = false; return nullptr; }
        if (it->second.dims != dims) { if (ok) err = "weights: tensor has the wrong shape: " + name; ok = false; return nullptr; }
        return it->second.data;
    };
    struct Fix { const float** dst; size_t at; };
    std::vector<Fix> fix;
    auto want = [&](const float** dst, const std::string& name, std::vector<int> dims) {
        const float* p = get(name, dims);
        size_t n = 1;
        for (int d : dims) n *= (size_t)d;
        fix.push_back({dst, put(p, p ? n : 0)});
    };
    UlunasEngine* e = new UlunasEngine();
    auto bail = [&](int st) { delete e; return st; };
    e->device = device; e->L = in_len; e->n_win = n_win; e->T = in_len / kUHop + 1;
    // static: the trim [256 : raw - 256] = 256 (T - 1) samples; dynamic (:43, :888-889): the ISTFT keeps everything after the first half window (256 T samples) and the
    // wrapper slices audio[..., :audio_len] with audio_len = the CALLER-rate input length
    e->syn_len = dynamic_keep > 0 ? kUHop * e->T : kUHop * (e->T - 1);
    e->out_len_ = dynamic_keep > 0 ? std::min(e->syn_len, dynamic_keep) : e->syn_len;
    auto conv = [&](ConvDesc& d, const std::string& wname, const std::string& aname, int cin, int cout, int fi, int fo, int kt, int kf, int stride, int g, int deconv,
                    bool act, int shuffle) {
        d = ConvDesc{nullptr, nullptr, nullptr, nullptr, nullptr, cin, cout, fi, fo, kt, kf, stride, g, deconv, shuffle};
        if (deconv) want(&d.w, wname + "_w", {cin, cout / g, kt, kf});
        else want(&d.w, wname + "_w", {cout, cin / g, kt, kf});
        want(&d.b, wname + "_b", {cout});
        if (act) {
            want(&d.pos, aname + "pos", {cout, fo});
            want(&d.neg, aname + "neg", {cout, fo});
            want(&d.abias, aname + "bias", {cout, fo});
        }
    };
    // transposed copies for the time-attention GRU (lanes read consecutive floats)
    std::vector<std::vector<float>> keep;
    auto ctfa = [&](CtfaW& c, const std::string& p, int C) {
        const int H = 2 * C;
        const float* wih = get(p + "ta_weight_ih_l0", {3 * H, C});
        const float* whh = get(p + "ta_weight_hh_l0", {3 * H, H});
        const float* fcw = get(p + "ta_fc_w", {C, H});
        if (!ok) return;
        std::vector<float> a((size_t)C * 3 * H), b((size_t)H * 3 * H), f((size_t)H * C);
        for (int g = 0; g < 3; ++g)
            for (int j = 0; j < H; ++j) {
                for (int k = 0; k < C; ++k) a[((size_t)k * 3 + g) * H + j] = wih[((size_t)g * H + j) * C + k];
                for (int k = 0; k < H; ++k) b[((size_t)k * 3 + g) * H + j] = whh[((size_t)g * H + j) * H + k];
            }
        for (int cc = 0; cc < C; ++cc)
            for (int k = 0; k < H; ++k) f[(size_t)k * C + cc] = fcw[(size_t)cc * H + k];
        fix.push_back({&c.ta_wih_t, put(a.data(), a.size())});
        fix.push_back({&c.ta_whh_t, put(b.data(), b.size())});
        fix.push_back({&c.ta_fc_t, put(f.data(), f.size())});
        want(&c.ta_bih, p + "ta_bias_ih_l0", {3 * H});
        want(&c.ta_bhh, p + "ta_bias_hh_l0", {3 * H});
        want(&c.ta_fc_b, p + "ta_fc_b", {C});
        for (int dir = 0; dir < 2; ++dir) {
            const std::string sfx = dir ? "_reverse" : "";
            const float *wi = get(p + "fa_weight_ih_l0" + sfx, {12, 4}), *wh = get(p + "fa_weight_hh_l0" + sfx, {12, 4}), *bi = get(p + "fa_bias_ih_l0" + sfx, {12}),
                        *bh = get(p + "fa_bias_hh_l0" + sfx, {12});
            if (!ok) return;
            std::vector<float> pk(120);
            memcpy(&pk[0], wi, 48 * 4); memcpy(&pk[48], wh, 48 * 4); memcpy(&pk[96], bi, 12 * 4); memcpy(&pk[108], bh, 12 * 4);
            fix.push_back({dir ? &c.fa_b : &c.fa_f, put(pk.data(), pk.size())});
        }
        want(&c.fa_fc_w, p + "fa_fc_w", {4, 8});
        want(&c.fa_fc_b, p + "fa_fc_b", {4});
    };
    auto make_block = [&](Block& bk, const std::string& p, int type, int cin, int cout, int width, int kt, int kf, int stride, int g, int deconv, int last) {
        const int in_width = stride == 2 ? (deconv ? width / 2 + 1 : width * 2 - 1) : width;
        bk = Block{};
        bk.type = type; bk.cin = cin; bk.cout = cout; bk.width = width; bk.in_width = in_width; bk.kt = kt; bk.kf = kf; bk.stride = stride; bk.groups = g; bk.deconv = deconv;
        bk.last = last;
        if (type == 0) conv(bk.conv[0], p + "conv", p + "act_", cin, cout, in_width, width, kt, kf, stride, g, deconv, !last, 0);
        else if (type == 1) {
            conv(bk.conv[0], p + "pconv", p + "pconv_act_", cin, cout, in_width, in_width, 1, 1, 1, g, 0, true, g == 2);
            conv(bk.conv[1], p + "dconv", p + "dconv_act_", cout, cout, in_width, width, kt, kf, stride, cout, deconv, !last, 0);
        } else {
            conv(bk.conv[0], p + "pconv1", p + "pconv1_act_", cin, cout, in_width, in_width, 1, 1, 1, g, 0, true, g == 2);
            conv(bk.conv[1], p + "dconv", p + "dconv_act_", cout, cout, in_width, width, kt, kf, stride, cout, deconv, true, 0);
            conv(bk.conv[2], p + "pconv2", "", cout, cout, width, width, 1, 1, 1, g, 0, false, 0);
        }
        ctfa(bk.ctfa, p + "ctfa_", cout);
    };
    int cin = 1;
    for (int i = 0; i < 5; ++i) {
        make_block(e->blocks[i], "encoder.en_convs." + std::to_string(i) + ".", types[i], cin, channels[i], widths[i], kts[i], kfs[i], strides[i], groups[i], 0, 0);
        cin = channels[i];
    }
    int j = 0;
    for (int i = 4; i >= 1; --i, ++j) {
        make_block(e->blocks[5 + j], "decoder.de_convs." + std::to_string(j) + ".", types[i], cin, channels[i - 1], widths[i - 1], kts[i], kfs[i], strides[i], groups[i], 1, 0);
        cin = channels[i - 1];
    }
    for (int i = 5; i < 9; ++i)
        if (e->blocks[i].type == 2 && e->blocks[i].cin == e->blocks[i].cout && e->blocks[i].stride == 1) ok = false;   // residual on a skip-summed input: not in this architecture
    make_block(e->blocks[9], "decoder.de_convs.4.", types[0], cin, 1, kUErb, kts[0], kfs[0], strides[0], groups[0], 1, 1);
    want(&e->erb, "erb_filters", {kUBands, kUHigh});
    {   // streams: window, window-square sum and twiddles of the one-frame transforms
        std::vector<float> w(kUNfft), den(kUHop), t512(2 * kUNfft), t256(2 * kUHalf);
        const float step = (float)(2.0 * M_PI / (double)kUNfft);                 // torch.hann_window (periodic) in fp32, as make_window() of ade_stft.hip
        for (int n = 0; n < kUNfft; ++n) w[n] = cosf((float)n * step) * (-0.5f) + 0.5f;
        for (int n = 0; n < kUHop; ++n) den[n] = (0.0f + w[kUHop + n] * w[kUHop + n]) + w[n] * w[n];      // frame t - 1's second half first, as the one-shot overlap-add sums
        for (int m = 0; m < kUNfft; ++m) { const double a = 2.0 * M_PI * (double)m / (double)kUNfft; t512[2 * m] = (float)cos(a); t512[2 * m + 1] = (float)-sin(a); }
        for (int m = 0; m < kUHalf; ++m) { const double a = 2.0 * M_PI * (double)m / (double)kUHalf; t256[2 * m] = (float)cos(a); t256[2 * m + 1] = (float)-sin(a); }
        fix.push_back({&e->swin, put(w.data(), w.size())});
        fix.push_back({&e->sden, put(den.data(), den.size())});
        fix.push_back({&e->stw512, put(t512.data(), t512.size())});
        fix.push_back({&e->stw256, put(t256.data(), t256.size())});
        if (!fft::make_plan(kUHalf, &e->p256)) ok = false;
    }
    // DPGRNN x 2 in GTCRN's lane formats
    for (int i = 0; i < 2 && ok; ++i) {
        const std::string p = "dpgrnn." + std::to_string(i) + ".";
        std::vector<float> ig(16 * 42), og(16 * 54);
        for (int grp = 0; grp < 2 && ok; ++grp) {
            const std::string r = p + "intra_rnn.rnn" + std::to_string(grp + 1) + ".";
            for (int dir = 0; dir < 2; ++dir) {
                const std::string sfx = dir ? "_reverse" : "";
                const float *wih = get(r + "weight_ih_l0" + sfx, {12, 8}), *whh = get(r + "weight_hh_l0" + sfx, {12, 4}), *bih = get(r + "bias_ih_l0" + sfx, {12}),
                            *bhh = get(r + "bias_hh_l0" + sfx, {12});
                if (!ok) break;
                for (int u = 0; u < 4; ++u) pack_gru_lane(&ig[(grp * 8 + dir * 4 + u) * 42], wih, whh, bih, bhh, 4, u);
            }
            const std::string q = p + "inter_rnn.rnn" + std::to_string(grp + 1) + ".";
            const float *wih = get(q + "weight_ih_l0", {24, 8}), *whh = get(q + "weight_hh_l0", {24, 8}), *bih = get(q + "bias_ih_l0", {24}), *bhh = get(q + "bias_hh_l0", {24});
            if (!ok) break;
            for (int u = 0; u < 8; ++u) pack_gru_lane(&og[(grp * 8 + u) * 54], wih, whh, bih, bhh, 8, u);
        }
        if (!ok) break;
        fix.push_back({&e->dp[i].intra_gru, put(ig.data(), ig.size())});
        fix.push_back({&e->dp[i].inter_gru, put(og.data(), og.size())});
        const char* part[2] = {"intra", "inter"};
        for (int k = 0; k < 2; ++k) {
            const float* fw = get(p + part[k] + "_fc.weight", {16, 16});
            if (!ok) break;
            std::vector<float> ft(256);
            for (int a = 0; a < 16; ++a)
                for (int co = 0; co < 16; ++co) ft[a * 16 + co] = fw[co * 16 + a];
            fix.push_back({&e->dp[i].fc[k], put(ft.data(), 256)});
            want(&e->dp[i].fc_b[k], p + part[k] + "_fc.bias", {16});
            want(&e->dp[i].ln_w[k], p + part[k] + "_ln.weight", {kFw, 16});
            want(&e->dp[i].ln_b[k], p + part[k] + "_ln.bias", {kFw, 16});
        }
    }
    if (!ok) return bail(err.find("missing") != std::string::npos ? ADE_ERR_MISSING_KEY : ADE_ERR_SHAPE_MISMATCH);
    if (hipSetDevice(device) != hipSuccess) return bail(ufail(err, ADE_ERR_DEVICE, "hipSetDevice failed"));
    if (hipMalloc((void**)&e->d_w, arena.size() * sizeof(float)) != hipSuccess || hipMemcpy(e->d_w, arena.data(), arena.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return bail(ufail(err, ADE_ERR_DEVICE, "upload of the UL-UNAS weights failed"));
    for (auto& f : fix) *f.dst = e->d_w + f.at;
    {   // supports of the ERB triangles, both ways
        const float* ef = tensors.find("erb_filters")->second.data;
        std::vector<int> tab(2 * kUBands + 2 * kUHigh, 0);
        for (int b2 = 0; b2 < kUBands; ++b2) {
            int lo = kUHigh, hi = 0;
            for (int k = 0; k < kUHigh; ++k)
                if (ef[(size_t)b2 * kUHigh + k] != 0.0f) { lo = std::min(lo, k); hi = std::max(hi, k + 1); }
            tab[b2] = lo < hi ? lo : 0;
            tab[kUBands + b2] = lo < hi ? hi : 0;
        }
        for (int k = 0; k < kUHigh; ++k) {
            int lo = kUBands, hi = 0;
            for (int b2 = 0; b2 < kUBands; ++b2)
                if (ef[(size_t)b2 * kUHigh + k] != 0.0f) { lo = std::min(lo, b2); hi = std::max(hi, b2 + 1); }
            tab[2 * kUBands + k] = lo < hi ? lo : 0;
            tab[2 * kUBands + kUHigh + k] = lo < hi ? hi : 0;
        }
        if (hipMalloc((void**)&e->d_tab, tab.size() * sizeof(int)) != hipSuccess || hipMemcpy(e->d_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
            return bail(ufail(err, ADE_ERR_DEVICE, "upload of the ERB tables failed"));
    }
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_ulu_ta<32>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);   // 88 KB at 32 channels
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_ulu_ta<24>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_ulu_ta2<32>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);  // 49 KB of recurrent weights + 48 KB of projections + 24 KB
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_ulu_ta2<24>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_ulu_ta2<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_ulu_ta2<12>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    ade_stft_config cfg{kUNfft, kUNfft, kUHop, "hann", nullptr, 1, "reflect"};          // UL-UNAS/Export_UL_UNAS.py:33-37, 936-957
    if (ade_stft_create(&cfg, device, &e->plan) != ADE_OK) return bail(ufail(err, ADE_ERR_DEVICE, std::string("ul_unas: STFT plan: ") + ade_stft_last_error(nullptr)));
    if (dynamic_keep > 0) (void)ade_stft_keep_tail(e->plan, 1);
    *out = e;
    return ADE_OK;
}

int UlunasEngine::reserve(int calls, std::string& err) {
    if (calls <= capacity) return ADE_OK;
    const int batch = calls * n_win;
    UL_HIP(hipSetDevice(device));
    UL_HIP(hipDeviceSynchronize());
    if (ws) (void)hipFree(ws);
    ws = nullptr;
    capacity = 0;
    const size_t B = batch, nfr = B * T, act = nfr * 1600;             // widest activation: 65 bins x 24 channels per frame
    struct Carve { float** p; size_t n; };
    std::vector<Carve> cs = {{&xf, B * L}, {&spec, B * 2 * kUBins * T}, {&yf, B * syn_len}, {&bufA, act}, {&bufB, act}, {&bufC, act}, {&bufD, act}, {&dpa, nfr * kFw * kCh}, {&dpb, nfr * kFw * kCh}, {&zt, nfr * 32},
                             {&pfreq, nfr * 132}, {&at, nfr * 32}, {&fah, nfr * 33 * 8}, {&rnn, nfr * kFw * kCh}, {&dpm, nfr * kFw * kCh}, {&mask_tap, nfr * kUBins}};
    for (int i = 0; i < 5; ++i) cs.push_back({&skip[i], nfr * (size_t)blocks[i].width * blocks[i].cout});
    size_t total = 0;
    for (auto& c : cs) total += (c.n + 63) & ~(size_t)63;
    UL_HIP(hipMalloc((void**)&ws, total * sizeof(float)));
    size_t at_ = 0;
    for (auto& c : cs) { *c.p = ws + at_; at_ += (c.n + 63) & ~(size_t)63; }
    for (int k = 0; k + 1 < groups_; ++k) {
        if (!side[k]) UL_HIP(hipStreamCreateWithFlags(&side[k], hipStreamNonBlocking));
        if (!ev_join[k]) UL_HIP(hipEventCreateWithFlags(&ev_join[k], hipEventDisableTiming));
    }
    if (!ev_fork) UL_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    // let the STFT plan size its frame buffer now (it allocates lazily), so that run() never allocates
    UL_HIP(hipMemset(spec, 0, B * 2 * kUBins * T * sizeof(float)));
    if (ade_stft_synthesize(plan, spec, batch, T, yf, nullptr) != ADE_OK) return ufail(err, ADE_ERR_DEVICE, std::string("ul_unas: ") + ade_stft_last_error(plan));
    capacity = calls;
    return ADE_OK;
}

void UlunasEngine::ctfa(hipStream_t s, const Block& bk, const float* x, const float* res, float* out, int B, int shuffle) {
    const int F = bk.width, C = bk.cout, H = (F + 3) / 4;
    const long long nfr = (long long)B * T;
    const size_t ta_lds = ta2 ? (size_t)(64 * 3 * 2 * C + 64 * 2 * C + 64 * C + (C >= 32 ? 4 * C * C : 0)) * sizeof(float)
                              : (size_t)(C * 3 * 2 * C + 2 * C * 3 * 2 * C + 2 * C * C + 64 * C) * sizeof(float);
    float* ta_state = live ? live->ta + live->ta_off[&bk - blocks] : nullptr;      // a push: the recurrence continues from the stream's state
#define ADE_ULU_TA(CC)                                                                                                                                  \
    if (ta2) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ulu_ta2<CC>), dim3((unsigned)B), dim3(256), ta_lds, s, (const float*)zt, bk.ctfa.ta_wih_t, bk.ctfa.ta_whh_t, \
                                bk.ctfa.ta_bih, bk.ctfa.ta_bhh, bk.ctfa.ta_fc_t, bk.ctfa.ta_fc_b, at, T, ta_state);                                      \
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ulu_ta<CC>), dim3((unsigned)B), dim3(256), ta_lds, s, (const float*)zt, bk.ctfa.ta_wih_t, bk.ctfa.ta_whh_t, \
                            bk.ctfa.ta_bih, bk.ctfa.ta_bhh, bk.ctfa.ta_fc_t, bk.ctfa.ta_fc_b, at, T, ta_state)
    switch (C) {               // the channel counts of ULUNAS() (:665); create() rejects anything else
        case 1: ADE_ULU_TA(1); break;
        case 12: ADE_ULU_TA(12); break;
        case 16: ADE_ULU_TA(16); break;
        case 24: ADE_ULU_TA(24); break;
        default: ADE_ULU_TA(32); break;
    }
#undef ADE_ULU_TA
    hipLaunchKernelGGL(k_ulu_fa_gru, dim3((unsigned)((nfr * 2 + 255) / 256)), dim3(256), 0, s, (const float*)pfreq, bk.ctfa.fa_f, bk.ctfa.fa_b, fah, F, H, nfr);
    const long long total = nfr * F * C;
    hipLaunchKernelGGL(k_ulu_apply, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, (const float*)at, (const float*)fah, bk.ctfa.fa_fc_w, bk.ctfa.fa_fc_b, res,
                       out, F, C, H, shuffle, total);
}

// one encoder / decoder block (:264-273, :342-357, :433-453); x2 (decoder skip) is added to the input; result in dst
float* UlunasEngine::run_block(hipStream_t s, const Block& bk, const float* x, const float* x2, float* t0, float* t1, float* dst, int B) {
    auto conv = [&](const ConvDesc& d, const float* in, const float* in2, float* o, bool stats) {
        const int wsize = d.Cout * (d.Cin / d.groups) * d.kt * d.kf;      // same element count for Conv2d and ConvTranspose2d layouts
        const size_t stage = (size_t)d.kt * d.Fi * d.Cin + wsize, sq = stats ? (size_t)d.Fo * d.Cout : 0;
        const dim3 grid((unsigned)((long long)B * T));
        const size_t lds = std::max(stage, sq) * sizeof(float);
        float *z = stats ? zt : nullptr, *pq = stats ? pfreq : nullptr;
        const ClipFrames clip{in, in2};
        PushFrames push{in, in2, nullptr, nullptr, d.kt - 1};
        if (live && d.kt > 1) {        // a push: the taps before its first frame come from the stream's history (one convolution per block has kt > 1), which this launch renews
            const size_t at_ = live->hist_off[&bk - blocks];
            push.hist_in = live->hist[live->cur] + at_;
            push.hist_out = live->flushing ? nullptr : live->hist[live->cur ^ 1] + at_;
        }
#define ADE_ULU_CONV(KT, KF, S, DC) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ulu_conv<KT, KF, S, DC, ClipFrames>), grid, dim3(256), lds, s, clip, d, o, T, wsize, z, pq)
#define ADE_ULU_CONV_T(KT, KF, S, DC)                                                                                                                          \
    if (push.hist_in) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ulu_conv<KT, KF, S, DC, PushFrames>), grid, dim3(256), lds, s, push, d, o, T, wsize, z, pq);       \
    else ADE_ULU_CONV(KT, KF, S, DC)
        const int key = d.kt * 1000 + d.kf * 100 + d.stride * 10 + d.deconv;       // create() admits exactly these shapes
        switch (key) {
            case 1110: ADE_ULU_CONV(1, 1, 1, false); break;
            case 3320: ADE_ULU_CONV_T(3, 3, 2, false); break;
            case 3321: ADE_ULU_CONV_T(3, 3, 2, true); break;
            case 2320: ADE_ULU_CONV_T(2, 3, 2, false); break;
            case 2321: ADE_ULU_CONV_T(2, 3, 2, true); break;
            case 2310: ADE_ULU_CONV_T(2, 3, 1, false); break;
            case 2311: ADE_ULU_CONV_T(2, 3, 1, true); break;
            case 1510: ADE_ULU_CONV(1, 5, 1, false); break;
            default: ADE_ULU_CONV(1, 5, 1, true); break;     // 1511
        }
#undef ADE_ULU_CONV_T
#undef ADE_ULU_CONV
    };
    const int tail_shuffle = (!bk.last && bk.groups == 2) ? 1 : 0;
    if (bk.type == 0) {
        conv(bk.conv[0], x, x2, t0, true);
        ctfa(s, bk, t0, nullptr, dst, B, tail_shuffle);
    } else if (bk.type == 1) {
        conv(bk.conv[0], x, x2, t0, false);
        conv(bk.conv[1], t0, nullptr, t1, true);
        ctfa(s, bk, t1, nullptr, dst, B, 0);
    } else {
        conv(bk.conv[0], x, x2, t0, false);
        conv(bk.conv[1], t0, nullptr, t1, false);
        conv(bk.conv[2], t1, nullptr, t0, true);
        const float* res = (bk.cin == bk.cout && bk.stride == 1) ? x : nullptr;      // use_residual (:397, :448-449); never together with a skip input (checked at create)
        ctfa(s, bk, t0, res, dst, B, tail_shuffle);
    }
    return dst;
}

int UlunasEngine::run(hipStream_t s, const int16_t* d_in, int batch, int16_t* d_out, float* d_f32, std::string& err) {
    if (batch == 0) return ADE_OK;
    int st = reserve(batch, err);
    if (st != ADE_OK) return st;
    const int B = batch * n_win;
    auto flat = [&](long long total) { return dim3((unsigned)((total + 255) / 256)); };
    if (float_in) hipLaunchKernelGGL(k_ulu_f2f, flat((long long)B * L), dim3(256), 0, s, float_in, xf, (long long)B * L);
    else hipLaunchKernelGGL(k_ulu_pcm2f, flat((long long)B * L), dim3(256), 0, s, d_in, xf, (long long)B * L);
    if (ade_stft_analyze(plan, xf, B, L, spec, (void*)s) != ADE_OK) return ufail(err, ADE_ERR_DEVICE, std::string("ul_unas: ") + ade_stft_last_error(plan));
    // the network per row group (see groups_): every buffer between the two STFTs is row-major in the clip, so a group is the same launch sequence on shifted pointers
    const int floor_rows = getenv("ADE_ULU_GROUPS") ? 1 : 16;          // (an explicit request groups any batch: the tests run three rows in three groups)
    const int G = B >= floor_rows * groups_ ? groups_ : 1, per = (B + G - 1) / G;
    if (G > 1) {
        UL_HIP(hipEventRecord(ev_fork, s));
        for (int k = 1; k < G; ++k) {
            const int r0 = k * per, nr = std::min(per, B - r0);
            if (nr <= 0) break;
            UL_HIP(hipStreamWaitEvent(side[k - 1], ev_fork, 0));
            shift_rows(r0);
            run_net(side[k - 1], nr);
            shift_rows(-r0);
            UL_HIP(hipEventRecord(ev_join[k - 1], side[k - 1]));
        }
        run_net(s, per);
        for (int k = 1; k < G && k * per < B; ++k) UL_HIP(hipStreamWaitEvent(s, ev_join[k - 1], 0));
    } else run_net(s, B);
    if (ade_stft_synthesize(plan, spec, B, T, yf, (void*)s) != ADE_OK) return ufail(err, ADE_ERR_DEVICE, std::string("ul_unas: ") + ade_stft_last_error(plan));
    hipLaunchKernelGGL(k_ulu_f2pcm, flat((long long)B * out_len_), dim3(256), 0, s, (const float*)yf, d_out, d_f32, syn_len, out_len_, (long long)B * out_len_);
    UL_HIP(hipGetLastError());
    return ADE_OK;
}

void UlunasEngine::shift_rows(long long rows) {
    const long long fr = rows * T;
    spec += rows * 2 * kUBins * T; mask_tap += fr * kUBins;
    bufA += fr * 1600; bufB += fr * 1600; bufC += fr * 1600; bufD += fr * 1600;
    dpa += fr * kFw * kCh; dpb += fr * kFw * kCh; rnn += fr * kFw * kCh; dpm += fr * kFw * kCh;
    zt += fr * 32; pfreq += fr * 132; at += fr * 32; fah += fr * 33 * 8;
    for (int i = 0; i < 5; ++i) skip[i] += fr * blocks[i].width * blocks[i].cout;
}

// feature extraction .. mask on the spectrum for B consecutive clips starting at the buffers' current row
void UlunasEngine::run_net(hipStream_t s, int B) {
    const long long nfr = (long long)B * T;
    auto flat = [&](long long total) { return dim3((unsigned)((total + 255) / 256)); };
    hipLaunchKernelGGL(k_ulu_feat, flat(nfr * kUErb), dim3(256), 0, s, (const float*)spec, erb, (const int*)d_tab, (const int*)(d_tab + kUBands), bufC, T, nfr * kUErb);
    const float* x = bufC;
    for (int i = 0; i < 5; ++i) x = run_block(s, blocks[i], x, nullptr, bufA, bufB, skip[i], B);
    // DPGRNN x 2 on (B, T, 33, 16): GTCRN's kernels (Export_UL_UNAS.py:561-574 == GTCRN's DPGRNN)
    const float* in = x;
    for (int i = 0; i < 2; ++i) {
        float* o = i == 0 ? dpa : dpb;
        launch_intra_gru(s, View{in, nullptr}, dp[i].intra_gru, rnn, (int)nfr);
        launch_fc_ln_res(s, rnn, View{in, nullptr}, dp[i].fc[0], dp[i].fc_b[0], dp[i].ln_w[0], dp[i].ln_b[0], dpm, B, T);
        if (live) hipLaunchKernelGGL(k_ulu_stream_inter_gru, dim3((unsigned)((B * kFw + 15) / 16)), dim3(256), 0, s, (const float*)dpm, dp[i].inter_gru, rnn, B, T, live->inter[i]);
        else launch_inter_gru(s, dpm, dp[i].inter_gru, rnn, B, T);
        launch_fc_ln_res(s, rnn, View{dpm, nullptr}, dp[i].fc[1], dp[i].fc_b[1], dp[i].ln_w[1], dp[i].ln_b[1], o, B, T);
        in = o;
    }
    // decoder: block i runs on x + en_outs[4 - i] (:647-648)
    const float* dx = in;
    for (int i = 0; i < 5; ++i) {
        float* dst = (i & 1) ? bufD : bufC;
        run_block(s, blocks[5 + i], dx, skip[4 - i], bufA, bufB, dst, B);
        dx = dst;
    }
    // sigmoid, ERB split, real mask on the spectrum (:649, :734-736, :880); ISTFT; PCM tail (:955, :908)
    hipLaunchKernelGGL(k_ulu_mask, flat(nfr * kUBins), dim3(256), 0, s, dx, erb, (const int*)(d_tab + 2 * kUBands), (const int*)(d_tab + 2 * kUBands + kUHigh), spec, mask_tap, T,
                       nfr * kUBins);
}

// ---- streams ----------------------------------------------------------------------------------------------------------------------------------------------------
int UlunasEngine::stream_create(int n_streams, int frames_per_push, void** state, std::string& err) {
    *state = nullptr;
    if (frames_per_push == 1)
        return ufail(err, ADE_ERR_BAD_VALUE, "ade_stream_create: ul_unas: frames_per_push = 1 is not supported: the first push must hold the 257 samples the head reflection reads "
                                             "(2 <= frames_per_push <= 4096)");
    if (n_streams < 1 || frames_per_push < 2 || frames_per_push > 4096)
        return ufail(err, ADE_ERR_BAD_VALUE, "ade_stream_create: ul_unas needs n_streams >= 1 and 2 <= frames_per_push <= 4096");
    const size_t S = (size_t)n_streams, nfr = S * frames_per_push;
    if (nfr * 1600 > 0x7fffffffULL) return ufail(err, ADE_ERR_BAD_VALUE, "ade_stream_create: ul_unas: n_streams * frames_per_push exceeds the launch grid");
    std::unique_ptr<UlunasStream> st(new UlunasStream());
    st->S = n_streams; st->F = frames_per_push;
    auto up = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    size_t n_hist = 0, n_ta = 0;
    for (int i = 0; i < 10; ++i) {
        st->hist_off[i] = n_hist;
        st->ta_off[i] = n_ta;
        const int nc = blocks[i].type == 0 ? 1 : blocks[i].type == 1 ? 2 : 3;
        for (int c = 0; c < nc; ++c) {
            const ConvDesc& d = blocks[i].conv[c];
            if (d.kt > 1) n_hist += (S * (d.kt - 1) * d.Fi * d.Cin + 63) & ~(size_t)63;       // (at most one per block)
        }
        n_ta += (S * 2 * blocks[i].cout + 63) & ~(size_t)63;
    }
    const size_t b_carry = up(S * kUCarry * sizeof(int16_t)), b_hist = up(n_hist * sizeof(float)), b_half = up(S * kUHop * sizeof(float)), b_ta = up(n_ta * sizeof(float)),
                 b_inter = up(S * kFw * kCh * sizeof(float));
    UlunasWork& w = st->work;
    w.T = frames_per_push;
    const size_t act = nfr * 1600;             // the carve of reserve(), a push's frames in place of a call's
    struct Carve { float** p; size_t n; };
    std::vector<Carve> cs = {{&w.spec, S * 2 * kUBins * frames_per_push}, {&w.bufA, act}, {&w.bufB, act}, {&w.bufC, act}, {&w.bufD, act}, {&w.dpa, nfr * kFw * kCh}, {&w.dpb, nfr * kFw * kCh},
                             {&w.zt, nfr * 32}, {&w.pfreq, nfr * 132}, {&w.at, nfr * 32}, {&w.fah, nfr * 33 * 8}, {&w.rnn, nfr * kFw * kCh}, {&w.dpm, nfr * kFw * kCh},
                             {&st->frames, nfr * kUNfft}};
    for (int i = 0; i < 5; ++i) cs.push_back({&w.skip[i], nfr * (size_t)blocks[i].width * blocks[i].cout});
    size_t total = 2 * b_carry + 2 * b_hist + 2 * b_half + b_ta + 2 * b_inter;
    st->reset_bytes = total;
    for (auto& c : cs) total += up(c.n * sizeof(float));
    if (hipSetDevice(device) != hipSuccess || hipMalloc(&st->block, total) != hipSuccess) {
        (void)hipGetLastError();
        return ufail(err, ADE_ERR_DEVICE, "ade_stream_create: hipMalloc of the UL-UNAS stream state failed");
    }
    char* p = (char*)st->block;
    for (int i = 0; i < 2; ++i) { st->carry[i] = (int16_t*)p; p += b_carry; }
    for (int i = 0; i < 2; ++i) { st->hist[i] = (float*)p; p += b_hist; }
    for (int i = 0; i < 2; ++i) { st->half[i] = (float*)p; p += b_half; }
    st->ta = (float*)p; p += b_ta;
    for (int i = 0; i < 2; ++i) { st->inter[i] = (float*)p; p += b_inter; }
    for (auto& c : cs) { *c.p = (float*)p; p += up(c.n * sizeof(float)); }
    *state = st.release();
    return ADE_OK;
}

int UlunasEngine::stream_reset(void* state, hipStream_t s, std::string& err) {
    UlunasStream* st = (UlunasStream*)state;
    UL_HIP(hipMemsetAsync(st->block, 0, st->reset_bytes, s));
    st->hops = 0;
    st->cur = 0;
    return ADE_OK;
}

// A push (d_in set: F frames per stream) or the flush (d_in null: frame K, one per stream), everything on `s`.
int UlunasEngine::stream_step(UlunasStream* st, hipStream_t s, const int16_t* d_in, int16_t* d_out, float* d_f32, std::string& err) {
    const bool flush = d_in == nullptr, fresh = st->hops == 0;
    const int S = st->S, F = flush ? 1 : st->F, N = S * F, nxt = st->cur ^ 1;
    const float2 *tw512 = reinterpret_cast<const float2*>(stw512), *tw256 = reinterpret_cast<const float2*>(stw256);
    UlunasWork& w = st->work;
    // 1. analysis of the frames this step completes, and the next carried input
    hipLaunchKernelGGL(k_ulu_stream_analysis, dim3((unsigned)(flush ? N : N + S)), dim3(256), 0, s, d_in, (const int16_t*)st->carry[st->cur], st->carry[nxt], F * kUHop, F, N,
                       flush ? 2 : (fresh ? 1 : 0), p256, tw256, tw512, swin, w.spec);
    // 2. the network on the stream's buffers with T = F, continued from the stream's state (run_block / ctfa / run_net read `live`)
    const UlunasWork mine = *this;
    static_cast<UlunasWork&>(*this) = w;
    T = F;
    st->flushing = flush;
    live = st;
    run_net(s, S);
    live = nullptr;
    static_cast<UlunasWork&>(*this) = mine;
    // 3. one inverse transform per frame; overlap-add, window-square sum, PCM tail, the next carried half
    hipLaunchKernelGGL(k_ulu_stream_synthesis, dim3((unsigned)N), dim3(256), 0, s, (const float*)w.spec, F, p256, tw256, tw512, swin, st->frames);
    const long long total = (long long)N * kUHop, total_all = total + (flush ? 0 : (long long)S * kUHop);
    hipLaunchKernelGGL(k_ulu_stream_out, dim3((unsigned)((total_all + 255) / 256)), dim3(256), 0, s, (const float*)st->frames, (const float*)st->half[st->cur],
                       flush ? (float*)nullptr : st->half[nxt], sden, F, fresh ? 1 : 0, d_out, d_f32, total, total_all);
    UL_HIP(hipGetLastError());
    if (!flush) { st->cur = nxt; st->hops += st->F; }
    return ADE_OK;
}

int UlunasEngine::stream_push(void* state, hipStream_t s, const int16_t* d_in, int16_t* d_out, float* d_f32, std::string& err) {
    return stream_step((UlunasStream*)state, s, d_in, d_out, d_f32, err);
}

// The last hop: frame K, whose second half is the reflection of the carried samples, added to the carried half frame.
int UlunasEngine::stream_flush(void* state, hipStream_t s, int16_t* d_out, float* d_f32, std::string& err) {
    UlunasStream* st = (UlunasStream*)state;
    if (st->hops < 2) return ufail(err, ADE_ERR_BAD_VALUE, "ade_stream_flush: ul_unas: nothing pushed since the last reset");
    return stream_step(st, s, nullptr, d_out, d_f32, err);
}

void UlunasEngine::stream_destroy(void* state) {
    UlunasStream* st = (UlunasStream*)state;
    if (!st) return;
    (void)hipSetDevice(device);
    if (st->block) (void)hipFree(st->block);
    delete st;
}

int UlunasEngine::tap(hipStream_t s, const char* name, int batch, float* out, size_t count, size_t* written, std::string& err) {
    const size_t n = (size_t)batch * n_win * T * kUBins;
    if (strcmp(name, "mask") != 0) return ufail(err, ADE_ERR_NOT_FOUND, std::string("unknown tap: ") + name);
    if (!mask_tap || batch <= 0) return ufail(err, ADE_ERR_NOT_FOUND, "tap has no data yet");
    if (count < n) return ufail(err, ADE_ERR_SHAPE_MISMATCH, "tap buffer too small");
    UL_HIP(hipStreamSynchronize(s));
    UL_HIP(hipMemcpy(out, mask_tap, n * sizeof(float), hipMemcpyDeviceToHost));
    *written = n;
    return ADE_OK;
}

}  // namespace ade
