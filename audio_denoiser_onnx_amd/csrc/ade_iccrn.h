// ade_iccrn.h — the ICCRN building material that SDAEC (csrc/ade_sdaec.hip) and Deep Echo (csrc/ade_deep_echo.hip) share: the clip mean, the loaders and stores of
// the dense analysis / synthesis products and of the hoisted LSTM input products, the cepstral unit's products, the frame-local CFB kernel, the plane statistics, the
// overlap-add gather, the recurrence kernel k_sd_lstm<H> (see the header of csrc/ade_sdaec.hip for its derivation) and the builder of the STFT tables.  Everything
// here has internal linkage: each of the two translation units compiles its own copy.
#pragma once
#include "ade_gemm.h"
#include "ade_internal.h"

#include <cmath>
#include <vector>

namespace ade {

namespace {

using namespace dev;

constexpr int kN = 319, kHopS = 160, kF = 160, kC = 20, kCb = 81, kFrameLd = 320;

// ---- front ------------------------------------------------------------------------------------------------------------------------------------------------------
// source row of (clip, channel): the caller's rows are [call][channel 0 = near end, 1 = far end][n_win windows of L]
__device__ __forceinline__ size_t src_row(int clip, int ch, int n_win, int L) {
    const int call = clip / n_win, w = clip - call * n_win;
    return (((size_t)call * 2 + ch) * n_win + w) * (size_t)L;
}

// one workgroup per (clip, channel): the mean of the clip's samples / 32768 (:398-399)
__global__ __launch_bounds__(256) void k_sd_mean(const int16_t* __restrict__ pcm, const float* __restrict__ fpcm, int L, int n_win, float* __restrict__ mean) {
    __shared__ double red[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    const size_t base = src_row(row >> 1, row & 1, n_win, L);
    double s = 0.0;
    for (int n = tid; n < L; n += 256) s += fpcm ? (double)fpcm[base + n] : (double)pcm[base + n];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) mean[row] = (float)(red[0] / (double)L * (1.0 / 32768.0));
}

struct FrameB {                // B(k, n): sample k of frame n = (clip * 2 + channel) * T + t: (x / 32768 - mean), zero in the constant centre pad
    static constexpr bool kAlongN = false;
    const int16_t* pcm;
    const float* fpcm;
    const float* mean;
    int L, T, n_win;
    __device__ float operator()(int k, int n) const {
        const int row = n / T, t = n - row * T, p = t * kHopS + k - kN / 2;
        if (p < 0 || p >= L) return 0.0f;
        const size_t at = src_row(row >> 1, row & 1, n_win, L) + p;
        return (fpcm ? fpcm[at] : (float)pcm[at]) * (1.0f / 32768.0f) - mean[row];
    }
};
struct SpecStore {             // rows 0 .. 159 the real parts, 160 .. 319 the imaginary parts -> [frame][bin] (re, im)
    float* spec;
    __device__ void operator()(int m, int n, float v) const { spec[((size_t)n * kF + (m < kF ? m : m - kF)) * 2 + (m >= kF ? 1 : 0)] = v; }
};

// ---- the hoisted input products of the LSTMs: stores and loaders ---------------------------------------------------------------------------------------------------
// The product is computed with the POSITIONS as rows (m = (clip * T + frame) * 160 + bin, or frame * 81 + cepstral bin) and the stacked, row-permuted W_ih as columns
// (n = dir * 4 H + unit * 4 + gate), through the GEMM's float4 store form: a lane's four results are the four gates of one unit of one position, one 16-byte store, and the
// four lane groups of a tile cover 64 contiguous bytes.   xg[(dir * positions + m) * 4 H + unit * 4 + gate]
struct XgStore {
    static constexpr bool kCtx = true;
    static constexpr bool kV4 = true;
    float* xg;
    const float* bias;        // [dirs * 4 H] b_ih + b_hh, permuted like the rows of W_ih
    int H4;
    size_t n_pos;
    __host__ __device__ bool can_v4(int N) const { return (N & 3) == 0; }
    __device__ gemm::None row(int) const { return gemm::None{}; }
    __device__ float col(int n) const { return bias[n]; }
    __device__ gemm::None pre(int, int, gemm::None) const { return gemm::None{}; }
    __device__ void operator()(int m, int n, float v, gemm::None, float b, gemm::None) const {
        const int dir = n / H4;
        xg[((size_t)dir * n_pos + m) * H4 + (n - dir * H4)] = v + b;
    }
    __device__ float4 col4(int n) const { return *reinterpret_cast<const float4*>(bias + n); }
    __device__ gemm::None pre4(int, int, gemm::None) const { return gemm::None{}; }
    __device__ void store4(int m, int n, float4 v, gemm::None, const float4& b, gemm::None) const {
        const int dir = n / H4;
        *reinterpret_cast<float4*>(xg + ((size_t)dir * n_pos + m) * H4 + (n - dir * H4)) = make_float4(v.x + b.x, v.y + b.y, v.z + b.z, v.w + b.w);
    }
};
struct LnLoadA {               // A(m, k) = LayerNorm(x)[m][k]: x [frame][rows][C] with the frame's (mean, rstd) in stats and the (rows, C) affine
    static constexpr bool kAlongK = true;
    const float* x;
    const float2* stats;
    const float* w;
    const float* b;
    int rows, C;
    __device__ float operator()(int m, int k) const {
        const int fr = m / rows, r = m - fr * rows;
        const float2 s = stats[fr];
        return (x[(size_t)m * C + k] - s.x) * s.y * w[r * C + k] + b[r * C + k];
    }
};
struct Cat2A {                 // A(m, k) = k < ca ? a[m][k] : b[m][k - ca]
    static constexpr bool kAlongK = true;
    const float* a;
    const float* b;
    int ca, cb;
    __device__ float operator()(int m, int k) const { return k < ca ? a[(size_t)m * ca + k] : b[(size_t)m * cb + (k - ca)]; }
};
struct Cat2B {                 // B(k, n) = k < ca ? a[n][k] : b[n][k - ca]
    static constexpr bool kAlongN = false;
    const float* a;
    const float* b;
    int ca, cb;
    __device__ float operator()(int k, int n) const { return k < ca ? a[(size_t)n * ca + k] : b[(size_t)n * cb + (k - ca)]; }
};
struct StoreNM {               // out[n][m] = v + bias[m]; mul: ... * mul[n][m] into out2 as well (lstm_out and e5 * lstm_out, :272-273)
    static constexpr bool kCtx = true;
    float* out;
    const float* bias;
    int ld;
    const float* mul;
    float* out2;
    __device__ float row(int m) const { return bias[m]; }
    __device__ gemm::None col(int) const { return gemm::None{}; }
    __device__ float pre(int m, int n, float) const { return mul ? mul[(size_t)n * ld + m] : 0.0f; }
    __device__ void operator()(int m, int n, float v, float b, gemm::None, float e) const {
        v += b;
        out[(size_t)n * ld + m] = v;
        if (mul) out2[(size_t)n * ld + m] = e * v;
    }
};

// ---- the cepstral unit's products ------------------------------------------------------------------------------------------------------------------------------------
struct PlaneB {                // B(k, n = frame * 20 + c) = z[frame][k][c]
    static constexpr bool kAlongN = true;
    const float* z;
    int rows;
    __device__ float operator()(int k, int n) const { const int fr = n / kC, c = n - fr * kC; return z[((size_t)fr * rows + k) * kC + c]; }
};
struct CepsStore {             // table row m = 2 bin + (re, im) -> sp[frame][bin][(re, im) * 20 + c]
    float* sp;
    __device__ void operator()(int m, int n, float v) const { const int fr = n / kC, c = n - fr * kC; sp[((size_t)fr * kCb + (m >> 1)) * (2 * kC) + (m & 1) * kC + c] = v; }
};
struct CepsMulB {              // B(k, n): the packed [re bins | im bins] of (processed * stft) (:121-124): processed = lin, stft = sp
    static constexpr bool kAlongN = true;
    const float* lin;
    const float* sp;
    __device__ float operator()(int k, int n) const {
        const int fr = n / kC, c = n - fr * kC, im = k >= kCb ? 1 : 0, bin = k - im * kCb;
        const size_t at = ((size_t)fr * kCb + bin) * (2 * kC) + c;
        const float pr = lin[at], pi = lin[at + kC], sr = sp[at], si = sp[at + kC];
        return im ? pr * si + pi * sr : pr * sr - pi * si;
    }
};
struct ResidualStore {         // out[frame][m][c] = v + y[frame][m][c] (:93)
    static constexpr bool kCtx = true;
    float* out;
    const float* y;
    __device__ gemm::None row(int) const { return gemm::None{}; }
    __device__ size_t col(int n) const { const int fr = n / kC, c = n - fr * kC; return (size_t)fr * kF * kC + c; }
    __device__ float pre(int m, int n, gemm::None) const { const int fr = n / kC, c = n - fr * kC; return y[(size_t)fr * kF * kC + (size_t)m * kC + c]; }
    __device__ void operator()(int m, int, float v, gemm::None, size_t at, float r) const { out[at + (size_t)m * kC] = v + r; }
};

// ---- synthesis ---------------------------------------------------------------------------------------------------------------------------------------------------
struct InvA {                  // A(j, k) = inverse table row k (packed re | im bins), sample j
    static constexpr bool kAlongK = false;
    const float* p;
    __device__ float operator()(int m, int k) const { return p[(size_t)k * kFrameLd + m]; }
};
struct SpecOutB {              // B(k, n) = packed [re bins | im bins] of the output spectrum of frame n, [frame][bin][re, im]
    static constexpr bool kAlongN = false;
    const float* e;
    __device__ float operator()(int k, int n) const { return e[((size_t)n * kF + (k < kF ? k : k - kF)) * 2 + (k >= kF ? 1 : 0)]; }
};
struct FrameStore {
    float* p;
    __device__ void operator()(int m, int n, float v) const { p[(size_t)n * kFrameLd + m] = v; }
};
// overlap-add as a gather: samples [159, 159 + L) of the raw sum, * 1 / window-square sum (the f32 waveform), * 32767, clamp, .to(int16) (:429-441)
__global__ __launch_bounds__(256) void k_sd_ola(const float* __restrict__ frames, const float* __restrict__ inv_ws, int T, int L, int16_t* __restrict__ pcm, float* __restrict__ f32,
                                                long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long clip = i / L;
    const int m = (int)(i - clip * L), p = m + kN / 2;
    int t_hi = p / kHopS;
    if (t_hi > T - 1) t_hi = T - 1;
    const int t_lo = p < kN ? 0 : (p - kN) / kHopS + 1;
    float s = 0.0f;
    for (int t = t_lo; t <= t_hi; ++t) s += frames[((size_t)clip * T + t) * kFrameLd + (p - t * kHopS)];
    const float w = s * inv_ws[m];
    if (f32) f32[i] = w;
    if (pcm) pcm[i] = (int16_t)(int)fminf(fmaxf(w * 32767.0f, -32768.0f), 32767.0f);
}

// ---- LayerNorm statistics of a contiguous plane: two-pass, fp32 ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_sum(float v, float* red) {      // 256 threads; red: 4 floats of LDS
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                                    // the previous use of red is over
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void k_sd_stats(const float* __restrict__ x, int plane, float eps, float2* __restrict__ stats) {
    __shared__ float red[4];
    const float* p = x + (size_t)blockIdx.x * plane;
    float s = 0.0f;
    for (int i = threadIdx.x; i < plane; i += 256) s += p[i];
    const float mu = block_sum(s, red) * (1.0f / (float)plane);
    float q = 0.0f;
    for (int i = threadIdx.x; i < plane; i += 256) { const float d = p[i] - mu; q += d * d; }
    const float var = block_sum(q, red) * (1.0f / (float)plane);
    if (threadIdx.x == 0) stats[blockIdx.x] = make_float2(mu, 1.0f / sqrtf(var + eps));
}

// ---- the frame-local part of a CFB (:82-94): one workgroup per frame, the planes in LDS ---------------------------------------------------------------------------------
struct CfbW {
    const float *ln0_w, *ln0_b, *ln1_w, *ln1_b, *ln2_w, *ln2_b;      // (160, C_in) / (160, 20)
    const float *gate_t, *gate_b, *input_t, *input_b;                // [C_in][20] (transposed), [20]
    const float *conv_t, *conv_b;                                    // [tap][c_in][c_out], [20]
    float eps0, eps1, eps2;
};
constexpr int kCfbLds = kF * 2 * kC + 2 * kF * kC + 2 * 2 * kC * kC + 3 * kC * kC + 8;      // X, GX, R, gate / input weights, conv weights, reduction scratch
template <int CIN>
__global__ __launch_bounds__(256) void k_sd_cfb(const float* __restrict__ xa, const float* __restrict__ xb, CfbW w, float* __restrict__ y, float* __restrict__ z) {
    HIP_DYNAMIC_SHARED(float, lds)
    float* X = lds;                          // [160][CIN]
    float* GX = X + kF * CIN;                // [160][20]
    float* R = GX + kF * kC;                 // [160][20]
    float* Wg = R + kF * kC;                 // [CIN][20]
    float* Wi = Wg + CIN * kC;               // [CIN][20]
    float* Wc = Wi + CIN * kC;               // [3][20][20]
    float* red = Wc + 3 * kC * kC;
    const int tid = threadIdx.x;
    const size_t fr = blockIdx.x;
    // the plane: C_in = 40 is cat([xa, xb]) along the channels (:274-277)
    for (int i = tid; i < kF * CIN; i += 256) {
        const int f = i / CIN, c = i - f * CIN;
        X[i] = c < kC ? xa[(fr * kF + f) * kC + c] : xb[(fr * kF + f) * kC + (c - kC)];
    }
    for (int i = tid; i < CIN * kC; i += 256) { Wg[i] = w.gate_t[i]; Wi[i] = w.input_t[i]; }
    for (int i = tid; i < 3 * kC * kC; i += 256) Wc[i] = w.conv_t[i];
    __syncthreads();
    float s = 0.0f;
    for (int i = tid; i < kF * CIN; i += 256) s += X[i];
    const float mu0 = block_sum(s, red) * (1.0f / (float)(kF * CIN));
    float q = 0.0f;
    for (int i = tid; i < kF * CIN; i += 256) { const float d = X[i] - mu0; q += d * d; }
    const float rs0 = 1.0f / sqrtf(block_sum(q, red) * (1.0f / (float)(kF * CIN)) + w.eps0);
    // gate and input Linears, g * x and x - g x
    float s1 = 0.0f, s2 = 0.0f;
    for (int i = tid; i < kF * kC; i += 256) {
        const int f = i / kC, o = i - f * kC;
        float g = w.gate_b[o], xi = w.input_b[o];
        const float* xr = X + f * CIN;
        const float* lw = w.ln0_w + f * CIN;
        const float* lb = w.ln0_b + f * CIN;
#pragma unroll 4
        for (int c = 0; c < CIN; ++c) {
            const float v = xr[c];
            g += Wg[c * kC + o] * ((v - mu0) * rs0 * lw[c] + lb[c]);
            xi += Wi[c * kC + o] * v;
        }
        const float gx = xi / (1.0f + expf(-g));
        GX[i] = gx;
        R[i] = xi - gx;
        s1 += gx;
        s2 += xi - gx;
    }
    const float mu1 = block_sum(s1, red) * (1.0f / (float)(kF * kC));
    const float mu2 = block_sum(s2, red) * (1.0f / (float)(kF * kC));
    float q1 = 0.0f, q2 = 0.0f;
    for (int i = tid; i < kF * kC; i += 256) {
        const float d1 = GX[i] - mu1, d2 = R[i] - mu2;
        q1 += d1 * d1;
        q2 += d2 * d2;
    }
    const float rs1 = 1.0f / sqrtf(block_sum(q1, red) * (1.0f / (float)(kF * kC)) + w.eps1);
    const float rs2 = 1.0f / sqrtf(block_sum(q2, red) * (1.0f / (float)(kF * kC)) + w.eps2);
    // LN1 in place (the convolution reads its neighbours), LN2 straight to memory
    for (int i = tid; i < kF * kC; i += 256) {
        GX[i] = (GX[i] - mu1) * rs1 * w.ln1_w[i] + w.ln1_b[i];
        z[fr * kF * kC + i] = (R[i] - mu2) * rs2 * w.ln2_w[i] + w.ln2_b[i];
    }
    __syncthreads();
    for (int i = tid; i < kF * kC; i += 256) {
        const int f = i / kC, o = i - f * kC;
        float a = w.conv_b[o];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int ff = f - 1 + k;
            if (ff < 0 || ff >= kF) continue;               // padding = 1: zeros
            const float* g = GX + ff * kC;
            const float* cw = Wc + k * kC * kC + o;
#pragma unroll 4
            for (int c = 0; c < kC; ++c) a += cw[c * kC] * g[c];
        }
        y[fr * kF * kC + i] = a;
    }
}

// ---- the recurrence (see the header) -------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(n_seq / 64), directions); 4 wavefronts of 16 sequences.  whh: [dir][4 H][H] (PyTorch), xg as XgStore lays it out.  Position of (seq, step) =
// (seq / sdiv) * outer + (seq % sdiv) * inner + step * sstep; h goes to out[position * ldo + dir * H + unit].
struct LstmGeo { float* out; int sdiv, ldo; size_t outer, inner, sstep, n_pos; };
template <int H>
__global__ __launch_bounds__(256) void k_sd_lstm(const float* __restrict__ xg, const float* __restrict__ whh, int n_seq, int S, LstmGeo o) {
    constexpr int NT = H / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, j = lane & 15, dir = blockIdx.y;
    const int seq0 = ((int)blockIdx.x * 4 + wave) * 16;
    if (seq0 >= n_seq) return;                                                    // wave-uniform
    const int seq = seq0 + j, sq = seq < n_seq ? seq : n_seq - 1;                 // lanes past the end recompute the last sequence and store nothing
    const float* W = whh + (size_t)dir * 4 * H * H;
    float a[NT][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int ks = 0; ks < NT; ++ks) a[t][ks] = W[((j & 3) * H + 4 * t + (j >> 2)) * H + 4 * ks + q];
    float h[NT], c[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { h[t] = 0.0f; c[t] = 0.0f; }
    const size_t pos0 = (size_t)(sq / o.sdiv) * o.outer + (size_t)(sq % o.sdiv) * o.inner;
    const float* xs = xg + ((size_t)dir * o.n_pos + pos0) * (4 * H) + q * 4;      // + step * sstep * 4 H + t * 16
    const size_t xstep = o.sstep * (4 * H);
    float* os = o.out + pos0 * o.ldo + dir * H + q;
    float4 nx[NT];
    {
        const int s0 = dir ? S - 1 : 0;
#pragma unroll
        for (int t = 0; t < NT; ++t) nx[t] = *reinterpret_cast<const float4*>(xs + (size_t)s0 * xstep + t * 16);
    }
    for (int it = 0; it < S; ++it) {
        const int step = dir ? S - 1 - it : it;
        v4f d[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) d[t] = v4f{nx[t].x, nx[t].y, nx[t].z, nx[t].w};
        if (it + 1 < S) {                                                          // the next step's pre-activations, under this step's products
            const int sn = dir ? step - 1 : step + 1;
#pragma unroll
            for (int t = 0; t < NT; ++t) nx[t] = *reinterpret_cast<const float4*>(xs + (size_t)sn * xstep + t * 16);
        }
#pragma unroll
        for (int ks = 0; ks < NT; ++ks)
#pragma unroll
            for (int t = 0; t < NT; ++t) d[t] = mfma16x16x4(a[t][ks], h[ks], d[t]);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float gi = sigmoid_f(d[t][0]), gf = sigmoid_f(d[t][1]), gg = tanh_f(d[t][2]), go = sigmoid_f(d[t][3]);
            c[t] = gf * c[t] + gi * gg;
            h[t] = go * tanh_f(c[t]);
        }
        if (seq < n_seq) {
            float* op = os + (size_t)step * o.sstep * o.ldo;
#pragma unroll
            for (int t = 0; t < NT; ++t) op[4 * t] = h[t];
        }
    }
}

// ---- the STFT tables -------------------------------------------------------------------------------------------------------------------------------------------------
// fwd: [2 * 160][319], inv: [2 * 160][320], inv_ws: [window_len]
inline void stft_tables(float* fwd, float* inv, float* inv_ws, int window_len, int T) {
    // the windowed DFT tables as STFT_Process builds them: periodic Hamming in fp32 (torch.hamming_window), fp32 angles fl(fl(2 pi / N * f) * t) (SDAEC/STFT_Process.py:207-244)
    std::vector<float> win(kN);
    for (int n = 0; n < kN; ++n) win[n] = (float)(0.54 - 0.46 * cos(2.0 * M_PI * n / kN));
    {
        const float c32 = (float)(2.0 * M_PI / kN);
        for (int f = 0; f < kF; ++f) {
            const float cf = c32 * (float)f, sc = f == 0 ? 1.0f : 2.0f;          // odd n_fft: no Nyquist bin
            for (int t = 0; t < kN; ++t) {
                const float om = cf * (float)t, c = cosf(om), sn = sinf(om);
                fwd[(size_t)f * kN + t] = c * win[t];
                fwd[(size_t)(kF + f) * kN + t] = -sn * win[t];
                inv[(size_t)f * kFrameLd + t] = (sc * c * (1.0f / (float)kN)) * win[t];
                inv[(size_t)(kF + f) * kFrameLd + t] = (sc * -sn * (1.0f / (float)kN)) * win[t];
            }
        }
        std::vector<float> wsum((size_t)kN + (size_t)kHopS * (T - 1), 0.0f);     // conv_transpose1d(ones, window^2) in fp32
        for (int t = 0; t < T; ++t)
            for (int n = 0; n < kN; ++n) wsum[(size_t)t * kHopS + n] += win[n] * win[n];
        for (int m = 0; m < window_len; ++m) inv_ws[m] = 1.0f / wsum[kN / 2 + m];       // kN / 2 + L <= kN + 160 (T - 1)
    }
}

}  // namespace

}  // namespace ade
