// Unit check of csrc/ade_fft.h (the mixed-radix Stockham FFT of one frame in LDS).  Host simulator and gfx950.
//   fft_unit ARG [ARG ...]      one line per check and size, exit status non-zero on a mismatch
//     N      fft::forward on the make_plan plan against a double-precision O(N^2) DFT of the same fp32 input, with 256 and with 32 threads; G thread groups transforming G
//            different inputs side by side in one 256-thread workgroup (as k_stft_fft_analyze runs them; G = 8 while 8 x 2 buffers fit in 128 KB of LDS) against the
//            same inputs transformed one per workgroup: word for word.  For the sizes ade_fft.h knows at compile time also forward_static<N> (64 and 256 threads) and
//            forward_wave<N> (one wavefront) against forward: word for word, the result read from the buffer result_in_first<N>() names.
//     rH     the real transform of n = 2 H samples from the H-point forward + split_bin against the double real DFT, and the frame rebuilt from that half spectrum by
//            merge_bin_conj + forward + conjugate and 1 / n (merge_bin_conj's W is twice the half-length spectrum) against the input.
//     plan   make_plan on the host over every n <= 8192.
// Error metric: max |got - ref| / max |ref| (spectra), max |got - x| (rebuilt frames, |x| <= 1).  Bound 2e-6: the operator's own host-simulator gate for a whole STFT, which
// its transform alone has to meet; fp32 Stockham round-off is a few eps x sqrt(passes) of the spectrum's RMS, i.e. some 1e-7 of its maximum.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../audio_denoiser_onnx_amd/csrc/ade_fft.h"

using namespace ade;

static const double kTol = 2e-6;
static const size_t kLdsMax = 128 * 1024;

#define CHECK_HIP(expr)                                                                                  \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) { printf("fft_unit: %s -> %s\n", #expr, hipGetErrorString(e_)); exit(2); } \
    } while (0)

// blockDim.x / per thread groups, each transforming its own input in its own pair of buffers; item = block * groups + group
__global__ __launch_bounds__(256) void k_forward(const float2* __restrict__ in, float2* __restrict__ out, fft::Plan p, const float2* __restrict__ tw, int per) {
    HIP_DYNAMIC_SHARED(float2, lds)
    const int n = p.n, g = (int)threadIdx.x / per, lt = (int)threadIdx.x - g * per;
    const size_t item = (size_t)blockIdx.x * (blockDim.x / per) + g;
    float2 *A = lds + (size_t)g * 2 * n, *B = A + n;
    for (int i = lt; i < n; i += per) A[i] = in[item * n + i];
    const float2* r = fft::forward(A, B, p, tw, lt, per);
    for (int i = lt; i < n; i += per) out[item * n + i] = r[i];
}

template <int N>
__global__ __launch_bounds__(256) void k_static(const float2* __restrict__ in, float2* __restrict__ out, const float2* __restrict__ tw) {
    HIP_DYNAMIC_SHARED(float2, lds)
    float2 *A = lds, *B = lds + N;
    const int tid = threadIdx.x, gt = blockDim.x;
    for (int i = tid; i < N; i += gt) A[i] = in[i];
    fft::forward_static<N>(A, B, tw, tid, gt);
    __syncthreads();
    const float2* r = fft::result_in_first<N>() ? A : B;
    for (int i = tid; i < N; i += gt) out[i] = r[i];
}

template <int N>
__global__ __launch_bounds__(64) void k_wave(const float2* __restrict__ in, float2* __restrict__ out, const float2* __restrict__ tw) {
    HIP_DYNAMIC_SHARED(float2, lds)
    const int lane = threadIdx.x;
    for (int i = lane; i < N; i += 64) lds[i] = in[i];
    dev::wave_sync();
    fft::forward_wave<N>(lds, tw, lane);
    for (int i = lane; i < N; i += 64) out[i] = lds[i];
}

// x: n = 2 h real samples -> spec: h + 1 bins (forward + split_bin) -> back: n samples (merge_bin_conj + forward, conjugated, / n)
__global__ __launch_bounds__(256) void k_real(const float* __restrict__ x, float2* __restrict__ spec, float* __restrict__ back, fft::Plan ph, const float2* __restrict__ twh,
                                              const float2* __restrict__ twn) {
    HIP_DYNAMIC_SHARED(float2, lds)
    const int h = ph.n, tid = threadIdx.x;
    float2 *A = lds, *B = lds + h, *X = lds + 2 * h;
    for (int m = tid; m < h; m += 256) A[m] = make_float2(x[2 * m], x[2 * m + 1]);
    const float2* r = fft::forward(A, B, ph, twh, tid, 256);
    for (int f = tid; f <= h; f += 256) {
        X[f] = fft::split_bin(r, f, h, twn);
        spec[f] = X[f];
    }
    __syncthreads();
    for (int f = tid; f < h; f += 256) A[f] = fft::merge_bin_conj(X[f], X[h - f], twn[f]);
    const float2* q = fft::forward(A, B, ph, twh, tid, 256);
    const float inv = 1.0f / (float)(2 * h);
    for (int m = tid; m < h; m += 256) {
        back[2 * m] = q[m].x * inv;
        back[2 * m + 1] = -q[m].y * inv;
    }
}

static std::vector<float2> twiddles(int n) {      // exp(-2 pi i m / n) from double angles, as every user of the header builds its table
    std::vector<float2> tw((size_t)n);
    for (int m = 0; m < n; ++m) {
        const double a = 2.0 * M_PI * (double)m / (double)n;
        tw[m] = make_float2((float)cos(a), (float)-sin(a));
    }
    return tw;
}

template <class T>
static T* upload(const std::vector<T>& v) {
    T* d = nullptr;
    CHECK_HIP(hipMalloc((void**)&d, v.size() * sizeof(T)));
    CHECK_HIP(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <class T>
static std::vector<T> download(const T* d, size_t n) {
    CHECK_HIP(hipDeviceSynchronize());
    std::vector<T> v(n);
    CHECK_HIP(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
}
static size_t words_differ(const float2* a, const float2* b, size_t n) {
    size_t d = 0;
    for (size_t i = 0; i < n; ++i) d += memcmp(&a[i], &b[i], sizeof(float2)) != 0;
    return d;
}

template <int N>
static void launch_static(const float2* in, float2* out, const float2* tw, int gt) {
    hipLaunchKernelGGL((k_static<N>), dim3(1), dim3(gt), 2 * N * sizeof(float2), (hipStream_t)0, in, out, tw);
}
template <int N>
static void launch_wave(const float2* in, float2* out, const float2* tw) {
    hipLaunchKernelGGL((k_wave<N>), dim3(1), dim3(64), N * sizeof(float2), (hipStream_t)0, in, out, tw);
}
#define FFT_UNIT_SIZES(M) M(512) M(400) M(2048) M(1920) M(64) M(60)

static int run_complex(int n) {
    fft::Plan p;
    if (!fft::make_plan(n, &p)) { printf("fft n=%d: make_plan refused the size -> FAIL\n", n); return 1; }
    int G = 8;
    while (G > 1 && (size_t)G * 2 * n * sizeof(float2) > kLdsMax) G /= 2;
    const int per = 256 / G;
    std::vector<float2> x((size_t)G * n);
    unsigned s = 4321u + 7u * (unsigned)n;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 32768.0f - 1.0f; };
    for (auto& v : x) { v.x = rnd(); v.y = rnd(); }
    // double DFT of input 0, double twiddles
    std::vector<double> c((size_t)n), sn((size_t)n), rr((size_t)n), ri((size_t)n);
    for (int m = 0; m < n; ++m) { c[m] = cos(2.0 * M_PI * m / n); sn[m] = -sin(2.0 * M_PI * m / n); }
    double ref_max = 0.0;
    for (int k = 0; k < n; ++k) {
        double ar = 0.0, ai = 0.0;
        int m = 0;
        for (int j = 0; j < n; ++j) {
            ar += (double)x[j].x * c[m] - (double)x[j].y * sn[m];
            ai += (double)x[j].x * sn[m] + (double)x[j].y * c[m];
            m += k;
            if (m >= n) m -= n;
        }
        rr[k] = ar; ri[k] = ai;
        ref_max = fmax(ref_max, fmax(fabs(ar), fabs(ai)));
    }
    const std::vector<float2> tw = twiddles(n);
    float2 *d_x = upload(x), *d_tw = upload(tw), *d_out = nullptr;
    CHECK_HIP(hipMalloc((void**)&d_out, x.size() * sizeof(float2)));
    CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_forward), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    int rc = 0;
    auto rel_err = [&](const float2* got) {
        double worst = 0.0;
        for (int k = 0; k < n; ++k) {
            const double dr = fabs((double)got[k].x - rr[k]), di = fabs((double)got[k].y - ri[k]);
            worst = (dr == dr && di == di) ? fmax(worst, fmax(dr, di)) : 1e30;
        }
        return worst / ref_max;
    };
    auto fill = [&]() { CHECK_HIP(hipMemset(d_out, 0xff, x.size() * sizeof(float2))); };
    // one group of 256 threads
    fill();
    hipLaunchKernelGGL(k_forward, dim3(1), dim3(256), 2 * (size_t)n * sizeof(float2), (hipStream_t)0, (const float2*)d_x, d_out, p, (const float2*)d_tw, 256);
    CHECK_HIP(hipGetLastError());
    const std::vector<float2> y256 = download(d_out, (size_t)n);
    const double e256 = rel_err(y256.data());
    // one group of 32 threads
    fill();
    hipLaunchKernelGGL(k_forward, dim3(1), dim3(32), 2 * (size_t)n * sizeof(float2), (hipStream_t)0, (const float2*)d_x, d_out, p, (const float2*)d_tw, 32);
    CHECK_HIP(hipGetLastError());
    const std::vector<float2> y32 = download(d_out, (size_t)n);
    const double e32 = rel_err(y32.data());
    const size_t d32 = words_differ(y32.data(), y256.data(), (size_t)n);       // (a butterfly's arithmetic does not depend on which thread runs it)
    // the G inputs one per workgroup (256 / G threads each), then side by side in one workgroup
    fill();
    hipLaunchKernelGGL(k_forward, dim3(G), dim3(per), 2 * (size_t)n * sizeof(float2), (hipStream_t)0, (const float2*)d_x, d_out, p, (const float2*)d_tw, per);
    CHECK_HIP(hipGetLastError());
    const std::vector<float2> single = download(d_out, x.size());
    fill();
    hipLaunchKernelGGL(k_forward, dim3(1), dim3(256), (size_t)G * 2 * n * sizeof(float2), (hipStream_t)0, (const float2*)d_x, d_out, p, (const float2*)d_tw, per);
    CHECK_HIP(hipGetLastError());
    const std::vector<float2> side = download(d_out, x.size());
    const size_t dside = words_differ(side.data(), single.data(), x.size()), d0 = words_differ(single.data(), y256.data(), (size_t)n);
    {
        const bool ok = e256 <= kTol && e32 <= kTol && d32 == 0 && dside == 0 && d0 == 0;
        printf("fft n=%d passes %d: forward vs double DFT %.3e (256 threads) %.3e (32 threads) (tol %.1e), 32 vs 256 threads %zu words differ, %d groups side by side vs alone %zu words differ -> %s\n",
               n, p.passes, e256, e32, kTol, d32 + d0, G, dside, ok ? "OK" : "FAIL");
        rc |= ok ? 0 : 1;
    }
    if (fft::static_size(n)) {
        size_t ds64 = 0, ds256 = 0, dw = 0;
#define FFT_UNIT_STATIC(NN)                                                                       \
        if (n == NN) {                                                                            \
            fill(); launch_static<NN>(d_x, d_out, d_tw, 64); CHECK_HIP(hipGetLastError());        \
            ds64 = words_differ(download(d_out, (size_t)n).data(), y256.data(), (size_t)n);       \
            fill(); launch_static<NN>(d_x, d_out, d_tw, 256); CHECK_HIP(hipGetLastError());       \
            ds256 = words_differ(download(d_out, (size_t)n).data(), y256.data(), (size_t)n);      \
            fill(); launch_wave<NN>(d_x, d_out, d_tw); CHECK_HIP(hipGetLastError());              \
            dw = words_differ(download(d_out, (size_t)n).data(), y256.data(), (size_t)n);         \
        }
        FFT_UNIT_SIZES(FFT_UNIT_STATIC)
#undef FFT_UNIT_STATIC
        const bool ok = ds64 == 0 && ds256 == 0 && dw == 0;
        printf("fft n=%d: forward_static vs forward %zu (64 threads) %zu (256 threads) words differ, forward_wave vs forward %zu words differ -> %s\n", n, ds64, ds256, dw,
               ok ? "OK" : "FAIL");
        rc |= ok ? 0 : 1;
    }
    CHECK_HIP(hipFree(d_x)); CHECK_HIP(hipFree(d_tw)); CHECK_HIP(hipFree(d_out));
    return rc;
}

static int run_real(int h) {
    const int n = 2 * h;
    fft::Plan ph;
    if (!fft::make_plan(h, &ph)) { printf("real h=%d: make_plan refused the size -> FAIL\n", h); return 1; }
    std::vector<float> x((size_t)n);
    unsigned s = 99u + 13u * (unsigned)h;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 32768.0f - 1.0f; };
    for (auto& v : x) v = rnd();
    std::vector<double> rr((size_t)h + 1), ri((size_t)h + 1);
    double ref_max = 0.0;
    for (int f = 0; f <= h; ++f) {
        double ar = 0.0, ai = 0.0;
        for (int j = 0; j < n; ++j) {
            const double a = 2.0 * M_PI * (double)(((long long)f * j) % n) / (double)n;
            ar += (double)x[j] * cos(a);
            ai -= (double)x[j] * sin(a);
        }
        rr[f] = ar; ri[f] = ai;
        ref_max = fmax(ref_max, fmax(fabs(ar), fabs(ai)));
    }
    const std::vector<float2> twh = twiddles(h), twn = twiddles(n);
    float* d_x = upload(x);
    float2 *d_twh = upload(twh), *d_twn = upload(twn), *d_spec = nullptr;
    float* d_back = nullptr;
    CHECK_HIP(hipMalloc((void**)&d_spec, ((size_t)h + 1) * sizeof(float2)));
    CHECK_HIP(hipMalloc((void**)&d_back, (size_t)n * sizeof(float)));
    CHECK_HIP(hipMemset(d_spec, 0xff, ((size_t)h + 1) * sizeof(float2)));
    CHECK_HIP(hipMemset(d_back, 0xff, (size_t)n * sizeof(float)));
    hipLaunchKernelGGL(k_real, dim3(1), dim3(256), (size_t)(3 * h + 1) * sizeof(float2), (hipStream_t)0, (const float*)d_x, d_spec, d_back, ph, (const float2*)d_twh,
                       (const float2*)d_twn);
    CHECK_HIP(hipGetLastError());
    const std::vector<float2> spec = download(d_spec, (size_t)h + 1);
    const std::vector<float> back = download(d_back, (size_t)n);
    double es = 0.0, eb = 0.0;
    for (int f = 0; f <= h; ++f) {
        const double dr = fabs((double)spec[f].x - rr[f]), di = fabs((double)spec[f].y - ri[f]);
        es = (dr == dr && di == di) ? fmax(es, fmax(dr, di)) : 1e30;
    }
    es /= ref_max;
    for (int j = 0; j < n; ++j) {
        const double d = fabs((double)back[j] - (double)x[j]);
        eb = d == d ? fmax(eb, d) : 1e30;
    }
    const bool ok = es <= kTol && eb <= kTol;
    printf("real h=%d (n=%d): forward + split_bin vs double real DFT %.3e, merge_bin_conj + forward vs the frame %.3e (tol %.1e) -> %s\n", h, n, es, eb, kTol, ok ? "OK" : "FAIL");
    CHECK_HIP(hipFree(d_x)); CHECK_HIP(hipFree(d_twh)); CHECK_HIP(hipFree(d_twn)); CHECK_HIP(hipFree(d_spec)); CHECK_HIP(hipFree(d_back));
    return ok ? 0 : 1;
}

static int run_plan() {      // host only
    int rc = 0, smooth = 0, most = 0, at_most = 0, refused_smooth = 0, accepted_other = 0, bad_product = 0;
    fft::Plan p;
    const int refuse[] = {7, 44, 1022, 8191, 1, 0, -1, -4};
    for (int n : refuse)
        if (fft::make_plan(n, &p)) { printf("plan: make_plan(%d) returned true -> FAIL\n", n); rc = 1; }
    for (int n = 2; n <= 8192; ++n) {
        int m = n;
        for (int q : {2, 3, 5}) while (m % q == 0) m /= q;
        const bool ok = fft::make_plan(n, &p);
        if (m != 1) { accepted_other += ok; continue; }
        ++smooth;
        if (!ok) { ++refused_smooth; continue; }
        long long prod = 1;
        bool radices = p.passes >= 1 && p.passes <= fft::kMaxPasses && p.n == n;
        for (int i = 0; i < p.passes && i < fft::kMaxPasses; ++i) {
            radices = radices && (p.radix[i] == 2 || p.radix[i] == 3 || p.radix[i] == 4 || p.radix[i] == 5);
            prod *= p.radix[i];
        }
        bad_product += !(radices && prod == n);
        if (p.passes > most) { most = p.passes; at_most = 0; }
        at_most += p.passes == most;
    }
    const bool ok = rc == 0 && refused_smooth == 0 && accepted_other == 0 && bad_product == 0 && most <= fft::kMaxPasses;
    printf("plan: %d 5-smooth sizes in [2, 8192]: %d refused, %d with a wrong radix product; %d other sizes accepted; most passes %d (%d sizes; kMaxPasses %d) -> %s\n", smooth,
           refused_smooth, bad_product, accepted_other, most, at_most, fft::kMaxPasses, ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}

int main(int argc, char** argv) {
    int rc = 0;
    if (argc < 2) return run_plan() | run_complex(60) | run_real(45);
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "plan")) rc |= run_plan();
        else if (argv[i][0] == 'r') rc |= run_real(atoi(argv[i] + 1));
        else rc |= run_complex(atoi(argv[i]));
        fflush(stdout);
    }
    return rc;
}
