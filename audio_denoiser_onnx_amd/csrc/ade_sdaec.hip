// ade_sdaec.hip — SDAEC (the ICCRN echo canceller with its alpha predictor) on the MI355X.
//
// Reference: SDAEC.forward (SDAEC/Export_SDAEC.py:382-444), NET.forward (:261-284), CFB (:65-96), CepsUnit (:99-125), CH_LSTM_F / CH_LSTM_T (:287-343) and the folder's
// STFT_Process (stft_B / istft_B, 319 / 319 / 160, periodic Hamming, constant centre pad, static window-square norm).  Two inputs per call -- channel 0 the near-end
// microphone, channel 1 the far-end reference (the export's input order, :501) -- and one output.  A call is n_win windows of L samples back to back (USE_BATCH_FOLD):
// every window is an independent clip with its own mean and zero LSTM states.  fp32 throughout.
//
// Every activation is (clip, frame, bin, channel) with the channel contiguous.  N = clips * frames.  The launch sequence of a call (88 launches whatever T and the batch):
//   front (7)   k_sd_mean; the analysis as a dense product with the reference's fp32-angle tables (319 is not 5-smooth); k_sd_power (frame powers); k_sd_feat (alpha = the
//               causal 10-tap 2-channel convolution of the powers, far spectrum * |alpha|, the 4 network inputs per bin); in_ch_lstm: input product, recurrence;
//               then in_fused (Linear on [h_fwd, h_bwd, x], :264-266) as a product                                                                        -> e0
//   CFB (7 each, ten of them)
//               k_sd_cfb: one workgroup per frame holds the (160, C_in) plane in LDS: LN0 -> gate Linear -> sigmoid, input Linear, g * x, LN1 -> 3-tap convolution
//                         along the bins (-> y), LN2(x - g x) (-> z); LayerNorm statistics are two-pass (mean, then the centred squares) in fp32
//               cepstral DFT: [162 x 160] table x z on the matrix cores -> (81, [re 20 | im 20]) per frame
//               k_sd_stats: mean / rstd of the (81, 40) plane;   the LSTM's input product with that LayerNorm applied in its loader;   k_sd_lstm<20>, both directions
//               Linear 40 -> 40 on the matrix cores;   inverse table [160 x 162]: the complex multiply (:122-123) in its loader, + y in its store       -> the block's output
//   middle (6)  k_sd_stats of e5; layer 0: input product (LayerNorm in the loader), k_sd_lstm<40> along time; layer 1 the same; Linear 40 -> 20 with e5 * (.) in its store
//   back (5)    out_ch_lstm: input product on [e0, d1], k_sd_lstm<20> along time; out_fused (Linear on [h, d1]) -> spectrum; the synthesis as a dense product; k_sd_ola
//
// THE RECURRENCES (k_sd_lstm<H>): every LSTM's W_ih x + b_ih + b_hh is hoisted out of its step loop and computed for all steps at once by csrc/ade_gemm.h; the store of
// that product lays the pre-activations out [direction][position][unit][gate i, f, g, o], so a lane fetches the four gates of one unit as one float4.  A wavefront
// owns 16 sequences.  The recurrent product of a step, gates(4 H x 16) += W_hh(4 H x H) h(H x 16), runs on v_mfma_f32_16x16x4_f32 (exact fp32) with the rows of W_hh
// permuted so that tile t, row 4 q + r is gate r of unit 4 t + q: lane (q = lane >> 4, j = lane & 15) then receives, in the four accumulator registers of tile t, the four
// gates of unit 4 t + q of sequence j -- and the B operand of k-step t of the NEXT step is h of unit 4 t + q of sequence j, which is what that lane has just computed.  h and
// c never leave their lanes, W_hh sits in registers for the whole sequence ((H / 4)^2 of them), nothing but the pre-activations is read and nothing but h is written inside
// the loop.  The reverse direction walks the steps from the last to the first; both start from zero at their own first element.
#include "ade_iccrn.h"
#include "../../include/ade.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace ade {

namespace {

constexpr int kAlphaK = 10;
constexpr int kCfbs = 10;

// ---- front (the mean, the analysis loaders and everything else the two ICCRN families share: csrc/ade_iccrn.h) ---------------------------------------------------
// one wavefront per (row, frame): sum of re^2 + im^2 over the 160 bins (:411)
__global__ __launch_bounds__(256) void k_sd_power(const float2* __restrict__ spec, float* __restrict__ power, int frames) {
    const int fr = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    float s = 0.0f;
    if (fr < frames)
        for (int f = lane; f < kF; f += 64) {
            const float2 v = spec[(size_t)fr * kF + f];
            s += v.x * v.x + v.y * v.y;
        }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (fr < frames && lane == 0) power[fr] = s;
}

// one thread per (clip, frame, bin): alpha[t] = bias + sum_k (w_mix[k] P_mix[t - 9 + k] + w_far[k] P_far[t - 9 + k]) with zeros before frame 0 (:416-418), the far
// spectrum * |alpha| (:420), the network's four inputs (mix re, mix im, far re, far im)
__global__ __launch_bounds__(256) void k_sd_feat(const float2* __restrict__ spec, const float* __restrict__ power, const float* __restrict__ aw, int T, long long total,
                                                 float4* __restrict__ feat, float* __restrict__ alpha) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int f = (int)(i % kF);
    const long long ct = i / kF;
    const int t = (int)(ct % T);
    const long long clip = ct / T;
    const float* pm = power + (size_t)clip * 2 * T;
    const float* pf = pm + T;
    float a = aw[2 * kAlphaK];
    for (int k = 0; k < kAlphaK; ++k) {
        const int u = t - (kAlphaK - 1) + k;
        if (u >= 0) a += aw[k] * pm[u] + aw[kAlphaK + k] * pf[u];
    }
    if (f == 0) alpha[ct] = a;
    const float2 m = spec[((size_t)clip * 2 * T + t) * kF + f], r = spec[((size_t)(clip * 2 + 1) * T + t) * kF + f];
    const float g = fabsf(a);
    feat[i] = make_float4(m.x, m.y, r.x * g, r.y * g);
}

}  // namespace

struct SdaecEngine : SubEngine {
    int device = 0, L = 0, n_win = 1, T = 0;
    float* d_w = nullptr;                       // one arena: weights, tables, norms
    std::map<std::string, size_t> off;          // tensor name -> float offset into the arena
    float eps_ln = 0.0f;
    struct Cfb { CfbW w; int cin; float ceps_eps; const float *ceps_w, *ceps_b, *w_ih, *w_hh, *bias, *lin_w, *lin_b; } cfb[kCfbs];
    const float *fwd = nullptr, *inv = nullptr, *inv_ws = nullptr, *alpha_w = nullptr, *ceps_dft = nullptr, *ceps_idft = nullptr;
    int capacity = 0;
    float* ws = nullptr;
    float *mean = nullptr, *spec = nullptr, *power = nullptr, *feat = nullptr, *alpha = nullptr, *xg = nullptr, *hbuf = nullptr, *e[6] = {}, *dbuf[2] = {}, *m5 = nullptr,
          *lstm_out = nullptr, *ybuf = nullptr, *zbuf = nullptr, *sp = nullptr, *lin = nullptr, *stats = nullptr, *spec_out = nullptr, *frames_buf = nullptr, *d1 = nullptr;
    int last_clips = 0;

    ~SdaecEngine() override {
        (void)hipSetDevice(device);
        if (d_w) (void)hipFree(d_w);
        if (ws) (void)hipFree(ws);
    }
    const float* at(const std::string& k) const { return d_w + off.at(k); }
    int frames() const override { return T; }
    int in_len() const override { return L * n_win; }
    int out_len() const override { return L * n_win; }
    int channels() const override { return 2; }          // near end, far end (Export_SDAEC.py:501)
    int out_channels() const override { return 1; }
    bool accepts_float_input() const override { return true; }
    int reserve(int batch, std::string& err) override;
    int run(hipStream_t s, const int16_t* d_in, int batch, int16_t* d_out, float* d_f32, std::string& err) override;
    int tap(hipStream_t s, const char* name, int batch, float* out, size_t count, size_t* written, std::string& err) override;
};

namespace {
int sfail(std::string& err, int st, const std::string& msg) { err = msg; return st; }
#define SD_HIP(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) return sfail(err, ADE_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)
const char* const kCfbNames[kCfbs] = {"e1", "e2", "e3", "e4", "e5", "d5", "d4", "d3", "d2", "d1"};
}  // namespace

int sdaec_create(const std::map<std::string, Tensor>& tensors, int window_len, int n_win, int device, SubEngine** out, std::string& err) {
    *out = nullptr;
    if (window_len < 2 * kHopS) return sfail(err, ADE_ERR_SHAPE_MISMATCH, "sdaec: input_audio_length shorter than two 160-sample hops");
    if (n_win < 1) return sfail(err, ADE_ERR_BAD_VALUE, "sdaec: no fold window");
    std::vector<float> arena;
    std::map<std::string, size_t> off;
    auto push = [&](size_t n) { const size_t o = arena.size(); arena.resize(o + ((n + 63) & ~(size_t)63), 0.0f); return o; };
    const Tensor* found = nullptr;
    auto want = [&](const std::string& name, std::vector<int> dims) -> int {
        auto it = tensors.find(name);
        if (it == tensors.end()) return sfail(err, ADE_ERR_MISSING_KEY, "weights: tensor missing: " + name);
        if (it->second.dims != dims) return sfail(err, ADE_ERR_SHAPE_MISMATCH, "weights: tensor has the wrong shape: " + name);
        found = &it->second;
        return ADE_OK;
    };
    auto copy = [&](const std::string& name, std::vector<int> dims) -> int {      // the tensor as it is
        const int st = want(name, dims);
        if (st != ADE_OK) return st;
        const size_t o = push(found->count);
        memcpy(&arena[o], found->data, found->count * sizeof(float));
        off[name] = o;
        return ADE_OK;
    };
    auto transposed = [&](const std::string& name, int rows, int cols) -> int {    // (rows, cols) -> [cols][rows]
        const int st = want(name, {rows, cols});
        if (st != ADE_OK) return st;
        const size_t o = push(found->count);
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) arena[o + (size_t)c * rows + r] = found->data[(size_t)r * cols + c];
        off[name + ".t"] = o;
        return ADE_OK;
    };
    // an LSTM's input side for XgStore: the stacked W_ih with row (dir, gate, unit) moved to (dir, unit, gate), and b_ih + b_hh in the same order
    auto lstm_in = [&](const std::string& prefix, const std::string& suffix, int dirs, int H, int K) -> int {
        std::vector<int> wd = dirs > 1 ? std::vector<int>{dirs, 4 * H, K} : std::vector<int>{4 * H, K};
        std::vector<int> bd = dirs > 1 ? std::vector<int>{dirs, 4 * H} : std::vector<int>{4 * H};
        int st = want(prefix + ".w_ih" + suffix, wd);
        if (st != ADE_OK) return st;
        const Tensor* wi = found;
        st = want(prefix + ".b_ih" + suffix, bd);
        if (st != ADE_OK) return st;
        const Tensor* bi = found;
        st = want(prefix + ".b_hh" + suffix, bd);
        if (st != ADE_OK) return st;
        const size_t ow = push(wi->count), ob = push(bi->count);
        for (int d = 0; d < dirs; ++d)
            for (int g = 0; g < 4; ++g)
                for (int u = 0; u < H; ++u) {
                    const size_t from = (size_t)d * 4 * H + g * H + u, to = (size_t)d * 4 * H + u * 4 + g;
                    memcpy(&arena[ow + to * K], wi->data + from * K, K * sizeof(float));
                    arena[ob + to] = bi->data[from] + found->data[from];
                }
        off[prefix + ".w_ih" + suffix] = ow;
        off[prefix + ".bias" + suffix] = ob;
        return ADE_OK;
    };
    auto eps_of = [&](const std::string& name, float* v) -> int {
        const int st = want(name, {1});
        if (st == ADE_OK) *v = found->data[0];
        return st;
    };
#define SD_TRY(expr) do { const int _st = (expr); if (_st != ADE_OK) return _st; } while (0)
    float eps[kCfbs][4], eps_ln = 0.0f;
    {   // alpha: [w_mix 10 | w_far 10 | bias]
        SD_TRY(want("alpha_kernel", {2, kAlphaK}));
        const size_t o = push(2 * kAlphaK + 1);
        memcpy(&arena[o], found->data, 2 * kAlphaK * sizeof(float));
        SD_TRY(want("alpha_bias", {1}));
        arena[o + 2 * kAlphaK] = found->data[0];
        off["alpha"] = o;
    }
    SD_TRY(lstm_in("in_lstm", "", 2, kC, 4));
    SD_TRY(copy("in_lstm.w_hh", {2, 4 * kC, kC}));
    SD_TRY(copy("in_fused_w", {kC, 2 * kC + 4}));
    SD_TRY(copy("in_fused_b", {kC}));
    for (int i = 0; i < kCfbs; ++i) {
        const std::string n = kCfbNames[i];
        const int cin = i >= 6 ? 2 * kC : kC;
        SD_TRY(copy(n + ".ln0_w", {kF, cin}));
        SD_TRY(copy(n + ".ln0_b", {kF, cin}));
        SD_TRY(copy(n + ".ln1_w", {kF, kC}));
        SD_TRY(copy(n + ".ln1_b", {kF, kC}));
        SD_TRY(copy(n + ".ln2_w", {kF, kC}));
        SD_TRY(copy(n + ".ln2_b", {kF, kC}));
        SD_TRY(copy(n + ".ceps_ln_w", {kCb, 2 * kC}));
        SD_TRY(copy(n + ".ceps_ln_b", {kCb, 2 * kC}));
        SD_TRY(eps_of(n + ".ln0_eps", &eps[i][0]));
        SD_TRY(eps_of(n + ".ln1_eps", &eps[i][1]));
        SD_TRY(eps_of(n + ".ln2_eps", &eps[i][2]));
        SD_TRY(eps_of(n + ".ceps_ln_eps", &eps[i][3]));
        SD_TRY(transposed(n + ".gate_w", kC, cin));
        SD_TRY(copy(n + ".gate_b", {kC}));
        SD_TRY(transposed(n + ".input_w", kC, cin));
        SD_TRY(copy(n + ".input_b", {kC}));
        {   // conv (out, in, tap) -> [tap][in][out]
            SD_TRY(want(n + ".conv_w", {kC, kC, 3}));
            const size_t o = push(3 * kC * kC);
            for (int oc = 0; oc < kC; ++oc)
                for (int ic = 0; ic < kC; ++ic)
                    for (int k = 0; k < 3; ++k) arena[o + ((size_t)k * kC + ic) * kC + oc] = found->data[((size_t)oc * kC + ic) * 3 + k];
            off[n + ".conv_w.t"] = o;
        }
        SD_TRY(copy(n + ".conv_b", {kC}));
        SD_TRY(lstm_in(n + ".lstm", "", 2, kC, 2 * kC));
        SD_TRY(copy(n + ".lstm.w_hh", {2, 4 * kC, kC}));
        SD_TRY(copy(n + ".lin_w", {2 * kC, 2 * kC}));
        SD_TRY(copy(n + ".lin_b", {2 * kC}));
    }
    SD_TRY(copy("ln_w", {kF, kC}));
    SD_TRY(copy("ln_b", {kF, kC}));
    SD_TRY(eps_of("ln_eps", &eps_ln));
    SD_TRY(lstm_in("t_lstm", "0", 1, 2 * kC, kC));
    SD_TRY(copy("t_lstm.w_hh0", {8 * kC, 2 * kC}));
    SD_TRY(lstm_in("t_lstm", "1", 1, 2 * kC, 2 * kC));
    SD_TRY(copy("t_lstm.w_hh1", {8 * kC, 2 * kC}));
    SD_TRY(copy("t_lin_w", {kC, 2 * kC}));
    SD_TRY(copy("t_lin_b", {kC}));
    SD_TRY(lstm_in("out_lstm", "", 1, kC, 2 * kC));
    SD_TRY(copy("out_lstm.w_hh", {4 * kC, kC}));
    SD_TRY(copy("out_fused_w", {2, 2 * kC}));
    SD_TRY(copy("out_fused_b", {2}));
    SD_TRY(copy("ceps_dft", {2 * kCb, kF}));
    SD_TRY(copy("ceps_idft", {kF, 2 * kCb}));
#undef SD_TRY

    const int T = (window_len - 1) / kHopS + 1;                    // STATIC_SIGNAL_LENGTH (:33)
    const size_t o_fwd = push((size_t)2 * kF * kN), o_inv = push((size_t)2 * kF * kFrameLd), o_iws = push(window_len);
    stft_tables(&arena[o_fwd], &arena[o_inv], &arena[o_iws], window_len, T);
    SdaecEngine* d = new SdaecEngine();
    d->device = device;
    d->L = window_len;
    d->n_win = n_win;
    d->T = T;
    d->off = off;
    d->eps_ln = eps_ln;
    auto bail = [&](int st) { delete d; return st; };
    if (hipSetDevice(device) != hipSuccess) return bail(sfail(err, ADE_ERR_DEVICE, "hipSetDevice failed"));
    if (hipMalloc((void**)&d->d_w, arena.size() * sizeof(float)) != hipSuccess) return bail(sfail(err, ADE_ERR_DEVICE, "hipMalloc of the SDAEC weights failed"));
    if (hipMemcpy(d->d_w, arena.data(), arena.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return bail(sfail(err, ADE_ERR_DEVICE, "upload of the SDAEC weights failed"));
    d->fwd = d->d_w + o_fwd;
    d->inv = d->d_w + o_inv;
    d->inv_ws = d->d_w + o_iws;
    d->alpha_w = d->at("alpha");
    d->ceps_dft = d->at("ceps_dft");
    d->ceps_idft = d->at("ceps_idft");
    for (int i = 0; i < kCfbs; ++i) {
        const std::string n = kCfbNames[i];
        auto& c = d->cfb[i];
        c.cin = i >= 6 ? 2 * kC : kC;
        c.w = CfbW{d->at(n + ".ln0_w"), d->at(n + ".ln0_b"), d->at(n + ".ln1_w"), d->at(n + ".ln1_b"), d->at(n + ".ln2_w"), d->at(n + ".ln2_b"),
                   d->at(n + ".gate_w.t"), d->at(n + ".gate_b"), d->at(n + ".input_w.t"), d->at(n + ".input_b"), d->at(n + ".conv_w.t"), d->at(n + ".conv_b"),
                   eps[i][0], eps[i][1], eps[i][2]};
        c.ceps_eps = eps[i][3];
        c.ceps_w = d->at(n + ".ceps_ln_w");
        c.ceps_b = d->at(n + ".ceps_ln_b");
        c.w_ih = d->at(n + ".lstm.w_ih");
        c.w_hh = d->at(n + ".lstm.w_hh");
        c.bias = d->at(n + ".lstm.bias");
        c.lin_w = d->at(n + ".lin_w");
        c.lin_b = d->at(n + ".lin_b");
    }
    static_assert(kCfbLds * sizeof(float) <= 64 * 1024, "the CFB kernel's planes fit the default dynamic LDS limit");
    *out = d;
    return ADE_OK;
}

int SdaecEngine::reserve(int calls, std::string& err) {
    if (calls <= capacity) return ADE_OK;
    if ((long long)calls * n_win * T * kF * 2 * kC > 0x7fffffffLL)                // the products' column indices and the kernels' element indices are 32-bit
        return sfail(err, ADE_ERR_BAD_VALUE, "sdaec: batch * frames too large for one call");
    SD_HIP(hipSetDevice(device));
    SD_HIP(hipDeviceSynchronize());
    if (ws) (void)hipFree(ws);
    ws = nullptr;
    capacity = 0;
    const size_t N = (size_t)calls * n_win, NT = N * T, P = NT * kF * kC;
    const size_t sizes[] = {N * 2, NT * 2 * kF * 2, NT * 2, NT * kF * 4, NT, NT * kF * 8 * kC /* xg: 160 gate rows per position */, NT * kF * 2 * kC,
                            P, P, P, P, P, P, P, P, P, P, P, P, NT * kCb * 2 * kC, NT * kCb * 2 * kC, NT * 2, NT * kF * 2, NT * kFrameLd};
    constexpr int kBufs = sizeof(sizes) / sizeof(sizes[0]);
    size_t total = 0;
    for (size_t s : sizes) total += (s + 63) & ~(size_t)63;
    SD_HIP(hipMalloc((void**)&ws, total * sizeof(float)));
    float* p[kBufs];
    size_t o = 0;
    for (int i = 0; i < kBufs; ++i) { p[i] = ws + o; o += (sizes[i] + 63) & ~(size_t)63; }
    mean = p[0]; spec = p[1]; power = p[2]; feat = p[3]; alpha = p[4]; xg = p[5]; hbuf = p[6];
    for (int i = 0; i < 6; ++i) e[i] = p[7 + i];
    dbuf[0] = p[13]; dbuf[1] = p[14]; m5 = p[15]; lstm_out = p[16]; ybuf = p[17]; zbuf = p[18];
    sp = p[19]; lin = p[20]; stats = p[21]; spec_out = p[22]; frames_buf = p[23];
    capacity = calls;
    return ADE_OK;
}

int SdaecEngine::run(hipStream_t s, const int16_t* d_in, int batch, int16_t* d_out, float* d_f32, std::string& err) {
    if (batch == 0) return ADE_OK;
    int st = reserve(batch, err);
    if (st != ADE_OK) return st;
    const int N = batch * n_win, NT = N * T, NP = NT * kF;          // clips, frames, positions
    float2* st2 = reinterpret_cast<float2*>(stats);
    // a bidirectional LSTM along `steps` bins of every frame: xg -> hbuf [frame][step][2 H]
    auto lstm_f = [&](const float* w_hh, int steps) {
        hipLaunchKernelGGL(k_sd_lstm<kC>, dim3((unsigned)((NT + 63) / 64), 2), dim3(256), 0, s, (const float*)xg, w_hh, NT, steps,
                           LstmGeo{hbuf, 1, 2 * kC, (size_t)steps, 0, 1, (size_t)NT * steps});
    };
    // an LSTM along time, one sequence per (clip, bin): xg -> out [clip][frame][bin][H]
    auto lstm_t20 = [&](const float* w_hh, float* out) {
        hipLaunchKernelGGL(k_sd_lstm<kC>, dim3((unsigned)((N * kF + 63) / 64), 1), dim3(256), 0, s, (const float*)xg, w_hh, N * kF, T,
                           LstmGeo{out, kF, kC, (size_t)T * kF, 1, (size_t)kF, (size_t)NP});
    };
    auto lstm_t40 = [&](const float* w_hh, float* out) {
        hipLaunchKernelGGL(k_sd_lstm<2 * kC>, dim3((unsigned)((N * kF + 63) / 64), 1), dim3(256), 0, s, (const float*)xg, w_hh, N * kF, T,
                           LstmGeo{out, kF, 2 * kC, (size_t)T * kF, 1, (size_t)kF, (size_t)NP});
    };
    // front
    hipLaunchKernelGGL(k_sd_mean, dim3((unsigned)(N * 2)), dim3(256), 0, s, d_in, float_in, L, n_win, mean);
    gemm::launch(s, gemm::RowMajorA{fwd, kN}, FrameB{d_in, float_in, mean, L, T, n_win}, SpecStore{spec}, 2 * kF, 2 * NT, kN);
    hipLaunchKernelGGL(k_sd_power, dim3((unsigned)((2 * NT + 3) / 4)), dim3(256), 0, s, reinterpret_cast<const float2*>(spec), power, 2 * NT);
    hipLaunchKernelGGL(k_sd_feat, grid1((long long)NP, 256), dim3(256), 0, s, reinterpret_cast<const float2*>(spec), (const float*)power, alpha_w, T, (long long)NP,
                       reinterpret_cast<float4*>(feat), alpha);
    gemm::launch(s, gemm::RowMajorA{feat, 4}, gemm::WeightNK{at("in_lstm.w_ih"), 4}, XgStore{xg, at("in_lstm.bias"), 4 * kC, (size_t)NP}, NP, 8 * kC, 4);
    lstm_f(at("in_lstm.w_hh"), kF);
    gemm::launch(s, gemm::RowMajorA{at("in_fused_w"), 2 * kC + 4}, Cat2B{hbuf, feat, 2 * kC, 4}, StoreNM{e[0], at("in_fused_b"), kC, nullptr, nullptr}, kC, NP, 2 * kC + 4);
    // one CFB: (xa | xb) -> out
    auto run_cfb = [&](int i, const float* xa, const float* xb, float* out) {
        const Cfb& c = cfb[i];
        if (c.cin == kC)
            hipLaunchKernelGGL(k_sd_cfb<kC>, dim3((unsigned)NT), dim3(256), kCfbLds * sizeof(float), s, xa, xb, c.w, ybuf, zbuf);
        else
            hipLaunchKernelGGL(k_sd_cfb<2 * kC>, dim3((unsigned)NT), dim3(256), kCfbLds * sizeof(float), s, xa, xb, c.w, ybuf, zbuf);
        gemm::launch(s, gemm::RowMajorA{ceps_dft, kF}, PlaneB{zbuf, kF}, CepsStore{sp}, 2 * kCb, NT * kC, kF);
        hipLaunchKernelGGL(k_sd_stats, dim3((unsigned)NT), dim3(256), 0, s, (const float*)sp, kCb * 2 * kC, c.ceps_eps, st2);
        gemm::launch(s, LnLoadA{sp, st2, c.ceps_w, c.ceps_b, kCb, 2 * kC}, gemm::WeightNK{c.w_ih, 2 * kC}, XgStore{xg, c.bias, 4 * kC, (size_t)NT * kCb}, NT * kCb, 8 * kC, 2 * kC);
        lstm_f(c.w_hh, kCb);
        gemm::launch(s, gemm::RowMajorA{c.lin_w, 2 * kC}, gemm::WeightNK{hbuf, 2 * kC}, StoreNM{lin, c.lin_b, 2 * kC, nullptr, nullptr}, 2 * kC, NT * kCb, 2 * kC);
        gemm::launch(s, gemm::RowMajorA{ceps_idft, 2 * kCb}, CepsMulB{lin, sp}, ResidualStore{out, ybuf}, kF, NT * kC, 2 * kCb);
    };
    for (int i = 0; i < 5; ++i) run_cfb(i, e[i], nullptr, e[i + 1]);
    // middle: ch_lstm(ln(e5)) (:272), two layers along time, Linear 40 -> 20, e5 * (.)
    hipLaunchKernelGGL(k_sd_stats, dim3((unsigned)NT), dim3(256), 0, s, (const float*)e[5], kF * kC, eps_ln, st2);
    gemm::launch(s, LnLoadA{e[5], st2, at("ln_w"), at("ln_b"), kF, kC}, gemm::WeightNK{at("t_lstm.w_ih0"), kC}, XgStore{xg, at("t_lstm.bias0"), 8 * kC, (size_t)NP}, NP, 8 * kC, kC);
    lstm_t40(at("t_lstm.w_hh0"), hbuf);
    gemm::launch(s, gemm::RowMajorA{hbuf, 2 * kC}, gemm::WeightNK{at("t_lstm.w_ih1"), 2 * kC}, XgStore{xg, at("t_lstm.bias1"), 8 * kC, (size_t)NP}, NP, 8 * kC, 2 * kC);
    lstm_t40(at("t_lstm.w_hh1"), hbuf);
    gemm::launch(s, gemm::RowMajorA{at("t_lin_w"), 2 * kC}, gemm::WeightNK{hbuf, 2 * kC}, StoreNM{lstm_out, at("t_lin_b"), kC, e[5], m5}, kC, NP, 2 * kC);
    // decoder (:273-277)
    run_cfb(5, m5, nullptr, dbuf[0]);
    run_cfb(6, e[4], dbuf[0], dbuf[1]);
    run_cfb(7, e[3], dbuf[1], dbuf[0]);
    run_cfb(8, e[2], dbuf[0], dbuf[1]);
    run_cfb(9, e[1], dbuf[1], dbuf[0]);
    d1 = dbuf[0];
    // back: out_ch_lstm on [e0, d1] along time, the fused output Linear on [h, d1] (:278-281), synthesis
    gemm::launch(s, Cat2A{e[0], d1, kC, kC}, gemm::WeightNK{at("out_lstm.w_ih"), 2 * kC}, XgStore{xg, at("out_lstm.bias"), 4 * kC, (size_t)NP}, NP, 4 * kC, 2 * kC);
    lstm_t20(at("out_lstm.w_hh"), hbuf);
    gemm::launch(s, gemm::RowMajorA{at("out_fused_w"), 2 * kC}, Cat2B{hbuf, d1, kC, kC}, StoreNM{spec_out, at("out_fused_b"), 2, nullptr, nullptr}, 2, NP, 2 * kC);
    gemm::launch(s, InvA{inv}, SpecOutB{spec_out}, FrameStore{frames_buf}, kN, NT, 2 * kF);
    const long long total = (long long)N * L;
    hipLaunchKernelGGL(k_sd_ola, grid1(total, 256), dim3(256), 0, s, (const float*)frames_buf, inv_ws, T, L, d_out, d_f32, total);
    SD_HIP(hipGetLastError());
    last_clips = N;
    return ADE_OK;
}

int SdaecEngine::tap(hipStream_t s, const char* name, int batch, float* out, size_t count, size_t* written, std::string& err) {
    if (!ws || batch <= 0 || batch > capacity || batch * n_win != last_clips) return sfail(err, ADE_ERR_NOT_FOUND, "tap has no data yet");
    const size_t NT = (size_t)batch * n_win * T;
    const float* src = nullptr;
    size_t n = 0;
    if (strcmp(name, "alpha") == 0) { src = alpha; n = NT; }                                   // [clip][frame]
    else if (strcmp(name, "e0") == 0) { src = e[0]; n = NT * kF * kC; }                        // [clip][frame][bin][channel]
    else if (strcmp(name, "e5") == 0) { src = e[5]; n = NT * kF * kC; }
    else if (strcmp(name, "lstm_out") == 0) { src = lstm_out; n = NT * kF * kC; }
    else if (strcmp(name, "d1") == 0) { src = d1; n = NT * kF * kC; }
    else if (strcmp(name, "spec_out") == 0) { src = spec_out; n = NT * kF * 2; }               // [clip][frame][bin] (re, im)
    else return sfail(err, ADE_ERR_NOT_FOUND, std::string("unknown tap: ") + name);
    if (count < n) return sfail(err, ADE_ERR_SHAPE_MISMATCH, "tap buffer too small");
    SD_HIP(hipStreamSynchronize(s));
    SD_HIP(hipMemcpy(out, src, n * sizeof(float), hipMemcpyDeviceToHost));
    *written = n;
    return ADE_OK;
}

}  // namespace ade
