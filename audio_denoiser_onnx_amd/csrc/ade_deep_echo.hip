// ade_deep_echo.hip — Deep Echo AEC (the ICCRN echo-path estimator) on the MI355X.
//
// Reference: DeepEchoAEC.forward (Deep_Echo_AEC/Export_Deep_Echo.py:372-426), NET.forward and NET.apply_echo_path (:303-342), CFB (:79-108), CepsUnit (:111-178),
// LayerNorm (:181-208), CH_LSTM_T / CH_LSTM_F (:217-268) and the folder's STFT_Process (stft_B / istft_B, 319 / 319 / 160, periodic Hamming, constant centre pad, static
// window-square norm).  Two inputs per call -- channel 0 the near-end microphone, channel 1 the far-end reference (the export's input order, :490) -- and one output.  A
// call is n_win windows of L samples back to back (USE_BATCH_FOLD): every window is an independent clip with its own mean, zero LSTM states and its own zero tap history.
// fp32 throughout.
//
// The network is SDAEC's building material (csrc/ade_iccrn.h) at a fifth of the depth -- two CFBs, no skip concatenations, no alpha predictor -- with another output
// stage: it does not emit a spectrum but a 10-tap complex echo path per bin and frame, and the output spectrum is mix - sum_k far[t - 9 + k] * path_k[t].
//
// Every activation is (clip, frame, bin, channel) with the channel contiguous.  N = clips * frames.  The launch sequence of a call (31 launches whatever T and the batch):
//   front (6)   k_sd_mean; the analysis as a dense product with the reference's fp32-angle tables; k_de_feat (the 4 network inputs per bin in the checkpoint's
//               complex-major order); in_ch_lstm: input product, recurrence; then in_fused (Linear on [h_fwd, h_bwd, x], :319-320) as a product               -> e0
//   cfb_e1 (7)  the seven launches of SDAEC's CFB (see csrc/ade_sdaec.hip), C_in = 20                                                                       -> e1
//   middle (6)  k_sd_stats of e1; layer 0: input product (LayerNorm in the loader), k_sd_lstm<40> along time; layer 1 the same; Linear 40 -> 20 with e1 * (.) in its store
//   cfb_d1 (7)  on e1 * lstm_out, with cfb_e1's cepstral tables (:316, :325-326)                                                                            -> d1
//   back (5)    out_ch_lstm: input product on [e0, d1], k_sd_lstm<20> along time; k_de_echo; the synthesis as a dense product; k_sd_ola
//
// THE OUTPUT STAGE (k_de_echo): one lane per (clip, frame, bin).  The lane's 40 inputs [h of out_ch_lstm | d1] are ten 16-byte loads (each half is 80 contiguous bytes);
// the 20 x 40 weights and 20 biases of out_ch_lstm.linear folded into out_conv are the same for every lane, so they are read at wave-uniform addresses (scalar loads
// through the constant cache, a 64-bit register pair per packed FMA) and never occupy a vector register; a path value is 20 packed FMAs on (even, odd) input pairs and
// one add of the two halves.  The ten far-end bins and the mix come straight from the analysis spectrum: a tap before the clip's frame 0 is skipped, not clamped, and the
// spectrum's rows are per clip, so frame 0 of a clip never sees the clip before it.  No LDS, no scratch.
#include "ade_iccrn.h"
#include "../../include/ade.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace ade {

namespace {

constexpr int kOrder = 10;                 // ECHO_ORDER (:37)
constexpr int kPath = 2 * kOrder;          // path values per position: [re taps | im taps] (the reshape at :340)
constexpr int kEchoIn = 2 * kC;

// one thread per (clip, frame, bin): the network's four inputs [near re, far re, near im, far im] (:398-401)
__global__ __launch_bounds__(256) void k_de_feat(const float2* __restrict__ spec, int T, long long total, float4* __restrict__ feat) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int f = (int)(i % kF);
    const long long ct = i / kF;
    const int t = (int)(ct % T);
    const long long clip = ct / T;
    const float2 m = spec[((size_t)clip * 2 * T + t) * kF + f], r = spec[((size_t)(clip * 2 + 1) * T + t) * kF + f];
    feat[i] = make_float4(m.x, r.x, m.y, r.y);
}

// one thread per (clip, frame, bin): path = W [h | d1] + b (:338-340), est = sum_k far[t - 9 + k] * (path[k] + i path[10 + k]) (:303-311), out = mix - est (:341).
// w: [20][40] row-major, b: [20]; h, d1: [position][20]; spec: [(clip, channel)][frame][bin] (re, im); path: [position][20]; out: [position] (re, im)
__global__ __launch_bounds__(256) void k_de_echo(const float4* __restrict__ h, const float4* __restrict__ d1, const float* __restrict__ w, const float* __restrict__ b,
                                                 const float2* __restrict__ spec, int T, long long total, float4* __restrict__ path, float2* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;                                          // lanes past the last position load and store nothing
    const int f = (int)(i % kF);
    const long long ct = i / kF;
    const int t = (int)(ct % T);
    const long long clip = ct / T;
    v2f x[kEchoIn / 2];
#pragma unroll
    for (int q = 0; q < kC / 4; ++q) {
        const float4 a = h[i * (kC / 4) + q], c = d1[i * (kC / 4) + q];
        x[2 * q] = mk2(a.x, a.y);
        x[2 * q + 1] = mk2(a.z, a.w);
        x[kC / 2 + 2 * q] = mk2(c.x, c.y);
        x[kC / 2 + 2 * q + 1] = mk2(c.z, c.w);
    }
    const cfptr cw = cptr(w), cb = cptr(b);
    float p[kPath];
#pragma unroll
    for (int c = 0; c < kPath; ++c) {
        const cfptr wr = cw + c * kEchoIn;                            // wave-uniform: the same row for every lane, a scalar register pair per packed FMA
        v2f acc = mk2(wr[0], wr[1]) * x[0];
#pragma unroll
        for (int j = 1; j < kEchoIn / 2; ++j) acc += mk2(wr[2 * j], wr[2 * j + 1]) * x[j];
        p[c] = (acc[0] + acc[1]) + cb[c];
    }
#pragma unroll
    for (int q = 0; q < kPath / 4; ++q) path[i * (kPath / 4) + q] = make_float4(p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]);
    const float2* far = spec + ((size_t)(clip * 2 + 1) * T) * kF + f;       // the clip's own far-end rows
    float er = 0.0f, ei = 0.0f;
#pragma unroll
    for (int k = 0; k < kOrder; ++k) {
        const int u = t - (kOrder - 1) + k;
        if (u < 0) continue;                                         // before the clip's frame 0: the delay bank's zero padding (:304)
        const float2 v = far[(size_t)u * kF];
        er += v.x * p[k] - v.y * p[kOrder + k];
        ei += v.x * p[kOrder + k] + v.y * p[k];
    }
    const float2 m = spec[((size_t)clip * 2 * T + t) * kF + f];
    out[i] = make_float2(m.x - er, m.y - ei);
}

}  // namespace

struct DeepEchoEngine : SubEngine {
    int device = 0, L = 0, n_win = 1, T = 0;
    float* d_w = nullptr;                       // one arena: weights, tables, norms
    std::map<std::string, size_t> off;          // tensor name -> float offset into the arena
    float eps_ln = 0.0f;
    struct Cfb { CfbW w; float ceps_eps; const float *ceps_w, *ceps_b, *w_ih, *w_hh, *bias, *lin_w, *lin_b; } cfb[2];
    const float *fwd = nullptr, *inv = nullptr, *inv_ws = nullptr, *ceps_dft = nullptr, *ceps_idft = nullptr;
    int capacity = 0;
    float* ws = nullptr;
    float *mean = nullptr, *spec = nullptr, *feat = nullptr, *xg = nullptr, *hbuf = nullptr, *e0 = nullptr, *e1 = nullptr, *m1 = nullptr, *lstm_out = nullptr, *d1 = nullptr,
          *ybuf = nullptr, *zbuf = nullptr, *sp = nullptr, *lin = nullptr, *stats = nullptr, *path = nullptr, *spec_out = nullptr, *frames_buf = nullptr;
    int last_clips = 0;

    ~DeepEchoEngine() override {
        (void)hipSetDevice(device);
        if (d_w) (void)hipFree(d_w);
        if (ws) (void)hipFree(ws);
    }
    const float* at(const std::string& k) const { return d_w + off.at(k); }
    int frames() const override { return T; }
    int in_len() const override { return L * n_win; }
    int out_len() const override { return L * n_win; }
    int channels() const override { return 2; }          // near end, far end (Export_Deep_Echo.py:490)
    int out_channels() const override { return 1; }
    bool accepts_float_input() const override { return true; }
    int reserve(int batch, std::string& err) override;
    int run(hipStream_t s, const int16_t* d_in, int batch, int16_t* d_out, float* d_f32, std::string& err) override;
    int tap(hipStream_t s, const char* name, int batch, float* out, size_t count, size_t* written, std::string& err) override;
};

namespace {
int dfail(std::string& err, int st, const std::string& msg) { err = msg; return st; }
#define DE_HIP(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) return dfail(err, ADE_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)
const char* const kDeCfbNames[2] = {"e1", "d1"};
}  // namespace

int deep_echo_create(const std::map<std::string, Tensor>& tensors, int window_len, int n_win, int device, SubEngine** out, std::string& err) {
    *out = nullptr;
    if (window_len < 2 * kHopS) return dfail(err, ADE_ERR_SHAPE_MISMATCH, "deep_echo: input_audio_length shorter than two 160-sample hops");
    if (n_win < 1) return dfail(err, ADE_ERR_BAD_VALUE, "deep_echo: no fold window");
    std::vector<float> arena;
    std::map<std::string, size_t> off;
    auto push = [&](size_t n) { const size_t o = arena.size(); arena.resize(o + ((n + 63) & ~(size_t)63), 0.0f); return o; };
    const Tensor* found = nullptr;
    auto want = [&](const std::string& name, std::vector<int> dims) -> int {
        auto it = tensors.find(name);
        if (it == tensors.end()) return dfail(err, ADE_ERR_MISSING_KEY, "weights: tensor missing: " + name);
        if (it->second.dims != dims) return dfail(err, ADE_ERR_SHAPE_MISMATCH, "weights: tensor has the wrong shape: " + name);
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
#define DE_TRY(expr) do { const int _st = (expr); if (_st != ADE_OK) return _st; } while (0)
    float eps[2][4], eps_ln = 0.0f;
    DE_TRY(lstm_in("in_lstm", "", 2, kC, 4));
    DE_TRY(copy("in_lstm.w_hh", {2, 4 * kC, kC}));
    DE_TRY(copy("in_fused_w", {kC, 2 * kC + 4}));
    DE_TRY(copy("in_fused_b", {kC}));
    for (int i = 0; i < 2; ++i) {
        const std::string n = kDeCfbNames[i];
        DE_TRY(copy(n + ".ln0_w", {kF, kC}));
        DE_TRY(copy(n + ".ln0_b", {kF, kC}));
        DE_TRY(copy(n + ".ln1_w", {kF, kC}));
        DE_TRY(copy(n + ".ln1_b", {kF, kC}));
        DE_TRY(copy(n + ".ln2_w", {kF, kC}));
        DE_TRY(copy(n + ".ln2_b", {kF, kC}));
        DE_TRY(copy(n + ".ceps_ln_w", {kCb, 2 * kC}));
        DE_TRY(copy(n + ".ceps_ln_b", {kCb, 2 * kC}));
        DE_TRY(eps_of(n + ".ln0_eps", &eps[i][0]));
        DE_TRY(eps_of(n + ".ln1_eps", &eps[i][1]));
        DE_TRY(eps_of(n + ".ln2_eps", &eps[i][2]));
        DE_TRY(eps_of(n + ".ceps_ln_eps", &eps[i][3]));
        DE_TRY(transposed(n + ".gate_w", kC, kC));
        DE_TRY(copy(n + ".gate_b", {kC}));
        DE_TRY(transposed(n + ".input_w", kC, kC));
        DE_TRY(copy(n + ".input_b", {kC}));
        {   // conv (out, in, tap) -> [tap][in][out]
            DE_TRY(want(n + ".conv_w", {kC, kC, 3}));
            const size_t o = push(3 * kC * kC);
            for (int oc = 0; oc < kC; ++oc)
                for (int ic = 0; ic < kC; ++ic)
                    for (int k = 0; k < 3; ++k) arena[o + ((size_t)k * kC + ic) * kC + oc] = found->data[((size_t)oc * kC + ic) * 3 + k];
            off[n + ".conv_w.t"] = o;
        }
        DE_TRY(copy(n + ".conv_b", {kC}));
        DE_TRY(lstm_in(n + ".lstm", "", 2, kC, 2 * kC));
        DE_TRY(copy(n + ".lstm.w_hh", {2, 4 * kC, kC}));
        DE_TRY(copy(n + ".lin_w", {2 * kC, 2 * kC}));
        DE_TRY(copy(n + ".lin_b", {2 * kC}));
    }
    DE_TRY(copy("ln_w", {kF, kC}));
    DE_TRY(copy("ln_b", {kF, kC}));
    DE_TRY(eps_of("ln_eps", &eps_ln));
    DE_TRY(lstm_in("t_lstm", "0", 1, 2 * kC, kC));
    DE_TRY(copy("t_lstm.w_hh0", {8 * kC, 2 * kC}));
    DE_TRY(lstm_in("t_lstm", "1", 1, 2 * kC, 2 * kC));
    DE_TRY(copy("t_lstm.w_hh1", {8 * kC, 2 * kC}));
    DE_TRY(copy("t_lin_w", {kC, 2 * kC}));
    DE_TRY(copy("t_lin_b", {kC}));
    DE_TRY(lstm_in("out_lstm", "", 1, kC, 2 * kC));
    DE_TRY(copy("out_lstm.w_hh", {4 * kC, kC}));
    DE_TRY(copy("echo_w", {kPath, kEchoIn}));
    DE_TRY(copy("echo_b", {kPath}));
    DE_TRY(copy("ceps_dft", {2 * kCb, kF}));
    DE_TRY(copy("ceps_idft", {kF, 2 * kCb}));
#undef DE_TRY

    const int T = (window_len - 1) / kHopS + 1;                    // MODEL_STFT_FRAMES (:49)
    // The folder's ISTFT is built with static_norm_divisor (:454): it DIVIDES the overlap-add by the window-square sum (STFT_Process.py:253-254, :305-306) where SDAEC's
    // multiplies by the stored reciprocal.  k_sd_ola multiplies by a table, so the table holds the correctly rounded fp32 reciprocals: s * fl(1 / w) lies within one
    // ulp of s / w (6e-8 relative), three orders of magnitude inside the family's waveform gate.
    const size_t o_fwd = push((size_t)2 * kF * kN), o_inv = push((size_t)2 * kF * kFrameLd), o_iws = push(window_len);
    stft_tables(&arena[o_fwd], &arena[o_inv], &arena[o_iws], window_len, T);
    DeepEchoEngine* d = new DeepEchoEngine();
    d->device = device;
    d->L = window_len;
    d->n_win = n_win;
    d->T = T;
    d->off = off;
    d->eps_ln = eps_ln;
    auto bail = [&](int st) { delete d; return st; };
    if (hipSetDevice(device) != hipSuccess) return bail(dfail(err, ADE_ERR_DEVICE, "hipSetDevice failed"));
    if (hipMalloc((void**)&d->d_w, arena.size() * sizeof(float)) != hipSuccess) return bail(dfail(err, ADE_ERR_DEVICE, "hipMalloc of the Deep Echo weights failed"));
    if (hipMemcpy(d->d_w, arena.data(), arena.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return bail(dfail(err, ADE_ERR_DEVICE, "upload of the Deep Echo weights failed"));
    d->fwd = d->d_w + o_fwd;
    d->inv = d->d_w + o_inv;
    d->inv_ws = d->d_w + o_iws;
    d->ceps_dft = d->at("ceps_dft");
    d->ceps_idft = d->at("ceps_idft");
    for (int i = 0; i < 2; ++i) {
        const std::string n = kDeCfbNames[i];
        auto& c = d->cfb[i];
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

int DeepEchoEngine::reserve(int calls, std::string& err) {
    if (calls <= capacity) return ADE_OK;
    if ((long long)calls * n_win * T * kF * 2 * kC > 0x7fffffffLL)                // the products' column indices and the kernels' element indices are 32-bit
        return dfail(err, ADE_ERR_BAD_VALUE, "deep_echo: batch * frames too large for one call");
    DE_HIP(hipSetDevice(device));
    DE_HIP(hipDeviceSynchronize());
    if (ws) (void)hipFree(ws);
    ws = nullptr;
    capacity = 0;
    const size_t N = (size_t)calls * n_win, NT = N * T, P = NT * kF * kC;
    const size_t sizes[] = {N * 2, NT * 2 * kF * 2, NT * kF * 4, NT * kF * 8 * kC /* xg: 160 gate rows per position */, NT * kF * 2 * kC,
                            P, P, P, P, P, P, P, NT * kCb * 2 * kC, NT * kCb * 2 * kC, NT * 2, P, NT * kF * 2, NT * kFrameLd};
    constexpr int kBufs = sizeof(sizes) / sizeof(sizes[0]);
    size_t total = 0;
    for (size_t s : sizes) total += (s + 63) & ~(size_t)63;
    DE_HIP(hipMalloc((void**)&ws, total * sizeof(float)));
    float* p[kBufs];
    size_t o = 0;
    for (int i = 0; i < kBufs; ++i) { p[i] = ws + o; o += (sizes[i] + 63) & ~(size_t)63; }
    mean = p[0]; spec = p[1]; feat = p[2]; xg = p[3]; hbuf = p[4];
    e0 = p[5]; e1 = p[6]; m1 = p[7]; lstm_out = p[8]; d1 = p[9]; ybuf = p[10]; zbuf = p[11];
    sp = p[12]; lin = p[13]; stats = p[14]; path = p[15]; spec_out = p[16]; frames_buf = p[17];
    capacity = calls;
    return ADE_OK;
}

int DeepEchoEngine::run(hipStream_t s, const int16_t* d_in, int batch, int16_t* d_out, float* d_f32, std::string& err) {
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
    hipLaunchKernelGGL(k_de_feat, grid1((long long)NP, 256), dim3(256), 0, s, reinterpret_cast<const float2*>(spec), T, (long long)NP, reinterpret_cast<float4*>(feat));
    gemm::launch(s, gemm::RowMajorA{feat, 4}, gemm::WeightNK{at("in_lstm.w_ih"), 4}, XgStore{xg, at("in_lstm.bias"), 4 * kC, (size_t)NP}, NP, 8 * kC, 4);
    lstm_f(at("in_lstm.w_hh"), kF);
    gemm::launch(s, gemm::RowMajorA{at("in_fused_w"), 2 * kC + 4}, Cat2B{hbuf, feat, 2 * kC, 4}, StoreNM{e0, at("in_fused_b"), kC, nullptr, nullptr}, kC, NP, 2 * kC + 4);
    // one CFB: x -> out (the seven launches of SDAEC's run_cfb, C_in = 20)
    auto run_cfb = [&](int i, const float* x, float* out) {
        const Cfb& c = cfb[i];
        hipLaunchKernelGGL(k_sd_cfb<kC>, dim3((unsigned)NT), dim3(256), kCfbLds * sizeof(float), s, x, (const float*)nullptr, c.w, ybuf, zbuf);
        gemm::launch(s, gemm::RowMajorA{ceps_dft, kF}, PlaneB{zbuf, kF}, CepsStore{sp}, 2 * kCb, NT * kC, kF);
        hipLaunchKernelGGL(k_sd_stats, dim3((unsigned)NT), dim3(256), 0, s, (const float*)sp, kCb * 2 * kC, c.ceps_eps, st2);
        gemm::launch(s, LnLoadA{sp, st2, c.ceps_w, c.ceps_b, kCb, 2 * kC}, gemm::WeightNK{c.w_ih, 2 * kC}, XgStore{xg, c.bias, 4 * kC, (size_t)NT * kCb}, NT * kCb, 8 * kC, 2 * kC);
        lstm_f(c.w_hh, kCb);
        gemm::launch(s, gemm::RowMajorA{c.lin_w, 2 * kC}, gemm::WeightNK{hbuf, 2 * kC}, StoreNM{lin, c.lin_b, 2 * kC, nullptr, nullptr}, 2 * kC, NT * kCb, 2 * kC);
        gemm::launch(s, gemm::RowMajorA{ceps_idft, 2 * kCb}, CepsMulB{lin, sp}, ResidualStore{out, ybuf}, kF, NT * kC, 2 * kCb);
    };
    run_cfb(0, e0, e1);
    // middle: ch_lstm(ln(e1)) (:329), two layers along time, Linear 40 -> 20, e1 * (.)
    hipLaunchKernelGGL(k_sd_stats, dim3((unsigned)NT), dim3(256), 0, s, (const float*)e1, kF * kC, eps_ln, st2);
    gemm::launch(s, LnLoadA{e1, st2, at("ln_w"), at("ln_b"), kF, kC}, gemm::WeightNK{at("t_lstm.w_ih0"), kC}, XgStore{xg, at("t_lstm.bias0"), 8 * kC, (size_t)NP}, NP, 8 * kC, kC);
    lstm_t40(at("t_lstm.w_hh0"), hbuf);
    gemm::launch(s, gemm::RowMajorA{hbuf, 2 * kC}, gemm::WeightNK{at("t_lstm.w_ih1"), 2 * kC}, XgStore{xg, at("t_lstm.bias1"), 8 * kC, (size_t)NP}, NP, 8 * kC, 2 * kC);
    lstm_t40(at("t_lstm.w_hh1"), hbuf);
    gemm::launch(s, gemm::RowMajorA{at("t_lin_w"), 2 * kC}, gemm::WeightNK{hbuf, 2 * kC}, StoreNM{lstm_out, at("t_lin_b"), kC, e1, m1}, kC, NP, 2 * kC);
    run_cfb(1, m1, d1);
    // back: out_ch_lstm on [e0, d1] along time (:338), the echo path and its application (:339-341), synthesis
    gemm::launch(s, Cat2A{e0, d1, kC, kC}, gemm::WeightNK{at("out_lstm.w_ih"), 2 * kC}, XgStore{xg, at("out_lstm.bias"), 4 * kC, (size_t)NP}, NP, 4 * kC, 2 * kC);
    lstm_t20(at("out_lstm.w_hh"), hbuf);
    hipLaunchKernelGGL(k_de_echo, grid1((long long)NP, 256), dim3(256), 0, s, reinterpret_cast<const float4*>(hbuf), reinterpret_cast<const float4*>(d1), at("echo_w"),
                       at("echo_b"), reinterpret_cast<const float2*>(spec), T, (long long)NP, reinterpret_cast<float4*>(path), reinterpret_cast<float2*>(spec_out));
    gemm::launch(s, InvA{inv}, SpecOutB{spec_out}, FrameStore{frames_buf}, kN, NT, 2 * kF);
    const long long total = (long long)N * L;
    hipLaunchKernelGGL(k_sd_ola, grid1(total, 256), dim3(256), 0, s, (const float*)frames_buf, inv_ws, T, L, d_out, d_f32, total);
    DE_HIP(hipGetLastError());
    last_clips = N;
    return ADE_OK;
}

int DeepEchoEngine::tap(hipStream_t s, const char* name, int batch, float* out, size_t count, size_t* written, std::string& err) {
    if (!ws || batch <= 0 || batch > capacity || batch * n_win != last_clips) return dfail(err, ADE_ERR_NOT_FOUND, "tap has no data yet");
    const size_t NT = (size_t)batch * n_win * T;
    const float* src = nullptr;
    size_t n = 0;
    if (strcmp(name, "e0") == 0) { src = e0; n = NT * kF * kC; }                               // [clip][frame][bin][channel]
    else if (strcmp(name, "e1") == 0) { src = e1; n = NT * kF * kC; }
    else if (strcmp(name, "lstm_out") == 0) { src = lstm_out; n = NT * kF * kC; }
    else if (strcmp(name, "d1") == 0) { src = d1; n = NT * kF * kC; }
    else if (strcmp(name, "path") == 0) { src = path; n = NT * kF * kPath; }                   // [clip][frame][bin][re taps 0 .. 9 | im taps 0 .. 9]
    else if (strcmp(name, "spec_out") == 0) { src = spec_out; n = NT * kF * 2; }               // [clip][frame][bin] (re, im)
    else return dfail(err, ADE_ERR_NOT_FOUND, std::string("unknown tap: ") + name);
    if (count < n) return dfail(err, ADE_ERR_SHAPE_MISMATCH, "tap buffer too small");
    DE_HIP(hipStreamSynchronize(s));
    DE_HIP(hipMemcpy(out, src, n * sizeof(float), hipMemcpyDeviceToHost));
    *written = n;
    return ADE_OK;
}

}  // namespace ade
