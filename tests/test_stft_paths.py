"""The generic STFT operator's three formulations (csrc/ade_stft.hip) on the device, each against a float64 numpy reference written here (independent of oracle/):

  run form    k_stft_run_analyze<N> / k_stft_run_synth<N, POLAR, TWL>: the compile-time sizes 512, 400, 2048, 1920, 64, 60 while the hop leaves the run inside the LDS budget
  plan form   k_stft_fft_analyze / k_stft_fft_synth<POLAR> on the run-time fft::Plan + k_stft_ola: every other 5-smooth size, and the static ones when ade_stft_create
              switches run_form off (small hops, ADE_STFT_RUN=0)
  dense form  gemm::launch with FrameB / SpecA / PolarSpecA + k_stft_ola: sizes with a prime factor above 5

tests/test_stft_process.py runs the models' own configurations, all of which take the run form; here every case states the branch it takes (`_dispatch` repeats the host
arithmetic of ade_stft_create / run_synth and every case asserts the branch it was written for).

Error metric: max |got - ref64| / max |ref64| for spectra, max |got - ref64| for waveforms (inputs uniform in [-1, 1]).  Gates: 1e-5 on the device (the operator's existing
gate), 5e-5 for an un-centred synthesis (the first / last hop divides by hamming's 0.08^2), 2e-6 / 3e-6 under the host simulator (test_stft_process.py's).  A polar
synthesis is compared with the float64 synthesis of mag cos(phase), mag sin(phase) of the SAME fp32 magnitudes and phases, so it has the rectangular gate.  No sample is masked:
every case asserts that the reference's overlap-added squared synthesis window is >= 1e-3 at every returned sample; only the keep_tail tail of a hann window goes below, and there
an absolute error e of the overlap-added numerator becomes e / w^2: allowed = gate x max(1, 1e-3 / w^2).

Worst figures measured on one MI355X, per form and size over that size's cases (every case prints its own as a `STFTPATH` line):

  form and n_fft / hop                          analysis synthesis     polar round trip
  plan 4/1                                       5.8e-08   1.2e-07   4.7e-07    6.0e-08
  plan 6/6                                       7.8e-08   6.3e-07   8.6e-07          -
  plan 45/9                                      1.2e-07   8.7e-07   8.4e-07    1.8e-07
  plan 250/100                                   1.4e-07   1.0e-06   1.4e-06    3.6e-07
  plan 256/64                                    1.6e-07   1.1e-06   1.2e-06    2.4e-07
  plan 480/160                                   1.3e-07   1.2e-06   1.1e-06    2.4e-07
  plan 729/243                                   1.6e-07   1.0e-06   1.2e-06    3.6e-07
  plan 1024/256                                  1.5e-07   1.4e-06   1.2e-06    2.4e-07
  plan 4096/1024                                 1.6e-07   1.5e-06   1.6e-06    3.0e-07
  plan 6561/2187                                 1.9e-07   2.0e-06   1.6e-06    4.8e-07
  plan 8192/4096                                 1.3e-07   1.6e-06   1.7e-06    4.2e-07
  plan, static size 512/16                       1.7e-07   3.5e-07   3.6e-07    3.6e-07
  plan, static size 2048/64                      1.4e-07   3.6e-07   4.4e-07    3.6e-07
  plan, static size 512/256 (ADE_STFT_RUN=0)     1.3e-07   2.3e-07   2.6e-07    3.0e-07
  plan, static size 400/100 (ADE_STFT_RUN=0)     1.1e-07   2.4e-07   2.4e-07    3.0e-07
  run 2048/512 (twiddles in global memory)       1.3e-07   2.4e-07   2.5e-07    3.0e-07
  run 1920/480 (twiddles in global memory)       1.0e-07   2.5e-07   2.3e-07    3.0e-07
  run 512/64                                     1.2e-07   2.4e-07   2.8e-07    3.0e-07
  run 64/32                                      1.0e-07   2.0e-07   1.9e-07    2.4e-07
  run 60/15                                      1.2e-07   3.0e-07   2.5e-07    2.4e-07
  dense 44/11                                    2.2e-07   2.9e-07   4.1e-07    1.8e-07
  dense 1001/250                                 1.3e-06   2.4e-06   2.3e-06    1.1e-06
  dense 1022/511                                 1.1e-06   2.1e-06   2.0e-06    2.2e-06
  windows / tail, plan 250/100                   1.4e-07   1.6e-06   1.0e-06          -
  windows / tail, dense 44/11                    1.6e-07   5.2e-07   5.6e-07          -
  shortest input, stream, batches, plan 250/100  1.3e-07   3.5e-07         -          -
  shortest input, stream, batches, dense 44/11   2.2e-07   1.9e-07         -          -

The plan and run forms stay at or below the simulator's 2e-6 everywhere; their largest synthesis figures (1e-6 to 2e-6) are the single-frame un-centred cases and the kept
tails, where one frame alone is divided by hamming's squared ends (down to 0.0064: a frame error of 1e-8 shows as 1.6e-6).  Only the dense form at n_fft ~ 1000 goes
above 2e-6 (2.4e-6): each of its outputs is an fp32 MFMA sum of K = 1001 .. 1024 products, whose round-off grows with sqrt(K) to K where an FFT's grows with log K.
"""
import ctypes as C
import ctypes.util
import functools
import os

import numpy as np
import pytest

from ade_testlib import GOLD, hipsim_library
from audio_denoiser_onnx_amd import _lib

GATE_GPU = dict(spec=1e-5, wave=1e-5, wave_uncentred=5e-5)
GATE_SIM = dict(spec=2e-6, wave=3e-6, wave_uncentred=5e-5)
DEN_MIN = 1e-3


# ---- the float64 reference -------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cosf():
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.cosf.restype, m.cosf.argtypes = C.c_float, [C.c_float]
    return m.cosf


@functools.lru_cache(maxsize=None)
def ref_window(name, win_length, n_fft):
    """make_window's values: fp32 cosf of an fp32 step (the C library's cosf, as the operator's host code calls it), centre pad / crop to n_fft; promoted to float64.
    The window is an input of the transform under test, not part of it."""
    sym = name.endswith("_sym")
    base = name[:-4] if sym else name
    if base == "hamming_periodic":
        base = "hamming"
    alpha, beta = {"hann": (0.5, 0.5), "hann_sqrt": (0.5, 0.5), "hamming": (0.54, 0.46)}[base]
    alpha, beta = np.float32(alpha), np.float32(beta)
    step = np.float32(2.0 * np.pi / float(win_length - 1 if sym else win_length))
    raw = np.empty(win_length, np.float32)
    cosf = _cosf()
    for n in range(win_length):
        v = np.float32(cosf(np.float32(n) * step)) * (-beta) + alpha
        raw[n] = np.sqrt(v) if base == "hann_sqrt" else v
    w = np.zeros(n_fft, np.float32)
    if win_length <= n_fft:
        left = (n_fft - win_length) // 2
        w[left:left + win_length] = raw
    else:
        start = (win_length - n_fft) // 2
        w[:] = raw[start:start + n_fft]
    return w.astype(np.float64)


def ref_stft(x, n_fft, hop, wa, center, pad_mode):
    """(B, L) -> (B, 2F, T) float64, real rows then imaginary rows."""
    x = np.asarray(x, np.float64)
    if center:
        x = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect" if pad_mode == "reflect" else "constant")
    T = (x.shape[1] - n_fft) // hop + 1
    frames = np.stack([x[:, t * hop:t * hop + n_fft] for t in range(T)], axis=1) * wa          # (B, T, N)
    Z = np.fft.rfft(frames, axis=2).transpose(0, 2, 1)                                              # (B, F, T)
    return np.concatenate([Z.real, Z.imag], axis=1)


def ref_istft(spec, n_fft, hop, ws, center, keep_tail=False):
    """(B, 2F, T) -> (waveform (B, n) float64, overlap-added squared window at the same n samples)."""
    spec = np.asarray(spec, np.float64)
    B, F2, T = spec.shape
    F = F2 // 2
    Z = (spec[:, :F] + 1j * spec[:, F:]).transpose(0, 2, 1).copy()                                  # (B, T, F)
    Z[:, :, 0] = Z[:, :, 0].real                                                                    # the imaginary parts of DC and Nyquist do not contribute
    if n_fft % 2 == 0:
        Z[:, :, F - 1] = Z[:, :, F - 1].real
    frames = np.fft.irfft(Z, n=n_fft, axis=2) * ws
    raw = n_fft + hop * (T - 1)
    y, den = np.zeros((B, raw)), np.zeros(raw)
    for t in range(T):
        y[:, t * hop:t * hop + n_fft] += frames[:, t]
        den[t * hop:t * hop + n_fft] += ws * ws
    if center:
        start, n = n_fft // 2, raw - (n_fft // 2 if keep_tail else n_fft)
    else:
        start, n = 0, raw
    den = den[start:start + n]
    with np.errstate(divide="ignore", invalid="ignore"):
        return y[:, start:start + n] / den, den


def _dispatch(n_fft, hop, frames=None, run_env=True):
    """The branch ade_stft_create picks, from its host arithmetic: ("dense", None), ("plan", pairs per workgroup) or ("run", whether run_synth copies the twiddles into LDS)."""
    m = n_fft
    for q in (2, 3, 5):
        while m % q == 0:
            m //= q
    if m != 1:
        return "dense", None
    if n_fft in (512, 400, 2048, 1920, 64, 60) and run_env:
        gt = 64 if n_fft <= 512 else (256 if n_fft // 4 <= 256 else 512)
        groups, budget = 512 // gt, 150 * 1024
        fixed = 0 if gt == 64 else groups * n_fft * 8
        halo = (n_fft + hop - 1) // hop - 1
        rpa, rps = max(groups, 2), groups
        while 2 * rps < 4 * halo:
            rps *= 2
        if not (rpa * (n_fft + 1) * 8 + fixed + n_fft * 8 > budget or rps * (n_fft + 1) * 8 + fixed > budget or 2 * rps <= halo):
            twl = None
            if frames is not None:
                rp, pairs = rps, (frames + halo + 1) // 2
                while rp // 2 >= pairs and rp // 2 >= groups:
                    rp //= 2
                twl = rp * (n_fft + 1) * 8 + fixed + n_fft * 8 <= budget
            return "run", twl
    G = 1
    while G < 8 and 2 * G * n_fft <= 4096:
        G *= 2
    return "plan", G


def _rel(got, ref):
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _wave(got, ref, den, gate):
    """(worst error where the window sum is >= DEN_MIN, worst error / allowance over all samples); allowance = gate x max(1, DEN_MIN / den)."""
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = np.abs(got - ref)
    body = den >= DEN_MIN
    return float(err[:, body].max()), float((err / (gate * np.maximum(1.0, DEN_MIN / den))).max())


def _report(tag, **figs):
    print("STFTPATH " + tag + " " + " ".join(f"{k}={v:.3e}" for k, v in figs.items()))


def _synthesis_input(ref, n_fft):
    """The reference spectrum in fp32 with IMAGINARY parts put on the DC and Nyquist bins: an inverse real transform ignores them (the reference's inverse table has zero
    sine rows there), so the operator has to as well -- a real signal's own spectrum, whose values there are zero, would not show whether it does."""
    spec = ref.astype(np.float32)
    F = spec.shape[1] // 2
    rng = np.random.default_rng(n_fft)
    scale = 0.5 * float(np.abs(spec).max())
    spec[:, F] = rng.uniform(-scale, scale, spec[:, F].shape)
    if n_fft % 2 == 0:
        spec[:, 2 * F - 1] = rng.uniform(-scale, scale, spec[:, F].shape)
    return spec


def _polar(spec32):
    F = spec32.shape[1] // 2
    mag = np.ascontiguousarray(np.hypot(spec32[:, :F], spec32[:, F:]))
    ph = np.ascontiguousarray(np.arctan2(spec32[:, F:], spec32[:, :F]))
    m64, p64 = mag.astype(np.float64), ph.astype(np.float64)
    return mag, ph, np.concatenate([m64 * np.cos(p64), m64 * np.sin(p64)], axis=1)


# ---- device memory: host arrays under the simulator, torch tensors on the GPU -------------------------------------------------------------------------------------------------
class _SimMem:
    gate = GATE_SIM

    def __init__(self):
        self.lib = hipsim_library()

    def put(self, a):
        return np.ascontiguousarray(a, np.float32)

    def empty(self, shape):
        return np.full(shape, np.nan, np.float32)

    def ptr(self, a):
        return a.ctypes.data

    def get(self, a):
        return a


class _GpuMem:
    gate = GATE_GPU

    def __init__(self):
        self.lib = _lib.get_library()

    def put(self, a):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
        torch.cuda.synchronize()
        return t

    def empty(self, shape):
        import torch
        t = torch.full(tuple(shape), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()               # (the operator runs on a non-blocking stream of its own)
        return t

    def ptr(self, a):
        return C.c_void_p(a.data_ptr())

    def get(self, a):
        return a.cpu().numpy()


class _Op:
    """One ade_stft handle; every status code is checked, no result is read after a non-zero one."""

    def __init__(self, mem, n_fft, hop, win_length=None, window="hamming", synthesis_window=None, center=True, pad="reflect", keep_tail=False):
        self.mem, self.c = mem, mem.lib.c
        self.n_fft, self.hop, self.center, self.pad, self.keep_tail = n_fft, hop, center, pad, keep_tail
        win_length = win_length or n_fft
        self.wa = ref_window(window, win_length, n_fft)
        self.ws = ref_window(synthesis_window or window, win_length, n_fft)
        cfg = _lib.StftConfig(n_fft, win_length, hop, window.encode(), synthesis_window.encode() if synthesis_window else None, int(center), pad.encode())
        self.h, self.keep = C.c_void_p(), []
        st = self.c.ade_stft_create(C.byref(cfg), 0, C.byref(self.h))
        assert st == _lib.ADE_OK, self.c.ade_stft_last_error(None)
        if keep_tail:
            self.ok(self.c.ade_stft_keep_tail(self.h, 1))

    def ok(self, st):
        assert st == _lib.ADE_OK, (st, self.c.ade_stft_last_error(self.h))

    def close(self):
        if self.h:
            self.c.ade_stft_destroy(self.h)
            self.h = C.c_void_p()

    def length_for(self, frames):
        return (frames - 1) * self.hop + self.n_fft - (2 * (self.n_fft // 2) if self.center else 0) + self.hop // 2

    def frames(self, length):
        t = C.c_int()
        self.ok(self.c.ade_stft_frames(self.h, length, C.byref(t)))
        return t.value

    def analyze(self, x, stream=None):
        m = self.mem
        d_x, d_s = m.put(x), m.empty((x.shape[0], 2 * (self.n_fft // 2 + 1), self.frames(x.shape[1])))
        self.keep.append(d_x)                  # (with a caller's stream the call returns before the kernels ran: the input must outlive this function)
        self.ok(self.c.ade_stft_analyze(self.h, m.ptr(d_x), x.shape[0], x.shape[1], m.ptr(d_s), stream))
        return d_s

    def out_len(self, frames):
        n = C.c_int()
        self.ok(self.c.ade_stft_output_length(self.h, frames, C.byref(n)))
        return n.value

    def synthesize(self, spec, stream=None):
        """spec: a host array (uploaded) or device memory from analyze()"""
        m = self.mem
        d_s = m.put(spec) if isinstance(spec, np.ndarray) else spec
        B, T = int(d_s.shape[0]), int(d_s.shape[2])
        d_y = m.empty((B, self.out_len(T)))
        self.keep.append(d_s)
        self.ok(self.c.ade_stft_synthesize(self.h, m.ptr(d_s), B, T, m.ptr(d_y), stream))
        return d_y

    def synthesize_polar(self, mag, ph):
        m = self.mem
        d_m, d_p = m.put(mag), m.put(ph)
        d_y = m.empty((mag.shape[0], self.out_len(mag.shape[2])))
        self.ok(self.c.ade_stft_synthesize_polar(self.h, m.ptr(d_m), m.ptr(d_p), mag.shape[0], mag.shape[2], m.ptr(d_y), None))
        return d_y

    def ref_analysis(self, x):
        return ref_stft(x, self.n_fft, self.hop, self.wa, self.center, self.pad)

    def ref_synthesis(self, spec):
        return ref_istft(spec, self.n_fft, self.hop, self.ws, self.center, self.keep_tail)


def _signal(seed, batch, length):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (batch, length)).astype(np.float32)


def _check_operator(mem, tag, n_fft, hop, frames, batch=3, roundtrip=False, **cfg):
    """Analysis, synthesis and polar synthesis of one configuration through the ctypes entry points."""
    op = _Op(mem, n_fft, hop, **cfg)
    try:
        gate = mem.gate
        wave_gate = gate["wave"] if op.center else gate["wave_uncentred"]
        L = op.length_for(frames)
        x = _signal(n_fft * 131 + hop, batch, L)
        assert op.frames(L) == frames
        ref = op.ref_analysis(x)
        d_spec = op.analyze(x)
        ea = _rel(mem.get(d_spec), ref)
        spec32 = _synthesis_input(ref, n_fft)
        want, den = op.ref_synthesis(spec32)
        static = want.shape[1] if not op.keep_tail else hop * (frames - 1)
        assert den[:static].min() >= DEN_MIN               # no returned sample depends on a vanishing window sum (bar the keep_tail tail)
        es, rs = _wave(mem.get(op.synthesize(spec32)), want, den, wave_gate)
        mag, ph, rect = _polar(spec32)
        want_p, _ = op.ref_synthesis(rect)
        ep, rp = _wave(mem.get(op.synthesize_polar(mag, ph)), want_p, den, wave_gate)
        figs = dict(analysis=ea, synthesis=es, polar=ep)
        if roundtrip:                                      # the operator's own spectrum back: wa = ws, every sample of the input inside full overlap
            assert op.center and 2 * hop <= n_fft and op.wa is op.ws
            y = mem.get(op.synthesize(d_spec))
            n = min(L, y.shape[1])
            figs["roundtrip"], rr = _wave(y[:, :n], x[:, :n].astype(np.float64), den[:n], wave_gate)
            assert rr <= 1.0, figs
        _report(tag, **figs)
        assert ea <= gate["spec"] and rs <= 1.0 and rp <= 1.0, figs
    finally:
        op.close()


# ---- the reference against the project's oracle -------------------------------------------------------------------------------------------------------------------------------
def test_reference_agrees_with_the_oracle():
    """ZipEnhancer's 400 / 100 hann (test_hipsim_generic_stft_small's case): this file's float64 reference and oracle_stft / oracle_istft with exact tables agree within
    2e-6, the gate that test holds the operator to against the oracle (the oracle multiplies fp32 tables -- cos x window / N rounded to fp32 -- and returns fp32)."""
    from oracle_lib import oracle_istft, oracle_set_generic_exact_dft, oracle_stft
    g = np.load(os.path.join(GOLD, "stft_zipenhancer.npz"))
    x = np.ascontiguousarray(g["x"][:, :1300])
    n_fft, win, hop = int(g["n_fft"]), int(g["win_length"]), int(g["hop"])
    w = ref_window("hann", win, n_fft)
    oracle_set_generic_exact_dft(True)
    try:
        o_spec = oracle_stft(x, n_fft, win, hop, "hann", True, "reflect")
        o_y = oracle_istft(o_spec, n_fft, win, hop, "hann", True)
    finally:
        oracle_set_generic_exact_dft(False)
    ref = ref_stft(x, n_fft, hop, w, True, "reflect")
    y, den = ref_istft(o_spec, n_fft, hop, w, True)
    e_spec, e_y = _rel(o_spec.astype(np.float64), ref), float(np.abs(o_y - y).max())
    _report("reference-vs-oracle", spectrum=e_spec, waveform=e_y)
    assert den.min() >= DEN_MIN and e_spec <= 2e-6 and e_y <= 2e-6


# ---- plan form ----------------------------------------------------------------------------------------------------------------------------------------------------------------------
# 5-smooth sizes that are none of the compile-time ones: make_plan succeeds, static_size() is false -> k_stft_fft_analyze / k_stft_fft_synth<POLAR> + k_stft_ola with
# G = pairs_per_group frame pairs of 256 / G threads per workgroup (8 up to 512 points, 4 up to 1024, 2 up to 2048, then 1).
PLAN_SIZES = [(4, 1),          # minimum size, 8 pairs of 32 threads (one butterfly per pass), hop 1
              (6, 6),          # hop = n_fft, no overlap
              (45, 9),         # odd, no Nyquist bin
              (250, 100),      # hop does not divide n_fft
              (256, 64),       # 8 pairs per workgroup
              (480, 160),
              (729, 243),      # odd, radix 3 only
              (1024, 256),     # 4 pairs
              (4096, 1024),    # 1 pair
              (6561, 2187),    # eight passes
              (8192, 4096)]    # 128 KB of LDS: the limit ade_stft_create raises the kernels to


def _plan_variants(sizes):
    out = []
    for n_fft, hop in sizes:
        G = _dispatch(n_fft, hop)[1]
        # an odd frame count (the last pair half empty, idle pair groups when G > 3), reflection padding, and the operator's own spectrum back where frames overlap fully
        out.append(pytest.param(n_fft, hop, 5, dict(roundtrip=2 * hop <= n_fft), id=f"{n_fft}/{hop}-5frames"))
        # a single frame, no centre padding
        out.append(pytest.param(n_fft, hop, 1, dict(center=False), id=f"{n_fft}/{hop}-1frame-uncentred"))
        # more than 2 G frames: a row spans several workgroups, the last one with idle pair groups; zero padding; the dynamic-length trim
        out.append(pytest.param(n_fft, hop, 2 * G + 3, dict(pad="constant", keep_tail=True), id=f"{n_fft}/{hop}-{2 * G + 3}frames-zeros-tail"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,hop,frames,cfg", _plan_variants(PLAN_SIZES))
def test_gpu_plan_form(n_fft, hop, frames, cfg):
    assert _dispatch(n_fft, hop)[0] == "plan"
    _check_operator(_GpuMem(), f"plan {n_fft}/{hop} T={frames}", n_fft, hop, frames, **cfg)


@pytest.mark.hipsim
@pytest.mark.parametrize("n_fft,hop,frames,cfg", _plan_variants([(4, 1), (6, 6), (250, 100)]))
def test_hipsim_plan_form(n_fft, hop, frames, cfg):
    assert _dispatch(n_fft, hop)[0] == "plan"
    _check_operator(_SimMem(), f"sim plan {n_fft}/{hop} T={frames}", n_fft, hop, frames, **cfg)


def _check_process(tag, n_fft, hop, frames):
    """The same three checks through STFT_Process (hamming, centre padding, reflection) plus the round trip."""
    import torch
    from audio_denoiser_onnx_amd.stft_process import STFT_Process
    gate = GATE_GPU
    L = (frames - 1) * hop + hop // 2
    x = _signal(n_fft * 7 + hop, 3, L)
    w = ref_window("hamming", n_fft, n_fft)
    ref = ref_stft(x, n_fft, hop, w, True, "reflect")
    assert ref.shape[2] == frames
    stft = STFT_Process("stft_B", n_fft, n_fft, hop, 0, "hamming", True, "reflect")
    spec = stft(torch.from_numpy(x).cuda()[:, None, :])
    ea = _rel(spec.cpu().numpy(), ref)
    spec32 = _synthesis_input(ref, n_fft)
    want, den = ref_istft(spec32, n_fft, hop, w, True)
    assert den.min() >= DEN_MIN
    istft = STFT_Process("istft_B", n_fft, n_fft, hop, frames, "hamming", True, "reflect")
    es, rs = _wave(istft(torch.from_numpy(spec32).cuda()).cpu().numpy().reshape(3, -1), want, den, gate["wave"])
    mag, ph, rect = _polar(spec32)
    want_p, _ = ref_istft(rect, n_fft, hop, w, True)
    polar = STFT_Process("istft_A", n_fft, n_fft, hop, frames, "hamming", True, "reflect")
    ep, rp = _wave(polar(torch.from_numpy(mag).cuda(), torch.from_numpy(ph).cuda()).cpu().numpy().reshape(3, -1), want_p, den, gate["wave"])
    y = istft(spec).cpu().numpy().reshape(3, -1)
    n = min(L, y.shape[1])
    er, rr = _wave(y[:, :n], x[:, :n].astype(np.float64), den[:n], gate["wave"])
    _report(tag, analysis=ea, synthesis=es, polar=ep, roundtrip=er)
    assert ea <= gate["spec"] and rs <= 1.0 and rp <= 1.0 and rr <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,hop,frames,run_env", [
    # 512 / 16: halo = 31 frames, so the synthesis run doubles from 8 pairs until 2 rps >= 4 halo -> 64 pairs x 513 x 8 bytes = 263 KB > the 150 KB budget: run_form off
    (512, 16, 37, True),
    # 2048 / 64: halo = 31, one thread group of 512 -> 64 pairs x 2049 x 8 bytes = 1 MB: run_form off.  19 frames: reflection needs more than 1024 samples
    (2048, 64, 19, True),
    # the models' own hops with ADE_STFT_RUN=0: the run form is switched off by hand
    (512, 256, 7, False),
    (400, 100, 7, False)])
def test_gpu_plan_form_at_static_sizes(n_fft, hop, frames, run_env, monkeypatch):
    if not run_env:
        monkeypatch.setenv("ADE_STFT_RUN", "0")            # read by ade_stft_create
    else:
        monkeypatch.delenv("ADE_STFT_RUN", raising=False)
    monkeypatch.delenv("ADE_STFT_RUN_PAIRS", raising=False)
    assert _dispatch(n_fft, hop, run_env=run_env)[0] == "plan"
    _check_process(f"plan(static size) {n_fft}/{hop} T={frames}" + ("" if run_env else " ADE_STFT_RUN=0"), n_fft, hop, frames)


# ---- run form: variants the models' configurations do not reach ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,hop,frames,twl", [
    # 2048 / 512: halo 3 -> rps = 8 (16 >= 12); one thread group of 512: 8 x 2049 x 8 + 16 KB ping-pong = 147 520 bytes fits the 153 600 budget, + 16 KB of twiddles does
    # not -> k_stft_run_synth<2048, POLAR, false>.  9 frames: (9 + 3 + 1) / 2 = 6 pairs, so run_pairs_for keeps all 8
    (2048, 512, 9, False),
    # 1920 / 480: halo 3 -> rps = 8: 8 x 1921 x 8 + 15 360 = 138 304 fits, + 15 360 = 153 664 misses the budget by 64 bytes -> k_stft_run_synth<1920, POLAR, false>
    (1920, 480, 7, False),
    # 512 / 64: halo 7 of a 32-frame run (rps = 16): each workgroup owns 25 frames and recomputes 7; 61 frames = 3 workgroups per row -> <512, POLAR, true>, wave form
    (512, 64, 61, True),
    # the two small compile-time sizes on the device: 64 / 32 (halo 1) and 60 / 15 (halo 3, radices 4 3 5), 8 pairs per run, 37 frames = 3 workgroups per row
    (64, 32, 37, True),
    (60, 15, 37, True)])
def test_gpu_run_form_variants(n_fft, hop, frames, twl, monkeypatch):
    monkeypatch.delenv("ADE_STFT_RUN", raising=False)
    monkeypatch.delenv("ADE_STFT_RUN_PAIRS", raising=False)
    assert _dispatch(n_fft, hop, frames) == ("run", twl)
    _check_process(f"run {n_fft}/{hop} T={frames} twiddles in {'LDS' if twl else 'global memory'}", n_fft, hop, frames)


# ---- dense form -----------------------------------------------------------------------------------------------------------------------------------------------------------------------
# a prime factor above 5 (11; 7 x 11 x 13; 2 x 7 x 73): make_plan fails -> gemm::launch(RowMajorA, FrameB) / (SpecA | PolarSpecA, RowMajorB) + k_stft_ola
DENSE = [
    pytest.param(44, 11, 5, dict(roundtrip=True), id="44/11-5frames"),                                     # M = 46, N = 15: one partial 128 x 128 tile, reflection in FrameB
    pytest.param(44, 11, 3, dict(center=False, pad="constant"), id="44/11-3frames-uncentred"),            # center_pad 0
    pytest.param(44, 11, 47, dict(pad="constant", keep_tail=True), id="44/11-47frames-zeros-tail"),       # 3 x 47 = 141 frame columns: two tiles, the last partial; zeros; the tail
    pytest.param(1001, 250, 5, dict(roundtrip=True), id="1001/250-5frames"),                               # odd, K = 1001 (no 16-byte loads, K tail), F2 = 1002
    pytest.param(1001, 250, 47, dict(pad="constant", keep_tail=True), id="1001/250-47frames-zeros-tail"),
    pytest.param(1001, 250, 2, dict(center=False, pad="constant"), id="1001/250-2frames-uncentred"),
    pytest.param(1022, 511, 5, dict(roundtrip=True), id="1022/511-5frames"),                               # F2 = 1024
    pytest.param(1022, 511, 1, dict(center=False), id="1022/511-1frame-uncentred"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,hop,frames,cfg", DENSE)
def test_gpu_dense_form(n_fft, hop, frames, cfg):
    assert _dispatch(n_fft, hop)[0] == "dense"
    _check_operator(_GpuMem(), f"dense {n_fft}/{hop} T={frames}", n_fft, hop, frames, **cfg)


@pytest.mark.hipsim
@pytest.mark.parametrize("n_fft,hop,frames,cfg", [pytest.param(77, 19, 5, dict(roundtrip=True), id="77/19-5frames"),
                                                  pytest.param(77, 19, 47, dict(pad="constant", keep_tail=True), id="77/19-47frames-zeros-tail")])
def test_hipsim_dense_form(n_fft, hop, frames, cfg):
    assert _dispatch(n_fft, hop)[0] == "dense"
    _check_operator(_SimMem(), f"sim dense {n_fft}/{hop} T={frames}", n_fft, hop, frames, **cfg)


# ---- edges common to the plan and dense forms ----------------------------------------------------------------------------------------------------------------------------------
EDGE_SIZES = [pytest.param(250, 100, id="plan-250/100"), pytest.param(44, 11, id="dense-44/11")]


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,hop", EDGE_SIZES)
@pytest.mark.parametrize("cfg", [
    pytest.param(dict(win_factor=0.8), id="short-window"),              # win_length < n_fft: zero-padded window, centre-padded, hop <= win_length / 2
    pytest.param(dict(win_factor=1.25), id="cropped-window"),           # win_length > n_fft
    pytest.param(dict(window="hamming_sym", synthesis_window="hamming_periodic"), id="two-windows"),
    pytest.param(dict(window="hann", keep_tail=True), id="hann-tail"),  # the tail's window sum vanishes: the 1 / w^2 allowance
    pytest.param(dict(window="hann_sqrt", keep_tail=False), id="hann-sqrt"),
])
def test_gpu_windows_and_tail(n_fft, hop, cfg):
    cfg = dict(cfg)
    f = cfg.pop("win_factor", None)
    if f:
        cfg["win_length"] = int(n_fft * f) // 2 * 2
        hop = min(hop, cfg["win_length"] // 2)
    _check_operator(_GpuMem(), f"edge {n_fft}/{hop} {cfg}", n_fft, hop, 9, **cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,hop", EDGE_SIZES)
def test_gpu_shortest_input_and_one_shorter(n_fft, hop):
    """n_fft / 2 + 1 samples is the shortest input the reflection guard of ade_stft_frames admits; one fewer is ADE_ERR_SHAPE_MISMATCH from every entry that takes a length."""
    mem = _GpuMem()
    op = _Op(mem, n_fft, hop)
    try:
        L = n_fft // 2 + 1
        x = _signal(L, 3, L)
        ref = op.ref_analysis(x)
        ea = _rel(mem.get(op.analyze(x)), ref)
        _report(f"edge {n_fft}/{hop} shortest input L={L}", analysis=ea)
        assert ea <= mem.gate["spec"]
        t = C.c_int(-7)
        assert op.c.ade_stft_frames(op.h, L - 1, C.byref(t)) == _lib.ADE_ERR_SHAPE_MISMATCH and t.value == -7
        d_x, d_s = mem.put(x[:, :L - 1]), mem.empty(ref.shape)
        assert op.c.ade_stft_analyze(op.h, mem.ptr(d_x), 3, L - 1, mem.ptr(d_s), None) == _lib.ADE_ERR_SHAPE_MISMATCH
        assert np.isnan(mem.get(d_s)).all()                # nothing was written
    finally:
        op.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,hop", EDGE_SIZES)
def test_gpu_caller_stream_growing_batch_and_empty_batch(n_fft, hop):
    import torch
    mem = _GpuMem()
    op = _Op(mem, n_fft, hop)
    try:
        frames = 9
        L = op.length_for(frames)
        x = _signal(n_fft + 17, 5, L)
        ref = op.ref_analysis(x)
        spec32 = _synthesis_input(ref, n_fft)
        want, den = op.ref_synthesis(spec32)
        assert den.min() >= DEN_MIN
        # a caller-supplied stream: the calls return without waiting; the results are read after synchronising that stream
        s = torch.cuda.Stream()
        sp = C.c_void_p(s.cuda_stream)
        assert s.cuda_stream != 0
        d_spec = op.analyze(x[:2], stream=sp)
        d_y = op.synthesize(spec32[:2], stream=sp)          # (first synthesize of the handle: allocates the frame buffer for batch 2)
        s.synchronize()
        ea = _rel(mem.get(d_spec), ref[:2])
        es, rs = _wave(mem.get(d_y), want[:2], den, mem.gate["wave"])
        # a second call with a larger batch on the same handle: the frame buffer is reallocated in between
        e2, r2 = _wave(mem.get(op.synthesize(spec32)), want, den, mem.gate["wave"])
        e3, r3 = _wave(mem.get(op.synthesize(spec32[:1])), want[:1], den, mem.gate["wave"])     # and a smaller one again, in the larger buffer
        _report(f"edge {n_fft}/{hop} stream / batches 2, 5, 1", analysis=ea, synthesis=es, larger=e2, smaller=e3)
        assert ea <= mem.gate["spec"] and rs <= 1.0 and r2 <= 1.0 and r3 <= 1.0
        # batch 0: ADE_OK and nothing touched, with or without buffers
        d_x, d_s, d_o = mem.put(x), mem.empty(ref.shape), mem.empty(want.shape)
        assert op.c.ade_stft_analyze(op.h, mem.ptr(d_x), 0, L, mem.ptr(d_s), None) == _lib.ADE_OK
        assert op.c.ade_stft_synthesize(op.h, mem.ptr(d_s), 0, frames, mem.ptr(d_o), None) == _lib.ADE_OK
        assert op.c.ade_stft_synthesize_polar(op.h, mem.ptr(d_s), mem.ptr(d_s), 0, frames, mem.ptr(d_o), None) == _lib.ADE_OK
        assert op.c.ade_stft_analyze(op.h, None, 0, L, None, None) == _lib.ADE_OK
        torch.cuda.synchronize()
        assert np.isnan(mem.get(d_s)).all() and np.isnan(mem.get(d_o)).all()
    finally:
        op.close()
