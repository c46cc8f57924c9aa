"""csrc/ade_fft.h unit-checked on its own (tests/unit/fft_unit.hip): fft::forward against a double-precision DFT with 256 and 32 threads per transform and with several
thread groups side by side in one workgroup; forward_static<N> / forward_wave<N> word for word against forward (the bit-identity the header states); split_bin /
merge_bin_conj as the real transform of 2 h samples and its way back at the engines' half lengths; make_plan over every n <= 8192 on the host.
CPU: the same source under the host simulator at small sizes; GPU: built by hipcc for gfx950 on the box, up to 8192 points (128 KB of LDS) and the eight-pass sizes."""
import pytest

from test_gemm16 import _build_gpu, _build_sim, _run

SMALL = [4, 6, 8, 9, 10, 25, 45, 60, 64, 96, 250, 256]
REAL = ["r256", "r320", "r960", "r1024", "r45"]          # DFSMN-AEC / NKF-AEC / UL-UNAS (256), DFSMN-AEC (320), DFSMN 48 kHz (960, 1024), one odd half length


@pytest.mark.hipsim
def test_hipsim_fft_forward_static_wave_and_real_split():
    _run(_build_sim("fft_unit"), "plan", *SMALL, 512, 400, "r45", "r256", "r320")


@pytest.mark.gpu
def test_gpu_fft_forward_static_wave_and_real_split():
    _run(_build_gpu("fft_unit"), "plan", *SMALL, 320, 480, 640, 729, 960, 1024, 1536, 3125, 4096, 8192,
         6561, 4374, 5832, 7776,                # exactly kMaxPasses passes
         1920, 2048, 400, 512,                  # the compile-time sizes (with 64 and 60 above): forward_static, forward_wave
         *REAL)
