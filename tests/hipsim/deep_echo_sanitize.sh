#!/bin/bash
# Sanitizer run of the Deep Echo engine on the CPU (TEST INFRASTRUCTURE, host only): the simulator sources plus tests/hipsim/deep_echo_sanitize_main.cpp as ONE
# stand-alone program built with -fsanitize=address,undefined, run on the L = 1600 x 2 case of tests/test_deep_echo_hipsim.py.  The program is never loaded into
# Python; Python only writes its three input files and compares its output with the float64 oracle afterwards.
set -e
cd "$(dirname "$0")/../.."
B=tests/hipsim/_build
mkdir -p $B
C=audio_denoiser_onnx_amd/csrc
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wno-unused-function -Wno-unknown-pragmas -I tests/hipsim \
    -x c++ $C/ade_kernels.hip $C/ade_fused.hip $C/ade_engine.hip $C/ade_stft.hip $C/ade_dfsmn.hip $C/ade_melband.hip $C/ade_mossformer.hip $C/ade_ulunas.hip \
    $C/ade_hgtcrn.hip $C/ade_zipenhancer.hip $C/ade_sdaec.hip $C/ade_deep_echo.hip \
    -x c++ tests/hipsim/hipsim.cpp tests/hipsim/deep_echo_sanitize_main.cpp -o $B/deep_echo_sanitize -lpthread -ldl
python - <<'PY'
import json, os, sys
import numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
from deep_echo_oracle import fixture_state
from audio_denoiser_onnx_amd import deep_echo, weights
B = "tests/hipsim/_build"
io = np.load("tests/golden/deep_echo_seed0_io.npz")
rows = np.stack([np.stack([io[f"near{i}"][4000:5600], io[f"far{i}"][4000:5600]]) for i in range(2)])
rows.astype(np.int16).tofile(os.path.join(B, "deep_echo_sanitize_in.i16"))
open(os.path.join(B, "deep_echo_sanitize.adew"), "wb").write(weights.pack_blob(deep_echo.state_to_blob_tensors(fixture_state("tests/golden"))))
json.dump(deep_echo.metadata(1600), open(os.path.join(B, "deep_echo_sanitize_manifest.json"), "w"))
PY
ASAN_OPTIONS=detect_leaks=1 LSAN_OPTIONS=suppressions=tests/hipsim/lsan.supp:print_suppressions=0 $B/deep_echo_sanitize $B/deep_echo_sanitize_manifest.json $B/deep_echo_sanitize.adew $B/deep_echo_sanitize_in.i16 2 $B/deep_echo_sanitize_out.i16
python - <<'PY'
import sys
import numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
from deep_echo_oracle import DeepEchoOracle, fixture_state
from audio_denoiser_onnx_amd import deep_echo
B = "tests/hipsim/_build"
rows = np.fromfile(B + "/deep_echo_sanitize_in.i16", np.int16).reshape(2, 2, 1600)
out = np.fromfile(B + "/deep_echo_sanitize_out.i16", np.int16).reshape(2, 1600)
want, _, _ = DeepEchoOracle(deep_echo.state_to_blob_tensors(fixture_state("tests/golden"))).forward(rows[:, 0], rows[:, 1])
d = int(np.abs(out.astype(np.int32) - want.astype(np.int32)).max())
print("sanitized run vs oracle: PCM max diff", d, "LSB")
assert d <= 1
PY
