"""Network geometries, seeded weights and seeded signals for the AEC sweep (tests/test_aec_geometry.py, tools/make_golden_dfsmn_aec.py --geometry).

The committed seed-0 blobs hold one geometry: D = 128, six identical layers of H = 64, lorder 20, dilation 2, every GEMM contraction length a multiple of 16 and
both PReLU slopes 0.25.  The table below leaves that point in every direction the engines read from the blob.  The weights are generated (weightgen.tensor: a hash
of the tensor's name, independent of the numpy version), not committed: a blob per geometry would be 0.3-0.5 MB.

Within a geometry ``dilation * (lorder - 1)`` is the same for every layer: the reference's graph shares one left pad between the layers, so only such a network
runs through it (tests/golden/aec_geom_<name>.npz holds its outputs).
"""
from __future__ import annotations

import os
from collections import OrderedDict, namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

Geometry = namedtuple("Geometry", "seed D H lorder dilation skip slope_in slope_out")

# What each one reaches (csrc/ade_gemm.h: 128-row tiles, slabs of 16 along K, float4 fetches when K % 4 == 0):
#   tails      K = 100 ends inside a slab on the float4 path, K = 33 forces the scalar fetch, Hmax comes from the LAST layer, three (lorder, dilation) pairs
#   scalar     depth 1, D % 4 != 0: every GEMM with K = D on the scalar path, M smaller than one tile
#   two_tiles  M = 130 spans two row tiles, K = 129 / 130 leave tails of 1 and 2, Hmax from the FIRST layer, H = 5, dilation 12 >= the frame count
#   no_memory  lorder 1: the memory is w[c][0] * h, and with the skip the layer adds h twice
GEOMETRIES = OrderedDict([
    ("tails", Geometry(11, 100, (52, 33, 64), (13, 7, 4), (1, 2, 4), (1, 0, 1), 0.10, 0.40)),
    ("scalar", Geometry(12, 90, (17,), (3,), (5,), (0,), 0.40, 0.05)),
    ("two_tiles", Geometry(13, 130, (129, 5), (2, 13), (12, 1), (1, 1), 0.25, 0.10)),
    ("no_memory", Geometry(14, 64, (32, 48), (1, 1), (1, 3), (0, 1), 0.30, 0.30)),
])

W_LONG, W_SHORT, W_FOLD = 3200, 1280, 1600      # 9 / 3 / 4 mask frames, 13 / 6 / 7 back-end frames; 1280 is the smallest window above 1024 the engine accepts
FOLD_SECONDS = 0.1                              # batch_window_seconds of the folded shape: windows of 1600, a call of 3200 samples is two of them
NKF_LENGTHS = (3200, 3000)                      # 3000 is no multiple of the 256-sample hop: T = 12, 2816 samples kept
N_ROWS = 4                                      # 0: echo + near-end noise, 1: far end silent, 2: all zero, 3: another echo row (the second folded call)


def state(name):
    """-> (nkf_state, dfsmn_state, skip_connect, dilation): the arguments of ``dfsmn_aec.state_to_blob_tensors``."""
    from audio_denoiser_onnx_amd import weightgen
    g = GEOMETRIES[name]
    assert len(g.H) == len(g.lorder) == len(g.dilation) == len(g.skip)
    assert len({d * (lo - 1) for d, lo in zip(g.dilation, g.lorder)}) == 1, "the reference shares one left pad between the layers"
    nkf = dict(weightgen.dfsmn_aec_state(g.seed, width=1, hidden=1, depth=0)[0])      # the NKF half as bench builds it, NKF_GAIN_LAYER_SCALE on the gain layer
    nkf["kg_net.fc_in.1.prelu.weight"] = np.full((1,), g.slope_in, np.float32)
    nkf["kg_net.fc_out.1.prelu.weight"] = np.full((1,), g.slope_out, np.float32)
    feat, bins, net = 240, 321, {}

    def put(key, shape, fan_in, gain=1.0):
        net[key] = weightgen.tensor(key, shape, gain / np.sqrt(fan_in), g.seed)

    put("linear1.linear.weight", (g.D, feat), feat)
    put("linear1.linear.bias", (g.D,), 100.0)
    for i, (h, lo) in enumerate(zip(g.H, g.lorder)):
        put(f"deepfsmn.{i}.linear.weight", (h, g.D), g.D, 2.0)
        put(f"deepfsmn.{i}.linear.bias", (h,), 100.0)
        put(f"deepfsmn.{i}.project.weight", (g.D, h), h, 1.2)
        put(f"deepfsmn.{i}.conv1.weight", (g.D, 1, lo, 1), 50.0)
    put("linear2.weight", (bins, g.D), g.D, 0.9)
    put("linear2.bias", (bins,), 100.0)
    put("linear3.weight", (1, g.D), g.D, 0.9)
    put("linear3.bias", (1,), 100.0)
    # log-mel of int16-scale power sits around 5 .. 25: a per-feature shift / scale brings it to unit range, as a trained normaliser would
    net["feature.shift"] = (np.float32(-15.0) + weightgen.tensor("feature.shift", (feat,), 1.0, g.seed)).astype(np.float32)
    net["feature.scale"] = (np.float32(0.2) * (np.float32(1.0) + weightgen.tensor("feature.scale", (feat,), 0.1, g.seed))).astype(np.float32)
    return nkf, net, [bool(s) for s in g.skip], list(g.dilation)


def blob_tensors(name):
    from audio_denoiser_onnx_amd import dfsmn_aec
    return dfsmn_aec.state_to_blob_tensors(*state(name))


def nkf_blob(name) -> bytes:
    """The NKF half alone, for a model_family nkf_aec handle: the same weights, the same two distinct slopes."""
    from audio_denoiser_onnx_amd.nkf_aec import state_to_blob_tensors
    from audio_denoiser_onnx_amd.weights import pack_blob
    return pack_blob(state_to_blob_tensors(state(name)[0]))


def signals(name, length=W_LONG):
    """-> (near, far), int16 (N_ROWS, length).  The far end is noise; the near end a delayed, scaled copy of it plus independent noise.

    The noise is coloured by the one-pole filter 1 / (1 - 0.97 z^-1), the inverse of the fbank's pre-emphasis, so that every mel band of the features has a
    comparable level.  ``feat`` is the logarithm of a band power: its absolute error is the relative error of that power, and an fp32 transform's rounding is
    relative to the whole frame (about 1e-7 of its norm), not to the band.  White noise after the 0.97 pre-emphasis leaves the lowest mel band some 35 dB under
    the frame's level and the echo band 0.15 of that, where that rounding alone is 3e-4 in the logarithm -- above 1e-5 of the tap's peak (measured under the
    host simulator on white noise: 3.1e-4 against a gate of 2.59e-4, in band 0 of the echo block only).

    What these signals therefore leave untested, on purpose: the feature kernel's accuracy on a band far under the frame's level.  There the engine is less
    accurate than the reference: on white noise the reference's own fp32 run stays within 2.3e-5 of the float64 oracle with its own tables, over every row,
    while the engine's echo block (near - 1.15 temp_aec, formed from the split of one complex 1024-point FFT that carries both signals) is 1e-4 to 3e-4 from
    the oracle in its lowest bands and about 1e-5 in the near-end and temp_aec blocks.  The fixtures record each distance over all rows (``<tap>_all_rows``)
    next to the row-0 figure the gates read."""
    from audio_denoiser_onnx_amd import weightgen
    g = GEOMETRIES[name]
    lead = 256                                           # samples of filter run-in, dropped

    def noise(key, amp):
        white = weightgen.tensor("signal." + key, (length + lead,), amp, g.seed).astype(np.float64)
        out, y = np.empty_like(white), 0.0
        for i, v in enumerate(white.tolist()):           # plain IEEE double recursion: the same bits everywhere
            y = 0.97 * y + v
            out[i] = y
        return out

    def pcm(x):
        return np.clip(np.round(x), -32768, 32767).astype(np.int16)

    near, far = np.zeros((N_ROWS, length), np.int16), np.zeros((N_ROWS, length), np.int16)
    for row, (delay, gain) in ((0, (37, 0.6)), (3, (11, 0.35))):
        f = noise(f"far{row}", 1500.0)
        far[row] = pcm(f[lead:])
        near[row] = pcm(gain * f[lead - delay:lead - delay + length] + noise(f"near{row}", 400.0)[lead:])
    near[1] = pcm(noise("near1", 1000.0)[lead:])          # far end silent: the echo estimate is exactly zero
    return near, far


def fixture(name):
    """tests/golden/aec_geom_<name>.npz (tools/make_golden_dfsmn_aec.py --geometry): the inputs, the reference's outputs and row-0 taps, the blob's SHA-256 and
    the recorded distances between the reference's fp32 run and the float64 oracle.  ``fp64_distance[mode][tap]`` / ``[tap + "_peak"]`` are taken on row 0, as
    dfsmn_aec_seed0_taps.npz takes them, and are what the gates read; ``[tap + "_all_rows"]`` is the same distance over every row of the long shape."""
    return np.load(os.path.join(GOLD, f"aec_geom_{name}.npz"))


def gate(dist, key, contract=None):
    """The project's standing rule (docstring of tests/test_dfsmn_aec_gpu.py): 1e-5 of the tap's peak (``contract`` overrides: 1e-4 for a waveform); where the
    recorded distance between two independent evaluations exceeds a third of that, 3 x the recorded distance."""
    c = 1e-5 * dist[key + "_peak"] if contract is None else contract
    return 3.0 * dist[key] if dist[key] > c / 3.0 else c
