"""bench.py's launcher contract: `--gpus N` means N ranks.  A line is only ever printed for the GPU count that was asked for:
started bare with N > 1 the script re-executes itself under torch.distributed.run with N ranks; inside a launcher whose WORLD_SIZE differs it exits non-zero."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gpus_flag_decides_the_world(bench):
    assert bench.check_world(1, {}) == ("run", 1)
    assert bench.check_world(2, {}) == ("relaunch", 2)
    assert bench.check_world(8, {"WORLD_SIZE": "8"}) == ("run", 8)
    assert bench.check_world(1, {"WORLD_SIZE": "1"}) == ("run", 1)
    for gpus, world in ((2, "1"), (8, "4"), (1, "2")):
        with pytest.raises(SystemExit) as e:
            bench.check_world(gpus, {"WORLD_SIZE": world})
        assert e.value.code == 2
    with pytest.raises(SystemExit):
        bench.check_world(0, {})


def test_relaunch_is_one_rank_per_gpu_on_loopback(bench):
    cmd = bench.relaunch_command(4, ["--gpus", "4", "--steps", "5"], 29511)
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29511"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "5"] and cmd[-5].endswith("bench.py")


def _lines_with_n_gpus(text):
    out = []
    for ln in text.splitlines():
        try:
            d = json.loads(ln)
        except ValueError:
            continue
        if isinstance(d, dict) and "n_gpus" in d:
            out.append(d)
    return out


def test_mismatched_launcher_prints_no_line():
    """What the round-5 script did: `--gpus 2` inside a one-rank environment ran one rank and printed n_gpus: 1.  Now: exit code 2, no JSON line."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and not _lines_with_n_gpus(r.stdout), (r.returncode, r.stdout[-400:])
    assert "WORLD_SIZE = 1" in r.stderr


def test_bare_gpus_2_relaunches_two_ranks_and_never_reports_one():
    """Bare `python bench.py --gpus 2`: two ranks are started (torch.distributed.run on 127.0.0.1).  In this container there is no GPU, so both ranks stop at the
    engine's no-CPU-path check: the exit code is non-zero and, whatever happened, no line with n_gpus == 1 was printed."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--host-steps", "0", "--cpu-seconds", "0",
                        "--other-steps", "0", "--no-stft-operator"], env=env, capture_output=True, text=True, timeout=600)
    lines = _lines_with_n_gpus(r.stdout)
    assert all(d["n_gpus"] == 2 for d in lines), lines
    import torch
    if not torch.cuda.is_available():
        assert r.returncode != 0 and not lines
        assert (r.stdout + r.stderr).count("bench.py needs a GPU") >= 1


def test_explicit_step_counts_always_hold(bench):
    """--steps / --warmup set the timed and warm-up step counts for every workload; only counts that are not given take the workload's default."""
    for wl in ("gtcrn", "zipenhancer", "melband", "mossformer", "dfsmn"):
        a = bench.parse_args(["--workload", wl, "--steps", "100", "--warmup", "10"])
        assert (a.steps, a.warmup) == (100, 10)
        a = bench.parse_args(["--workload", wl, "--steps", "7"])
        assert (a.steps, a.warmup) == (7, 10 if wl == "gtcrn" else 2)
    a = bench.parse_args([])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (100, 10, False, None)
    assert bench.parse_args(["--workload", "melband"]).steps == 10
    assert bench.parse_args(["--full", "--dump-outputs", "d"]).full


def test_dump_outputs_is_the_pcm_as_float32(bench, tmp_path):
    import torch
    pcm = np.random.default_rng(3).integers(-32768, 32768, (6, 1000)).astype(np.int16)
    bench.dump_outputs(str(tmp_path / "a"), torch.from_numpy(pcm))
    got = np.load(tmp_path / "a" / "pcm_out.npy")
    assert got.dtype == np.float32 and np.array_equal(got, pcm.astype(np.float32))


def test_dump_outputs_samples_whole_rows_in_order_above_the_limit(bench, tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 1000 * 3 + 5)
    pcm = np.arange(10)[:, None].astype(np.int16) * np.ones((1, 1000), np.int16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.from_numpy(pcm))
    a, b = np.load(tmp_path / "a" / "pcm_out.npy"), np.load(tmp_path / "b" / "pcm_out.npy")
    assert a.shape == (3, 1000) and a.nbytes <= bench.DUMP_LIMIT_BYTES and np.array_equal(a, b)
    rows = a[:, 0]
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, np.repeat(rows[:, None], 1000, axis=1))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    """A plain run prints the headline of exactly --steps timed steps and nothing beside it; --dump-outputs holds the int16 PCM of the timed path,
    which for the first two of the batch's synthetic chunks is the C oracle's within 1 LSB."""
    from audio_denoiser_onnx_amd.synth import synth_batch
    from ade_testlib import golden_blob
    from oracle_lib import GtcrnOracle
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = _lines_with_n_gpus(r.stdout)[-1]
    assert line["steps"] == 7 and line["warmup"] == 2 and line["n_gpus"] == 1 and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["unit"] == "audio-s/s" and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["host_inclusive"] is None and "other_workloads" not in line
    out = np.load(tmp_path / "pcm_out.npy")
    assert out.dtype == np.float32 and out.shape[0] == 256 and np.array_equal(out, np.round(out)) and np.abs(out).max() > 0
    ref_pcm, _ = GtcrnOracle(golden_blob(0), 16000).process(synth_batch(2, 16000))
    assert out.shape[1] == ref_pcm.shape[1]
    assert np.abs(out[:2].astype(np.int32) - ref_pcm.astype(np.int32)).max() <= 1
