"""bench.py's launch contract on a box without a GPU: `--gpus N` with no RANK in the environment must start N fresh
rank processes itself (the driver runs `python bench.py --gpus N`), each with the torch.distributed environment of its
rank, and must do so before anything touches the GPU; here the ranks then stop at "needs a HIP device"."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_gpus2_spawns_two_ranks_without_torchrun():
    import torch
    if torch.cuda.is_available():
        pytest.skip("CPU-only check (on a GPU box the ranks would really run)")
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1"])
    assert r.returncode == 1                                  # the ranks failed (no HIP device), loudly
    assert r.stderr.count("bench.py needs a HIP device") == 2, r.stderr      # ... and there were exactly two of them
    assert "a rank process failed" in r.stderr
    assert r.stdout.strip() == ""                             # no JSON line from a failed run


def test_world_size_mismatch_is_an_error_not_an_assert():
    r = _run(["--gpus", "4"], {"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "2"})
    assert r.returncode == 2 and "WORLD_SIZE=2 but --gpus 4" in r.stderr


def test_spawned_ranks_get_their_environment(tmp_path, monkeypatch):
    """spawn_ranks() hands every child RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / one shared MASTER_PORT."""
    sys.path.insert(0, ROOT)
    import bench
    seen = []

    class FakeProc:
        def __init__(self, cmd, env=None, stdout=None):
            seen.append((cmd, {k: env[k] for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}))

        def wait(self, timeout=None):
            return 0

        def poll(self):
            return 0

    monkeypatch.setattr(bench.subprocess, "Popen", FakeProc)
    monkeypatch.delenv("MASTER_PORT", raising=False)
    args = bench.parse_args(["--gpus", "4", "--steps", "3"])
    assert bench.spawn_ranks(args, ["--gpus", "4", "--steps", "3"]) == 0
    assert [e["RANK"] for _, e in seen] == ["0", "1", "2", "3"] and [e["LOCAL_RANK"] for _, e in seen] == ["0", "1", "2", "3"]
    assert all(e["WORLD_SIZE"] == "4" and e["MASTER_ADDR"] == "127.0.0.1" for _, e in seen)
    assert len({e["MASTER_PORT"] for _, e in seen}) == 1
    assert all(cmd[1].endswith("bench.py") and cmd[2:] == ["--gpus", "4", "--steps", "3"] for cmd, _ in seen)


def test_bytes_per_env_step_counts_the_depth_image():
    sys.path.insert(0, ROOT)
    import bench
    from gym_kmanip_amd.model import compile_model
    cm = compile_model("KManipSoloArm")
    assert bench.algorithmic_bytes_per_env_step(cm) == 1197
    assert bench.algorithmic_bytes_per_env_step(cm, 64) == 1197 + 64 * 64 * 4    # BASELINE config 5


def test_rank_path_refuses_a_collective_that_does_not_span_the_job(capsys):
    """bench.py's start-up self-check (run_rank, right after init_process_group): an all-reduce of ones must count WORLD_SIZE
    ranks; anything else is a loud non-zero exit instead of a whole-job value computed from part of the job."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.check_ranks_seen(8, 8, 0) == 0 and capsys.readouterr().err == ""
    assert bench.check_ranks_seen(1, 8, 3) == 4
    err = capsys.readouterr().err
    assert "sees 1 rank(s), WORLD_SIZE is 8" in err and "rank 3" in err


# ------------------------------------------------------------------------------------------------------------------
# the N > 1 start-up cannot hang: every wait for the peers is under bench.Deadline (VERDICT r5 task 2)
_HANG = r"""
import sys, threading, time
sys.path.insert(0, %r)
import bench

class FakeHangingBackend:                      # a rendezvous whose peer never arrives: blocks for ever, raises nothing
    def init_process_group(self, *a, **k):
        threading.Event().wait()

t0 = time.time()
try:
    with bench.Deadline("init_process_group('fakehang')", 1.0, rank=3):
        FakeHangingBackend().init_process_group("fakehang", rank=3, world_size=8)
except BaseException as e:                     # the deadline must END the process, not raise into a handler that could retry
    print("raised", type(e).__name__)
print("survived", time.time() - t0)
"""


def test_deadline_ends_a_rank_whose_rendezvous_hangs():
    import time
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", _HANG % ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 6, (r.returncode, r.stderr[-500:])
    assert "rank 3: init_process_group('fakehang') did not finish within 1 s" in r.stderr and "exiting 6" in r.stderr
    assert r.stderr.count("\n") == 1                           # ONE line of diagnosis
    assert "survived" not in r.stdout and "raised" not in r.stdout
    assert time.time() - t0 < 60


_GLOO_ALONE = r"""
import datetime, os, sys
sys.path.insert(0, %r)
import bench
import torch.distributed as dist
with bench.Deadline("init_process_group('gloo')", 3.0, rank=0):      # rank 0 of a TWO-rank job whose rank 1 was never started
    dist.init_process_group("gloo", rank=0, world_size=2, timeout=datetime.timedelta(seconds=600))
print("survived")
"""


def test_deadline_ends_a_real_gloo_rendezvous_whose_peer_never_comes():
    sys.path.insert(0, ROOT)
    import bench
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(bench.free_port()), RANK="0", WORLD_SIZE="2")
    r = subprocess.run([sys.executable, "-c", _GLOO_ALONE % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 6 and "did not finish within 3 s" in r.stderr and "survived" not in r.stdout, (r.returncode, r.stderr[-500:])


def test_deadline_is_silent_when_the_step_finishes_and_teardown_exits_zero():
    sys.path.insert(0, ROOT)
    import time
    import bench
    fired = []
    with bench.Deadline("quick", 5.0, rank=0, _exit=fired.append):
        pass
    time.sleep(0.05)
    assert fired == []
    with bench.Deadline("teardown", 0.05, rank=0, exit_code=0, _exit=fired.append):       # (after the JSON line: a hang must not cost the result)
        time.sleep(0.5)
    assert fired == [0]


def test_parent_stops_the_peers_of_a_rank_that_hit_its_deadline(monkeypatch):
    """A rank that exits 6 (its rendezvous deadline) must end the whole job: spawn_ranks kills the ranks still waiting."""
    sys.path.insert(0, ROOT)
    import bench
    procs = []

    class FakeProc:
        def __init__(self, cmd, env=None, stdout=None):
            self.rank = int(env["RANK"]); self.killed = False
            procs.append(self)

        def poll(self):
            if self.rank == 1:
                return 6                       # hit its deadline
            return -9 if self.killed else None   # rank 0 would wait for ever

        def kill(self):
            self.killed = True

        def wait(self, timeout=None):
            return -9

    monkeypatch.setattr(bench.subprocess, "Popen", FakeProc)
    monkeypatch.setattr(bench.time, "sleep", lambda s: None)
    assert bench.spawn_ranks(bench.parse_args(["--gpus", "2"]), ["--gpus", "2"]) == 1
    assert procs[0].killed and not procs[1].killed


def test_default_exchange_is_the_mainstream_path_and_the_line_records_the_knobs(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    assert bench.parse_args([]).gather_direct == "auto" and bench.parse_args([]).rendezvous_timeout == 90.0
    assert bench.resolve_gather_direct("auto") == ("off", None)                 # torch.distributed's all_gather_into_tensor
    assert bench.resolve_gather_direct("auto", "side") == ("side", "env")       # opt-in by environment ...
    assert bench.resolve_gather_direct("side") == ("side", "flag")              # ... or by flag
    assert bench.resolve_gather_direct("off", "side") == ("off", "flag")        # an explicit flag wins
    for k in [k for k in os.environ if k.startswith("KMANIP_")]:
        monkeypatch.delenv(k)
    assert bench.kmanip_env_vars() == {}
    monkeypatch.setenv("KMANIP_EPB", "2"); monkeypatch.setenv("KMANIP_SPREAD", "0"); monkeypatch.setenv("KMANIP_BENCH_SPAWNED", "1")
    assert bench.kmanip_env_vars() == {"KMANIP_EPB": "2", "KMANIP_SPREAD": "0"}


def test_run_timeout_bounds_the_timed_region_generously():
    """N > 1: the warm-up + timed steps run under the same watchdog as the start-up (a collective that never completes must not
    sit there until the driver's timeout); the automatic bound is far above a healthy run, --run-timeout overrides, 0 disables."""
    import types
    import bench
    a = types.SimpleNamespace(run_timeout=-1.0, warmup=5, steps=20)
    assert bench.run_timeout_seconds(a) == 120.0 + 0.25
    a.steps = 100000
    assert bench.run_timeout_seconds(a) > 1000.0             # 0.6 ms a step: a healthy 100 000-step run takes a minute
    a.run_timeout = 30.0
    assert bench.run_timeout_seconds(a) == 30.0
    a.run_timeout = 0.0
    assert bench.run_timeout_seconds(a) == 0.0               # Deadline(seconds=0) starts no timer
    d = bench.Deadline("x", 0.0)
    with d:
        assert d._timer is None


def test_timing_events_are_sampled_on_long_windows_only():
    """An event pair costs the step's stream ~5 us (1 % of a 4096-env step, inside `value`): windows of >= 256 steps time every
    (steps // 128)-th launch, the driver's 20-step window times every launch; --time-every overrides (tools/ab.sh: 1)."""
    import bench
    old = bench.TIME_EVERY
    try:
        bench.TIME_EVERY = 0
        assert [bench.timing_every(s) for s in (1, 20, 128, 255, 256, 1024, 4096)] == [1, 1, 1, 1, 2, 8, 32]
        assert 1024 // bench.timing_every(1024) == 128                       # the default run still times 128 launches
        bench.TIME_EVERY = 1
        assert bench.timing_every(1024) == 1
        assert bench.parse_args(["--time-every", "4"]).time_every == 4 and bench.parse_args([]).time_every == 0
    finally:
        bench.TIME_EVERY = old


def test_steps_must_be_a_real_count():
    import bench
    assert bench.parse_args(["--steps", "7", "--warmup", "0"]).steps == 7
    for bad in (["--steps", "0"], ["--steps", "-3"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_outputs_writes_float_arrays_within_budget(tmp_path):
    """--dump-outputs: float64 stays float64, uint8 / float32 become float32, small arrays are written whole, a large one as the
    same seeded sample every time, and the files stay inside the budget (64 MB in the bench; a small budget here)."""
    import numpy as np
    import torch
    import bench
    g = torch.Generator().manual_seed(3)
    obs = torch.rand((8, 5), dtype=torch.float64, generator=g)
    done = torch.tensor([0, 1, 0, 0, 1, 0, 0, 1], dtype=torch.uint8)
    cam = torch.randint(0, 256, (8, 48, 64, 3), dtype=torch.uint8, generator=g)
    budget = 3 * (4096 + 16 * 1024)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"obs": obs, "done": done, "camera_head": cam}, budget=budget)
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(p.name for p in a.iterdir()) == ["camera_head.npy", "done.npy", "manifest.json", "obs.npy"]
    assert sum(p.stat().st_size for p in a.glob("*.npy")) <= budget
    o, dn, c = (np.load(a / n) for n in ("obs.npy", "done.npy", "camera_head.npy"))
    assert o.dtype == np.float64 and np.array_equal(o, obs.numpy())
    assert dn.dtype == np.float32 and np.array_equal(dn, done.numpy().astype(np.float32))
    man = json.load(open(a / "manifest.json"))
    assert c.dtype == np.float32 and c.ndim == 1 and man["camera_head"]["sampled_elements"] == c.size < cam.numel()
    assert man["camera_head"]["shape"] == [8, 48, 64, 3] and man["camera_head"]["source_dtype"] == "uint8" and man["obs"]["sampled_elements"] is None
    idx = np.sort(np.random.default_rng(0).choice(cam.numel(), c.size, replace=False))
    assert np.array_equal(c, cam.numpy().reshape(-1)[idx].astype(np.float32))
    assert np.array_equal(c, np.load(b / "camera_head.npy"))              # the same elements on every run
    bench.dump_outputs(str(tmp_path / "r"), {"obs": obs}, rank=1, world=2)
    assert sorted(p.name for p in (tmp_path / "r").iterdir()) == ["manifest.rank1.json", "obs.rank1.npy"]


@pytest.mark.gpu
def test_dump_outputs_is_the_last_timed_step_and_repeats(tmp_path):
    """Two runs with the same arguments dump the same arrays bit for bit; a run with 3 more timed steps leaves every env's
    episode clock (sim_time = step in episode x CONTROL_TIMESTEP) exactly 3 steps further on: --steps is the count stepped."""
    import numpy as np
    from gym_kmanip_amd.model import CONTROL_TIMESTEP, MAX_EPISODE_STEPS
    base = ["--envs-per-gpu", "256", "--warmup", "2", "--no-variants", "--no-cpu-baseline"]
    dumps = {}
    for tag, k in (("a", 5), ("b", 5), ("c", 8)):
        r = _run(base + ["--steps", str(k), "--dump-outputs", str(tmp_path / tag)])
        assert r.returncode == 0, r.stderr[-2000:]
        assert json.loads(r.stdout.strip().splitlines()[-1])["steps"] == k
        dumps[tag] = {p.name: np.load(p) for p in (tmp_path / tag).glob("*.npy")}
    assert sorted(dumps["a"]) == ["done.npy", "obs.npy", "reward.npy", "sim_time.npy"]
    for name, v in dumps["a"].items():
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all(), name
        assert np.array_equal(v, dumps["b"][name]), name
    step_a, step_c = (np.rint(dumps[t]["sim_time.npy"] / CONTROL_TIMESTEP).astype(np.int64) for t in ("a", "c"))
    assert np.array_equal((step_c - step_a) % MAX_EPISODE_STEPS, np.full(256, 3)), (step_a[:8], step_c[:8])
