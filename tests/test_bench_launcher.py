"""bench.py's multi-GPU path on CPU: the --gpus N launcher, sharding and global diagnostics.

``--stub`` swaps the HIP sampler for a CPU AR(1) stand-in keyed by (seed, global chain id,
sweep) -- the same keying as the device Philox streams -- so a 2-rank run over gloo must
produce the same global R-hat / ESS as one process holding all the chains.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, full=True):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub",
                          "--steps", "6", "--warmup", "2", "--ess-burn", "4",
                          "--ess-window", "60", *(["--full"] if full else []), *args],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_plain_run_times_the_steps_only_and_dumps_its_last_step(tmp_path):
    """Without --full no ESS window is run (its fields are null) and the result line keeps
    the headline fields; --dump-outputs writes the last timed step as float64 arrays that
    two runs with the same arguments reproduce exactly."""
    import numpy as np
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    one = _run("--chains", "5", "--dump-outputs", a, full=False)
    _run("--chains", "5", "--dump-outputs", b, full=False)
    assert one["steps"] == 6 and one["warmup"] == 2
    assert one["unit"] == "chain-sweeps/s" and one["higher_is_better"] is True
    assert one["dtype"] == "f64" and one["value"] > 0 and one["ms_per_step"] > 0
    assert one["ess_per_sec"] is None and one["cpu_baseline"] is None
    assert one["ess_window"]["sweeps"] == 0 and one["ess_window"]["ess_total"] is None
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"chain_index.npy", "rec_x.npy", "rec_theta.npy", "theta.npy", "x.npy"} <= set(names)
    assert np.array_equal(np.load(os.path.join(a, "chain_index.npy")), np.arange(5.0))
    for nm in names:
        va, vb = np.load(os.path.join(a, nm)), np.load(os.path.join(b, nm))
        assert va.dtype == np.float64 and va.shape[0] == 5
        assert np.array_equal(va, vb), nm
    # the stub records a sweep's state before it moves the chain: the last record differs
    # from the state after the last step, and both are finite
    x, rx = np.load(os.path.join(a, "x.npy")), np.load(os.path.join(a, "rec_x.npy"))
    assert x.shape == rx.shape and np.isfinite(x).all() and not np.array_equal(x, rx)


def test_dump_outputs_samples_chains_beyond_its_budget(tmp_path, monkeypatch):
    """Past the size budget --dump-outputs keeps a fixed, seeded, sorted sample of the chains,
    the same rows of every array, and names them in chain_index."""
    import numpy as np

    import bench
    C = 40
    state = {"x": np.arange(C * 3, dtype=np.float64).reshape(C, 3),
             "status": np.arange(C, dtype=np.int32)}
    rec = {"x": np.arange(C * 2 * 3, dtype=np.float64).reshape(C, 2, 3)}
    per_chain = 8 * (1 + 3 + 1 + 3)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 10 * per_chain + 1)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), state, rec, 0, 1)
    got = {nm[:-4]: np.load(str(tmp_path / "a" / nm)) for nm in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["chain_index", "rec_x", "status", "x"]
    idx = got["chain_index"].astype(int)
    assert len(idx) == 10 and np.all(np.diff(idx) > 0) and idx.max() < C
    assert np.array_equal(got["x"], state["x"][idx])
    assert np.array_equal(got["rec_x"], rec["x"][idx, -1])
    assert got["status"].dtype == np.float64 and np.array_equal(got["status"], idx)
    assert sum(v.nbytes for v in got.values()) <= 10 * per_chain + 1
    assert np.array_equal(np.load(str(tmp_path / "b" / "chain_index.npy")), got["chain_index"])


def test_two_rank_launch_matches_one_process():
    two = _run("--gpus", "2", "--chains", "6")
    one = _run("--gpus", "1", "--chains", "12")
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1
    assert two["config"]["chains_total"] == one["config"]["chains_total"] == 12
    assert two["shards"] == [[0, 6], [6, 12]] and one["shards"] == [[0, 12]]
    # global diagnostics over ALL chains: identical draws -> identical R-hat and ESS
    w2, w1 = two["ess_window"], one["ess_window"]
    assert w2["chains"] == w1["chains"] == 12
    for k in w1["rhat_max"]:
        assert w2["rhat_max"][k] == w1["rhat_max"][k]
        assert w2["ess_total"][k] == w1["ess_total"][k]
    assert two["cpu_baseline"] is None


def test_launcher_reports_world_size_four():
    four = _run("--gpus", "4", "--chains", "3")
    assert four["n_gpus"] == 4 and four["config"]["chains_total"] == 12
    assert [s[0] for s in four["shards"]] == [0, 3, 6, 9]


def test_launcher_fails_fast_when_a_rank_dies():
    """One rank exits 3 right after init while its peers wait in a collective: the launcher
    must return non-zero within seconds and leave no rank process behind."""
    import time
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    t0 = time.time()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub",
                          "--gpus", "3", "--chains", "4", "--steps", "4", "--warmup", "1",
                          "--ess-burn", "2", "--ess-window", "20", "--stub-fail-rank", "1"],
                         env=env, capture_output=True, text=True, timeout=120)
    took = time.time() - t0
    assert out.returncode == 3, (out.returncode, out.stderr[-2000:])
    assert took < 60, took
    pids = [int(p) for ln in out.stderr.splitlines() if ln.startswith("bench launcher: rank pids")
            for p in ln.split()[4:]]
    assert len(pids) == 3
    for pid in pids:
        try:
            os.kill(pid, 0)
            alive = True
        except ProcessLookupError:
            alive = False
        assert not alive, f"rank process {pid} left running"


def test_global_diagnostics_converged_datasets_per_model():
    """bench.global_diagnostics with run_sims groups: per model, the ESS of the datasets whose
    every split R-hat <= 1.01 (config 4's ess_by_model[...]['converged_datasets'])."""
    import numpy as np

    import bench
    rng = np.random.default_rng(0)
    C, S = 16, 400
    dsid = np.repeat(np.arange(4), C)
    draws = rng.normal(size=(4 * C, S, 2))
    draws[dsid == 3, :, 0] += np.where(np.arange(C) < C // 2, 5.0, 0.0)[:, None]  # bimodal
    theta = rng.uniform(size=(4 * C, S))
    groups = np.array(["a", "a", "b", "b"])
    ess, rhat, by, conv = bench.global_diagnostics(draws, theta, dsid, ["p0", "p1"],
                                                   np.array([True] * 4), groups)
    assert conv["a"][1:] == [2, 2] and conv["b"][1:] == [1, 2]
    assert by["b"][1]["p0"] > 1.5 and max(by["a"][1].values()) <= 1.01
    # the converged datasets' ESS is the per-dataset ESS summed over them
    assert 0 < conv["b"][0]["p0"] < by["b"][0]["p0"]
