"""bench.py contract (host target, small n): one JSON line with the
BASELINE metric, and the fail-fast watchdog that turns a hung step into
exit code 124 instead of a run that holds the node until the driver's limit."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _bench(args, env_extra=None, timeout=300):
    env = dict(os.environ)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout)


def test_bench_json_line():
    r = _bench(["--dim", "512", "--nb", "128", "--steps", "1", "--warmup", "0", "--full", "--extras", "none"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert line["metric"] == base["metric"] and line["n_gpus"] == 1 and line["steps"] == 1
    assert set(line["routines"]) == {"dgemm", "dpotrf", "dgetrf", "dgeqrf"}
    assert all(v["check"] == "pass" for v in line["routines"].values())


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps, does no residual
    check and no extra config, and reports ms_per_step = one step of the four
    routines.  --dump-outputs writes what the last timed step returned, as
    float64, identically in two runs with the same arguments; C, L and R are
    compared with numpy on the same generated inputs (n = 256 <= the sample
    size, so whole matrices are written)."""
    import numpy as np
    import slate_d35_amd as s

    n, nb, steps, warmup = 256, 64, 2, 1
    args = ["--dim", str(n), "--nb", str(nb), "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs"]
    runs = []
    for d in ("a", "b"):
        r = _bench(args + [str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-2000:]
        runs.append(r)
    line = _last_json(runs[0].stdout)
    assert line["steps"] == steps and line["configs"] == {}
    assert all(v["steps"] == steps and "check" not in v for v in line["routines"].values())
    assert runs[0].stderr.count(" timed: ") == 4 * steps and runs[0].stderr.count(" warm: ") == 4 * warmup
    assert abs(line["ms_per_step"] - sum(v["ms"] for v in line["routines"].values())) < 1e-2
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["dgemm_C.npy", "dgeqrf_QR.npy", "dgeqrf_T0.npy", "dgetrf_LU.npy", "dgetrf_piv.npy",
                     "dpotrf_L.npy"]
    out = {}
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and x.size > 0 and np.array_equal(x, y), f
        out[f[:-4]] = x
    assert sum(x.nbytes for x in out.values()) <= 64 << 20

    def gen(kind, seed):
        M = s.Matrix(n, n, nb, np.float64)
        M.insertLocalTiles(s.Target.Host)
        s._slate.generate_matrix_d(kind, M, seed, -1.0, s.opts("h"))
        return s.to_numpy(M)

    eps = np.finfo(np.float64).eps
    last = 100 + warmup + steps - 1     # seed of the last timed step
    A, B = gen("rands", 1), gen("rands", 2)
    assert np.abs(out["dgemm_C"] - A @ B).max() <= 4 * n * eps * np.abs(A).max() * np.abs(B).max()
    S, L = gen("spd", last), out["dpotrf_L"]
    assert np.array_equal(L, np.tril(L))
    assert np.abs(L @ L.T - S).max() <= 8 * n * eps * np.abs(S).max()
    G = gen("rands", last)
    assert out["dgetrf_LU"].shape == (n, n) and out["dgetrf_piv"].shape == (n, 2)
    R, Rref = np.triu(out["dgeqrf_QR"]), np.linalg.qr(G, mode="r")
    assert np.abs(np.abs(R) - np.abs(Rref)).max() <= 8 * n * eps * np.abs(G).max() * np.sqrt(n)


def test_bench_watchdog_exits_124():
    # host target on two threads: the n = 4096 QR step then takes far longer than
    # the 1 s limit on any machine (a GPU finishes it in 0.1 s and nothing would fire)
    r = _bench(["--target", "h", "--dim", "4096", "--routines", "dgeqrf", "--steps", "1", "--warmup", "0",
                "--extras", "none", "--check", "no"],
               env_extra={"SLATE_BENCH_STEP_TIMEOUT": "1", "OMP_NUM_THREADS": "2"})
    assert r.returncode == 124, (r.returncode, r.stderr[-2000:])
    assert "WATCHDOG rank 0: 'dgeqrf step 0'" in r.stderr


def _last_json(out):
    return json.loads([ln for ln in out.strip().splitlines() if ln.startswith("{")][-1])


def test_bench_self_launch_4_ranks():
    """`python3 bench.py --gpus 4` with no launcher environment spawns its own
    four rank processes (host target and host communicators, also where a GPU
    is visible: four ranks cannot share one device over RCCL without
    SLATE_BENCH_FAKE_HOSTS); the JSON reports what the communicators that
    were actually created saw."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--target", "h",
                        "--dim", "1024", "--nb", "128", "--steps", "1", "--warmup", "0", "--full", "--extras", "none"],
                       env=dict(env, OMP_NUM_THREADS="2"),
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _last_json(r.stdout)
    assert line["n_gpus"] == 4
    comm = line["config"]["comm"]
    assert comm["world"] == 4 and comm["row"] * comm["col"] == 4 and comm["grid"] == [2, 2]
    assert comm["launcher"] == "self" and len(comm["devices"]) == 4
    assert all(v["check"] == "pass" for v in line["routines"].values())
    # per-routine grids of the 4-GPU defaults (bench.GRID_PER, from the
    # critical-path sweep): QR and Cholesky on 4 x 1, the rest on the job's 2 x 2
    grids = {k: v["grid"] for k, v in line["routines"].items()}
    assert grids == {"dgemm": "2x2", "dpotrf": "4x1", "dgetrf": "2x2", "dgeqrf": "4x1"}, grids


def test_bench_self_launch_propagates_failure():
    """A rank that fails (here: its watchdog fires) makes the launcher exit
    with that rank's code and stop the other ranks."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(SLATE_BENCH_STEP_TIMEOUT="1", OMP_NUM_THREADS="2", SLATE_BENCH_RANK_GRACE="20")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--target", "h", "--dim", "4096",
                        "--routines", "dgeqrf", "--steps", "1", "--warmup", "0", "--extras", "none", "--check", "no"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 124, (r.returncode, r.stderr[-2000:])
    assert "WATCHDOG" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 8])
def test_bench_self_launch_rccl_one_gpu(n):
    """`bench.py --gpus N` launched with no torchrun on the one-GPU box: N
    rank processes, each with its own NCCL_HOSTID (SLATE_BENCH_FAKE_HOSTS) so
    RCCL forms real N-rank communicators on one device.  Asserts the
    communicator sizes RCCL reports and the residual checks."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SLATE_COMM")}
    env.update(SLATE_BENCH_FAKE_HOSTS="1", OMP_NUM_THREADS="2", NCCL_DEBUG="WARN")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--dim", "4096",
                        "--nb", "256", "--steps", "1", "--warmup", "0", "--full", "--extras", "none"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    line = _last_json(r.stdout)
    comm = line["config"]["comm"]
    assert line["n_gpus"] == n and comm["backend"] == "rccl" and comm["world"] == n
    assert comm["row"] * comm["col"] == n and comm["devices"] == [0] * n
    assert all(v["check"] == "pass" for v in line["routines"].values())
