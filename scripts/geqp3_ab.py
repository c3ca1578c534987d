#!/usr/bin/env python3
"""geqp3 (QR with column pivoting) against geqrf on the same matrix, one GPU.

  python scripts/geqp3_ab.py [--out FILE] [--sizes 2048,4096,8192] [--nb 256]

Every size is a child process under its own time limit, one at a time; the
chain stops at the first size that fails.  Inside a size the two routines
alternate round by round on the same random float64 square matrix after one
warm-up round; the median over the timed rounds is reported.  geqp3 enqueues
without synchronising, so its split into pivot search and swap / product A^T v
/ other column kernels / trailing GEMMs / T factors comes from one extra run
with SLATE_GEQP3_PROFILE=1 (device events between the kernels; that run is not
in the medians), with the launches per column and the bytes the product reads
against the 6.3 TB/s copy rate."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTINES = ["geqrf", "geqp3"]
HBM = 6.3e12


def limit(n):
    return 120 + int(60 * (n / 4096.0) ** 2)   # seconds


def step(a, n):
    import numpy as np
    import slate_d35_amd as s
    nb = a.nb
    A = s.Matrix(n, n, nb, np.float64)
    A.insertLocalTiles(s.target_of("d"))
    total = {r: [] for r in ROUTINES}
    for rnd in range(a.rounds + 1):
        for r in ROUTINES:
            s._slate.generate_matrix_d("rands", A, 100 + rnd, -1.0, s.opts("d"))
            s.sync()
            t0 = time.perf_counter()
            if r == "geqrf":
                s.geqrf(A, target="d")
            else:
                jpvt, T = s.geqp3(A, target="d")
            s.sync()
            dt = time.perf_counter() - t0
            if r == "geqp3":
                assert sorted(jpvt.tolist()) == list(range(n))
            if rnd:
                total[r].append(dt)
    base = statistics.median(total["geqrf"])
    for r in ROUTINES:
        t = statistics.median(total[r])
        print(f"{r} n {n} nb {nb} float64  {t * 1e3:9.1f} ms  x{t / base:6.2f} of geqrf"
              f"  (min {min(total[r]) * 1e3:.1f}, max {max(total[r]) * 1e3:.1f})", flush=True)
    st = s.ops.geqp3_stats()
    launches = sum(v for k, v in st.items() if k.startswith("launches_"))
    print(f"    geqp3 n {n}: {st['columns']} columns, {st['panels']} panels, {launches} kernel launches = "
          f"{launches / st['columns']:.2f} per column, {st['norm_recomputes']} norm recomputes, "
          f"{st['host_syncs']} host sync", flush=True)
    # the split of geqp3, from device events of one extra run
    os.environ["SLATE_GEQP3_PROFILE"] = "1"
    s._slate.generate_matrix_d("rands", A, 100, -1.0, s.opts("d"))
    s.geqp3(A, target="d")
    s.sync()
    st = s.ops.geqp3_stats()
    nbytes = 8.0 * n ** 3 / 3   # sum over the columns of the trailing block
    print(f"    geqp3 split n {n} (device events, one profiled run): pivot + swap {st['ms_pivot']:.1f} ms, product "
          f"{st['ms_product']:.1f} ms, other column kernels {st['ms_panel']:.1f} ms, trailing GEMMs "
          f"{st['ms_gemm']:.1f} ms, T factors {st['ms_larft']:.1f} ms; the product reads {nbytes / 1e9:.1f} GB = "
          f"{nbytes / max(st['ms_product'], 1e-9) / 1e6:.0f} GB/s = "
          f"{100 * nbytes / max(st['ms_product'], 1e-9) * 1e3 / HBM:.1f} % of 6.3 TB/s", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", type=int, default=0, help="(internal) run one size in this process")
    ap.add_argument("--sizes", default="2048,4096,8192")
    ap.add_argument("--nb", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per routine (after one warm-up round)")
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, ROOT)
        step(a, a.step)
        return 0
    lines = [f"# geqp3_ab: geqp3 against geqrf, float64, square, nb {a.nb}, one GPU, rounds {a.rounds}; median of "
             "the timed rounds, routines alternating on the same matrix"]
    rc = 0
    for n in [int(x) for x in a.sizes.split(",") if x]:
        cmd = ["timeout", "-k", "10", str(limit(n)), sys.executable, os.path.abspath(__file__), "--step", str(n),
               "--nb", str(a.nb), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            lines.append(f"# n {n} ended with status {r.returncode}: stopping")
            print(lines[-1], flush=True)
            rc = r.returncode
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
