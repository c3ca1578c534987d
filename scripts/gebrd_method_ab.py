#!/usr/bin/env python3
"""A/B of Option::MethodGebrd on one GPU: svd through the two-stage reduction
(ge2tb + the host bulge chase tb2bd, the default) against the one-stage gebrd
(labrd panels with two device matrix-vector products per column).

  python scripts/gebrd_method_ab.py [--out FILE] [--sizes 2048,4096,8192] [--nb 256]

Every size is a child process under its own time limit, one at a time; the
chain stops at the first size that fails.  Inside a size the two methods
alternate round by round after one warm-up round, for method_svd "qr" and "dc"
with vectors and for a values-only call; the median over the timed rounds is
reported, for the whole svd and for the host trace blocks of its stages.
gebrd enqueues without synchronising, so its split into pass 1 / pass 2 /
panel / trailing GEMMs / T factors comes from one extra run with
SLATE_GEBRD_PROFILE=1 (device events between the kernels; that run is not in
the medians).  A last child times the two product kernels alone, beside
lb::gemv at the same shapes, and reports GB/s of the block's bytes against the
6.3 TB/s copy rate."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ["two_stage", "one_stage"]
BLOCKS = ["ge2tb", "tb2bd", "gebrd", "bdsqr", "bdsdc", "unmbr_gebrd", "unmbr_ge2tb_u", "unmbr_ge2tb_v",
          "unmbr_ge2tb_u_gemm", "unmbr_ge2tb_v_gemm"]
HBM = 6.3e12


def limit(n):
    return 180 + int(150 * (n / 4096.0) ** 2)   # seconds


def step(a, n):
    import numpy as np
    import slate_d35_amd as s
    nb = a.nb
    A, U, VT = (s.Matrix(n, n, nb, np.float64) for _ in range(3))
    for M in (A, U, VT):
        M.insertLocalTiles(s.target_of("d"))
    s.trace.on()
    for mode in ("qr", "dc", "vals"):
        total = {me: [] for me in METHODS}
        stage = {me: {b: [] for b in BLOCKS} for me in METHODS}
        values = {}
        for rnd in range(a.rounds + 1):
            for me in METHODS:
                s._slate.generate_matrix_d("rands", A, 100 + rnd, -1.0, s.opts("d"))
                s.sync()
                s.trace.clear()
                t0 = time.perf_counter()
                if mode == "vals":
                    w = s.svd_vals(A, target="d", method_gebrd=me)
                else:
                    w = s.svd(A, U, VT, target="d", method_gebrd=me, method_svd=mode)
                s.sync()
                dt = time.perf_counter() - t0
                assert np.all(np.diff(w) <= 0), me
                values[me] = w
                if rnd == 0:
                    continue
                total[me].append(dt)
                spans = {b: 0.0 for b in BLOCKS}
                for name, start, stop, lane in s.trace.events():
                    if lane < 100 and name in spans:
                        spans[name] += stop - start
                for b in BLOCKS:
                    stage[me][b].append(spans[b])
            assert np.abs(values["one_stage"] - values["two_stage"]).max() <= 1e-10 * values["two_stage"].max()
        base = statistics.median(total["two_stage"])
        what = "values only" if mode == "vals" else f"vectors, method_svd={mode}"
        for me in METHODS:
            t = statistics.median(total[me])
            print(f"svd n {n} nb {nb}  {what}  method_gebrd={me}  {t * 1e3:9.1f} ms  x{base / t:5.2f} vs two_stage"
                  f"  (min {min(total[me]) * 1e3:.1f}, max {max(total[me]) * 1e3:.1f})", flush=True)
            for b in BLOCKS:
                m = statistics.median(stage[me][b])
                if m > 0:
                    print(f"    {b:18s} {m * 1e3:9.1f} ms", flush=True)
    s.trace.off()
    # the split of gebrd, from device events of one extra run
    os.environ["SLATE_GEBRD_PROFILE"] = "1"
    s._slate.generate_matrix_d("rands", A, 100, -1.0, s.opts("d"))
    s.svd_vals(A, target="d", method_gebrd="one_stage")
    s.sync()
    st = s.ops.gebrd_stats()
    launches = sum(v for k, v in st.items() if k.startswith("launches_"))
    print(f"    gebrd split n {n} (device events, one profiled run): pass 1 {st['ms_pass1']:.1f} ms, pass 2 "
          f"{st['ms_pass2']:.1f} ms, other column kernels {st['ms_panel']:.1f} ms, trailing GEMMs {st['ms_gemm']:.1f} ms, "
          f"T factors {st['ms_larft']:.1f} ms; {st['columns']} columns, {launches} column-kernel launches, "
          f"{st['host_syncs']} host sync", flush=True)


def products(a):
    import torch
    import slate_d35_amd as s
    for m in (8192, 4096, 2048):
        A = torch.randn(m, m, dtype=torch.float64, device="cuda")
        x = torch.randn(m, dtype=torch.float64, device="cuda")
        reps = 200
        for name, fn in (("gemv_t_block (pass 1, A^T u)", s.ops.gemv_t_block), ("gemv_n_block (pass 2, A v)",
                                                                                s.ops.gemv_n_block)):
            for use_lb in (False, True):
                for _ in range(3):
                    fn(A, x, use_lb=use_lb)
                ts = []
                for _ in range(5):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(A, x, repeat=reps, use_lb=use_lb)     # reps products back to back, then one synchronisation
                    ts.append((time.perf_counter() - t0) / reps)
                t = statistics.median(ts)
                nbytes = m * m * 8
                who = "lb::gemv" if use_lb else "block kernel"
                print(f"{name} float64 order {m}, {who:12s}: {t * 1e6:8.1f} us per product ({reps} back to back, the "
                      f"reduction launch included; median of 5)  {nbytes / t / 1e9:7.1f} GB/s of the block's bytes = "
                      f"{100 * nbytes / t / HBM:4.1f} % of 6.3 TB/s", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", type=int, default=0, help="(internal) run one size in this process")
    ap.add_argument("--products", action="store_true", help="(internal) time the product kernels in this process")
    ap.add_argument("--sizes", default="2048,4096,8192")
    ap.add_argument("--nb", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per method (after one warm-up round)")
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    if a.step or a.products:
        sys.path.insert(0, ROOT)
        products(a) if a.products else step(a, a.step)
        return 0
    lines = [f"# gebrd_method_ab: svd, float64, nb {a.nb}, one GPU, rounds {a.rounds}; median of the timed rounds, "
             "methods alternating; stage lines are host trace blocks"]
    rc = 0
    sizes = [int(x) for x in a.sizes.split(",") if x]
    jobs = [(["--step", str(n)], limit(n)) for n in sizes] + [(["--products"], 120)]
    for extra, lim in jobs:
        cmd = ["timeout", "-k", "10", str(lim), sys.executable, os.path.abspath(__file__), *extra,
               "--nb", str(a.nb), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        if r.returncode != 0:
            lines.append(f"# {' '.join(extra)} ended with status {r.returncode}: stopping")
            print(lines[-1], flush=True)
            rc = r.returncode
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
