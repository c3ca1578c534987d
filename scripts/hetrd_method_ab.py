#!/usr/bin/env python3
"""A/B of Option::MethodHetrd on one GPU: heev with vectors through the
two-stage reduction (he2hb + the host bulge chase hb2st, the default) against
the one-stage hetrd (sytrd panels with a device symv per column).

  python scripts/hetrd_method_ab.py [--out FILE] [--sizes 2048,4096,8192] [--nb 256]

Every size is a child process under its own time limit, one at a time; the
chain stops at the first size that fails.  Inside a size the two methods
alternate round by round after one warm-up round; the median over the timed
rounds is reported, for the whole heev and for the host trace blocks of its
stages.  hetrd enqueues without synchronising, so its split into symv / panel
/ syr2k / T factors comes from one extra run with SLATE_HETRD_PROFILE=1
(device events between the kernels; that run is not in the medians).  A last
child times symv_lower alone and reports GB/s of stored bytes, m (m + 1) / 2
elements, against the 6.3 TB/s copy rate."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ["two_stage", "one_stage"]
BLOCKS = ["he2hb", "hb2st", "hetrd", "tridiag_eig", "unmtr_hb2st", "unmtr_he2hb", "unmtr_he2hb_gemm", "unmtr_hetrd"]
HBM = 6.3e12


def limit(n):
    return 120 + int(60 * (n / 4096.0) ** 2)   # seconds


def step(a, n):
    import numpy as np
    import slate_d35_amd as s
    nb = a.nb
    A, Z = (s.Matrix(n, n, nb, np.float64) for _ in range(2))
    for M in (A, Z):
        M.insertLocalTiles(s.target_of("d"))
    H = s.HermitianMatrix(s.Uplo.Lower, A)
    total = {me: [] for me in METHODS}
    stage = {me: {b: [] for b in BLOCKS} for me in METHODS}
    values = {}
    s.trace.on()
    for rnd in range(a.rounds + 1):
        for me in METHODS:
            s._slate.generate_matrix_d("rands", A, 100 + rnd, -1.0, s.opts("d"))
            s.sync()
            s.trace.clear()
            t0 = time.perf_counter()
            w = s.heev(H, Z, target="d", method_hetrd=me)
            s.sync()
            dt = time.perf_counter() - t0
            assert np.all(np.diff(w) >= 0), me
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
        assert np.abs(values["one_stage"] - values["two_stage"]).max() <= 1e-10 * np.abs(values["two_stage"]).max()
    s.trace.off()
    base = statistics.median(total["two_stage"])
    for me in METHODS:
        t = statistics.median(total[me])
        print(f"heev n {n} nb {nb}  method_hetrd={me}  {t * 1e3:9.1f} ms  x{base / t:5.2f} vs two_stage"
              f"  (min {min(total[me]) * 1e3:.1f}, max {max(total[me]) * 1e3:.1f})", flush=True)
        for b in BLOCKS:
            m = statistics.median(stage[me][b])
            if m > 0:
                print(f"    {b:18s} {m * 1e3:9.1f} ms", flush=True)
    # the split of hetrd, from device events of one extra run
    os.environ["SLATE_HETRD_PROFILE"] = "1"
    s._slate.generate_matrix_d("rands", A, 100, -1.0, s.opts("d"))
    s.heev(H, Z, target="d", method_hetrd="one_stage")
    s.sync()
    st = s.ops.hetrd_stats()
    launches = st["launches_column"] + st["launches_larfg"] + st["launches_symv"] + st["launches_correct"]
    print(f"    hetrd split (device events, one profiled run): symv {st['ms_symv']:.1f} ms, panel {st['ms_panel']:.1f} ms, "
          f"syr2k {st['ms_syr2k']:.1f} ms, T factors {st['ms_larft']:.1f} ms; {st['columns']} columns, "
          f"{launches} column-kernel launches, {st['host_syncs']} host sync", flush=True)


def symv(a):
    import torch
    import slate_d35_amd as s
    for m in (8192, 2048):
        A = torch.randn(m, m, dtype=torch.float64, device="cuda")
        x = torch.randn(m, dtype=torch.float64, device="cuda")
        for _ in range(3):
            s.ops.symv_lower(A, x)
        reps = 200
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.ops.symv_lower(A, x, repeat=reps)      # reps products back to back, then one synchronisation
            ts.append((time.perf_counter() - t0) / reps)
        t = statistics.median(ts)
        stored = m * (m + 1) / 2 * 8
        print(f"symv_lower float64 m {m}: {t * 1e6:8.1f} us per product ({reps} back to back, both launches and the "
              f"partial sums included; median of 5)  {stored / t / 1e9:7.1f} GB/s of stored bytes = "
              f"{100 * stored / t / HBM:4.1f} % of 6.3 TB/s", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", type=int, default=0, help="(internal) run one size in this process")
    ap.add_argument("--symv", action="store_true", help="(internal) time symv_lower in this process")
    ap.add_argument("--sizes", default="2048,4096,8192")
    ap.add_argument("--nb", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per method (after one warm-up round)")
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    if a.step or a.symv:
        sys.path.insert(0, ROOT)
        symv(a) if a.symv else step(a, a.step)
        return 0
    lines = [f"# hetrd_method_ab: heev with vectors, float64, nb {a.nb}, one GPU, rounds {a.rounds}; median of the "
             "timed rounds, methods alternating; stage lines are host trace blocks"]
    rc = 0
    jobs = [(["--step", str(n)], limit(n)) for n in (int(x) for x in a.sizes.split(","))] + [(["--symv"], 120)]
    for extra, lim in jobs:
        cmd = ["timeout", "-k", "10", str(lim), sys.executable, os.path.abspath(__file__), *extra,
               "--nb", str(a.nb), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
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
