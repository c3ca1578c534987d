#!/usr/bin/env python3
"""A/B of Option::MethodSVD on one GPU: svd with vectors through the bidiagonal
QR iteration (bdsqr, the default) against the divide and conquer (bdsdc).

  python scripts/svd_method_ab.py [--out FILE] [--sizes 2048,8192] [--nb 256]

Every size is a child process under its own time limit, one at a time; the
chain stops at the first size that fails.  Inside a size the two methods
alternate round by round after one warm-up round; the median over the timed
rounds is reported, for the whole svd and for the host trace blocks of the
bidiagonal stage (bdsqr against bdsdc and its parts).  After the timings the
deflation of the last divide and conquer is listed per tree level."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ["qr", "dc"]
BLOCKS = ["bdsqr", "bdsdc", "bdsdc_leaves", "bdsdc_m_deflate", "bdsdc_m_secular", "bdsdc_m_matrix", "bdsdc_m_gemm"]


def limit(n):
    return 120 + int(60 * (n / 4096.0) ** 2)   # seconds


def step(a, n):
    import numpy as np
    import slate_d35_amd as s
    nb = a.nb
    A, U, VT = (s.Matrix(n, n, nb, np.float64) for _ in range(3))
    for M in (A, U, VT):
        M.insertLocalTiles(s.target_of("d"))
    total = {me: [] for me in METHODS}
    stage = {me: {b: [] for b in BLOCKS} for me in METHODS}
    stats = None
    s.trace.on()
    for rnd in range(a.rounds + 1):
        for me in METHODS:
            s._slate.generate_matrix_d("rands", A, 100 + rnd, -1.0, s.opts("d"))
            s.sync()
            s.trace.clear()
            t0 = time.perf_counter()
            sv = s.svd(A, U, VT, target="d", method_svd=me)
            s.sync()
            dt = time.perf_counter() - t0
            assert np.all(np.diff(sv) <= 0) and sv[-1] >= 0, me
            if me == "dc":
                stats = s.ops.bdsdc_stats()
                assert stats["launches_secular"] > 0, stats
            if rnd == 0:
                continue
            total[me].append(dt)
            spans = {b: 0.0 for b in BLOCKS}
            for name, start, stop, lane in s.trace.events():
                if lane < 100 and name in spans:
                    spans[name] += stop - start
            for b in BLOCKS:
                stage[me][b].append(spans[b])
    s.trace.off()
    base = statistics.median(total["qr"])
    for me in METHODS:
        t = statistics.median(total[me])
        print(f"svd n {n} nb {nb}  method_svd={me}  {t * 1e3:9.1f} ms  x{base / t:5.2f} vs qr"
              f"  (min {min(total[me]) * 1e3:.1f}, max {max(total[me]) * 1e3:.1f})", flush=True)
        for b in BLOCKS:
            m = statistics.median(stage[me][b])
            if m > 0:
                print(f"    {b:16s} {m * 1e3:9.1f} ms", flush=True)
    print(f"    last dc: {stats['merges']} merges, {stats['deflated']} of {stats['columns']} columns deflated; "
          f"kernel launches secular {stats['launches_secular']}, zhat {stats['launches_zhat']}, "
          f"merge matrices {stats['launches_matrix']}", flush=True)
    for lev, (c, d) in enumerate(zip(stats["level_columns"], stats["level_deflated"])):
        print(f"    level {lev}: {d:6d} of {c:6d} columns deflated ({100.0 * d / max(c, 1):5.1f} %)", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", type=int, default=0, help="(internal) run one size in this process")
    ap.add_argument("--sizes", default="2048,8192")
    ap.add_argument("--nb", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per method (after one warm-up round)")
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, ROOT)
        step(a, a.step)
        return 0
    lines = [f"# svd_method_ab: float64, nb {a.nb}, one GPU, rounds {a.rounds}; median of the timed rounds, "
             "methods alternating; stage lines are host trace blocks"]
    rc = 0
    for n in (int(x) for x in a.sizes.split(",")):
        cmd = ["timeout", "-k", "10", str(limit(n)), sys.executable, os.path.abspath(__file__), "--step", str(n),
               "--nb", str(a.nb), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            lines.append(f"# size {n} ended with status {r.returncode}: stopping")
            print(lines[-1], flush=True)
            rc = r.returncode
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
