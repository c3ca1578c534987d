#!/usr/bin/env python3
"""A/B of the values-only tridiagonal / bidiagonal stage on one GPU: the host
QR iterations (sterf in heev, the values-only bdsqr in svd_vals; the defaults)
against Sturm-count bisection on the device (stebz / bdsbz, method_eig /
method_svd "bisection"), under both reduction methods.

  python scripts/values_method_ab.py [--out FILE] [--sizes 2048,4096,8192] [--nb 256]

Every size is a child process under its own time limit, one at a time; the
chain stops at the first size that fails.  Inside a size the two methods
alternate round by round after one warm-up round; the median over the timed
rounds is reported, for the whole driver and for the host trace blocks of its
stages (sterf / bdsqr against stebz / bdsbz).  Then the bisection stage alone,
on the (d, e) of a random tridiagonal / bidiagonal of the same order, for
P = 1, the powers of two up to 64 and the P the library chooses (median of 3,
the trace block of the stage: upload, launch, fetch and the one
synchronisation)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = ["he2hb", "hb2st", "hetrd", "sterf", "stebz", "ge2tb", "tb2bd", "gebrd", "bdsqr", "bdsbz"]


def limit(n):
    return 240 + int(240 * (n / 4096.0) ** 2)   # seconds


def spans_of(s, names):
    out = {b: 0.0 for b in names}
    for name, start, stop, lane in s.trace.events():
        if lane < 100 and name in out:
            out[name] += stop - start
    return out


def drivers(a, n, s, np):
    nb = a.nb
    A = s.Matrix(n, n, nb, np.float64)
    A.insertLocalTiles(s.target_of("d"))
    cases = [("svd_vals", "method_gebrd", "method_svd", "qr"), ("heev values only", "method_hetrd", "method_eig", "dc")]
    for what, red_key, meth_key, default in cases:
        for red in ("two_stage", "one_stage"):
            methods = [default, "bisection"]
            total = {me: [] for me in methods}
            stage = {me: {b: [] for b in BLOCKS} for me in methods}
            values = {}
            for rnd in range(a.rounds + 1):
                for me in methods:
                    s._slate.generate_matrix_d("rands", A, 100 + rnd, -1.0, s.opts("d"))
                    s.sync()
                    s.trace.clear()
                    kw = {red_key: red, meth_key: me}
                    t0 = time.perf_counter()
                    if what == "svd_vals":
                        w = s.svd_vals(A, target="d", **kw)
                    else:
                        w = s.heev(s.HermitianMatrix(s.Uplo.Lower, A), None, target="d", **kw)
                    s.sync()
                    dt = time.perf_counter() - t0
                    values[me] = np.asarray(w)
                    if rnd == 0:
                        continue
                    total[me].append(dt)
                    sp = spans_of(s, BLOCKS)
                    for b in BLOCKS:
                        stage[me][b].append(sp[b])
                assert np.abs(values["bisection"] - values[default]).max() <= 1e-10 * np.abs(values[default]).max()
            base = statistics.median(total[default])
            for me in methods:
                t = statistics.median(total[me])
                print(f"{what} n {n} nb {nb}  {red_key}={red}  {meth_key}={me:9s} {t * 1e3:9.1f} ms  x{base / t:5.2f} vs "
                      f"{default}  (min {min(total[me]) * 1e3:.1f}, max {max(total[me]) * 1e3:.1f})", flush=True)
                for b in BLOCKS:
                    m = statistics.median(stage[me][b])
                    if m > 0:
                        print(f"    {b:8s} {m * 1e3:9.1f} ms", flush=True)
            st = s.ops.stebz_stats()
            print(f"    stebz_stats of the last bisection call: {st}", flush=True)


def stage_alone(a, n, s, np):
    rng = np.random.default_rng(n)
    d, e = rng.standard_normal(n), rng.standard_normal(n - 1)
    saved = os.environ.pop("SLATE_STEBZ_POINTS", None)
    for name, fn in (("bdsbz", s.bdsbz), ("stebz", s.stebz)):
        ref = None
        for p in ["chosen", 1, 2, 4, 8, 16, 32, 64]:
            if p == "chosen":
                os.environ.pop("SLATE_STEBZ_POINTS", None)
            else:
                os.environ["SLATE_STEBZ_POINTS"] = str(p)
            ts = []
            for rnd in range(4):
                s.trace.clear()
                w = fn(d, e, target="d")
                if rnd:
                    ts.append(spans_of(s, [name])[name])
            st = s.ops.stebz_stats()
            ref = w if ref is None else ref
            assert np.abs(w - ref).max() <= 64 * np.finfo(np.float64).eps * max(np.abs(d).max(), np.abs(e).max())
            print(f"{name} alone n {n} (order counted {st['n']}), device, P {str(p):6s} -> points {st['points']:2d}  "
                  f"{statistics.median(ts) * 1e3:9.2f} ms  (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f})  "
                  f"steps {st['steps']}, launches {st['launches']}, host_syncs {st['host_syncs']}", flush=True)
    os.environ.pop("SLATE_STEBZ_POINTS", None)
    if saved is not None:
        os.environ["SLATE_STEBZ_POINTS"] = saved


def step(a, n):
    import numpy as np
    import slate_d35_amd as s
    s.trace.on()
    drivers(a, n, s, np)
    stage_alone(a, n, s, np)
    s.trace.off()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", type=int, default=0, help="(internal) run one size in this process")
    ap.add_argument("--sizes", default="2048,4096,8192")
    ap.add_argument("--nb", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per method (after one warm-up round)")
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, ROOT)
        step(a, a.step)
        return 0
    lines = [f"# values_method_ab: values-only svd_vals and heev, float64, nb {a.nb}, one GPU, rounds {a.rounds}; "
             "median of the timed rounds, methods alternating; stage lines are host trace blocks"]
    rc = 0
    for n in [int(x) for x in a.sizes.split(",") if x]:
        cmd = ["timeout", "-k", "10", str(limit(n)), sys.executable, os.path.abspath(__file__), "--step", str(n),
               "--nb", str(a.nb), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        if r.returncode != 0:
            lines.append(f"# --step {n} ended with status {r.returncode}: stopping")
            print(lines[-1], flush=True)
            rc = r.returncode
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
