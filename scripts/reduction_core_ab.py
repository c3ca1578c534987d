#!/usr/bin/env python3
"""A/B of two builds of this project on the one-stage reductions hetrd, gebrd
and geqp3 on one GPU: the same bits, and the same speed.

  python scripts/reduction_core_ab.py PARENT_TREE NEW_TREE [--out FILE] [--rounds 5] [--skip-timing]

A tree is a checkout in which `make` has run (its slate_d35_amd package is
imported from there).  Two builds cannot live in one process, so every
measurement is a child process of this script that imports one of them; the
children run one at a time, each under its own time limit, and the chain stops
at the first one that fails.

Bits: one child per build runs every case below on the same seeded inputs and
prints the SHA-256 of every output (A as left, d, e or jpvt, the T and tau
arrays; y for the three products alone).  The two lists must be equal.
 - hetrd at n = 2, 66, 200; gebrd at 65 x 1, 130 x 130, 200 x 150; geqp3 at
   64 x 64, 200 x 150, 150 x 200, in float32 and float64; one float64 case each
   at order 3000 (more than one row tile per wave, more than one chunk)
 - geqp3 on the "lowrank" float32 and the "cancel" inputs of
   tests/test_geqp3.py, which must run the recompute kernel on both builds
 - symv_lower, gemv_t_block and gemv_n_block at m (or m x m + 2) = 1, 63, 65,
   1000 with a row and column offset of 3

Speed: float64, nb 256, n = 2048 and 4096.  A child times one call of each
routine after a warm-up call of it; the children alternate parent, new, parent
for `rounds` rounds.  The two parent series give two medians from interleaved
halves, whose distance is the spread of the measurement; the new median is
held against the median of all parent runs."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DTS = ("float32", "float64")
HETRD = [2, 66, 200]
GEBRD = [(65, 1), (130, 130), (200, 150)]
GEQP3 = [(64, 64), (200, 150), (150, 200)]
BIG = 3000
ALONE = [1, 63, 65, 1000]
TIMED = [2048, 4096]


def sha(x):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]


def hash_child():
    import numpy as np
    import torch
    import slate_d35_amd as s
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_geqp3 import make
    out = {}

    def mat(m, n, dt, seed, sym=False):
        a = np.random.default_rng(seed).standard_normal((m, n))
        return ((a + a.T) / 2 if sym else a).astype(dt)

    def put(key, A, vecs, Ts):
        out[key] = [sha(s.to_numpy(A))] + [sha(np.asarray(v)) for v in vecs] + \
                   [sha(s.to_numpy(t)) for T in Ts for t in T]

    def hetrd(n, dt):
        A = s.from_numpy(mat(n, n, dt, n, True), nb=64, target="d")
        d, e, T = s.hetrd(s.HermitianMatrix(s.Uplo.Lower, A), target="d")
        put(f"hetrd {dt} {n}", A, (d, e), (T,))

    def gebrd(m, n, dt):
        A = s.from_numpy(mat(m, n, dt, m + n), nb=64, target="d")
        d, e, TQ, TP = s.gebrd(A, target="d")
        put(f"gebrd {dt} {m}x{n}", A, (d, e), (TQ, TP))

    def geqp3(a, name, recompute=False):
        A = s.from_numpy(np.array(a), nb=64, target="d")
        jpvt, T = s.geqp3(A, target="d")
        rec = s.ops.geqp3_stats()["norm_recomputes"]
        assert not recompute or rec > 0, (name, rec)
        put(f"geqp3 {name}" + (f" norm_recomputes {rec}" if recompute else ""), A, (jpvt,), (T,))

    for dt in DTS:
        for n in HETRD:
            hetrd(n, dt)
        for m, n in GEBRD:
            gebrd(m, n, dt)
        for m, n in GEQP3:
            geqp3(mat(m, n, dt, m + 2 * n), f"{dt} {m}x{n}")
    geqp3(make("lowrank", np.float32), "lowrank float32", True)
    for dt in DTS:
        geqp3(make("cancel", np.dtype(dt)), f"cancel {dt}", True)
    hetrd(BIG, "float64")
    gebrd(BIG, BIG, "float64")
    geqp3(mat(BIG, BIG, "float64", 9), f"float64 {BIG}x{BIG}")
    # the three products alone: a row-major (cols x ld) tensor is the column-major ld x cols matrix
    off = 3
    for dt in DTS:
        for m in ALONE:
            rows, cols = m + 2 + off, m + off
            a = mat(cols, rows, dt, 7 * m)
            At = torch.from_numpy(a).to("cuda")
            xr = torch.from_numpy(mat(1, rows - off, dt, m + 1)[0].copy()).to("cuda")
            xc = torch.from_numpy(mat(1, cols - off, dt, m + 2)[0].copy()).to("cuda")
            out[f"symv_lower {dt} {m}"] = [sha(s.ops.symv_lower(At, xc, off).cpu().numpy())]
            out[f"gemv_t_block {dt} {m + 2}x{m}"] = [sha(s.ops.gemv_t_block(At, xr, off, off).cpu().numpy())]
            out[f"gemv_n_block {dt} {m + 2}x{m}"] = [sha(s.ops.gemv_n_block(At, xc, off, off).cpu().numpy())]
    print("RESULT " + json.dumps(out), flush=True)


def time_child():
    import numpy as np
    import slate_d35_amd as s
    out = {}
    for n in TIMED:
        a = np.random.default_rng(n).standard_normal((n, n))
        sym = (a + a.T) / 2
        runs = {"hetrd": lambda A: s.hetrd(s.HermitianMatrix(s.Uplo.Lower, A), target="d"),
                "gebrd": lambda A: s.gebrd(A, target="d"),
                "geqp3": lambda A: s.geqp3(A, target="d")}
        for name, fn in runs.items():
            for timed in (False, True):
                A = s.from_numpy(sym if name == "hetrd" else a, nb=256, target="d")
                s.sync()
                t0 = time.perf_counter()
                fn(A)
                s.sync()
                if timed:
                    out[f"{name} {n}"] = (time.perf_counter() - t0) * 1e3
    print("RESULT " + json.dumps(out), flush=True)


def child(tree, mode, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, tree], capture_output=True,
                       text=True, timeout=limit)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        sys.stdout.write(r.stdout[-3000:] + r.stderr[-3000:])
        raise SystemExit(f"child {mode} of {tree} failed with status {r.returncode}")
    return json.loads(lines[-1][7:])


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        sys.path.insert(0, os.path.abspath(sys.argv[3]))
        import slate_d35_amd as s
        assert os.path.abspath(s.__file__).startswith(os.path.abspath(sys.argv[3]) + os.sep), s.__file__
        assert s.device_available(), "a HIP device is needed"
        return hash_child() if sys.argv[2] == "hash" else time_child()
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-timing", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    hp, hn = child(a.parent, "hash", 300), child(a.new, "hash", 300)
    say("SHA-256 (first 16 digits) of every output: A as left | d, e or jpvt | T and tau arrays; y of the products")
    differ = [k for k in hp if hp[k] != hn.get(k)] + [k for k in hn if k not in hp]
    for k in hp:
        say(f"  {k:42s} {'same' if hp[k] == hn.get(k) else 'DIFFERENT'}  parent {' '.join(hp[k])}")
        if hp[k] != hn.get(k):
            say(f"  {'':42s}            new    {' '.join(hn.get(k, []))}")
    say(f"{len(hp)} cases, {len(differ)} with different bits" + (": " + ", ".join(differ) if differ else ""))
    if not a.skip_timing:
        series = {"parent_a": [], "new": [], "parent_b": []}
        for _ in range(a.rounds):
            for who in series:
                series[who].append(child(a.new if who == "new" else a.parent, "time", 300))
        say()
        say(f"milliseconds, float64, nb 256, one call after a warm-up call, median of {a.rounds} alternating runs")
        say(f"  {'case':12s} {'parent':>9s} {'new':>9s} {'new-parent':>11s} {'spread':>8s}  parent halves     verdict")
        for k in series["new"][0]:
            med = {w: statistics.median(r[k] for r in series[w]) for w in series}
            parent = statistics.median([r[k] for w in ("parent_a", "parent_b") for r in series[w]])
            spread = abs(med["parent_a"] - med["parent_b"])
            diff = med["new"] - parent
            verdict = "within the spread" if abs(diff) <= spread else \
                "faster by more than the spread" if diff < 0 else "SLOWER by more than the spread"
            say(f"  {k:12s} {parent:9.2f} {med['new']:9.2f} {diff:+11.2f} {spread:8.2f}  {med['parent_a']:7.2f} "
                f"{med['parent_b']:7.2f}  {verdict}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
