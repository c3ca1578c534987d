#!/usr/bin/env python3
"""A/B of Option::GemmPrecision on one GPU: the fp32 MFMA kernels ("native")
against the split-operand bf16 kernel (bf16, bf16x3, bf16x6; gemm_bf16s.hip).

  python scripts/gemm_lowprec_ab.py [--out FILE] [--n 32768] [--nb 1024]

Steps, each a child process under its own time limit, one at a time; the chain
stops at the first step that fails:
  gemm          the trailing-update shapes 32768 x 32768 x 1024 (NT and NN) and
                16384 x 16384 x 512 (NT and NN), C = C - A op(B)
  getrf_tntpiv  fp32 LU (tournament pivoting) at n, nb
  potrf         fp32 Cholesky (lower) at n, nb
Inside a step the modes alternate round by round after one warm-up round, and
the median over the timed rounds is reported.  TFLOP/s counts 2mnk (gemm),
2n^3/3 (LU) and n^3/3 (Cholesky) whatever the mode."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["native", "bf16", "bf16x3", "bf16x6"]
STEP_LIMIT = {"gemm": 240, "getrf_tntpiv": 300, "potrf": 300}   # seconds


def step_gemm(a):
    import torch
    import slate_d35_amd as s
    shapes = [(32768, 32768, 1024), (16384, 16384, 512)]
    if a.n < 32768:   # rehearsal sizes
        shapes = [(a.n, a.n, max(32, a.n // 32))]
    for (m, n, k) in shapes:
        g = torch.Generator(device="cuda").manual_seed(1)
        # column-major X = row-major tensor of X^T
        A = torch.rand((k, m), generator=g, device="cuda", dtype=torch.float32) * 2 - 1     # A: m x k
        Bt = torch.rand((k, n), generator=g, device="cuda", dtype=torch.float32) * 2 - 1    # B^T: n x k (NT)
        B = torch.rand((n, k), generator=g, device="cuda", dtype=torch.float32) * 2 - 1     # B: k x n (NN)
        C = torch.zeros((n, m), device="cuda", dtype=torch.float32)
        for form, tb, Bop in (("NT", "T", Bt), ("NN", "N", B)):
            def run(mode):
                if mode == "native":
                    s.ops.gemm("N", tb, -1.0, A, Bop, 1.0, C)
                else:
                    s.ops.gemm_lowprec(mode, "N", tb, -1.0, A, Bop, 1.0, C)
            times = {mo: [] for mo in MODES}
            for rnd in range(a.rounds + 1):
                for mo in MODES:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.reps):
                        run(mo)               # each call ends in a stream synchronize
                    dt = (time.perf_counter() - t0) / a.reps
                    if rnd > 0:
                        times[mo].append(dt)
            base = statistics.median(times["native"])
            for mo in MODES:
                t = statistics.median(times[mo])
                print(f"gemm {form} {m} x {n} x {k:5d}  {mo:7s} {t * 1e3:9.3f} ms  {2.0 * m * n * k / t / 1e12:7.1f} TFLOP/s"
                      f"  x{base / t:5.2f} vs native  (min {min(times[mo]) * 1e3:.3f}, max {max(times[mo]) * 1e3:.3f})",
                      flush=True)
        del A, B, Bt, C


def step_factor(a, which):
    import numpy as np
    import slate_d35_amd as s
    n, nb = a.n, a.nb
    M = s.Matrix(n, n, nb, np.float32)
    M.insertLocalTiles(s.target_of("d"))
    o = dict(target="d", lookahead=1)
    kind = "spd" if which == "potrf" else "rands"
    flops = n ** 3 / 3.0 if which == "potrf" else 2.0 * n ** 3 / 3.0
    times = {mo: [] for mo in MODES}
    for rnd in range(a.rounds + 1):
        for mo in MODES:
            s._slate.generate_matrix_s(kind, M, 100 + rnd, -1.0, s.opts("d"))
            c0 = s.ops.lowprec_gemm_calls()
            t0 = time.perf_counter()
            if which == "potrf":
                info = s.potrf(s.HermitianMatrix(s.Uplo.Lower, M), gemm_precision=mo, **o)
            else:
                info, _ = s.getrf_tntpiv(M, gemm_precision=mo, **o)
            dt = time.perf_counter() - t0
            assert info == 0, (which, mo, info)
            assert (s.ops.lowprec_gemm_calls() > c0) == (mo != "native"), (which, mo)
            if rnd > 0:
                times[mo].append(dt)
    base = statistics.median(times["native"])
    for mo in MODES:
        t = statistics.median(times[mo])
        print(f"s{which} n {n} nb {nb}  {mo:7s} {t * 1e3:9.1f} ms  {flops / t / 1e12:7.1f} TFLOP/s  x{base / t:5.2f} vs native"
              f"  (min {min(times[mo]) * 1e3:.1f}, max {max(times[mo]) * 1e3:.1f})", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", default="", help="(internal) run one step in this process")
    ap.add_argument("--steps", default="gemm,getrf_tntpiv,potrf")
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--nb", type=int, default=1024, help="tile size of the factorizations (the fp32 LU's in gesv_mixed)")
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds per mode (after one warm-up round)")
    ap.add_argument("--reps", type=int, default=5, help="gemm calls per timing")
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, ROOT)
        if a.step == "gemm":
            step_gemm(a)
        else:
            step_factor(a, a.step)
        return 0
    lines = [f"# gemm_lowprec_ab: n {a.n} nb {a.nb} rounds {a.rounds} reps {a.reps}; median of the timed rounds, "
             "modes alternating"]
    rc = 0
    for st in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT[st]), sys.executable, os.path.abspath(__file__), "--step", st,
               "--n", str(a.n), "--nb", str(a.nb), "--rounds", str(a.rounds), "--reps", str(a.reps)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            lines.append(f"# step {st} ended with status {r.returncode}: stopping")
            print(lines[-1], flush=True)
            rc = r.returncode
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
