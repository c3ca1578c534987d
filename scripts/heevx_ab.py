#!/usr/bin/env python3
"""A/B of the subset eigensolver on one GPU: heev with vectors (divide and
conquer, the default) against heevx for all pairs and for the index range
1 .. n / 10, under both reduction methods.

  python scripts/heevx_ab.py [--out profiles/heevx_ab.txt] [--sizes 2048,4096,8192] [--nb 256] [--all-max 2048]

The protocol of values_method_ab.py: every size is a child process under its
own time limit, one at a time; the chain stops at the first size that fails.
Inside a size the variants alternate round by round after one warm-up round;
the median over the timed rounds is reported for the whole driver and for the
host trace blocks of its stages.  stein's device time is split into solve /
orth / transpose by the events of SLATE_STEIN_PROFILE (stein_stats()).
heevx(All) puts every eigenvalue of a large matrix into one cluster, which
stein_orth orthonormalises on one CU in O(n^3): it is measured up to
--all-max only.  The report ends with the compiler's resource usage of the
kernels of csrc/kernels/stein.hip when hipcc is at hand."""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = ["he2hb", "hb2st", "hetrd", "tridiag_eig", "stebz", "stein", "unmtr_hb2st", "unmtr_he2hb_form",
          "unmtr_he2hb_gemm", "unmtr_he2hb", "unmtr_hetrd"]


def limit(n):
    return 240 + int(300 * (n / 4096.0) ** 2)   # seconds


def spans_of(s, names):
    out = {b: 0.0 for b in names}
    for name, start, stop, lane in s.trace.events():
        if lane < 100 and name in out:
            out[name] += stop - start
    return out


def step(a, n):
    os.environ["SLATE_STEIN_PROFILE"] = "1"
    import numpy as np
    import slate_d35_amd as s
    s.trace.on()
    nb = a.nb
    A = s.Matrix(n, n, nb, np.float64)
    A.insertLocalTiles(s.target_of(a.target))
    m10 = max(1, n // 10)
    variants = [("heev", n), ("heevx all", n), ("heevx 1..n/10", m10)]
    if n > a.all_max:
        variants = [v for v in variants if v[0] != "heevx all"]
    for red in ("two_stage", "one_stage"):
        total = {v: [] for v, _ in variants}
        stage = {v: {b: [] for b in BLOCKS} for v, _ in variants}
        split = {v: {k: [] for k in ("ms_solve", "ms_orth", "ms_transpose")} for v, _ in variants}
        stats, values = {}, {}
        for rnd in range(a.rounds + 1):
            for v, cols in variants:
                s._slate.generate_matrix_d("rands", A, 100 + rnd, -1.0, s.opts(a.target))
                Z = s.Matrix(n, cols, nb, np.float64)
                Z.insertLocalTiles(s.target_of(a.target))
                H = s.HermitianMatrix(s.Uplo.Lower, A)
                s.sync()
                s.trace.clear()
                t0 = time.perf_counter()
                if v == "heev":
                    w = s.heev(H, Z, target=a.target, method_hetrd=red)
                elif v == "heevx all":
                    w = s.heevx(H, Z, target=a.target, method_hetrd=red)
                else:
                    w = s.heevx(H, Z, range="index", il=1, iu=m10, target=a.target, method_hetrd=red)
                s.sync()
                dt = time.perf_counter() - t0
                values[v] = np.asarray(w)
                if v != "heev":
                    stats[v] = s.ops.stein_stats()
                if rnd == 0:
                    continue
                total[v].append(dt)
                sp = spans_of(s, BLOCKS)
                for b in BLOCKS:
                    stage[v][b].append(sp[b])
                if v != "heev":
                    for k in split[v]:
                        split[v][k].append(stats[v][k])
            for v, cols in variants:
                ref = values["heev"][:cols]
                assert np.abs(values[v] - ref).max() <= 1e-10 * np.abs(values["heev"]).max(), v
        base = statistics.median(total["heev"])
        for v, cols in variants:
            t = statistics.median(total[v])
            print(f"n {n} nb {nb}  method_hetrd={red}  {v:14s} m {cols:5d} {t * 1e3:10.1f} ms  x{base / t:5.2f} vs heev  "
                  f"(min {min(total[v]) * 1e3:.1f}, max {max(total[v]) * 1e3:.1f})", flush=True)
            for b in BLOCKS:
                mm = statistics.median(stage[v][b])
                if mm > 0:
                    print(f"    {b:17s} {mm * 1e3:10.1f} ms", flush=True)
            if v != "heev":
                sv = {k: statistics.median(x) for k, x in split[v].items()}
                print(f"    stein on the device: solve {sv['ms_solve']:.1f} ms, orth {sv['ms_orth']:.1f} ms, transpose "
                      f"{sv['ms_transpose']:.1f} ms", flush=True)
                st = {k: stats[v][k] for k in ("n", "values", "clusters", "largest_cluster", "rounds", "failed",
                                               "launches", "host_syncs")}
                print(f"    stein_stats: {st}", flush=True)
    s.trace.off()


def resource_report():
    """the kernel-resource-usage remarks of csrc/kernels/stein.hip, one line per kernel"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return ["# resource usage: hipcc not found"]
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "-std=c++17", "-O3", "--offload-arch=gfx950", "-Icsrc/include", "-Icsrc/kernels",
               "-D__HIP_PLATFORM_AMD__", "-Rpass-analysis=kernel-resource-usage", "-c", "csrc/kernels/stein.hip",
               "-o", os.path.join(tmp, "stein.o")]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out, cur = ["# kernel resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)"], {}
    for line in r.stdout.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        k, _, v = m.group(1).partition(":")
        k, v = k.strip(), v.strip()
        if k == "Function Name":
            cur = {"name": re.sub(r"^_ZN9slate_amd3dev12_GLOBAL__N_1\d+", "", v)}
        else:
            cur[k] = v
        if k.startswith("LDS Size"):
            out.append(f"{cur['name'][:40]:40s} VGPRs {cur.get('VGPRs', '?'):>3s}  SGPRs {cur.get('TotalSGPRs', '?'):>3s}  "
                       f"scratch {cur.get('ScratchSize [bytes/lane]', '?')}  spills {cur.get('VGPRs Spill', '?')}  "
                       f"occupancy {cur.get('Occupancy [waves/SIMD]', '?')}  LDS {v} B")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", type=int, default=0, help="(internal) run one size in this process")
    ap.add_argument("--sizes", default="2048,4096,8192")
    ap.add_argument("--nb", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per variant (after one warm-up round)")
    ap.add_argument("--all-max", type=int, default=2048, help="largest n at which heevx(All) is measured")
    ap.add_argument("--target", default="d", help="d (the measurement) or h (a dry run of the script)")
    ap.add_argument("--out", default="", help="also write the report to this file")
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, ROOT)
        step(a, a.step)
        return 0
    lines = [f"# heevx_ab: heev with vectors against heevx, float64, nb {a.nb}, one GPU, rounds {a.rounds}; median of "
             f"the timed rounds, variants alternating; stage lines are host trace blocks; heevx(All) up to n = {a.all_max}"]

    def save():
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    rc = 0
    for n in [int(x) for x in a.sizes.split(",") if x]:
        cmd = ["timeout", "-k", "10", str(limit(n)), sys.executable, os.path.abspath(__file__), "--step", str(n),
               "--nb", str(a.nb), "--rounds", str(a.rounds), "--all-max", str(a.all_max), "--target", a.target]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        lines += r.stdout.splitlines()
        save()
        if r.returncode != 0:
            lines.append(f"# --step {n} ended with status {r.returncode}: stopping")
            print(lines[-1], flush=True)
            rc = r.returncode
            break
    lines += resource_report()
    print("\n".join(lines[-8:]), flush=True)
    save()
    return rc


if __name__ == "__main__":
    sys.exit(main())
