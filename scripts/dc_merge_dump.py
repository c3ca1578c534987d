#!/usr/bin/env python3
"""Device-target outputs of everything that runs the divide-and-conquer merge
kernels (csrc/kernels/dc_merge.hip), as values plus the SHA-256 of every
output matrix, for a bit-for-bit comparison of two builds.

  python scripts/dc_merge_dump.py --out FILE [--compare OTHER.json]

Every case is a child process under its own time limit, one at a time; the
chain stops at the first case that fails.  With --compare the exit status is
1 if a case differs from OTHER.json; for differing values the largest
difference is printed in ulps.  Inputs are those of tests/test_bdsdc.py
(_stedc_input) and tests/bdsdc_cases.py (bidiagonal)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ([f"stedc_{k}_500" for k in ("toeplitz", "wilkinson", "graded", "cluster", "tinyoff")]
         + ["bdsdc_random_600_d", "bdsdc_cluster_600_d", "bdsdc_zerodiag_600_d", "bdsdc_random_257_d",
            "bdsdc_random_65_d", "bdsdc_random_600_s", "heev_300_s", "svd_dc_300x260_d"])
LIMIT = 120   # seconds per case


def sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def values(a):
    """exact and readable: the repr of every value as a Python float"""
    import numpy as np
    return [float(x).hex() for x in np.asarray(a, dtype=np.float64)]


def run_case(name):
    import numpy as np
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import slate_d35_amd as s
    part = name.split("_")
    if part[0] == "stedc":
        from test_bdsdc import _stedc_input
        n, nb = int(part[2]), 64
        d, e = _stedc_input(part[1], n)
        Q = s.from_numpy(np.zeros((n, n)), nb=nb, target="d")
        w = s.stedc_matrix(d, e, Q, target="d")
        return {"values": values(w), "q_sha256": sha(s.to_numpy(Q))}
    if part[0] == "bdsdc":
        from bdsdc_cases import bidiagonal
        n, dt = int(part[2]), np.float64 if part[3] == "d" else np.float32
        d, e, _ = bidiagonal(part[1], n)
        U = s.from_numpy(np.eye(n, dtype=dt), nb=64, target="d")
        VT = s.from_numpy(np.eye(n, dtype=dt), nb=64, target="d")
        sv = s.bdsdc_matrix(s.Job.Vec, s.Job.Vec, d.astype(dt), e.astype(dt), U, VT, target="d")
        assert s.ops.bdsdc_stats()["launches_matrix"] > 0
        return {"values": values(sv), "u_sha256": sha(s.to_numpy(U)), "vt_sha256": sha(s.to_numpy(VT))}
    rng = np.random.default_rng(11)
    if part[0] == "heev":
        n, nb = int(part[1]), 64
        a = rng.standard_normal((n, n)).astype(np.float32)
        A = s.HermitianMatrix(s.Uplo.Lower, s.from_numpy(a + a.T, nb=nb, target="d"))
        Z = s.from_numpy(np.zeros((n, n), np.float32), nb=nb, target="d")
        w = s.heev(A, Z, target="d")
        return {"values": values(w), "z_sha256": sha(s.to_numpy(Z))}
    assert part[0] == "svd", name
    m, n = (int(x) for x in part[2].split("x"))
    a = rng.standard_normal((m, n))
    A = s.from_numpy(a, nb=64, target="d")
    U = s.from_numpy(np.zeros((m, n)), nb=64, target="d")
    VT = s.from_numpy(np.zeros((n, n)), nb=64, target="d")
    sv = s.svd(A, U, VT, target="d", method_svd="dc")
    assert s.ops.bdsdc_stats()["launches_matrix"] > 0
    return {"values": values(sv), "u_sha256": sha(s.to_numpy(U)), "vt_sha256": sha(s.to_numpy(VT))}


def max_ulps(a, b):
    import numpy as np
    x = np.array([float.fromhex(v) for v in a])
    y = np.array([float.fromhex(v) for v in b])
    if x.shape != y.shape:
        return float("inf")
    return float((np.abs(x - y) / np.spacing(np.maximum(np.abs(x), np.abs(y)))).max()) if x.size else 0.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", default="", help="(internal) run one case in this process")
    ap.add_argument("--out", default="", help="write the results to this JSON file")
    ap.add_argument("--compare", default="", help="JSON file of another build")
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case)), flush=True)
        return 0
    res, rc = {}, 0
    for name in CASES:
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--case", name]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-3000:], end="")
            print(f"# case {name} ended with status {r.returncode}: stopping", flush=True)
            rc = r.returncode or 1
            break
        res[name] = json.loads(line[-1][7:])
        print(f"{name}: done", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    if rc or not a.compare:
        return rc
    with open(a.compare) as f:
        other = json.load(f)
    for name in CASES:
        if res[name] == other.get(name):
            print(f"{name}: identical")
            continue
        rc = 1
        o = other.get(name, {})
        diff = [k for k in res[name] if res[name][k] != o.get(k)]
        print(f"{name}: DIFFERS in {diff}; values differ by at most {max_ulps(res[name]['values'], o.get('values', []))} ulps")
    print("all cases identical" if rc == 0 else "some cases differ")
    return rc


if __name__ == "__main__":
    sys.exit(main())
