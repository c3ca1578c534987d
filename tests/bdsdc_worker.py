"""Multi-process checks of the bidiagonal divide and conquer, run under
torch.distributed.run by test_bdsdc.py (as dist_worker.py is by test_dist.py).

usage: bdsdc_worker.py P Q TARGET
Every rank runs the replicated divide and conquer, keeps its own part of the
distributed U / VT, and checks the gathered result against numpy.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

import torch  # noqa: F401,E402  (HIP runtime first)
import slate_d35_amd as s  # noqa: E402
from slate_d35_amd import parallel  # noqa: E402
from helpers import rnd  # noqa: E402
from bdsdc_cases import bidiagonal, check  # noqa: E402


def main():
    p, q, tg = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    parallel.init_grid(p, q, transport=os.environ.get("SLATE_TRANSPORT", "auto"))
    n, nb = 150, 32
    for kind in ("random", "cluster"):
        d, e, ref = bidiagonal(kind, n)
        U = s.from_numpy(np.eye(n), nb=nb, target=tg)
        VT = s.from_numpy(np.eye(n), nb=nb, target=tg)
        sv = s.bdsdc_matrix(s.Job.Vec, s.Job.Vec, d, e, U, VT, target=tg)
        check(d, e, ref, sv, s.to_numpy(U), s.to_numpy(VT))
    for dt in (np.float64, np.complex128):
        m, k = 150, 110
        a = rnd(m, k, dt, 9)
        A = s.from_numpy(a, nb=nb, target=tg)
        U = s.from_numpy(np.zeros((m, k), dt), nb=nb, target=tg)
        VT = s.from_numpy(np.zeros((k, k), dt), nb=nb, target=tg)
        sv = s.svd(A, U, VT, target=tg, method_svd="dc")
        ref = np.linalg.svd(a, compute_uv=False)
        assert np.allclose(sv, ref, atol=1e-10 * ref.max())
        u, vt = s.to_numpy(U), s.to_numpy(VT)
        assert np.linalg.norm(u @ np.diag(sv) @ vt - a) / (np.linalg.norm(a) * k) < 1e-10
    parallel.finalize()
    if parallel.world_rank() == 0:
        print("BDSDC_DIST_OK", p, q, tg, flush=True)


if __name__ == "__main__":
    main()
