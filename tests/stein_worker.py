"""Multi-process check of heevx's scope, run under torch.distributed.run by
test_stein.py (as hetrd_worker.py is by test_hetrd.py).

usage: stein_worker.py P Q TARGET
On a grid of more than one process heevx raises NotImplemented with a message
that names the grid; heev still solves the same matrix.
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
from helpers import refusal_text, rnd  # noqa: E402


def main():
    p, q, tg = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    parallel.init_grid(p, q, transport=os.environ.get("SLATE_TRANSPORT", "auto"))
    n, nb = 96, 32
    a = rnd(n, n, np.float64, 4)
    a = (a + a.T) / 2
    H = s.HermitianMatrix(s.Uplo.Lower, s.from_numpy(a, nb=nb, target=tg))
    want = (f"heevx: the subset driver needs a grid of one process (A is distributed over {p * q}); "
            "a distributed stein is not implemented")
    for mh in ("two_stage", "one_stage"):
        try:
            s.heevx(H, None, range="index", il=1, iu=5, target=tg, method_hetrd=mh)
        except Exception as ex:
            msg = str(ex)
            assert "grid of one process" in msg and "not implemented" in msg.lower(), msg
            assert refusal_text(ex) == want, msg
        else:
            raise AssertionError("heevx accepted a grid of two processes")
    w = s.heev(H, target=tg)
    ref = np.linalg.eigvalsh(a)
    assert np.abs(w - ref).max() <= 1e-10 * np.abs(ref).max()
    parallel.finalize()
    if parallel.world_rank() == 0:
        print("HEEVX_REFUSED_OK", p, q, tg, flush=True)


if __name__ == "__main__":
    main()
