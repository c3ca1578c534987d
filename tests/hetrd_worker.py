"""Multi-process check of the one-stage tridiagonal reduction's scope, run
under torch.distributed.run by test_hetrd.py (as bdsdc_worker.py is by
test_bdsdc.py).

usage: hetrd_worker.py P Q TARGET
On a grid of more than one process heev(method_hetrd="one_stage") and hetrd
raise NotImplemented with a message that names the grid; the two-stage
default still solves the same matrix.
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


def refused(fn, text):
    """fn raises slate::NotImplemented with this text, the grid's size (P Q = 2 here) named in it"""
    try:
        fn()
    except Exception as ex:
        msg = str(ex)
        assert "grid of one process" in msg and "not implemented" in msg.lower(), msg
        assert refusal_text(ex) == text, msg
        return True
    return False


def main():
    p, q, tg = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    parallel.init_grid(p, q, transport=os.environ.get("SLATE_TRANSPORT", "auto"))
    n, nb = 96, 32
    a = rnd(n, n, np.float64, 4)
    a = (a + a.T) / 2
    H = s.HermitianMatrix(s.Uplo.Lower, s.from_numpy(a, nb=nb, target=tg))
    assert refused(lambda: s.heev(H, target=tg, method_hetrd="one_stage"),
                   f"heev: the one-stage reduction needs a grid of one process (A is distributed over {p * q}); a distributed symv is not implemented")  # noqa: E501
    assert refused(lambda: s.hetrd(H, target=tg),
                   f"hetrd: the one-stage reduction needs a grid of one process (A is distributed over {p * q}); a distributed symv is not implemented")  # noqa: E501
    w = s.heev(H, target=tg)
    ref = np.linalg.eigvalsh(a)
    assert np.abs(w - ref).max() <= 1e-10 * np.abs(ref).max()
    parallel.finalize()
    if parallel.world_rank() == 0:
        print("HETRD_REFUSED_OK", p, q, tg, flush=True)


if __name__ == "__main__":
    main()
