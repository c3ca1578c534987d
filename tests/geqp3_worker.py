"""Multi-process check of the scope of the QR with column pivoting, run under
torch.distributed.run by test_geqp3.py (as gebrd_worker.py is by
test_gebrd.py).

usage: geqp3_worker.py P Q TARGET
On a grid of more than one process geqp3 and gelsy raise NotImplemented with a
message that names the grid; geqrf still factors the same matrix.
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
    assert refused(lambda: s.geqp3(s.from_numpy(a.copy(), nb=nb, target=tg), target=tg),
                   f"geqp3: the QR factorization with column pivoting needs a grid of one process (A is distributed over {p * q}); the distributed pivot search is not implemented")  # noqa: E501
    assert refused(lambda: s.gelsy(s.from_numpy(a.copy(), nb=nb, target=tg),
                                   s.from_numpy(a[:, :2].copy(), nb=nb, target=tg), 1e-8, target=tg),
                   f"gelsy: the QR factorization with column pivoting needs a grid of one process (A is distributed over {p * q}); the distributed pivot search is not implemented")  # noqa: E501
    A = s.from_numpy(a.copy(), nb=nb, target=tg)
    s.geqrf(A, target=tg)
    r = np.triu(s.to_numpy(A))
    assert np.abs(r.T @ r - a.T @ a).max() <= 1e-10 * np.abs(a.T @ a).max()
    parallel.finalize()
    if parallel.world_rank() == 0:
        print("GEQP3_REFUSED_OK", p, q, tg, flush=True)


if __name__ == "__main__":
    main()
