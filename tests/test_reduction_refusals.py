"""The refusals of the one-stage reductions (hetrd, gebrd, geqp3 and gelsy on
top of geqp3), word for word: the operand check is one function that takes the
routine's wording as arguments, and a message that an application or a log
filter matches must not change with it.  Complex type, multi-device matrix and
lambda layout here; the grid of more than one process is pinned in the same
way by hetrd_worker.py, gebrd_worker.py and geqp3_worker.py, which the grid
tests of test_hetrd.py, test_gebrd.py and test_geqp3.py run.
"""
import numpy as np
import pytest

import slate_d35_amd as s
from helpers import refusal_text, rnd

N = 40
HETRD = "the one-stage reduction"
GEBRD = "the one-stage bidiagonal reduction"
GEQP3 = "the QR factorization with column pivoting"


def complex_(m=N, n=N):
    return s.from_numpy(rnd(m, n, np.complex128, 1), nb=16)


def multi(m=N, n=N):
    return s.to_multi_device(rnd(m, n, np.float64, 2), nb=16, num_devices=2)


def lam(m=N, n=N):
    return s.matrix_layout(m, n, lambda i: 16, lambda j: 16, lambda i, j: 0)


def real(m=N, n=N):
    return s.from_numpy(rnd(m, n, np.float64, 3), nb=16)


def lower(A):
    return s.HermitianMatrix(s.Uplo.Lower, A)


CASES = [
    # complex type
    (lambda: s.hetrd(lower(complex_())),
     "hetrd: " + HETRD + " is implemented for real types only (A is complex)"),
    (lambda: s.gebrd(complex_()),
     "gebrd: " + GEBRD + " is implemented for real types only (A is complex)"),
    (lambda: s.geqp3(complex_()),
     "geqp3: " + GEQP3 + " is implemented for real types only (A is complex)"),
    (lambda: s.gelsy(complex_(), complex_(N, 2), 1e-8),
     "gelsy: " + GEQP3 + " is implemented for real types only (A is complex)"),
    # multi-device matrix
    (lambda: s.hetrd(lower(multi())),
     "hetrd: " + HETRD + " runs on one device (A is a multi-device matrix)"),
    (lambda: s.gebrd(multi()),
     "gebrd: " + GEBRD + " runs on one device (A is a multi-device matrix)"),
    (lambda: s.geqp3(multi()),
     "geqp3: " + GEQP3 + " runs on one device (A is a multi-device matrix)"),
    (lambda: s.gelsy(multi(), real(N, 2), 1e-8),
     "gelsy: " + GEQP3 + " runs on one device (A is a multi-device matrix)"),
    (lambda: s.gelsy(real(), multi(N, 2), 1e-8),
     "gelsy: " + GEQP3 + " runs on one device (BX is a multi-device matrix)"),
    # lambda layout
    (lambda: s.hetrd(lower(lam())),
     "hetrd: " + HETRD + " needs a block-cyclic operand (A has a lambda layout)"),
    (lambda: s.gebrd(lam()),
     "gebrd: " + GEBRD + " needs a block-cyclic operand (A has a lambda layout)"),
    (lambda: s.geqp3(lam()),
     "geqp3: " + GEQP3 + " needs a block-cyclic operand (A has a lambda layout)"),
    (lambda: s.gelsy(lam(), real(N, 2), 1e-8),
     "gelsy: " + GEQP3 + " needs a block-cyclic operand (A has a lambda layout)"),
    (lambda: s.gelsy(real(), lam(N, 2), 1e-8),
     "gelsy: " + GEQP3 + " needs a block-cyclic operand (BX has a lambda layout)"),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_refusal_text(case):
    fn, text = CASES[case]
    with pytest.raises(Exception) as ei:
        fn()
    assert refusal_text(ei.value) == text
