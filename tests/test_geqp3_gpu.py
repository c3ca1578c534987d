"""QR with column pivoting on the device (csrc/kernels/geqp3.hip): the inputs
and the checkers of test_geqp3.py on target "d", two shapes of more than one
workgroup per kernel and more than one chunk of the product, and the host and
the device agreeing on the pivots."""
import numpy as np
import pytest

import slate_d35_amd as s
from test_geqp3 import (KINDS, TINY, check_against_lapack, check_factor, check_gelsy_full_and_wide,
                        check_gelsy_lowrank, check_stats, check_unmqr, factor, make, run_kind)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("kind", KINDS)
def test_geqp3_inputs_device(kind, dt):
    jpvt, r = run_kind(kind, dt, "d")
    if dt == np.float64 and kind in ("random", "wide", "cancel"):
        check_against_lapack(kind, jpvt, r)
        # the host twin: the same algorithm, the same pivots
        assert np.array_equal(jpvt, factor(make(kind, dt), "h")[2])


@pytest.mark.parametrize("shape", TINY)
def test_geqp3_tiny_device(shape):
    a = np.random.default_rng(31).standard_normal(shape)
    A, T, jpvt, r, q = factor(a, "d")
    check_stats(a, "d", None)
    check_factor(a, jpvt, r, q)


@pytest.mark.parametrize("shape,dt", [((600, 257), np.float64), ((637, 600), np.float32)])
def test_geqp3_larger_device(shape, dt):
    a = np.random.default_rng(41).standard_normal(shape).astype(dt)
    A, T, jpvt, r, q = factor(a, "d")
    check_stats(a, "d", None)
    check_factor(a, jpvt, r, q)
    check_unmqr(A, T, q, "d")
    A2 = s.from_numpy(a.copy(), nb=64, target="d")
    jpvt2, _ = s.geqp3(A2, target="d")
    assert np.array_equal(jpvt, jpvt2) and np.array_equal(np.triu(s.to_numpy(A2))[:r.shape[0], :], r)


def test_geqp3_zero_column_device():
    a = np.random.default_rng(32).standard_normal((90, 70))
    a[:, 17] = 0
    A, T, jpvt, r, q = factor(a, "d")
    check_factor(a, jpvt, r, q)
    assert jpvt[-1] == 17 and np.all(r[-1] == 0)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_gelsy_lowrank_device(dt):
    check_gelsy_lowrank(dt, "d")


def test_gelsy_full_rank_wide_and_zero_device():
    check_gelsy_full_and_wide("d")
