"""Sturm-count bisection on the device (csrc/kernels/stebz.hip,
csrc/src/stebz.cc): the cases and bounds of test_stebz.py (stebz_cases.py) on
target "d", plus what only the device has: bit-reproducibility, one host
synchronisation, a launch count that does not depend on convergence, agreement
with the host twin, and P = 1 against P > 1 in fresh child processes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import slate_d35_amd as s
import stebz_cases as C
from test_stebz import run_native_tester

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TG = "d"


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", C.SIZES)
def test_sturm_count_exact(n, dt):
    C.check_sturm_count(n, dt, TG)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", C.SIZES)
def test_stebz_random(n, dt):
    C.check_stebz_random(n, dt, TG)


@pytest.mark.parametrize("n", C.SIZES[1:])
def test_stebz_laplacian_closed_form(n):
    C.check_stebz_laplacian(n, TG)


def test_stebz_structured():
    C.check_stebz_wilkinson(TG)
    C.check_stebz_direct_sum(TG)
    C.check_stebz_zero(TG)
    C.check_stebz_scaled(TG)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", C.SIZES)
def test_ranges(n, dt):
    C.check_ranges(n, dt, TG)


def test_refusals():
    C.check_refusals(TG)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", C.SIZES)
def test_bdsbz_random(n, dt):
    C.check_bdsbz_random(n, dt, TG)


@pytest.mark.parametrize("n", C.SIZES)
def test_bdsbz_ones_closed_form(n):
    C.check_bdsbz_ones(n, TG)


def test_bdsbz_zero_entry():
    C.check_bdsbz_zero_entry(TG)


def test_bdsbz_graded_float32():
    C.check_bdsbz_graded(TG)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", [130, 257])
def test_heev_bisection(n, dt):
    C.check_heev_bisection(n, dt, TG)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", [130, 257])
def test_svd_vals_bisection(n, dt):
    C.check_svd_vals_bisection(n, dt, TG)


def test_sygv_bisection():
    C.check_sygv_bisection(TG)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_device_contract(dt):
    """Two calls give the same bits; one host synchronisation; the launches
    are 1 + (range == value): one refinement launch in which every wave runs
    to its own stopping rule, plus the count at vl and vu for a range by
    value -- whether the values converge in a few steps (a diagonal matrix
    with a tiny coupling) or need them all; the host twin agrees within
    16 eps max|T|."""
    n = 257
    d, e, _ = C.random_tri(n, np.dtype(dt).name)
    early = ((np.arange(n) / n).astype(dt), np.full(n - 1, 1e-6, dt))
    for dd, ee in ((d, e), early):
        w1 = s.stebz(dd, ee, target=TG)
        st = s.ops.stebz_stats()
        assert st["launches"] == 1 and st["host_syncs"] == 1 and st["values"] == n, st
        assert np.array_equal(s.stebz(dd, ee, target=TG), w1)
        s.stebz(dd, ee, range="index", il=5, iu=9, target=TG)
        st = s.ops.stebz_stats()
        assert st["launches"] == 1 and st["host_syncs"] == 1, st
        wv = s.stebz(dd, ee, range="value", vl=-0.25, vu=0.6, target=TG)
        st = s.ops.stebz_stats()
        assert st["launches"] == 2 and st["host_syncs"] == 1 and st["values"] == len(wv), st
        assert np.abs(w1 - s.stebz(dd, ee, target="h")).max() <= 16 * C.eps(dt) * C.tmax(dd, ee)
    sd, se, _ = C.random_bi(n, np.dtype(dt).name)
    s1 = s.bdsbz(sd, se, target=TG)
    st = s.ops.stebz_stats()
    assert st["launches"] == 1 and st["host_syncs"] == 1 and st["n"] == 2 * n, st
    assert np.array_equal(s.bdsbz(sd, se, target=TG), s1)
    assert np.abs(s1 - s.bdsbz(sd, se, target="h")).max() <= 16 * C.eps(dt) * C.tmax(sd, se)


@pytest.mark.parametrize("points", [1, 8])
def test_points_in_child(points):
    env = dict(os.environ, SLATE_STEBZ_POINTS=str(points))
    r = subprocess.run([sys.executable, os.path.join(HERE, "stebz_worker.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and f"STEBZ_WORKER_OK points={points}" in out, out[-4000:]


def test_native_tester_device():
    run_native_tester("d")
