"""Inverse iteration on the device (csrc/kernels/stein.hip, csrc/src/stein.cc)
and heevx / syevx on it: the cases and bounds of test_stein.py
(stein_cases.py) on target "d", plus what only the device has:
bit-reproducibility, one host synchronisation, a launch count that does not
depend on the data, and the host twin within the same bounds."""
import numpy as np
import pytest

import slate_d35_amd as s
import stein_cases as C
from test_stein import run_native_tester

pytestmark = pytest.mark.gpu

TG = "d"


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("case,n,kw", C.CASES, ids=C.CASE_IDS)
def test_stein(case, n, kw, dt):
    C.check_stein_case(case, n, kw, dt, TG)


def test_stein_small_and_empty():
    C.check_stein_small(TG)


def test_stein_refusals():
    C.check_stein_refusals(TG)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_device_contract(dt):
    """Two calls give the same bits; one host synchronisation; the launches
    are 5 (1 + (clusters > 0)) + 1 whatever the data; the host twin, on the
    same values, is within the bounds too."""
    n = 257
    d, e = C.tridiagonal("random", np.dtype(dt).name, n)
    w = s.stebz(d, e, target=TG)
    z1 = s.stein(d, e, w, target=TG)
    st = s.ops.stein_stats()
    assert st["host_syncs"] == 1 and st["failed"] == 0 and st["rounds"] == 5 and st["clusters"] > 0, st
    assert st["launches"] == 5 * 2 + 1, st
    assert np.array_equal(s.stein(d, e, w, target=TG), z1)
    zh = s.stein(d, e, w, target="h")
    assert s.ops.stein_stats()["failed"] == 0
    rb, ob = C.bounds("random", dt)
    for z in (z1, zh):
        r, o = C.measures(d, e, w, z, dt)
        assert r <= rb and o <= ob, (r, o)
    # no cluster: the orthonormalisation is not launched
    w = s.stebz(d, e, range="index", il=1, iu=1, target=TG)
    s.stein(d, e, w, target=TG)
    st = s.ops.stein_stats()
    assert st["clusters"] == 0 and st["launches"] == 5 + 1 and st["host_syncs"] == 1, st


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_launches_do_not_depend_on_the_data(dt):
    """The same n = 1500 and m = 64 (values 700 .. 763) for a random T (several
    small clusters, three rounds to accept) and for a nearly diagonal T
    (d = k / n, e = 1e-6: one cluster of 64 whose start vectors are accepted
    almost at once): the same number of launches, one synchronisation each."""
    n = 1500
    rng = np.random.default_rng(1000 + n)
    rand = (rng.standard_normal(n).astype(dt), rng.standard_normal(n - 1).astype(dt))
    early = ((np.arange(n) / n).astype(dt), np.full(n - 1, 1e-6, dt))
    launches = []
    for dd, ee in (rand, early):
        w = s.stebz(dd, ee, range="index", il=700, iu=763, target=TG)
        z = s.stein(dd, ee, w, target=TG)
        st = s.ops.stein_stats()
        assert st["n"] == n and st["values"] == 64 and st["clusters"] > 0, st
        assert st["host_syncs"] == 1 and st["failed"] == 0, st
        launches.append(st["launches"])
        r, o = C.measures(dd, ee, w, z, dt)
        rb, ob = C.bounds("random", dt)
        assert r <= rb and o <= ob, (r, o)
    assert launches[0] == launches[1] == 5 * 2 + 1, launches


@pytest.mark.parametrize("mh", ["two_stage", "one_stage"])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", [130, 257])
def test_heevx(n, dt, mh):
    C.check_heevx(n, dt, mh, TG)


def test_heevx_complex_two_stage():
    C.check_heevx(130, np.complex128, "two_stage", TG)


def test_heevx_leaves_a_and_syevx():
    C.check_heevx_unmodified(TG)


def test_heevx_refusals():
    C.check_heevx_refusals(TG)


def test_native_tester_device():
    run_native_tester("d")


def test_python_tester_device(capsys):
    from slate_d35_amd import tester
    rc = tester.main(["stein", "heevx", "--dim", "300", "--nb", "64", "--type", "s,d", "--target", "d"])
    out = capsys.readouterr().out
    assert rc == 0 and "all tests passed" in out, out
    assert s.ops.stein_stats()["launches"] > 0 and s.ops.stein_stats()["failed"] == 0
