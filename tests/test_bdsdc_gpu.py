"""Bidiagonal divide and conquer on the device target: the three kernels of
csrc/kernels/dc_merge.hip (secular roots, z-hat, merge columns) with the MFMA
GEMM merges, against numpy with the bounds of bdsdc_cases.check, and svd with
method_svd="dc" on the device."""
import numpy as np
import pytest

import slate_d35_amd as s
from helpers import rnd
from bdsdc_cases import bidiagonal, check

pytestmark = pytest.mark.gpu


def run_device(kind, n, dtype=np.float64, nb=64):
    d, e, ref = bidiagonal(kind, n)
    factor = 1.0
    if dtype == np.float32:
        d, e = d.astype(np.float32), e.astype(np.float32)
        d64, e64 = d.astype(np.float64), e.astype(np.float64)
        ref = np.linalg.svd(np.diag(d64) + np.diag(e64, 1), compute_uv=False)
        factor = float(np.finfo(np.float32).eps / np.finfo(np.float64).eps)
    U = s.from_numpy(np.eye(n, dtype=dtype), nb=nb, target="d")
    VT = s.from_numpy(np.eye(n, dtype=dtype), nb=nb, target="d")
    sv = s.bdsdc_matrix(s.Job.Vec, s.Job.Vec, d, e, U, VT, target="d")
    st = s.ops.bdsdc_stats()
    check(d.astype(np.float64), e.astype(np.float64), ref, sv, s.to_numpy(U), s.to_numpy(VT), factor)
    assert st["merges"] > 0
    assert st["launches_secular"] > 0 and st["launches_zhat"] > 0 and st["launches_matrix"] > 0, st
    return st


@pytest.mark.parametrize("kind", ["random", "graded", "cluster", "zerodiag"])
def test_bdsdc_device_kinds(kind):
    st = run_device(kind, 600)
    if kind == "cluster":
        assert st["deflated"] > 0


def test_bdsdc_device_float32():
    run_device("random", 600, np.float32)


@pytest.mark.parametrize("n", [257, 65])
def test_bdsdc_device_small(n):
    """k below one wave, odd sizes, k no multiple of 4."""
    run_device("random", n)


@pytest.mark.parametrize("dt", [np.float64, np.complex128])
def test_svd_method_dc_device(dt):
    m, n, nb = 300, 260, 64
    tol = 1e-10          # test_eig.py's svd tolerance for float64 / complex128
    a = rnd(m, n, dt, 9)
    ref = np.linalg.svd(a, compute_uv=False)
    out = {}
    for method in ("dc", "qr"):
        A = s.from_numpy(a, nb=nb, target="d")
        U = s.from_numpy(np.zeros((m, n), dt), nb=nb, target="d")
        VT = s.from_numpy(np.zeros((n, n), dt), nb=nb, target="d")
        sv = s.svd(A, U, VT, target="d", method_svd=method)
        u, vt = s.to_numpy(U), s.to_numpy(VT)
        assert np.allclose(sv, ref, atol=tol * ref.max()), method
        assert np.linalg.norm(u @ np.diag(sv) @ vt - a) / (np.linalg.norm(a) * n) < tol, method
        assert np.linalg.norm(u.conj().T @ u - np.eye(n)) / n < tol, method
        assert np.linalg.norm(vt @ vt.conj().T - np.eye(n)) / n < tol, method
        out[method] = sv
        if method == "dc":
            st = s.ops.bdsdc_stats()
            assert st["launches_secular"] > 0 and st["launches_zhat"] > 0 and st["launches_matrix"] > 0, st
    assert np.allclose(out["dc"], out["qr"], atol=tol * ref.max())
