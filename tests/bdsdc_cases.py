"""Inputs, oracle and checks shared by test_bdsdc.py and test_bdsdc_gpu.py.

Oracle: numpy.linalg.svd of the dense bidiagonal in float64.  Bounds: the
project's float64 bounds of test_stedc_secular_hard / test_bdsqr_device_vectors,
with b2 = ||B||_2 from numpy; float32 results get them times eps32 / eps64."""
import functools

import numpy as np

KINDS = ["random", "graded", "cluster", "ones", "zerodiag", "split", "tiny"]


@functools.lru_cache(maxsize=None)
def bidiagonal(kind, n, scale=1.0):
    """(d, e, reference singular values) -- computed once, arrays read-only."""
    rng = np.random.default_rng(1000 + n)
    d, e = rng.standard_normal(n), rng.standard_normal(max(n - 1, 0))
    if kind == "graded":
        d, e = np.logspace(0, -15, n), 0.1 * np.logspace(0, -15, n - 1)
    elif kind == "cluster":
        d = np.ones(n)
        d[::7] = 1 + 1e-12
        e = np.full(n - 1, 1e-9)
    elif kind == "ones":
        d, e = np.ones(n), np.ones(n - 1)
    elif kind == "zerodiag":
        d[n // 2] = 0.0
    elif kind == "split":
        e[n // 3] = 0.0
        e[(2 * n) // 3] = 0.0
    elif kind == "tiny":
        d[::9] = 1e-20
    else:
        assert kind == "random", kind
    d, e = d * scale, e * scale
    ref = np.linalg.svd(np.diag(d) + np.diag(e, 1), compute_uv=False)
    for a in (d, e, ref):
        a.setflags(write=False)
    return d, e, ref


def check(d, e, ref, sv, u, vt, factor=1.0):
    """The four checks; every figure is printed before it is asserted."""
    n = len(d)
    sv, u, vt = np.asarray(sv, dtype=np.float64), np.asarray(u, dtype=np.float64), np.asarray(vt, dtype=np.float64)
    assert sv.shape == (n,) and u.shape == (n, n) and vt.shape == (n, n)
    b2 = ref.max() if ref.max() > 0 else 1.0
    # norms of B / b2: the same inequalities, safe at 1e+-150
    b = (np.diag(d) + np.diag(e, 1)) / b2
    dsig = np.abs(sv - ref).max() / b2
    res = np.linalg.norm(b - (u * (sv / b2)[None, :]) @ vt)
    ou = np.linalg.norm(u.T @ u - np.eye(n))
    ov = np.linalg.norm(vt @ vt.T - np.eye(n))
    print(f"n={n} dsig={dsig:.3e} (<= {1e-13 * n * factor:.1e}) res={res:.3e} ou={ou:.3e} ov={ov:.3e} "
          f"(<= {1e-14 * n * factor:.1e})")
    assert np.all(sv >= 0) and np.all(np.diff(sv) <= 0), "sigma not nonnegative descending"
    assert dsig <= 1e-13 * n * factor
    assert res <= 1e-14 * n * factor
    assert ou <= 1e-14 * n * factor
    assert ov <= 1e-14 * n * factor
