"""One-stage bidiagonal reduction on the device (csrc/kernels/gebrd.hip,
csrc/src/gebrd.cc): the two product kernels, gebrd and unmbr_gebrd, and svd
with either method_gebrd.  Bounds are those of test_gebrd.py; the product
kernels take symv_lower's bound."""
import numpy as np
import pytest

import slate_d35_amd as s
from helpers import rnd
from test_gebrd import check_apply, check_reduction, reduce_and_factors, svd_checked, tol

pytestmark = pytest.mark.gpu

BLOCKS = [(1, 1), (65, 1), (1, 65), (63, 64), (64, 16), (65, 17), (200, 65), (513, 130)]


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("shape", BLOCKS)
def test_product_kernels(shape, dt):
    """Blocks at (ro, co) of a column-major matrix whose leading dimension is
    its rows + 3: the base is element-aligned only; everything outside the
    block is NaN."""
    import torch
    mr, nc = shape
    scale = np.finfo(dt).eps / np.finfo(np.float64).eps
    for off in range(4):
        ro, co = off, 3 - off
        rows, cols = mr + ro, nc + co
        rng = np.random.default_rng(1000 * mr + 10 * nc + off)
        blk = rng.standard_normal((mr, nc)).astype(dt)
        stored = np.full((rows + 3, cols), np.nan, dt)     # column-major (rows + 3) x cols
        stored[ro:rows, co:] = blk
        # a row-major (cols x ld) tensor is the column-major ld x cols matrix; the kernels take the
        # block that runs to the last row, so the rows of the matrix end where the block does
        At = torch.from_numpy(np.ascontiguousarray(stored.T)).to("cuda")[:, :rows]
        assert cols == 1 or At.stride(0) == rows + 3    # (one column has no stride to speak of)
        b64 = blk.astype(np.float64)
        for name, fn, k, xlen, ref_of in (("gemv_t_block", s.ops.gemv_t_block, mr, mr, lambda x: b64.T @ x),
                                          ("gemv_n_block", s.ops.gemv_n_block, nc, nc, lambda x: b64 @ x)):
            x = rng.standard_normal(xlen).astype(dt)
            xt = torch.from_numpy(x).to("cuda")
            y1 = fn(At, xt, ro, co).cpu().numpy()
            y2 = fn(At, xt, ro, co).cpu().numpy()
            ref = ref_of(x.astype(np.float64))
            bound = 1e-13 * scale * k * np.abs(b64).max() * np.abs(x).max()
            err = np.abs(y1 - ref).max()
            print(f"{name} {np.dtype(dt).name} {mr}x{nc} at ({ro},{co}): err {err:.3e} bound {bound:.3e}")
            assert np.all(np.isfinite(y1))
            assert err <= bound
            assert np.array_equal(y1, y2)


LAUNCHES = ("launches_column", "launches_larfg_u", "launches_pass1", "launches_finish_y", "launches_larfg_v",
            "launches_pass2", "launches_finish_x")


@pytest.mark.parametrize("extra", [0, 37])
@pytest.mark.parametrize("n", [2, 65, 130, 257, 600])
def test_gebrd_device(n, extra):
    a = rnd(n + extra, n, np.float64, n + extra)
    A, TQ, TP, d, e, q, p = reduce_and_factors(a, 64, "d")
    st = s.ops.gebrd_stats()
    check_reduction(a, d, e, q, p, tol(np.float64))
    launches = [st[k] for k in LAUNCHES]
    print("gebrd_stats", n, st)
    assert st["columns"] == n and all(v > 0 for v in launches)
    assert sum(launches) <= 8 * st["columns"] + 4 * st["panels"]
    assert st["host_syncs"] <= 2
    # two runs give the same bits
    d2, e2, _, _ = s.gebrd(s.from_numpy(a.copy(), nb=64, target="d"), target="d")
    assert np.array_equal(d, np.asarray(d2)) and np.array_equal(e, np.asarray(e2))


def test_gebrd_device_float32():
    a = rnd(637, 600, np.float32, 7)
    A, TQ, TP, d, e, q, p = reduce_and_factors(a, 64, "d")
    check_reduction(a, d, e, q, p, tol(np.float32))


def test_unmbr_gebrd_device():
    """Both factors, both sides, both ops, 40 right-hand sides."""
    n = 257
    a = rnd(n + 37, n, np.float64, 21)
    A, TQ, TP, d, e, q, p = reduce_and_factors(a, 64, "d")
    check_apply(A, TQ, "q", q, n + 37, "d", tol(np.float64), k=40)
    check_apply(A, TP, "p", p, n, "d", tol(np.float64), k=40)


@pytest.mark.parametrize("method_svd", ["qr", "dc"])
@pytest.mark.parametrize("n,nb", [(300, 64), (700, 256)])
def test_svd_device_both_methods(n, nb, method_svd):
    a = rnd(n, n, np.float64, n)
    out = {}
    for method in ("two_stage", "one_stage"):
        out[method] = svd_checked(a, nb, "d", method_gebrd=method, method_svd=method_svd)
    assert np.abs(out["one_stage"] - out["two_stage"]).max() <= tol(np.float64) * out["two_stage"].max()
    assert s.ops.gebrd_stats()["launches_pass1"] == n - 1


def test_svd_device_rectangular_and_vals():
    a = rnd(400, 300, np.float64, 9)
    sv = svd_checked(a, 64, "d", method_gebrd="one_stage")
    v = np.asarray(s.svd_vals(s.from_numpy(a.copy(), nb=64, target="d"), target="d", method_gebrd="one_stage"))
    assert np.abs(v - sv).max() <= tol(np.float64) * sv.max()


def test_svd_device_clustered():
    """300 singular values in three clusters of width 1e-12."""
    n = 300
    rng = np.random.default_rng(3)
    sig = np.repeat([0.25, 1.0, 2.0], n // 3) + 1e-12 * rng.random(n)
    u, _ = np.linalg.qr(rng.standard_normal((n, n)))
    v, _ = np.linalg.qr(rng.standard_normal((n, n)))
    a = (u * sig) @ v.T
    for ms in ("qr", "dc"):
        svd_checked(a, 64, "d", method_gebrd="one_stage", method_svd=ms)
