"""One-stage bidiagonal reduction on the host target (csrc/src/gebrd.cc,
host::gebrd): the stage routines gebrd / unmbr_gebrd, svd / gesvd / svd_vals
with method_gebrd="one_stage", the refusals, the C option array and both
testers.  Tolerances are test_eig.py's: 1e-10 for float64, 1e-3 for float32."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import slate_d35_amd as s
from helpers import rnd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "slate_d35_amd")


def tol(dt):
    return 1e-3 if dt == np.float32 else 1e-10


def bidiag(d, e, m):
    """The m x n upper bidiagonal B (rows n..m-1 zero)."""
    n = len(d)
    b = np.zeros((m, n), np.float64)
    b[:n, :] = np.diag(np.asarray(d, np.float64)) + np.diag(np.asarray(e, np.float64), 1)
    return b


def nan_padding(A, tg):
    """NaN into the rows of the local array between the matrix's m and its
    leading dimension (all columns but the last, whose padding may end the
    allocation)."""
    import torch
    lt = s.local_tensor(A, device=(tg == "d"))
    m, n = lt.shape
    ld = lt.stride(1)
    if n > 1 and ld > m and lt.stride(0) == 1:
        pad = torch.as_strided(lt, (ld - m, n - 1), (1, ld), lt.storage_offset() + m)
        pad.fill_(float("nan"))
        if tg == "d":
            torch.cuda.synchronize()
    return ld - m


def reduce_and_factors(a, nb, tg):
    """gebrd of a (leading-dimension padding NaN on the way in) and the explicit Q (m x m), P (n x n)."""
    m, n = a.shape
    dt = a.dtype.type
    A = s.from_numpy(a.copy(), nb=nb, target=tg)
    nan_padding(A, tg)
    d, e, TQ, TP = s.gebrd(A, target=tg)
    Q = s.from_numpy(np.eye(m, dtype=dt), nb=nb, target=tg)
    s.unmbr_gebrd("q", s.Side.Left, s.Op.NoTrans, A, TQ, Q, target=tg)
    P = s.from_numpy(np.eye(n, dtype=dt), nb=nb, target=tg)
    s.unmbr_gebrd("p", s.Side.Left, s.Op.NoTrans, A, TP, P, target=tg)
    return A, TQ, TP, np.asarray(d), np.asarray(e), s.to_numpy(Q), s.to_numpy(P)


def check_reduction(a, d, e, q, p, t):
    m, n = a.shape
    assert d.shape == (n,) and e.shape == (max(n - 1, 0),)
    assert all(np.all(np.isfinite(x)) for x in (d, e, q, p))
    b = bidiag(d, e, m)
    q = q.astype(np.float64)
    p = p.astype(np.float64)
    a = a.astype(np.float64)
    assert np.linalg.norm(q @ b @ p.T - a) / (n * max(np.linalg.norm(a), np.finfo(np.float64).tiny)) < t
    assert np.linalg.norm(q.T @ q - np.eye(m)) / m < t
    assert np.linalg.norm(p.T @ p - np.eye(n)) / n < t
    ref = np.linalg.svd(a, compute_uv=False)
    got = np.linalg.svd(b, compute_uv=False)
    assert np.abs(got - ref).max() <= t * max(ref.max(), np.finfo(np.float64).tiny)


def check_apply(A, T, vect, f, rows, tg, t, k=None):
    """Left / Right with NoTrans / Trans against the explicit factor f (order rows)."""
    k = rows if k is None else k
    for side in (s.Side.Left, s.Side.Right):
        for op in (s.Op.NoTrans, s.Op.Trans):
            c = rnd(rows, k, np.float64, 3) if side == s.Side.Left else rnd(k, rows, np.float64, 3)
            C = s.from_numpy(c, nb=64, target=tg)
            s.unmbr_gebrd(vect, side, op, A, T, C, target=tg)
            ff = f if op == s.Op.NoTrans else f.T
            ref = ff @ c if side == s.Side.Left else c @ ff
            assert np.abs(s.to_numpy(C) - ref).max() <= t * max(1.0, np.abs(c).max()) * rows, (vect, side, op)


@pytest.mark.parametrize("extra", [0, 37])
@pytest.mark.parametrize("n", [1, 2, 3, 65, 130, 257])
def test_gebrd_stage_routines(n, extra):
    m = n + extra
    a = rnd(m, n, np.float64, n + extra)
    A, TQ, TP, d, e, q, p = reduce_and_factors(a, 64, "h")
    check_reduction(a, d, e, q, p, tol(np.float64))
    st = s.ops.gebrd_stats()
    assert st["columns"] == n and st["panels"] == (n + 63) // 64
    check_apply(A, TQ, "q", q, m, "h", tol(np.float64), k=min(m, 40))
    check_apply(A, TP, "p", p, n, "h", tol(np.float64), k=min(n, 40))


def test_gebrd_float32():
    a = rnd(167, 130, np.float32, 5)
    A, TQ, TP, d, e, q, p = reduce_and_factors(a, 64, "h")
    check_reduction(a, d, e, q, p, tol(np.float32))


@pytest.mark.parametrize("kind", ["zero", "bidiagonal"])
def test_gebrd_degenerate(kind):
    """Every reflector tail is zero: all finite, d and e the input's bidiagonal up to sign."""
    m, n = 110, 70
    a = np.zeros((m, n))
    if kind == "bidiagonal":
        rng = np.random.default_rng(4)
        a[:n, :] = np.diag(rng.standard_normal(n)) + np.diag(rng.standard_normal(n - 1), 1)
    A, TQ, TP, d, e, q, p = reduce_and_factors(a, 64, "h")
    assert all(np.all(np.isfinite(x)) for x in (d, e, q, p))
    assert np.allclose(np.abs(d), np.abs(np.diag(a[:n, :])), rtol=0, atol=1e-14)
    assert np.allclose(np.abs(e), np.abs(np.diag(a[:n, :], 1)), rtol=0, atol=1e-14)
    t = tol(np.float64)
    assert np.linalg.norm(q.T @ q - np.eye(m)) / m < t and np.linalg.norm(p.T @ p - np.eye(n)) / n < t
    assert np.linalg.norm(q @ bidiag(d, e, m) @ p.T - a) <= t * n * max(1.0, np.linalg.norm(a))


def svd_checked(a, nb, tg="h", **kw):
    m, n = a.shape
    k = min(m, n)
    A = s.from_numpy(a.copy(), nb=nb, target=tg)
    U = s.from_numpy(np.zeros((m, k), a.dtype), nb=nb, target=tg)
    VT = s.from_numpy(np.zeros((k, n), a.dtype), nb=nb, target=tg)
    sv = np.asarray(s.svd(A, U, VT, target=tg, **kw))
    u, vt = s.to_numpy(U).astype(np.float64), s.to_numpy(VT).astype(np.float64)
    t = tol(a.dtype.type)
    a64 = a.astype(np.float64)
    ref = np.linalg.svd(a64, compute_uv=False)
    assert np.all(np.isfinite(sv)) and np.all(np.isfinite(u)) and np.all(np.isfinite(vt))
    assert np.all(np.diff(sv) <= 0)
    assert np.abs(sv - ref).max() <= t * ref.max(), kw
    assert np.linalg.norm((u * sv) @ vt - a64) / (k * np.linalg.norm(a64)) < t, kw
    assert np.linalg.norm(u.T @ u - np.eye(k)) / k < t, kw
    assert np.linalg.norm(vt @ vt.T - np.eye(k)) / k < t, kw
    return sv


@pytest.mark.parametrize("method_svd", ["qr", "dc"])
@pytest.mark.parametrize("nb", [32, 64])
def test_svd_one_stage(nb, method_svd):
    a = rnd(200, 200, np.float64, 11)
    svd_checked(a, nb, method_gebrd="one_stage", method_svd=method_svd)
    assert s.ops.gebrd_stats()["columns"] == 200


@pytest.mark.parametrize("shape", [(260, 200), (500, 200), (200, 300)])
def test_svd_one_stage_shapes(shape):
    """Direct path, QR pre-reduction (m > 5/3 n), LQ pre-reduction (n > m)."""
    a = rnd(shape[0], shape[1], np.float64, 12)
    one = svd_checked(a, 64, method_gebrd="one_stage")
    two = svd_checked(a, 64, method_gebrd="two_stage")
    assert np.abs(one - two).max() <= tol(np.float64) * two.max()
    assert s.ops.gebrd_stats()["columns"] == 200


def test_svd_one_stage_rank_deficient_vals_and_gesvd():
    n = 200
    rng = np.random.default_rng(5)
    a = rng.standard_normal((n, 50)) @ rng.standard_normal((50, n))
    for ms in ("qr", "dc"):
        sv = svd_checked(a, 64, method_gebrd="one_stage", method_svd=ms)
        assert sv[50:].max() <= tol(np.float64) * sv[0]
    ref = np.linalg.svd(a, compute_uv=False)
    v = np.asarray(s.svd_vals(s.from_numpy(a.copy(), nb=64), method_gebrd="one_stage"))
    assert np.abs(v - ref).max() <= tol(np.float64) * ref.max()
    v = np.asarray(s.gesvd(s.from_numpy(a.copy(), nb=64), method_gebrd="one_stage"))
    assert np.abs(v - ref).max() <= tol(np.float64) * ref.max()


@pytest.mark.parametrize("scale", [1e-170, 1e170])
def test_svd_one_stage_range_guard(scale):
    n = 200
    a = rnd(n, n, np.float64, 13)
    ref = np.linalg.svd(a, compute_uv=False) * scale
    A = s.from_numpy(a * scale, nb=64)
    U = s.from_numpy(np.zeros((n, n)), nb=64)
    VT = s.from_numpy(np.zeros((n, n)), nb=64)
    sv = np.asarray(s.svd(A, U, VT, method_gebrd="one_stage"))
    u, vt = s.to_numpy(U), s.to_numpy(VT)
    assert np.all(np.isfinite(sv)) and np.all(np.isfinite(u)) and np.all(np.isfinite(vt))
    assert np.abs(sv - ref).max() <= tol(np.float64) * ref.max()
    assert np.linalg.norm((u * (sv / scale)) @ vt - a) / (n * np.linalg.norm(a)) < tol(np.float64)


def test_refusals():
    assert s.MethodGebrd.TwoStage != s.MethodGebrd.OneStage
    ac = (rnd(40, 40, np.float64, 3) + 1j * rnd(40, 40, np.float64, 4)).astype(np.complex128)
    with pytest.raises(Exception, match="real types"):
        s.svd_vals(s.from_numpy(ac, nb=16), method_gebrd="one_stage")
    with pytest.raises(Exception, match="real types"):
        s.gebrd(s.from_numpy(ac, nb=16))
    a = rnd(40, 40, np.float64, 4)
    with pytest.raises(Exception, match="m >= n"):
        s.gebrd(s.from_numpy(rnd(30, 40, np.float64, 5), nb=16))
    with pytest.raises(Exception, match="method_gebrd"):
        s.svd_vals(s.from_numpy(a.copy(), nb=16), method_gebrd="three_stage")
    # the default and the explicit two-stage path agree bit for bit
    w0 = np.asarray(s.svd_vals(s.from_numpy(a.copy(), nb=16)))
    w2 = np.asarray(s.svd_vals(s.from_numpy(a.copy(), nb=16), method_gebrd="two_stage"))
    assert np.array_equal(w0, w2)


def _free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_grid_of_two_refused():
    """A 1 x 2 host grid: NotImplemented, naming the grid; two stages still run."""
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "2")
    env["SLATE_TRANSPORT"] = "host"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(HERE, "gebrd_worker.py"), "1", "2", "h"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "GEBRD_REFUSED_OK" in out, out[-4000:]


C_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include "slate_amd/c_api.h"
int main(void) {
    const int64_t n = 150, nb = 32;
    double *A = malloc(sizeof(double) * n * n), *U = calloc(n * n, sizeof(double)), *V = calloc(n * n, sizeof(double));
    double *S1 = malloc(sizeof(double) * n), *S2 = malloc(sizeof(double) * n);
    int rc[3];
    for (int pass = 0; pass < 3; ++pass) {
        srand(5);
        for (int64_t j = 0; j < n; ++j)
            for (int64_t i = 0; i < n; ++i) A[i + j * n] = (double)rand() / RAND_MAX - 0.5;
        slate_Options opts[2] = {{slate_Option_Target, 'H', 0.0},
                                 {slate_Option_MethodGebrd,
                                  pass == 0 ? slate_MethodGebrd_TwoStage : pass == 1 ? slate_MethodGebrd_OneStage : 77,
                                  0.0}};
        slate_Matrix_r64 As = slate_Matrix_create_fromLAPACK_r64(n, n, A, n, nb);
        slate_Matrix_r64 Us = slate_Matrix_create_fromLAPACK_r64(n, n, U, n, nb);
        slate_Matrix_r64 Vs = slate_Matrix_create_fromLAPACK_r64(n, n, V, n, nb);
        rc[pass] = slate_svd_r64(As, pass == 0 ? S1 : S2, Us, Vs, 2, opts);
        slate_Matrix_destroy_r64(As);
        slate_Matrix_destroy_r64(Us);
        slate_Matrix_destroy_r64(Vs);
    }
    double err = 0, mx = 0;
    for (int64_t i = 0; i < n; ++i) { err = fmax(err, fabs(S1[i] - S2[i])); mx = fmax(mx, fabs(S1[i])); }
    printf("option %d values %d %d rc %d %d %d err %.3e\n", (int)slate_Option_MethodGebrd,
           (int)slate_MethodGebrd_TwoStage, (int)slate_MethodGebrd_OneStage, rc[0], rc[1], rc[2], err / mx);
    return (rc[0] == 0 && rc[1] == 0 && rc[2] != 0 && err <= 1e-10 * mx) ? 0 : 1;
}
"""


def test_c_option_array(tmp_path):
    """slate_Option_MethodGebrd = 69 in a C option array: both values run and
    agree, a value outside the enum fails."""
    src = tmp_path / "gebrd_opt.c"
    src.write_text(C_SRC)
    exe = tmp_path / "gebrd_opt"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT}/csrc/include", str(src), f"-L{PKG}", "-lslate_amd",
                    f"-Wl,-rpath,{PKG}", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "option 69 values 50 49" in r.stdout, r.stdout
    f90 = open(os.path.join(ROOT, "csrc", "api", "slate_c_api.f90")).read()
    assert "slate_Option_MethodGebrd = 69" in f90 and "slate_MethodGebrd_OneStage = 49" in f90
    assert "slate_MethodGebrd_TwoStage = 50" in f90


def test_native_tester_gebrd():
    r = subprocess.run(["make", "tester"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    port = _free_port()
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               SLATE_MASTER_PORT=str(port), SLATE_COMM="host", OMP_NUM_THREADS="2")
    r = subprocess.run([os.path.join(ROOT, "bin", "slate_tester"), "gebrd,unmbr_gebrd,svd", "--method-gebrd",
                        "one_stage", "--type", "s,d", "--dim", "150", "--nb", "32", "--target", "h"], env=env,
                       capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "all tests passed" in out, out[-4000:]
    assert out.count("pass") >= 6 and out.count("method_gebrd=one_stage") == 2, out[-4000:]


def test_python_tester_gebrd(capsys):
    from slate_d35_amd import tester
    rc = tester.main(["gebrd", "unmbr_gebrd", "svd", "--method-gebrd", "one_stage", "--dim", "150", "--nb", "32",
                      "--type", "s,d", "--target", "h"])
    out = capsys.readouterr().out
    assert rc == 0 and "all tests passed" in out, out
    assert out.count("method_gebrd=one_stage") == 2, out
    assert s.ops.gebrd_stats()["columns"] == 150
