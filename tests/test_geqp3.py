"""QR with column pivoting on the host target (csrc/src/geqp3.cc, host::geqp3):
geqp3 / unmqr_geqp3 / gelsy, the counters, the refusals, the C functions, the
Fortran module and both testers.  The inputs and the checkers are shared with
test_geqp3_gpu.py.  Tolerances are test_gebrd.py's: 1e-10 for float64, 1e-3
for float32."""
import os
import subprocess
import sys

import numpy as np
import pytest

import slate_d35_amd as s
from test_gebrd import _free_port, tol

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "slate_d35_amd")

KINDS = ["random", "wide", "lowrank", "cancel", "kahan"]
TINY = [(1, 1), (2, 2), (65, 1), (1, 65), (64, 64), (65, 65)]
_CACHE = {}


def make(kind, dt):
    """The named input, float64 or float32, the same array on every call (read only)."""
    key = (kind, np.dtype(dt).name)
    if key in _CACHE:
        return _CACHE[key]
    f32 = np.dtype(dt) == np.float32
    rng = np.random.default_rng({"random": 11, "wide": 12, "lowrank": 13, "cancel": 14, "kahan": 15}[kind])
    if kind == "random":
        a = rng.standard_normal((137, 100))
    elif kind == "wide":
        a = rng.standard_normal((70, 150))
    elif kind == "lowrank":
        a = rng.standard_normal((130, 40)) @ rng.standard_normal((97, 40)).T
        a = a + (1e-5 if f32 else 1e-11) * rng.standard_normal((130, 97))
    elif kind == "cancel":
        base = rng.standard_normal((200, 65)) * np.logspace(0, -4 if f32 else -9, 65)
        a = np.hstack([base, base * (1 + (1e-3 if f32 else 1e-7) * rng.standard_normal((200, 65)))])
    elif kind == "kahan":
        n, c = 90, 0.285
        sn = np.sqrt(1 - c * c)
        a = np.diag(sn ** np.arange(n)) @ (np.eye(n) - c * np.triu(np.ones((n, n)), 1))
    else:
        raise ValueError(kind)
    a = np.asfortranarray(a.astype(dt))
    a.setflags(write=False)
    _CACHE[key] = a
    return a


def factor(a, tg, nb=64):
    """geqp3 of a: (A, T, jpvt, R (k x n), Q (m x m, from unmqr_geqp3 on the identity))."""
    m, n = a.shape
    A = s.from_numpy(np.array(a), nb=nb, target=tg)
    jpvt, T = s.geqp3(A, target=tg)
    r = np.triu(s.to_numpy(A))[:min(m, n), :]
    Q = s.from_numpy(np.eye(m, dtype=a.dtype), nb=nb, target=tg)
    s.unmqr_geqp3(s.Side.Left, s.Op.NoTrans, A, T, Q, target=tg)
    return A, T, jpvt, r, s.to_numpy(Q)


def check_factor(a, jpvt, r, q, pivots=True):
    """The permutation, the two residuals, the pivoting property and the
    non-increasing diagonal; figures printed before they are asserted."""
    m, n = a.shape
    k = min(m, n)
    dt = a.dtype.type
    t = tol(dt)
    eps = float(np.finfo(dt).eps)
    assert jpvt.dtype == np.int64 and jpvt.shape == (n,)
    assert sorted(jpvt.tolist()) == list(range(n))
    assert r.shape == (k, n) and q.shape == (m, m)
    assert np.all(np.isfinite(r)) and np.all(np.isfinite(q))
    a64, r64, q64 = a.astype(np.float64), r.astype(np.float64), q.astype(np.float64)
    res = np.abs(a64[:, jpvt] - q64[:, :k] @ r64).max()
    orth = np.abs(q64.T @ q64 - np.eye(m)).max()
    print(f"residual {res:.3e} (bound {t * np.abs(a64).max():.3e})  orthogonality {orth:.3e} (bound {t:.1e})")
    assert res <= t * np.abs(a64).max()
    assert orth <= t
    if not pivots:
        return
    bound = 1 + 4 * np.sqrt(eps)
    worst = 0.0
    d = np.abs(np.diag(r64))
    for i in range(k):
        if i + 1 < n:
            rest = np.sqrt((r64[i:, i + 1:] ** 2).sum(axis=0)).max()
            if d[i] > 0:
                worst = max(worst, rest / d[i])
            assert rest <= bound * d[i], (i, rest, d[i])
        if i + 1 < k:
            assert d[i + 1] <= bound * d[i], (i, d[i + 1], d[i])
    print(f"pivoting property: worst ratio {worst:.10f} (bound {bound:.10f})")


def check_unmqr(A, T, q, tg):
    """Both sides, both ops, 40 columns, against the explicit Q."""
    m = q.shape[0]
    dt = q.dtype.type
    rng = np.random.default_rng(3)
    q64 = q.astype(np.float64)
    for side in (s.Side.Left, s.Side.Right):
        for op in (s.Op.NoTrans, s.Op.Trans):
            c = rng.standard_normal((m, 40) if side == s.Side.Left else (40, m)).astype(dt)
            C = s.from_numpy(c.copy(), nb=64, target=tg)
            s.unmqr_geqp3(side, op, A, T, C, target=tg)
            ff = q64 if op == s.Op.NoTrans else q64.T
            ref = ff @ c if side == s.Side.Left else c @ ff
            assert np.abs(s.to_numpy(C) - ref).max() <= tol(dt) * max(1.0, np.abs(c).max()) * m, (side, op)


def check_stats(a, tg, recomputes):
    """The counters of the last geqp3; recomputes: True (> 0), False (== 0) or None (not checked)."""
    st = s.ops.geqp3_stats()
    m, n = a.shape
    assert st["columns"] == min(m, n) and st["panels"] == (min(m, n) + 63) // 64
    assert st["host_syncs"] <= 2
    launches = [v for key, v in st.items() if key.startswith("launches_")]
    assert len(launches) >= 7
    if tg == "d" and n > 1:
        assert all(v > 0 for v in launches), st
    if tg == "h":
        assert all(v == 0 for v in launches), st
    print(f"norm_recomputes {st['norm_recomputes']}")
    if recomputes is True:
        assert st["norm_recomputes"] > 0
    elif recomputes is False:
        assert st["norm_recomputes"] == 0
    return st


RECOMPUTES = {"random": False, "wide": True, "lowrank": True, "cancel": True, "kahan": None}


def run_kind(kind, dt, tg):
    a = make(kind, dt)
    A, T, jpvt, r, q = factor(a, tg)
    check_stats(a, tg, RECOMPUTES[kind])
    check_factor(a, jpvt, r, q)
    check_unmqr(A, T, q, tg)
    # two runs: the same pivots and the same bits
    A2 = s.from_numpy(np.array(a), nb=64, target=tg)
    jpvt2, _ = s.geqp3(A2, target=tg)
    assert np.array_equal(jpvt, jpvt2)
    assert np.array_equal(np.triu(s.to_numpy(A2))[:r.shape[0], :], r)
    return jpvt, r


def check_against_lapack(kind, jpvt, r):
    """float64: LAPACK's pivots and |diag R| (scipy's geqp3)."""
    sl = pytest.importorskip("scipy.linalg")
    a = make(kind, np.float64)
    rl, pl = sl.qr(np.array(a), mode="r", pivoting=True)
    assert np.array_equal(jpvt, pl), np.flatnonzero(jpvt != pl)[:5]
    k = min(a.shape)
    dl, dg = np.abs(np.diag(rl)[:k]), np.abs(np.diag(r)[:k])
    assert np.abs(dl - dg).max() <= 1e-12 * dl[0]


def lowrank_problem(dt):
    a = make("lowrank", dt)
    b = np.random.default_rng(21).standard_normal((a.shape[0], 3)).astype(dt)
    return a, b, (1e-4 if np.dtype(dt) == np.float32 else 1e-8)


def solve(a, b, rcond, tg, nb=64):
    """gelsy: (rank, X n x nrhs)."""
    m, n = a.shape
    bx = np.zeros((max(m, n), b.shape[1]), a.dtype)
    bx[:m] = b
    A = s.from_numpy(np.array(a), nb=nb, target=tg)
    BX = s.from_numpy(bx, nb=nb, target=tg)
    rank = s.gelsy(A, BX, rcond, target=tg)
    return rank, s.to_numpy(BX)[:n]


# float32 lowrank: the same pipeline (pivoted QR, diagonal rule, C = Q^T b, minimum-norm solution of
# the 40 x 97 row block, X = P y) built from scipy's float32 geqp3 differs from lstsq by 4.5e-6
# max|X| on this input (measured: the float32 noise over the smallest kept |R_kk|); 10 x that is allowed
LOWRANK_F32_PIPELINE = 4.5e-6


def check_gelsy_lowrank(dt, tg):
    a, b, rcond = lowrank_problem(dt)
    rank, x = solve(a, b, rcond, tg)
    assert rank == 40
    ref = np.linalg.lstsq(a.astype(np.float64), b.astype(np.float64), rcond=rcond)[0]
    err = np.abs(x - ref).max() / np.abs(ref).max()
    bound = 1e-9 if np.dtype(dt) == np.float64 else 10 * LOWRANK_F32_PIPELINE
    print(f"gelsy lowrank {np.dtype(dt).name}: |X - lstsq| / max|X| = {err:.3e} (bound {bound:.1e})")
    assert err <= bound


def check_gelsy_full_and_wide(tg):
    rng = np.random.default_rng(22)
    a = make("random", np.float64)
    b = rng.standard_normal((a.shape[0], 3))
    rank, x = solve(a, b, None, tg)
    ref = np.linalg.lstsq(a, b, rcond=None)[0]
    assert rank == a.shape[1]
    assert np.abs(x - ref).max() <= tol(np.float64) * np.linalg.cond(a) * np.abs(ref).max()
    a = make("wide", np.float64)
    b = rng.standard_normal((a.shape[0], 3))
    rank, x = solve(a, b, None, tg)
    ref = np.linalg.pinv(a) @ b
    assert rank == 70
    assert np.abs(x - ref).max() <= tol(np.float64) * np.linalg.cond(a) * np.abs(ref).max()
    # nothing to solve with
    rank, x = solve(np.zeros((50, 30)), rng.standard_normal((50, 2)), None, tg)
    assert rank == 0 and np.all(x == 0)


#------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("kind", KINDS)
def test_geqp3_inputs(kind, dt):
    jpvt, r = run_kind(kind, dt, "h")
    if dt == np.float64 and kind in ("random", "wide", "cancel"):
        check_against_lapack(kind, jpvt, r)


@pytest.mark.parametrize("shape", TINY)
def test_geqp3_tiny(shape):
    a = np.random.default_rng(31).standard_normal(shape)
    A, T, jpvt, r, q = factor(a, "h")
    check_stats(a, "h", None)
    check_factor(a, jpvt, r, q)


def test_geqp3_empty():
    for shape in [(0, 5), (5, 0)]:
        A = s.from_numpy(np.zeros(shape), nb=64, target="h")
        jpvt, T = s.geqp3(A, target="h")
        assert jpvt.tolist() == list(range(shape[1]))
        assert s.ops.geqp3_stats()["columns"] == 0


def test_geqp3_zero_column():
    """A zero column among random ones ends up last, with a zero row of R."""
    a = np.random.default_rng(32).standard_normal((90, 70))
    a[:, 17] = 0
    A, T, jpvt, r, q = factor(a, "h")
    check_factor(a, jpvt, r, q)
    assert jpvt[-1] == 17 and np.all(r[-1] == 0)
    z = np.zeros((40, 30))
    A, T, jpvt, r, q = factor(z, "h")
    check_factor(z, jpvt, r, q)
    assert np.all(r == 0) and jpvt.tolist() == list(range(30))


def test_geqp3_tile_size_does_not_matter():
    a = make("random", np.float64)
    _, _, j64, r64, _ = factor(a, "h", nb=64)
    _, _, j24, r24, _ = factor(a, "h", nb=24)
    assert np.array_equal(j64, j24) and np.array_equal(r64, r24)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_gelsy_lowrank(dt):
    check_gelsy_lowrank(dt, "h")


def test_gelsy_full_rank_wide_and_zero():
    check_gelsy_full_and_wide("h")


def test_gelsy_range_guard():
    """Tiny and huge entries are scaled into range first: the same rank, X scaled the other way."""
    a, b, _ = lowrank_problem(np.float64)
    ref = solve(a, b, 1e-8, "h")[1]
    for scale in (1e-170, 1e170):
        rank, x = solve(a * scale, b, 1e-8, "h")
        assert rank == 40
        assert np.abs(x * scale - ref).max() <= 1e-9 * np.abs(ref).max()


def test_refusals():
    ac = (make("random", np.float64)[:40, :30] * (1 + 1j)).astype(np.complex128)
    with pytest.raises(Exception, match="real types"):
        s.geqp3(s.from_numpy(ac, nb=16))
    with pytest.raises(Exception, match="real types"):
        s.gelsy(s.from_numpy(ac, nb=16), s.from_numpy(ac[:, :2].copy(), nb=16), 1e-8)
    L = s.matrix_layout(40, 30, lambda i: 16, lambda j: 16, lambda i, j: 0)
    with pytest.raises(Exception, match="lambda layout"):
        s.geqp3(L)
    a = np.array(make("random", np.float64)[:40, :30])
    A = s.from_numpy(a, nb=16)
    jpvt, T = s.geqp3(A)
    with pytest.raises(Exception, match="lambda layout"):
        s.unmqr_geqp3(s.Side.Left, s.Op.NoTrans, A, T, s.matrix_layout(40, 30, lambda i: 16, lambda j: 16,
                                                                      lambda i, j: 0))
    with pytest.raises(Exception, match="does not match"):
        s.unmqr_geqp3(s.Side.Left, s.Op.NoTrans, A, T, s.from_numpy(np.zeros((30, 5)), nb=16))
    with pytest.raises(Exception, match=r"max\(m, n\)"):
        s.gelsy(s.from_numpy(a.T.copy(), nb=16), s.from_numpy(np.zeros((30, 2)), nb=16), 1e-8)


def test_grid_of_two_refused():
    """A 1 x 2 host grid: NotImplemented, naming the grid; geqrf still runs."""
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "2")
    env["SLATE_TRANSPORT"] = "host"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(HERE, "geqp3_worker.py"), "1", "2", "h"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "GEQP3_REFUSED_OK" in out, out[-4000:]


C_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include "slate_amd/c_api.h"
/* a 60 x 40 matrix of rank 10: pivoted QR, Q^T applied to A P, then the rank-aware solve */
int main(void) {
    const int64_t m = 60, n = 40, r = 10, nb = 16;
    double *A = calloc(m * n, sizeof(double)), *A0 = malloc(sizeof(double) * m * n);
    double *X = malloc(sizeof(double) * m * r), *Y = malloc(sizeof(double) * n * r);
    double *C = malloc(sizeof(double) * m * n), *B = calloc(m, sizeof(double));
    int64_t *jpvt = malloc(sizeof(int64_t) * n), rank = -1;
    srand(7);
    for (int64_t i = 0; i < m * r; ++i) X[i] = (double)rand() / RAND_MAX - 0.5;
    for (int64_t i = 0; i < n * r; ++i) Y[i] = (double)rand() / RAND_MAX - 0.5;
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i < m; ++i) {
            for (int64_t k = 0; k < r; ++k) A[i + j * m] += X[i + k * m] * Y[j + k * n];
            A0[i + j * m] = A[i + j * m];
        }
    for (int64_t i = 0; i < m; ++i) B[i] = A0[i] + A0[i + m];   /* b = a_0 + a_1 */
    slate_Options opts[1] = {{slate_Option_Target, 'H', 0.0}};
    slate_Matrix_r64 As = slate_Matrix_create_fromLAPACK_r64(m, n, A, m, nb);
    slate_TriangularFactors_r64 T = slate_TriangularFactors_create_r64();
    int rc1 = slate_qr_factor_pivoted_r64(As, jpvt, T, 1, opts);
    int seen = 0;
    for (int64_t j = 0; j < n; ++j) seen += jpvt[j] >= 0 && jpvt[j] < n;
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i < m; ++i) C[i + j * m] = A0[i + jpvt[j] * m];
    slate_Matrix_r64 Cs = slate_Matrix_create_fromLAPACK_r64(m, n, C, m, nb);
    int rc2 = slate_qr_pivoted_multiply_by_q_r64('L', 'T', As, T, Cs, 1, opts);
    double err = 0, mx = 0;   /* Q^T A P = R */
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i < m; ++i) {
            const double ref = i <= j ? A[i + j * m] : 0.0;
            err = fmax(err, fabs(C[i + j * m] - ref));
            mx = fmax(mx, fabs(A0[i + j * m]));
        }
    slate_Matrix_destroy_r64(As);
    slate_Matrix_destroy_r64(Cs);
    slate_TriangularFactors_destroy_r64(T);
    slate_Matrix_r64 A2 = slate_Matrix_create_fromLAPACK_r64(m, n, A0, m, nb);
    slate_Matrix_r64 Bs = slate_Matrix_create_fromLAPACK_r64(m, 1, B, m, nb);
    int rc3 = slate_least_squares_solve_rank_r64(A2, Bs, 1e-10, &rank, 1, opts);
    slate_Matrix_destroy_r64(A2);
    slate_Matrix_destroy_r64(Bs);
    printf("rc %d %d %d seen %d rank %d err %.3e\n", rc1, rc2, rc3, seen, (int)rank, err / mx);
    return (rc1 == 0 && rc2 == 0 && rc3 == 0 && seen == n && rank == r && err <= 1e-12 * mx) ? 0 : 1;
}
"""


def test_c_api_and_fortran_module(tmp_path):
    src = tmp_path / "geqp3_c.c"
    src.write_text(C_SRC)
    exe = tmp_path / "geqp3_c"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT}/csrc/include", str(src), f"-L{PKG}", "-lslate_amd",
                    f"-Wl,-rpath,{PKG}", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f90 = open(os.path.join(ROOT, "csrc", "api", "slate_c_api.f90")).read()
    for name in ("slate_qr_factor_pivoted", "slate_qr_pivoted_multiply_by_q", "slate_least_squares_solve_rank"):
        for x in ("r32", "r64"):
            assert f"function {name}_{x}(" in f90, name
    assert "integer(c_int64_t) :: jpvt(*)" in f90


def test_native_tester_geqp3():
    r = subprocess.run(["make", "tester"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    port = _free_port()
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               SLATE_MASTER_PORT=str(port), SLATE_COMM="host", OMP_NUM_THREADS="2")
    r = subprocess.run([os.path.join(ROOT, "bin", "slate_tester"), "geqp3,gelsy", "--type", "s,d", "--dim", "200",
                        "--nb", "32", "--target", "h"], env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "all tests passed" in out, out[-4000:]
    assert out.count("pass") >= 4, out[-4000:]


def test_python_tester_geqp3(capsys):
    from slate_d35_amd import tester
    rc = tester.main(["geqp3", "gelsy", "--dim", "200", "--nb", "32", "--type", "s,d", "--target", "h"])
    out = capsys.readouterr().out
    assert rc == 0 and "all tests passed" in out, out
    assert out.count("pass") >= 4, out
    assert s.ops.geqp3_stats()["columns"] == 200
