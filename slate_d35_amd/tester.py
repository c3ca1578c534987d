"""Command-line tester (reference test/test.cc + test_*.cc):

    python -m slate_d35_amd.tester gemm potrf getrf --dim 1000:4000:1000 --nb 256 \
        --type d,z --target d --check y --repeat 2
    python -m torch.distributed.run --nproc-per-node 4 -m slate_d35_amd.tester gesv --grid 2x2

Every routine builds its operands with the counter-based generator (values do
not depend on the process grid), runs the driver, times it between device
synchronizations (MAX over ranks), and, with --check, evaluates the
reference tester's backward-error style residual against --tol * eps.  One
table row per (routine, type, dim, nb) is printed by rank 0.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

from . import _core as core
from . import models as M
from . import parallel
from . import _slate
from .utils import flops as F
from .utils.matgen import random_matrix

TYPES = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}


def eps(dt):
    return np.finfo(np.float32 if dt in (np.float32, np.complex64) else np.float64).eps


def parse_dims(spec):
    out = []
    for part in spec.split(","):
        if ":" in part:
            a, b, *c = [int(x) for x in part.split(":")]
            step = c[0] if c else a
            out.extend(range(a, b + 1, step))
        elif "x" in part:
            out.append(tuple(int(x) for x in part.split("x")))
        else:
            out.append(int(part))
    return out


# routines that take --gemm-precision (Option::GemmPrecision)
TAKES_GEMM_PRECISION = {"gemm", "getrf", "getrf_tntpiv", "getrf_nopiv", "potrf", "gesv_mixed", "gesv_mixed_gmres",
                        "posv_mixed", "posv_mixed_gmres"}


class Ctx:
    def __init__(self, a, dt, n, nb, name=""):
        self.a, self.dt, self.nb, self.name = a, dt, nb, name
        if isinstance(n, tuple):
            self.m, self.n = n[0], n[1]
            self.k = n[2] if len(n) > 2 else n[1]
        else:
            self.m = self.n = self.k = n
        self.target = a.target
        self.seed = 1

    def mat(self, m, n, kind="rands", seed=None):
        seed = self.seed if seed is None else seed
        self.seed += 1
        full = random_matrix(m, n, seed, self.dt, "rands" if kind in ("spd", "diag") else kind)
        if kind == "spd":
            full = (full + full.conj().T) / 2 + m * np.eye(m, dtype=self.dt)
        elif kind == "diag":
            full = full + m * np.eye(m, n, dtype=self.dt)
        return full.astype(self.dt), core.from_numpy(full.astype(self.dt), nb=self.nb, target=self.target)

    def gemm_precision(self):
        gp = getattr(self.a, "gemm_precision", None)
        return gp if gp and self.name in TAKES_GEMM_PRECISION else None

    def method_svd(self):
        ms = getattr(self.a, "method_svd", None)
        return ms if ms and (self.name == "svd" or (self.name == "svd_vals" and ms == "bisection")) else None

    def method_eig(self):
        me = getattr(self.a, "method_eig", None)
        return me if me and self.name in ("heev", "heev_vals") else None

    def method_hetrd(self):
        mh = getattr(self.a, "method_hetrd", None)
        return mh if mh and self.name in ("heev", "heevx") else None

    def method_gebrd(self):
        mg = getattr(self.a, "method_gebrd", None)
        return mg if mg and self.name in ("svd", "svd_vals") else None

    def opts(self):
        o = dict(target=self.target, lookahead=self.a.lookahead)
        if self.method_gebrd():
            o["method_gebrd"] = self.method_gebrd()
        if self.method_hetrd():
            o["method_hetrd"] = self.method_hetrd()
        if self.gemm_precision():
            o["gemm_precision"] = self.gemm_precision()
        if self.method_svd():
            o["method_svd"] = self.method_svd()
        if self.method_eig():
            o["method_eig"] = self.method_eig()
        return o


def backward(a, x, b):
    """||A x - b|| / (||A|| ||x|| n): the reference tester's solve check."""
    x = np.asarray(x)
    r = np.linalg.norm(a @ x - b)
    return r / max(np.linalg.norm(a) * np.linalg.norm(x) * a.shape[1], 1e-300)


def resid(x, ref):
    d = np.linalg.norm(np.asarray(x) - np.asarray(ref))
    return d / max(np.linalg.norm(np.asarray(ref)), 1e-300)


# Each routine: (flops(m, n, k), run(ctx) -> (seconds, error or None))
def _timed(fn):
    parallel_barrier()
    t0 = time.perf_counter()
    out = fn()
    _slate.sync()
    parallel_barrier()
    return time.perf_counter() - t0, out


def parallel_barrier():
    g = parallel.current_grid()
    if g is not None and g.p * g.q > 1:
        g.world.barrier()


def r_gemm(c):
    a, A = c.mat(c.m, c.k)
    b, B = c.mat(c.k, c.n)
    cc, Cm = c.mat(c.m, c.n)
    t, _ = _timed(lambda: M.gemm(1.5, A, B, -0.5, Cm, **c.opts()))
    err = resid(core.to_numpy(Cm), 1.5 * a @ b - 0.5 * cc) if c.a.check else None
    return t, err


def r_herk(c):
    a, A = c.mat(c.n, c.k)
    z, Z = c.mat(c.n, c.n)
    H = core.HermitianMatrix(core.Uplo.Lower, Z)
    t, _ = _timed(lambda: M.herk(1.0, A, 0.0, H, **c.opts()))
    err = resid(np.tril(core.to_numpy(Z)), np.tril(a @ a.conj().T)) if c.a.check else None
    return t, err


def r_trsm(c):
    t_, T = c.mat(c.m, c.m, "diag")
    b, B = c.mat(c.m, c.n)
    Tm = core.TriangularMatrix(core.Uplo.Lower, core.Diag.NonUnit, T)
    t, _ = _timed(lambda: M.trsm(core.Side.Left, 1.0, Tm, B, **c.opts()))
    err = resid(np.tril(t_) @ core.to_numpy(B), b) if c.a.check else None
    return t, err


def r_trmm(c):
    t_, T = c.mat(c.m, c.m)
    b, B = c.mat(c.m, c.n)
    Tm = core.TriangularMatrix(core.Uplo.Upper, core.Diag.NonUnit, T)
    t, _ = _timed(lambda: M.trmm(core.Side.Left, 2.0, Tm, B, **c.opts()))
    err = resid(core.to_numpy(B), 2.0 * np.triu(t_) @ b) if c.a.check else None
    return t, err


def r_hemm(c):
    h, H = c.mat(c.m, c.m, "spd")
    b, B = c.mat(c.m, c.n)
    cc, Cm = c.mat(c.m, c.n)
    Hm = core.HermitianMatrix(core.Uplo.Lower, H)
    t, _ = _timed(lambda: M.hemm(core.Side.Left, 1.0, Hm, B, 0.0, Cm, **c.opts()))
    err = resid(core.to_numpy(Cm), h @ b) if c.a.check else None
    return t, err


def r_potrf(c):
    a, A = c.mat(c.n, c.n, "spd")
    H = core.HermitianMatrix(core.Uplo.Lower, A)
    t, info = _timed(lambda: M.potrf(H, **c.opts()))
    err = None
    if c.a.check:
        L = np.tril(core.to_numpy(A))
        err = resid(L @ L.conj().T, a)
    return t, err


def r_posv(c):
    a, A = c.mat(c.n, c.n, "spd")
    b, B = c.mat(c.n, c.a.nrhs)
    H = core.HermitianMatrix(core.Uplo.Lower, A)
    t, info = _timed(lambda: M.posv(H, B, **c.opts()))
    err = resid(a @ core.to_numpy(B), b) if c.a.check else None
    return t, err


def _lu_check(c, a, A, piv):
    f = core.to_numpy(A)
    n = a.shape[0]
    L = np.tril(f, -1) + np.eye(n)
    U = np.triu(f)
    ip = [kk * c.nb + ti * c.nb + off for kk, pv in enumerate(piv) for (ti, off) in pv]
    pa = a.copy()
    for j, p in enumerate(ip):
        pa[[j, p]] = pa[[p, j]]
    return resid(L @ U, pa)


def r_getrf(c, method=None):
    a, A = c.mat(c.n, c.n)
    kw = c.opts()
    if method:
        kw["method_lu"] = method
    t, (info, piv) = _timed(lambda: M.getrf(A, **kw))
    return t, (_lu_check(c, a, A, piv) if c.a.check else None)


def r_getrf_tntpiv(c):
    return r_getrf(c, 2)


def r_gesv(c):
    a, A = c.mat(c.n, c.n)
    b, B = c.mat(c.n, c.a.nrhs)
    t, _ = _timed(lambda: M.gesv(A, B, **c.opts()))
    return t, (backward(a, core.to_numpy(B), b) if c.a.check else None)


def r_gesv_mixed(c, fn="gesv_mixed"):
    a, A = c.mat(c.n, c.n, "diag")
    b, B = c.mat(c.n, c.a.nrhs if fn == "gesv_mixed" else 1)
    X = core.from_numpy(np.zeros_like(b), nb=c.nb, target=c.target)
    t, _ = _timed(lambda: getattr(M, fn)(A, B, X, **c.opts()))
    return t, (resid(a @ core.to_numpy(X), b) if c.a.check else None)


def r_gesv_mixed_gmres(c):
    return r_gesv_mixed(c, "gesv_mixed_gmres")


def r_gesv_rbt(c):
    return r_gesv_mixed(c, "gesv_rbt")


def r_geqrf(c):
    a, A = c.mat(c.m, c.n)
    t, _ = _timed(lambda: M.geqrf(A, **c.opts()))
    err = None
    if c.a.check:
        r = np.triu(core.to_numpy(A))[: min(c.m, c.n)]
        # |R| = |Q^H A|: compare R^H R with A^H A
        err = resid(r.conj().T @ r, a.conj().T @ a)
    return t, err


def r_gels(c):
    a, A = c.mat(c.m, c.n)
    b, B = c.mat(max(c.m, c.n), c.a.nrhs)
    t, _ = _timed(lambda: M.gels(A, B, **c.opts()))
    err = None
    if c.a.check:
        # normal-equations residual ||A^H (A x - b)|| / (||A||^2 ||x|| n)
        x = core.to_numpy(B)[: c.n]
        r = a.conj().T @ (a @ x - b[: c.m])
        err = np.linalg.norm(r) / (np.linalg.norm(a) ** 2 * np.linalg.norm(x) * c.n)
    return t, err


def r_heev(c):
    a, A = c.mat(c.n, c.n, "spd")
    H = core.HermitianMatrix(core.Uplo.Lower, A)
    Z = core.from_numpy(np.zeros((c.n, c.n), c.dt), nb=c.nb, target=c.target)
    t, w = _timed(lambda: M.heev(H, Z, **c.opts()))
    err = None
    if c.a.check:
        z = core.to_numpy(Z)
        err = np.linalg.norm(a @ z - z * w) / (np.linalg.norm(a) * c.n)
    return t, err


def _sym(c):
    a, _ = c.mat(c.n, c.n)
    a = ((a + a.conj().T) / 2).astype(c.dt)
    return a, core.from_numpy(a, nb=c.nb, target=c.target)


def _tridiag(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def _real_only(c):
    if np.iscomplexobj(np.zeros(1, c.dt)):
        raise NotImplementedError("real types (the one-stage reduction)")


def r_hetrd(c):
    _real_only(c)
    a, A = _sym(c)
    H = core.HermitianMatrix(core.Uplo.Lower, A)
    t, (d, e, T) = _timed(lambda: M.hetrd(H, target=c.target))
    err = None
    if c.a.check:
        Q = core.from_numpy(np.eye(c.n, dtype=c.dt), nb=c.nb, target=c.target)
        M.unmtr_hetrd(core.Side.Left, core.Op.NoTrans, H, T, Q, target=c.target)
        q = core.to_numpy(Q)
        err = np.linalg.norm(q @ _tridiag(d, e) @ q.conj().T - a) / (np.linalg.norm(a) * c.n)
    return t, err


def r_unmtr_hetrd(c):
    _real_only(c)
    a, A = _sym(c)
    H = core.HermitianMatrix(core.Uplo.Lower, A)
    d, e, T = M.hetrd(H, target=c.target)
    b, C = c.mat(c.n, c.a.nrhs)
    t, _ = _timed(lambda: M.unmtr_hetrd(core.Side.Left, core.Op.ConjTrans, H, T, C, target=c.target))
    err = None
    if c.a.check:
        M.unmtr_hetrd(core.Side.Left, core.Op.NoTrans, H, T, C, target=c.target)
        err = resid(core.to_numpy(C), b)
    return t, err


def _bidiag(d, e, m):
    b = np.zeros((m, len(d)), dtype=np.asarray(d).dtype)
    b[:len(d), :] = np.diag(d) + np.diag(e, 1)
    return b


def r_gebrd(c):
    _real_only(c)
    if c.m < c.n:
        raise NotImplementedError("m >= n (the one-stage reduction)")
    a, A = c.mat(c.m, c.n)
    t, (d, e, TQ, TP) = _timed(lambda: M.gebrd(A, target=c.target))
    err = None
    if c.a.check:
        F = core.from_numpy(_bidiag(d, e, c.m).astype(c.dt), nb=c.nb, target=c.target)
        M.unmbr_gebrd("q", core.Side.Left, core.Op.NoTrans, A, TQ, F, target=c.target)
        M.unmbr_gebrd("p", core.Side.Right, core.Op.Trans, A, TP, F, target=c.target)
        err = np.linalg.norm(core.to_numpy(F) - a) / (np.linalg.norm(a) * c.n)
    return t, err


def r_unmbr_gebrd(c):
    _real_only(c)
    if c.m < c.n:
        raise NotImplementedError("m >= n (the one-stage reduction)")
    a, A = c.mat(c.m, c.n)
    d, e, TQ, TP = M.gebrd(A, target=c.target)
    b, C = c.mat(c.m, c.a.nrhs)
    t, _ = _timed(lambda: M.unmbr_gebrd("q", core.Side.Left, core.Op.Trans, A, TQ, C, target=c.target))
    err = None
    if c.a.check:
        M.unmbr_gebrd("q", core.Side.Left, core.Op.NoTrans, A, TQ, C, target=c.target)
        err = resid(core.to_numpy(C), b)
    return t, err


def r_geqp3(c):
    _real_only(c)
    a, A = c.mat(c.m, c.n)
    t, (jpvt, T) = _timed(lambda: M.geqp3(A, target=c.target))
    err = None
    if c.a.check:
        # ||A P - Q R|| / (||A|| n) and ||Q^T Q - I|| / m, Q from unmqr_geqp3 on the identity
        k = min(c.m, c.n)
        r = np.triu(core.to_numpy(A))[:k]
        Q = core.from_numpy(np.eye(c.m, dtype=c.dt), nb=c.nb, target=c.target)
        M.unmqr_geqp3(core.Side.Left, core.Op.NoTrans, A, T, Q, target=c.target)
        q = core.to_numpy(Q)
        d = np.abs(np.diag(r))
        ok = sorted(jpvt.tolist()) == list(range(c.n)) and np.all(d[1:] <= (1 + 4 * np.sqrt(eps(c.dt))) * d[:-1])
        err = max(np.linalg.norm(a[:, jpvt] - q[:, :k] @ r) / (np.linalg.norm(a) * c.n),
                  np.linalg.norm(q.T @ q - np.eye(c.m)) / c.m) if ok else float("inf")
    return t, err


def r_gelsy(c):
    _real_only(c)
    a, A = c.mat(c.m, c.n)
    b, B = c.mat(max(c.m, c.n), c.a.nrhs)
    t, rank = _timed(lambda: M.gelsy(A, B, target=c.target))
    err = None
    if c.a.check:
        # a random matrix has full rank: the normal-equations residual ||A^T (A x - b)|| / (||A||^2 ||x|| n)
        x = core.to_numpy(B)[: c.n]
        r = a.T @ (a @ x - b[: c.m])
        err = np.linalg.norm(r) / (np.linalg.norm(a) ** 2 * np.linalg.norm(x) * c.n)
        if rank != min(c.m, c.n):
            err = float("inf")
    return t, err


def r_svd(c):
    a, A = c.mat(c.m, c.n)
    k = min(c.m, c.n)
    U = core.from_numpy(np.zeros((c.m, k), c.dt), nb=c.nb, target=c.target)
    VT = core.from_numpy(np.zeros((k, c.n), c.dt), nb=c.nb, target=c.target)
    t, sv = _timed(lambda: M.svd(A, U, VT, **c.opts()))
    err = None
    if c.a.check:
        err = resid(core.to_numpy(U) @ np.diag(sv) @ core.to_numpy(VT), a)
    return t, err


def r_heev_vals(c):
    a, A = _sym(c)
    t, w = _timed(lambda: M.heev(core.HermitianMatrix(core.Uplo.Lower, A), None, **c.opts()))
    err = None
    if c.a.check:
        ref = np.linalg.eigvalsh(a.astype(np.complex128 if np.iscomplexobj(a) else np.float64))
        err = np.abs(w - ref).max() / (max(np.abs(ref).max(), 1e-300) * c.n)
    return t, err


def r_svd_vals(c):
    a, A = c.mat(c.m, c.n)
    t, sv = _timed(lambda: M.svd_vals(A, **c.opts()))
    err = None
    if c.a.check:
        ref = np.linalg.svd(a.astype(np.complex128 if np.iscomplexobj(a) else np.float64), compute_uv=False)
        err = np.abs(sv - ref).max() / (ref.max() * max(c.m, c.n))
    return t, err


def _bisect(c, bidiagonal):
    """stebz / bdsbz checked against the count alone: with delta = 16 eps
    max|T_ij|, value k (1-based, ascending) must have N(w_k - delta) <= k - 1
    and N(w_k + delta) >= k; for bdsbz N counts on the Golub-Kahan tridiagonal
    of order 2n.  The error is the number of values that miss a bound."""
    _real_only(c)
    n = c.n
    i = np.arange(n)
    d = (2 + (i % 7) / 10).astype(c.dt)
    e = (-1 + (i[:max(n - 1, 0)] % 5) / 20).astype(c.dt)
    fn = M.bdsbz if bidiagonal else M.stebz
    t, w = _timed(lambda: fn(d, e, target=c.target))
    if not c.a.check:
        return t, None
    if w.shape != (n,):
        return t, float(n)
    delta = c.dt(16) * np.finfo(c.dt).eps * max(np.abs(d).max(), np.abs(e).max() if e.size else 0)
    td, te, base = d, e, 0
    if bidiagonal:
        td = np.zeros(2 * n, c.dt)
        te = np.zeros(max(2 * n - 1, 0), c.dt)
        te[0::2] = d
        te[1::2] = e
        w, base = w[::-1], n
    from . import ops
    lo = ops.sturm_count(td, te, (w - delta).astype(c.dt), target=c.target)
    hi = ops.sturm_count(td, te, (w + delta).astype(c.dt), target=c.target)
    kk = base + 1 + np.arange(n)
    bad = int(np.sum(~((lo <= kk - 1) & (hi >= kk)))) + int(np.sum(np.diff(w) < 0))
    return t, float(bad)


def r_stebz(c):
    return _bisect(c, False)


def r_bdsbz(c):
    return _bisect(c, True)


def r_stein(c):
    """stein on the tridiagonal of stebz with that routine's values:
    r = max|T Z - Z diag(W)| / (n eps max|T_ij|) and o = max|Z^T Z - I| / (n eps);
    the error is max(r, o) eps."""
    _real_only(c)
    n = c.n
    i = np.arange(n)
    d = (2 + (i % 7) / 10).astype(c.dt)
    e = (-1 + (i[:max(n - 1, 0)] % 5) / 20).astype(c.dt)
    w = M.stebz(d, e, target=c.target)
    t, z = _timed(lambda: M.stein(d, e, w, target=c.target))
    if not c.a.check:
        return t, None
    from . import ops
    if z.shape != (n, n) or ops.stein_stats()["failed"]:
        return t, float(n)
    ep = float(np.finfo(c.dt).eps)
    T, Z, W = _tridiag(d, e).astype(np.float64), z.astype(np.float64), w.astype(np.float64)
    r = np.abs(T @ Z - Z * W).max() / (n * ep * np.abs(T).max())
    o = np.abs(Z.T @ Z - np.eye(n)).max() / (n * ep)
    return t, max(r, o) * ep, f"r={r:.3f} o={o:.3f}"


def r_heevx(c):
    """heevx for the index range 1 .. max(1, n / 10): ||A Z - Z Lambda|| /
    (n ||A||) and ||Z^H Z - I|| / n; the error is the larger."""
    a, A = c.mat(c.n, c.n, "spd")
    H = core.HermitianMatrix(core.Uplo.Lower, A)
    iu = max(1, c.n // 10)
    Z = core.from_numpy(np.zeros((c.n, iu), c.dt), nb=c.nb, target=c.target)
    t, w = _timed(lambda: M.heevx(H, Z, range="index", il=1, iu=iu, **c.opts()))
    if not c.a.check:
        return t, None
    if len(w) != iu:
        return t, float(c.n)
    z = core.to_numpy(Z)
    res = np.linalg.norm(a @ z - z * w) / (np.linalg.norm(a) * c.n)
    orth = np.linalg.norm(z.conj().T @ z - np.eye(iu)) / c.n
    return t, max(res, orth), f"m={iu} resid={res:.2e} orth={orth:.2e}"


def r_hesv(c):
    a, A = c.mat(c.n, c.n)
    a = (a + a.conj().T) / 2
    A = core.from_numpy(a, nb=c.nb, target=c.target)
    b, B = c.mat(c.n, c.a.nrhs)
    H = core.HermitianMatrix(core.Uplo.Lower, A)
    t, _ = _timed(lambda: M.hesv(H, B, **c.opts()))
    return t, (backward(a, core.to_numpy(B), b) if c.a.check else None)


def r_gbsv(c):
    kl = ku = max(1, c.nb // 4)
    a, _ = c.mat(c.n, c.n, "diag")
    a = np.tril(np.triu(a, -kl), ku)
    A = core.BandMatrix(kl, ku, core.from_numpy(a, nb=c.nb, target=c.target))
    b, B = c.mat(c.n, c.a.nrhs)
    t, _ = _timed(lambda: M.gbsv(A, B, **c.opts()))
    return t, (resid(a @ core.to_numpy(B), b) if c.a.check else None)


def r_genorm(c):
    a, A = c.mat(c.m, c.n)
    t, v = _timed(lambda: M.norm(core.Norm.One, A, **c.opts()))
    return t, (abs(v - np.linalg.norm(a, 1)) / np.linalg.norm(a, 1) if c.a.check else None)


def r_gecondest(c):
    a, A = c.mat(c.n, c.n, "diag")
    anorm = M.norm(core.Norm.One, A, **c.opts())
    M.getrf(A, **c.opts())
    t, rc = _timed(lambda: M.gecondest(core.Norm.One, A, anorm, **c.opts()))
    err = None
    if c.a.check:
        ref = 1 / np.linalg.cond(a, 1)
        err = 0.0 if ref * 0.999 <= abs(rc) <= 10 * ref else 1.0   # estimator within [1, 10] x
    return t, err


def r_trtri(c):
    t_, T = c.mat(c.n, c.n, "diag")
    Tm = core.TriangularMatrix(core.Uplo.Lower, core.Diag.NonUnit, T)
    t, _ = _timed(lambda: M.trtri(Tm, **c.opts()))
    return t, (resid(np.tril(core.to_numpy(T)) @ np.tril(t_), np.eye(c.n)) if c.a.check else None)


ROUTINES = {
    "gemm": (r_gemm, lambda m, n, k: F.gemm_flops(m, n, k)),
    "hemm": (r_hemm, lambda m, n, k: 2.0 * m * m * n),
    "herk": (r_herk, lambda m, n, k: F.herk_flops(n, k)),
    "trmm": (r_trmm, lambda m, n, k: 1.0 * m * m * n),
    "trsm": (r_trsm, lambda m, n, k: F.trsm_flops(m, n)),
    "potrf": (r_potrf, lambda m, n, k: F.potrf_flops(n)),
    "posv": (r_posv, lambda m, n, k: F.potrf_flops(n)),
    "getrf": (r_getrf, lambda m, n, k: F.getrf_flops(n)),
    "getrf_tntpiv": (r_getrf_tntpiv, lambda m, n, k: F.getrf_flops(n)),
    "gesv": (r_gesv, lambda m, n, k: F.getrf_flops(n)),
    "gesv_mixed": (r_gesv_mixed, lambda m, n, k: F.getrf_flops(n)),
    "gesv_mixed_gmres": (r_gesv_mixed_gmres, lambda m, n, k: F.getrf_flops(n)),
    "gesv_rbt": (r_gesv_rbt, lambda m, n, k: F.getrf_flops(n)),
    "geqrf": (r_geqrf, lambda m, n, k: F.geqrf_flops(m, n)),
    "gels": (r_gels, lambda m, n, k: F.geqrf_flops(m, n)),
    "heev": (r_heev, lambda m, n, k: 4.0 / 3.0 * n ** 3),
    "heev_vals": (r_heev_vals, lambda m, n, k: 4.0 / 3.0 * n ** 3),
    "svd_vals": (r_svd_vals, lambda m, n, k: 8.0 / 3.0 * n ** 3),
    "stebz": (r_stebz, lambda m, n, k: 0.0),
    "bdsbz": (r_bdsbz, lambda m, n, k: 0.0),
    "stein": (r_stein, lambda m, n, k: 0.0),
    "heevx": (r_heevx, lambda m, n, k: 4.0 / 3.0 * n ** 3),
    "hetrd": (r_hetrd, lambda m, n, k: 4.0 / 3.0 * n ** 3),
    "unmtr_hetrd": (r_unmtr_hetrd, lambda m, n, k: 0.0),
    "gebrd": (r_gebrd, lambda m, n, k: 4.0 * m * n * n - 4.0 / 3.0 * n ** 3),
    "unmbr_gebrd": (r_unmbr_gebrd, lambda m, n, k: 0.0),
    "svd": (r_svd, lambda m, n, k: 8.0 / 3.0 * n ** 3),
    "geqp3": (r_geqp3, lambda m, n, k: F.geqrf_flops(m, n)),
    "gelsy": (r_gelsy, lambda m, n, k: F.geqrf_flops(m, n)),
    "hesv": (r_hesv, lambda m, n, k: n ** 3 / 3.0),
    "gbsv": (r_gbsv, lambda m, n, k: 0.0),
    "genorm": (r_genorm, lambda m, n, k: 1.0 * m * n),
    "gecondest": (r_gecondest, lambda m, n, k: 0.0),
    "trtri": (r_trtri, lambda m, n, k: n ** 3 / 3.0),
}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("routines", nargs="+", help="routine names or 'all'")
    ap.add_argument("--dim", default="500", help="n, or a:b:step, or MxNxK list")
    ap.add_argument("--nb", default="256")
    ap.add_argument("--type", default="d")
    ap.add_argument("--target", default="d" if _slate.device_available() else "h")
    ap.add_argument("--grid", default="")
    ap.add_argument("--lookahead", type=int, default=1)
    ap.add_argument("--nrhs", type=int, default=10)
    ap.add_argument("--check", default="y")
    ap.add_argument("--tol", type=float, default=50.0)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--gemm-precision", default=None, choices=["native", "bf16", "bf16x3", "bf16x6"],
                    help="arithmetic of the fp32 trailing updates of gemm, getrf*, potrf and the mixed solvers")
    ap.add_argument("--method-svd", default=None, choices=["qr", "dc", "bisection"],
                    help="bidiagonal stage of svd: QR iteration (default) or divide and conquer; "
                         "bisection: of svd_vals (values only)")
    ap.add_argument("--method-eig", default=None, choices=["qr", "dc", "bisection"],
                    help="tridiagonal stage of heev / heev_vals; bisection: values only")
    ap.add_argument("--method-hetrd", default=None, choices=["two_stage", "one_stage"],
                    help="tridiagonal reduction of heev: two stages (default) or the one-stage hetrd")
    ap.add_argument("--method-gebrd", default=None, choices=["two_stage", "one_stage"],
                    help="bidiagonal reduction of svd: two stages (default) or the one-stage gebrd")
    a = ap.parse_args(argv)
    a.check = a.check.lower().startswith("y")
    world = parallel.world_size()
    if a.grid:
        p, q = (int(x) for x in a.grid.split("x"))
    else:
        p, q = parallel.choose_grid(world)
    parallel.init_grid(p, q)
    rank = parallel.world_rank()
    names = list(ROUTINES) if a.routines == ["all"] else a.routines
    hdr = f"{'routine':18s} {'type':4s} {'m':>6s} {'n':>6s} {'k':>6s} {'nb':>5s} {'p':>2s} {'q':>2s} " \
          f"{'error':>10s} {'time(s)':>10s} {'gflop/s':>10s}  status"
    if rank == 0:
        print(hdr)
    nfail = 0
    for name in names:
        if name not in ROUTINES:
            raise SystemExit(f"unknown routine {name}; available: {', '.join(ROUTINES)}")
        fn, fl = ROUTINES[name]
        for tch in a.type.split(","):
            dt = TYPES[tch]
            for dim in parse_dims(a.dim):
                for nb in parse_dims(a.nb):
                    for _ in range(a.repeat):
                        c = Ctx(a, dt, dim, nb, name)
                        try:
                            t, err, *note = fn(c)   # a routine may add a note to its row
                            ok = err is None or err <= a.tol * eps(dt)
                            status = "pass" if ok else "FAILED"
                        except NotImplementedError as e:  # precision not provided (e.g. mixed for s/c)
                            t, err, note, status = float("nan"), None, [], f"skip ({e})"
                            ok = True
                        nfail += 0 if ok else 1
                        gf = fl(c.m, c.n, c.k) / t / 1e9 if t == t and t > 0 else float("nan")
                        if rank == 0:
                            es = "NA" if err is None else f"{err:.2e}"
                            print(f"{name:18s} {tch:4s} {c.m:6d} {c.n:6d} {c.k:6d} {nb:5d} {p:2d} {q:2d} "
                                  f"{es:>10s} {t:10.4f} {gf:10.2f}  {status}"
                                  + (f"  {note[0]}" if note else "")
                                  + (f"  gemm_precision={c.gemm_precision()}" if c.gemm_precision() else "")
                                  + (f"  method_svd={c.method_svd()}" if c.method_svd() else "")
                                  + (f"  method_eig={c.method_eig()}" if c.method_eig() else "")
                                  + (f"  method_hetrd={c.method_hetrd()}" if c.method_hetrd() else "")
                                  + (f"  method_gebrd={c.method_gebrd()}" if c.method_gebrd() else ""),
                                  flush=True)
    if rank == 0:
        print(f"# {nfail} failed" if nfail else "# all tests passed")
    return 1 if nfail else 0


if __name__ == "__main__":
    sys.exit(main())
