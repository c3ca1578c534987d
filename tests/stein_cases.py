"""Cases shared by test_stein.py (host target) and test_stein_gpu.py (device
target): every check takes the target, so both files assert the same
properties with the same bounds.

Measures for stein (Z taken to float64, W the values passed in, eps of the
input precision):
    r = max |T Z - Z diag(W)| / (n eps max|T_ij|)
    o = max |Z^T Z - I| / (n eps)
The yardstick is LAPACK's stebz + stein on the same inputs.  TABLE records
what they give (r64, r32, o64, o32), measured on the CPU through
scipy.linalg.get_lapack_funcs(("stebz", "stein")).  The bound of a case and a
measure is 8 max(1, recorded): the floor of 1, which is n eps, because a
recorded 0.003 is luck, not a contract; the factor 8 because other start
vectors, a whole cluster orthonormalised per round and the project's own
bisection values change the constant but not the order.
test_stein.py::test_lapack_table recomputes TABLE where scipy is importable.

heevx: the values against heev and the residuals within drv_tol of
stebz_cases.py (1e-3 float32, 1e-10 float64).
"""
import functools

import numpy as np

import slate_d35_amd as s
import stebz_cases as B

RANDOM_SIZES = [2, 3, 65, 130, 257, 600]   # 65 / 130: one past a wave, one past two; 600: above the 512-entry LDS chunk

# case: (r float64, r float32, o float64, o float32) of LAPACK
TABLE = {
    "random": (0.31, 0.23, 0.25, 0.36),
    "random_subset": (0.004, 0.003, 0.014, 0.008),
    "wilkinson": (0.038, 0.014, 0.161, 0.304),
    "laplacian": (0.010, 0.007, 0.466, 0.354),
    "direct_sum": (0.022, 0.014, 0.531, 0.703),
    "cluster": (1.50, 1.50, 0.030, 0.007),
    "glued": (0.008, 0.182, 0.048, 0.030),
    "graded": (0.008, 0.009, 0.034, 0.056),
}
FACTOR = 8.0


def bounds(case, dt):
    r64, r32, o64, o32 = TABLE[case]
    r, o = (r32, o32) if dt == np.float32 else (r64, o64)
    return FACTOR * max(1.0, r), FACTOR * max(1.0, o)


def measures(d, e, w, z, dt):
    """(r, o) in float64 on the input as rounded to dt"""
    n = len(d)
    T = B.dense_tri(d, e)
    Z = np.asarray(z, np.float64)
    W = np.asarray(w, np.float64)
    if Z.shape[1] == 0:
        return 0.0, 0.0
    r = np.abs(T @ Z - Z * W[None, :]).max() / (n * B.eps(dt) * np.abs(T).max())
    o = np.abs(Z.T @ Z - np.eye(Z.shape[1])).max() / (n * B.eps(dt))
    return float(r), float(o)


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def tridiagonal(case, dtname, n=0):
    """(d, e) of a case in precision dtname; computed once, never modified."""
    dt = np.dtype(dtname).type
    ep = B.eps(dt)
    if case in ("random", "random_subset"):
        d, e, _ = B.random_tri(n, dtname)
        return d, e
    if case == "wilkinson":
        k = (n - 1) // 2
        d, e = np.abs(np.arange(-k, k + 1)).astype(dt), np.ones(n - 1, dt)
    elif case == "laplacian":
        d, e = np.full(n, 2.0, dt), np.full(n - 1, -1.0, dt)
    elif case == "direct_sum":   # the matrix of stebz_cases.check_stebz_direct_sum
        rng = np.random.default_rng(5)
        da, ea = rng.standard_normal(20), rng.standard_normal(19)
        dc, ec = rng.standard_normal(17), rng.standard_normal(16)
        d = np.concatenate([da, da, dc]).astype(dt)
        e = np.concatenate([ea, [0.0], ea, [0.0], ec]).astype(dt)
    elif case == "cluster":
        rng = np.random.default_rng(7)
        d = (1.0 + 64 * ep * rng.standard_normal(200)).astype(dt)
        e = np.full(199, 256 * ep, dt)
    elif case == "glued":
        d = np.tile(np.abs(np.arange(-10, 11)), 5).astype(dt)
        e = np.ones(104, dt)
        e[20::21] = np.sqrt(ep)
    elif case == "graded":
        d = (10.0 ** (-np.arange(65) / 8.0)).astype(dt)
        e = (d[:-1] / 2).astype(dt)
    else:
        raise KeyError(case)
    for a in (d, e):
        a.setflags(write=False)
    return d, e


# (case, n, range keywords)
CASES = ([("random", n, {}) for n in RANDOM_SIZES] +
         [("random_subset", 257, dict(range="index", il=5, iu=36)),
          ("wilkinson", 21, {}), ("wilkinson", 201, {}),
          ("wilkinson", 21, dict(range="index", il=1, iu=20)),       # cuts the top pair
          ("wilkinson", 201, dict(range="index", il=1, iu=200)),
          ("laplacian", 257, {}), ("direct_sum", 57, {}), ("cluster", 200, {}), ("glued", 105, {}),
          ("graded", 65, {})])
CASE_IDS = [f"{c}{n}{'_' + kw['range'] if kw else ''}" for c, n, kw in CASES]


def check_stein_case(case, n, kw, dt, tg):
    """stebz then stein on the target: shapes, the two measures within the
    bounds, nothing failed.  Returns (r, o)."""
    d, e = tridiagonal(case, np.dtype(dt).name, n)
    w = s.stebz(d, e, target=tg, **kw)
    z = s.stein(d, e, w, target=tg)
    st = s.ops.stein_stats()
    assert z.dtype == dt and z.shape == (len(d), len(w)), (z.dtype, z.shape)
    assert np.all(np.isfinite(z))
    r, o = measures(d, e, w, z, dt)
    rb, ob = bounds(case, dt)
    print(f"stein {case} n {len(d)} m {len(w)} {np.dtype(dt).name} {tg}: r {r:.3f} (bound {rb:.1f}) "
          f"o {o:.3f} (bound {ob:.1f}) clusters {st['clusters']} largest {st['largest_cluster']}")
    assert st["n"] == len(d) and st["values"] == len(w) and st["rounds"] == 5, st
    assert st["failed"] == 0, st
    assert r <= rb and o <= ob, (r, rb, o, ob)
    if case == "cluster":
        assert st["clusters"] == 1 and st["largest_cluster"] == 200, st   # spans four waves
    return r, o


def check_stein_small(tg):
    """n = 1, m = 0 (a value range that finds nothing), n = 0, the all-zero matrix"""
    for dt in (np.float64, np.float32):
        z = s.stein(np.array([3.0], dt), np.zeros(0, dt), np.array([3.0], dt), target=tg)
        assert z.dtype == dt and z.shape == (1, 1) and z[0, 0] == 1
        assert s.ops.stein_stats()["launches"] == 0
        d, e = tridiagonal("random", np.dtype(dt).name, 65)
        w = s.stebz(d, e, range="value", vl=-1e6, vu=-1e5, target=tg)
        assert len(w) == 0
        z = s.stein(d, e, w, target=tg)
        assert z.shape == (65, 0)
        st = s.ops.stein_stats()
        assert st["launches"] == 0 and st["values"] == 0 and st["n"] == 65, st
        assert s.stein(np.zeros(0, dt), np.zeros(0, dt), np.zeros(0, dt), target=tg).shape == (0, 0)
        z = s.stein(np.zeros(6, dt), np.zeros(5, dt), np.zeros(4, dt), target=tg)
        assert np.array_equal(z, np.eye(6, 4, dtype=dt))
        assert s.ops.stein_stats()["launches"] == 0


def check_stein_refusals(tg):
    d, e = np.arange(1.0, 6.0), np.ones(4)
    w = s.stebz(d, e, target="h")

    def refused(dd, ee, ww, text):
        try:
            s.stein(dd, ee, ww, target=tg)
        except Exception as ex:   # slate::Exception arrives as RuntimeError
            assert text in str(ex), str(ex)
        else:
            raise AssertionError(f"stein accepted an input that should raise ({text})")

    for bad in (np.nan, np.inf):
        db, eb, wb = d.copy(), e.copy(), w.copy()
        db[2] = eb[1] = wb[3] = bad
        refused(db, e, w, "NaN or Inf")
        refused(d, eb, w, "NaN or Inf")
        refused(d, e, wb, "NaN or Inf")
    refused(d, e, w[::-1].copy(), "not ascending")
    refused(d, e, np.concatenate([w, [w[-1] + 1.0]]), "m = 6 > n = 5")


# ---------------------------------------------------------------- heevx
def herm(n, dt, seed):
    if np.issubdtype(dt, np.complexfloating):
        rdt = np.float64 if dt == np.complex128 else np.float32
        a = (s.utils.random_matrix(n, n, seed=seed, dtype=rdt) +
             1j * s.utils.random_matrix(n, n, seed=seed + 100, dtype=rdt)).astype(dt)
        return ((a + a.conj().T) / 2).astype(dt)
    return B.sym(n, dt, seed)


def real_of(dt):
    return {np.complex128: np.float64, np.complex64: np.float32}.get(dt, dt)


def check_heevx(n, dt, mh, tg):
    """Range::All, an index range and a value range: values against heev,
    residual and orthogonality within drv_tol, zero columns beyond m; heev
    itself returns the same bits before and after."""
    a = herm(n, dt, n + 1)
    tol = B.drv_tol(real_of(dt))
    anorm = np.abs(a).max()

    def H():
        return s.HermitianMatrix(s.Uplo.Lower, s.from_numpy(a.copy(), nb=64, target=tg))

    def full():
        Z = s.from_numpy(np.zeros((n, n), dt), nb=64, target=tg)
        w = np.asarray(s.heev(H(), Z, target=tg))
        return w, s.to_numpy(Z)

    w0, z0 = full()
    vl, vu = float(w0[n // 3] + w0[n // 3 + 1]) / 2, float(w0[n // 2] + w0[n // 2 + 1]) / 2
    ranges = [(dict(range="all"), 0, n), (dict(range="index", il=5, iu=36), 4, 36),
              (dict(range="value", vl=vl, vu=vu), n // 3 + 1, n // 2 + 1)]
    for kw, k0, k1 in ranges:
        for zcols in (n, max(k1 - k0, 1) + 3):
            if zcols > n:
                continue
            Z = s.from_numpy(np.full((n, zcols), 7, dt), nb=64, target=tg)
            w = s.heevx(H(), Z, target=tg, method_hetrd=mh, **kw)
            m = len(w)
            assert m == k1 - k0, (kw, m, k0, k1)
            assert np.abs(w - w0[k0:k1]).max() <= tol * np.abs(w0).max(), kw
            z = s.to_numpy(Z)
            assert np.all(z[:, m:] == 0), kw
            z = z[:, :m].astype(np.complex128 if np.iscomplexobj(z) else np.float64)
            a64 = a.astype(z.dtype)
            res = np.abs(a64 @ z - z * w[None, :].astype(np.float64)).max()
            orth = np.abs(z.conj().T @ z - np.eye(m)).max()
            print(f"heevx {np.dtype(dt).name} n {n} {mh} {tg} {kw.get('range')} m {m}: res {res / anorm:.2e} "
                  f"orth {orth:.2e} tol {tol:.0e} failed {s.ops.stein_stats()['failed']}")
            assert res <= tol * anorm and orth <= tol, (kw, res, orth)
            st = s.ops.stein_stats()
            assert st["values"] == m and st["n"] == n
        # values only
        wv = s.heevx(H(), None, target=tg, method_hetrd=mh, **kw)
        assert np.array_equal(wv, w), kw
    w1, z1 = full()
    assert np.array_equal(w1, w0) and np.array_equal(z1, z0)   # the shared body left heev alone


def check_heevx_unmodified(tg):
    n, dt = 130, np.float64
    a = herm(n, dt, 9)
    A = s.from_numpy(a.copy(), nb=64, target=tg)
    Z = s.from_numpy(np.zeros((n, 40), dt), nb=64, target=tg)
    s.heevx(s.HermitianMatrix(s.Uplo.Lower, A), Z, range="index", il=1, iu=40, target=tg)
    assert np.array_equal(s.to_numpy(A), a)
    # syevx is the same on a SymmetricMatrix
    Z2 = s.from_numpy(np.zeros((n, 40), dt), nb=64, target=tg)
    w2 = s.syevx(s.SymmetricMatrix(s.Uplo.Lower, A), Z2, range="index", il=1, iu=40, target=tg)
    assert len(w2) == 40 and np.array_equal(s.to_numpy(Z2), s.to_numpy(Z))


def check_heevx_refusals(tg):
    n, dt = 130, np.float64
    a = herm(n, dt, 3)
    H = s.HermitianMatrix(s.Uplo.Lower, s.from_numpy(a.copy(), nb=64, target=tg))
    Z = s.from_numpy(np.zeros((n, 10), dt), nb=64, target=tg)
    try:
        s.heevx(H, Z, range="index", il=1, iu=20, target=tg)
    except Exception as ex:
        assert "m = 20" in str(ex), str(ex)
    else:
        raise AssertionError("a Z with too few columns accepted")
    c = herm(n, np.complex128, 4)
    Hc = s.HermitianMatrix(s.Uplo.Lower, s.from_numpy(c.copy(), nb=64, target=tg))
    try:
        s.heevx(Hc, None, target=tg, method_hetrd="one_stage")
    except Exception as ex:
        assert "real types only" in str(ex), str(ex)
    else:
        raise AssertionError("one-stage heevx with a complex type accepted")
    for kw in (dict(range="value", vl=1.0, vu=1.0), dict(range="index", il=0, iu=2), dict(range="index", il=3, iu=n + 1)):
        try:
            s.heevx(H, None, target=tg, **kw)
        except Exception as ex:
            assert "vl < vu" in str(ex) or "il <= iu" in str(ex), str(ex)
        else:
            raise AssertionError(f"heevx accepted {kw}")
    # heev with the bisection method and vectors is still refused
    Zf = s.from_numpy(np.zeros((n, n), dt), nb=64, target=tg)
    try:
        s.heev(H, Zf, target=tg, method_eig="bisection")
    except Exception as ex:
        assert "values only" in str(ex) and "inverse iteration" in str(ex), str(ex)
    else:
        raise AssertionError("vectors with bisection accepted")
