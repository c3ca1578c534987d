"""Cases shared by test_stebz.py (host target) and test_stebz_gpu.py (device
target): every check takes the target, so both files assert the same
properties with the same bounds.

Bounds (eps of the precision under test, max|T| the largest entry):
  * float32 against float64 numpy on the float32-rounded input:
    16 eps32 max|T|.  The counted matrix differs from T by about 2.5 eps per
    entry and || |T| ||_2 <= 3 max|T|, plus the final interval 2 eps |lambda|.
  * float64 against numpy in float64, which carries its own O(n eps) error:
    test_hetrd.py's 1e-10 max|ref|.
  * float64 against closed forms: 16 eps64 max|T|; for the bidiagonal
    d = e = 1 the relative bound 4 (2n - 1) eps.
"""
import functools

import numpy as np

import slate_d35_amd as s

SIZES = [1, 2, 63, 64, 65, 257, 1000]   # 63/64/65: the wave; 257: > 4 waves; 1000: crosses the 512-entry staging chunk


def eps(dt):
    return float(np.finfo(dt).eps)


def tmax(d, e):
    return max(np.abs(d).max() if len(d) else 0.0, np.abs(e).max() if len(e) else 0.0)


def dense_tri(d, e):
    d = np.asarray(d, np.float64)
    e = np.asarray(e, np.float64)
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def dense_bi(d, e):
    return np.diag(np.asarray(d, np.float64)) + np.diag(np.asarray(e, np.float64), 1)


@functools.lru_cache(maxsize=None)
def random_tri(n, dtname):
    """(d, e, float64 eigenvalues of the rounded input); computed once, never modified."""
    dt = np.dtype(dtname).type
    rng = np.random.default_rng(1000 + n)
    d = rng.standard_normal(n).astype(dt)
    e = rng.standard_normal(max(n - 1, 0)).astype(dt)
    ref = np.linalg.eigvalsh(dense_tri(d, e))
    for a in (d, e, ref):
        a.setflags(write=False)
    return d, e, ref


@functools.lru_cache(maxsize=None)
def random_bi(n, dtname):
    dt = np.dtype(dtname).type
    rng = np.random.default_rng(2000 + n)
    d = rng.standard_normal(n).astype(dt)
    e = rng.standard_normal(max(n - 1, 0)).astype(dt)
    ref = np.linalg.svd(dense_bi(d, e), compute_uv=False)
    for a in (d, e, ref):
        a.setflags(write=False)
    return d, e, ref


def bound_vs_numpy(dt, ref, d, e):
    """float32: the derived 16 eps32 max|T|; float64: numpy's own error, 1e-10 max|ref|."""
    if dt == np.float32:
        return 16 * eps(np.float32) * tmax(d, e)
    return 1e-10 * max(np.abs(ref).max(), np.finfo(np.float64).tiny)


def clear_shifts(ref, scale, dt, count, seed):
    """`count` shifts of precision dt, each at least 1e-3 scale away from every
    reference eigenvalue (checked; a shift that fails is drawn again)."""
    rng = np.random.default_rng(seed)
    lo, hi = ref.min() - 0.5 * scale, ref.max() + 0.5 * scale
    out = []
    for _ in range(100000):
        x = dt(rng.uniform(lo, hi))
        if np.abs(ref - np.float64(x)).min() >= 1e-3 * scale:
            out.append(x)
            if len(out) == count:
                break
    assert len(out) == count
    x = np.array(out, dt)
    assert np.all(np.abs(ref[None, :] - x.astype(np.float64)[:, None]).min(axis=1) >= 1e-3 * scale)
    return x


# ---------------------------------------------------------------- 1. the count
def check_sturm_count(n, dt, tg):
    d, e, ref = random_tri(n, np.dtype(dt).name)
    x = np.sort(clear_shifts(ref, tmax(d, e), dt, 50, 7 * n + 1))
    c = s.ops.sturm_count(d, e, x, target=tg)
    want = (ref[None, :] < x.astype(np.float64)[:, None]).sum(axis=1)
    assert c.dtype == np.int64 and c.shape == (50,)
    assert np.array_equal(c, want), (c, want)
    assert np.all(np.diff(c) >= 0)


# ---------------------------------------------------------------- 2. stebz, all
def check_stebz_random(n, dt, tg):
    d, e, ref = random_tri(n, np.dtype(dt).name)
    w = s.stebz(d, e, target=tg)
    assert w.dtype == dt and w.shape == (n,)
    err, b = np.abs(w - ref).max(), bound_vs_numpy(dt, ref, d, e)
    print(f"stebz random {np.dtype(dt).name} n {n} {tg}: err {err:.3e} bound {b:.3e}")
    assert err <= b
    assert np.all(np.diff(w) >= 0)
    st = s.ops.stebz_stats()
    assert st["n"] == n and st["values"] == n and st["points"] >= 1 and st["steps"] >= 1


def check_stebz_laplacian(n, tg):
    d, e = np.full(n, 2.0), np.full(n - 1, -1.0)
    k = np.arange(1, n + 1)
    ref = 2 - 2 * np.cos(k * np.pi / (n + 1))
    w = s.stebz(d, e, target=tg)
    err, b = np.abs(w - ref).max(), 16 * eps(np.float64) * 2.0
    print(f"stebz (-1, 2, -1) n {n} {tg}: err {err:.3e} bound {b:.3e}")
    assert err <= b


def check_stebz_wilkinson(tg):
    d = np.abs(np.arange(-10, 11)).astype(np.float64)
    e = np.ones(20)
    ref = np.linalg.eigvalsh(dense_tri(d, e))
    w = s.stebz(d, e, target=tg)
    assert np.all(np.diff(w) >= 0)
    assert np.abs(w - ref).max() <= 1e-10 * ref.max()
    assert 0 <= w[-1] - w[-2] <= 1e-12   # the top pair agrees to about 1e-14 and comes back in order
    assert abs((w[-1] - w[-2]) - (ref[-1] - ref[-2])) <= 2 * 16 * eps(np.float64) * 10.0


def check_stebz_direct_sum(tg):
    """diag(A, A, C) with two zero e: every eigenvalue of A twice, exactly."""
    rng = np.random.default_rng(5)
    da, ea = rng.standard_normal(20), rng.standard_normal(19)
    dc, ec = rng.standard_normal(17), rng.standard_normal(16)
    d = np.concatenate([da, da, dc])
    e = np.concatenate([ea, [0.0], ea, [0.0], ec])
    ref = np.linalg.eigvalsh(dense_tri(d, e))
    w = s.stebz(d, e, target=tg)
    assert w.shape == (57,) and np.all(np.diff(w) >= 0)
    assert np.abs(w - ref).max() <= 1e-10 * np.abs(ref).max()
    wa = s.stebz(da, ea, target=tg)
    b = 16 * eps(np.float64) * tmax(d, e)
    for lam in wa:
        near = np.abs(w - lam) <= b
        assert near.sum() >= 2, (lam, w[np.argsort(np.abs(w - lam))[:3]])


def check_stebz_zero(tg):
    for n in (1, 5, 64):
        w = s.stebz(np.zeros(n), np.zeros(n - 1), target=tg)
        assert w.shape == (n,) and np.all(w == 0)
        st = s.ops.stebz_stats()
        assert st["launches"] == 0 and st["values"] == n
        sv = s.bdsbz(np.zeros(n), np.zeros(n - 1), target=tg)
        assert sv.shape == (n,) and np.all(sv == 0)
    assert s.stebz(np.zeros(0), np.zeros(0), target=tg).shape == (0,)
    assert s.bdsbz(np.zeros(0), np.zeros(0), target=tg).shape == (0,)


def check_stebz_scaled(tg):
    d, e, _ = random_tri(257, "float64")
    w = s.stebz(d, e, target=tg)
    b = 16 * eps(np.float64) * tmax(d, e)
    for scale in (1e150, 1e-150):
        ws = s.stebz(d * scale, e * scale, target=tg)
        assert np.all(np.isfinite(ws))
        assert np.abs(ws / scale - w).max() <= b
    sd, se, _ = random_bi(65, "float64")
    sv = s.bdsbz(sd, se, target=tg)
    for scale in (1e150, 1e-150):
        ss = s.bdsbz(sd * scale, se * scale, target=tg)
        assert np.abs(ss / scale - sv).max() <= 16 * eps(np.float64) * tmax(sd, se)


# ---------------------------------------------------------------- 3. ranges
def check_ranges(n, dt, tg):
    d, e, ref = random_tri(n, np.dtype(dt).name)
    w = s.stebz(d, e, target=tg)
    pairs = [(1, 1), (n, n)]
    if n >= 5:
        pairs.append((3, n - 2))
    if n >= 70:
        pairs.append((60, 70))      # crosses the 64-eigenvalue boundary
    for il, iu in pairs:
        wi = s.stebz(d, e, range="index", il=il, iu=iu, target=tg)
        assert np.array_equal(wi, w[il - 1:iu]), (il, iu)
        assert s.ops.stebz_stats()["values"] == iu - il + 1
    if n >= 5:
        vl, vu = np.sort(clear_shifts(ref, tmax(d, e), dt, 2, 11 * n + 3))
        c = s.ops.sturm_count(d, e, np.array([vl, vu], dt), target=tg)
        wv = s.stebz(d, e, range=s.Range.Value, vl=vl, vu=vu, target=tg)
        assert len(wv) == c[1] - c[0] == ((ref >= vl) & (ref < vu)).sum()
        assert np.array_equal(wv, w[c[0]:c[1]])
    # everything below / above the spectrum
    assert len(s.stebz(d, e, range="value", vl=-1e6, vu=-1e5, target=tg)) == 0
    assert np.array_equal(s.stebz(d, e, range="value", vl=-1e6, vu=1e6, target=tg), w)


def check_refusals(tg):
    d, e = np.arange(1.0, 6.0), np.ones(4)
    for fn in (s.stebz, s.bdsbz):
        for kw in (dict(range="value", vl=1.0, vu=1.0), dict(range="value", vl=2.0, vu=1.0),
                   dict(range="index", il=0, iu=2), dict(range="index", il=3, iu=2),
                   dict(range="index", il=1, iu=6)):
            try:
                fn(d, e, target=tg, **kw)
            except Exception as ex:   # slate::Exception arrives as RuntimeError
                assert "vl < vu" in str(ex) or "il <= iu" in str(ex), str(ex)
            else:
                raise AssertionError(f"{fn.__name__} accepted {kw}")
        for bad in (np.nan, np.inf):
            db = d.copy()
            db[2] = bad
            for dd, ee in ((db, e), (d, np.array([1.0, bad, 1.0, 1.0]))):
                try:
                    fn(dd, ee, target=tg)
                except Exception as ex:
                    assert "NaN or Inf" in str(ex), str(ex)
                else:
                    raise AssertionError(f"{fn.__name__} accepted a non-finite entry")
    try:
        s.stebz(d, e, range="some", target=tg)
    except ValueError:
        pass
    else:
        raise AssertionError("range='some' accepted")


# ---------------------------------------------------------------- 4. bdsbz
def check_bdsbz_random(n, dt, tg):
    d, e, ref = random_bi(n, np.dtype(dt).name)
    sv = s.bdsbz(d, e, target=tg)
    assert sv.dtype == dt and sv.shape == (n,)
    err, b = np.abs(sv - ref).max(), bound_vs_numpy(dt, ref, d, e)
    print(f"bdsbz random {np.dtype(dt).name} n {n} {tg}: err {err:.3e} bound {b:.3e}")
    assert err <= b
    assert np.all(np.diff(sv) <= 0) and np.all(sv >= 0)
    assert s.ops.stebz_stats()["n"] == 2 * n and s.ops.stebz_stats()["values"] == n
    # only squares and moduli of the entries are used
    rng = np.random.default_rng(n)
    sd = np.where(rng.random(n) < 0.5, -1, 1).astype(dt)
    se = np.where(rng.random(max(n - 1, 0)) < 0.5, -1, 1).astype(dt)
    assert np.array_equal(s.bdsbz(d * sd, e * se, target=tg), sv)
    # index ranges count from the largest
    if n >= 70:
        for il, iu in ((1, 1), (n, n), (3, n - 2), (60, 70)):
            assert np.array_equal(s.bdsbz(d, e, range="index", il=il, iu=iu, target=tg), sv[il - 1:iu]), (il, iu)
        vl, vu = np.sort(clear_shifts(ref, tmax(d, e), dt, 2, 13 * n + 1))
        sel = (ref >= vl) & (ref < vu)
        assert np.array_equal(s.bdsbz(d, e, range="value", vl=vl, vu=vu, target=tg), sv[sel])
        assert np.array_equal(s.bdsbz(d, e, range="value", vl=-1.0, vu=1e6, target=tg), sv)


def check_bdsbz_ones(n, tg):
    sv = s.bdsbz(np.ones(n), np.ones(n - 1), target=tg)
    k = np.arange(1, n + 1)
    ref = 2 * np.cos(k * np.pi / (2 * n + 1))
    rel = (np.abs(sv - ref) / ref).max()
    print(f"bdsbz d = e = 1 n {n} {tg}: rel err {rel:.3e} bound {4 * (2 * n - 1) * eps(np.float64):.3e}")
    assert rel <= 4 * (2 * n - 1) * eps(np.float64)
    assert np.abs(sv - ref).max() <= 16 * eps(np.float64)


def check_bdsbz_zero_entry(tg):
    """One exact zero d_k: B is singular; the smallest value comes back at or
    below the floor sqrt(safe_min) max|B| and the call finishes."""
    d, e, _ = random_bi(65, "float64")
    d = d.copy()
    d[30] = 0.0
    ref = np.linalg.svd(dense_bi(d, e), compute_uv=False)
    sv = s.bdsbz(d, e, target=tg)
    floor = np.sqrt(np.finfo(np.float64).tiny) * tmax(d, e)
    assert 0 <= sv[-1] <= floor, sv[-1]
    assert np.abs(sv - ref).max() <= 1e-10 * ref.max()


def check_bdsbz_graded(tg):
    """float32, n = 65, d_i = 10^(-8 i / (n - 1)), e_i = d_i / 2: EVERY value
    relatively within 4 (2n - 1) eps32 = 3e-5 of the float64 reference (whose
    own relative error on the smallest value is about 1e-8).  A method with
    absolute accuracy only is off by O(1) on the small ones."""
    n = 65
    d = (10.0 ** (-8.0 * np.arange(n) / (n - 1))).astype(np.float32)
    e = (d[:-1] / 2).astype(np.float32)
    ref = np.linalg.svd(dense_bi(d, e), compute_uv=False)
    sv = s.bdsbz(d, e, target=tg)
    rel = (np.abs(sv.astype(np.float64) - ref) / ref).max()
    print(f"bdsbz graded float32 {tg}: rel err {rel:.3e} = {rel / eps(np.float32):.2f} eps32")
    assert sv.dtype == np.float32
    assert rel <= 4 * (2 * n - 1) * eps(np.float32)


# ---------------------------------------------------------------- 5. drivers
def drv_tol(dt):
    return 1e-3 if dt == np.float32 else 1e-10   # test_hetrd.py / test_gebrd.py


def sym(n, dt, seed):
    a = s.utils.random_matrix(n, n, seed=seed, dtype=dt)
    return ((a + a.T) / 2).astype(dt)


def check_heev_bisection(n, dt, tg):
    a = sym(n, dt, n + 1)

    def vals(**kw):
        A = s.from_numpy(a.copy(), nb=64, target=tg)
        return np.asarray(s.heev(s.HermitianMatrix(s.Uplo.Lower, A), None, target=tg, **kw))

    w0 = vals()
    assert np.array_equal(vals(method_eig="dc"), w0)          # the default path is untouched
    for mh in ("two_stage", "one_stage"):
        w = vals(method_eig="bisection", method_hetrd=mh)
        st = s.ops.stebz_stats()
        assert st["values"] == n and st["n"] == n
        assert np.abs(w - w0).max() <= drv_tol(dt) * np.abs(w0).max(), mh
    A = s.from_numpy(a.copy(), nb=64, target=tg)
    Z = s.from_numpy(np.zeros((n, n), dt), nb=64, target=tg)
    try:
        s.heev(s.HermitianMatrix(s.Uplo.Lower, A), Z, target=tg, method_eig="bisection")
    except Exception as ex:
        assert "values only" in str(ex) and "inverse iteration" in str(ex), str(ex)
    else:
        raise AssertionError("vectors with bisection accepted")


def check_svd_vals_bisection(n, dt, tg):
    a = s.utils.random_matrix(n + 7, n, seed=n + 2, dtype=dt)

    def vals(**kw):
        return np.asarray(s.svd_vals(s.from_numpy(a.copy(), nb=64, target=tg), target=tg, **kw))

    s0 = vals()
    assert np.array_equal(vals(method_svd="qr"), s0)
    for mg in ("two_stage", "one_stage"):
        sv = vals(method_svd="bisection", method_gebrd=mg)
        st = s.ops.stebz_stats()
        assert st["values"] == n and st["n"] == 2 * n
        assert np.abs(sv - s0).max() <= drv_tol(dt) * s0.max(), mg
        assert np.all(np.diff(sv) <= 0)
    U = s.from_numpy(np.zeros((n + 7, n), dt), nb=64, target=tg)
    try:
        s.svd(s.from_numpy(a.copy(), nb=64, target=tg), U, None, target=tg, method_svd="bisection")
    except Exception as ex:
        assert "values only" in str(ex), str(ex)
    else:
        raise AssertionError("vectors with bisection accepted")
    try:
        vals(method_svd="jacobi")
    except Exception as ex:
        assert "method_svd" in str(ex)
    else:
        raise AssertionError("unknown method_svd accepted")


def check_sygv_bisection(tg):
    n = 130
    a = sym(n, np.float64, 14)
    b = sym(n, np.float64, 15)
    b = b @ b.T / n + np.eye(n)
    li = np.linalg.inv(np.linalg.cholesky(b))
    ref = np.linalg.eigvalsh(li @ a @ li.T)
    A = s.SymmetricMatrix(s.Uplo.Lower, s.from_numpy(a.copy(), nb=64, target=tg))
    B = s.SymmetricMatrix(s.Uplo.Lower, s.from_numpy(b.copy(), nb=64, target=tg))
    w = np.asarray(s.sygv(1, A, B, None, target=tg, method_eig="bisection"))
    assert s.ops.stebz_stats()["values"] == n
    assert np.abs(w - ref).max() <= drv_tol(np.float64) * np.abs(ref).max()
