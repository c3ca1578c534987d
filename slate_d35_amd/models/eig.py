"""Eigenvalue / SVD drivers (reference src/heev.cc, hegv.cc, hegst.cc,
he2hb.cc, hb2st.cc, sterf.cc, steqr2.cc, stedc*.cc, svd.cc, ge2tb.cc,
tb2bd.cc, bdsqr.cc)."""
from ._wrap import call

__all__ = ["heev", "hegv", "hegst", "svd", "svd_vals", "gesvd", "eig", "eig_vals", "he2hb", "hb2st", "sterf",
           "steqr", "stedc", "ge2tb", "tb2bd", "bdsqr", "syev", "sygv", "hb2st_band", "unmtr_hb2st",
           "unmtr_he2hb", "tb2bd_band", "unmbr_tb2bd", "unmbr_ge2tb", "steqr2", "stedc_matrix", "bdsqr_matrix",
           "bdsdc", "bdsdc_matrix", "hetrd", "unmtr_hetrd", "gebrd", "unmbr_gebrd", "stebz", "bdsbz",
           "stein", "heevx", "syevx"]


def heev(A, Z=None, target=None, **kw):
    """Eigenvalues (ascending numpy array; vectors into Z if given) of a
    Hermitian matrix.  method_eig="dc" (divide and conquer, default) or "qr";
    "bisection" (values only, Z None): stebz in place of sterf."""
    import numpy as np
    return np.asarray(call("heev", A, A, Z, target=target, **kw))


def hegv(itype, A, B, Z=None, target=None, **kw):
    """Generalized Hermitian-definite eigenproblem (itype 1: A x = l B x,
    2: A B x = l x, 3: B A x = l x).  B is overwritten by its Cholesky factor."""
    import numpy as np
    return np.asarray(call("hegv", A, itype, A, B, Z, target=target, **kw))


def hegst(itype, A, B, target=None, **kw):
    return call("hegst", A, itype, A, B, target=target, **kw)


def svd(A, U=None, VT=None, target=None, **kw):
    """Singular values (descending numpy array); thin U (m x k) and VT
    (k x n), k = min(m, n), filled when given.  method_svd="qr" (bidiagonal
    QR iteration, default) or "dc" (divide and conquer, bdsdc); "bisection"
    (values only, U and VT None): bdsbz in place of the QR iteration.
    method_gebrd="two_stage" (ge2tb + tb2bd, default) or "one_stage" (gebrd:
    real types, one process), also for svd_vals and gesvd."""
    import numpy as np
    return np.asarray(call("svd", A, A, U, VT, target=target, **kw))


def svd_vals(A, target=None, **kw):
    return svd(A, None, None, target=target, **kw)


def eig(A, Z, **kw):
    return heev(A, Z, **kw)


def eig_vals(A, **kw):
    return heev(A, None, **kw)


def he2hb(A, target=None, **kw):
    return call("he2hb", A, A, target=target, **kw)


def hb2st(a, kd):
    """Band (dense numpy, Hermitian, bandwidth kd) -> (d, e) of the tridiagonal."""
    import numpy as np
    from .._core import native
    return native("hb2st", np.asarray(a).dtype)(np.asarray(a), kd)


def sterf(d, e, **kw):
    from .. import _slate
    return _slate.sterf(list(d), list(e))


def _range(range, vl, vu, il, iu):
    """(Range, vl, vu, il, iu) of the range arguments of stebz / bdsbz / heevx."""
    from .._core import Range
    if not isinstance(range, Range):
        try:
            range = {"all": Range.All, "a": Range.All, "value": Range.Value, "v": Range.Value,
                     "index": Range.Index, "i": Range.Index}[str(range).lower()]
        except KeyError:
            raise ValueError(f"range: \"all\", \"value\" or \"index\", not {range!r}") from None
    if range == Range.Value and (vl is None or vu is None):
        raise ValueError("range=\"value\" needs vl and vu")
    if range == Range.Index and (il is None or iu is None):
        raise ValueError("range=\"index\" needs il and iu")
    return (range, float(0 if vl is None else vl), float(0 if vu is None else vu),
            int(0 if il is None else il), int(0 if iu is None else iu))


def _bisect(bidiagonal, d, e, range, vl, vu, il, iu, target, kw):
    import numpy as np
    from .. import _slate
    from .._core import opts
    d = np.asarray(d)
    e = np.asarray(e)
    dt = np.result_type(d.dtype, e.dtype) if e.size else d.dtype
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        dt = np.dtype(np.float64)
    range, vl, vu, il, iu = _range(range, vl, vu, il, iu)
    return _slate.stebz("s" if dt == np.float32 else "d", bidiagonal, range,
                        vl, vu, il, iu, d.astype(np.float64).tolist(), e.astype(np.float64).tolist(), opts(target, **kw))


def stebz(d, e, range="all", vl=None, vu=None, il=None, iu=None, target=None, **kw):
    """Eigenvalues (ascending ndarray of d's precision) of the symmetric
    tridiagonal (d, e) by Sturm-count bisection.  range="all"; "index": the
    1-based il <= k <= iu of the ascending order; "value": those in [vl, vu).
    A subset has the bits of the same entries of the full result.  target="d"
    runs the gfx950 kernel (one launch, one host synchronisation), the host
    targets the same arithmetic with OpenMP across eigenvalues.  float32 and
    float64.  Raises on non-finite entries, vl >= vu or il / iu out of range."""
    return _bisect(False, d, e, range, vl, vu, il, iu, target, kw)


def bdsbz(d, e, range="all", vl=None, vu=None, il=None, iu=None, target=None, **kw):
    """Singular values (descending ndarray) of the upper bidiagonal (d, e) by
    bisection on its Golub-Kahan tridiagonal: high relative accuracy down to
    sqrt(safe_min) max|B|.  "index" counts from the largest (il = 1); the
    signs of d and e do not matter.  Arguments as for stebz."""
    return _bisect(True, d, e, range, vl, vu, il, iu, target, kw)


def stein(d, e, w, target=None, **kw):
    """Unit eigenvectors (ndarray n x m of d's precision, one column per
    value) of the symmetric tridiagonal (d, e) for the m ascending eigenvalues
    w, as stebz returns them, by inverse iteration: five rounds, clusters
    (values closer than 1e-3 |T|_1) orthonormalised after each.  target="d"
    runs the gfx950 kernels (launches that depend on n, m and the existence of
    a cluster only, one host synchronisation, reproducible bits), the host
    targets the same arithmetic with OpenMP.  ops.stein_stats() has the
    counters, among them `failed`.  Raises on non-finite entries, a w that is
    not ascending or more values than rows."""
    import numpy as np
    from .. import _slate
    from .._core import opts
    d = np.asarray(d)
    e = np.asarray(e)
    dt = np.result_type(d.dtype, e.dtype) if e.size else d.dtype
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        dt = np.dtype(np.float64)
    z, _ = _slate.stein("s" if dt == np.float32 else "d", d.astype(np.float64).tolist(),
                        e.astype(np.float64).tolist(), np.asarray(w, np.float64).tolist(), opts(target, **kw))
    return z


def heevx(A, Z=None, range="all", vl=None, vu=None, il=None, iu=None, target=None, **kw):
    """Eigenvalues of a range (ascending numpy array of m values; the range
    arguments of stebz) of a Hermitian matrix and, when Z is given (n rows, at
    least m columns), their eigenvectors in its first m columns, the others
    zero: the reduction of method_hetrd ("two_stage", default, or "one_stage",
    real types), stebz, stein, and the back-transforms on m columns only.  A
    is not modified.  One process, one device."""
    import numpy as np
    return np.asarray(call("heevx", A, A, Z, *_range(range, vl, vu, il, iu), target=target, **kw))


def syevx(A, Z=None, range="all", vl=None, vu=None, il=None, iu=None, target=None, **kw):
    """heevx for a real SymmetricMatrix (a HermitianMatrix is accepted too)."""
    import numpy as np
    name = "syevx" if type(A).__name__.startswith("SymmetricMatrix") else "heevx"
    return np.asarray(call(name, A, A, Z, *_range(range, vl, vu, il, iu), target=target, **kw))


def steqr(d, e, Z=None, **kw):
    from .. import _slate
    return _slate.steqr(list(d), list(e), Z is not None)


def stedc(d, e, **kw):
    from .. import _slate
    return _slate.stedc(list(d), list(e))


def ge2tb(A, target=None, **kw):
    return call("ge2tb", A, A, target=target, **kw)


def tb2bd(a, kd):
    """Upper band (dense numpy, bandwidth kd) -> (d, e) of the bidiagonal."""
    import numpy as np
    from .._core import native
    return native("tb2bd", np.asarray(a).dtype)(np.asarray(a), kd)


def bdsqr(d, e, **kw):
    from .. import _slate
    return _slate.bdsqr(list(d), list(e))


def gesvd(A, U=None, VT=None, target=None, **kw):
    """Compatibility name of svd (reference slate.hh gesvd)."""
    return svd(A, U, VT, target=target, **kw)


def syev(A, Z=None, target=None, **kw):
    """Real symmetric eigenproblem (A a SymmetricMatrix of a real type)."""
    import numpy as np
    return np.asarray(call("syev", A, A, Z, target=target, **kw))


def sygv(itype, A, B, Z=None, target=None, **kw):
    import numpy as np
    return np.asarray(call("sygv", A, itype, A, B, Z, target=target, **kw))


# ---- stage-level API on distributed matrices (reference slate.hh:1050-1334)
def hb2st_band(A, target=None, **kw):
    """HermitianBandMatrix -> (d, e, V): the real tridiagonal and the
    bulge-chasing reflectors (apply with unmtr_hb2st)."""
    return call("hb2st_band", A, A, target=target, **kw)


def unmtr_hb2st(side, op, V, C, target=None, **kw):
    return call("unmtr_hb2st", C, side, op, V, C, target=target, **kw)


def unmtr_he2hb(side, op, A, Ts, C, target=None, **kw):
    return call("unmtr_he2hb", C, side, op, A, Ts, C, target=target, **kw)


def tb2bd_band(A, target=None, **kw):
    """Upper TriangularBandMatrix -> (d, e, U, V) of A = U B V^H."""
    return call("tb2bd_band", A, A, target=target, **kw)


def unmbr_tb2bd(side, op, V, C, target=None, **kw):
    return call("unmbr_tb2bd", C, side, op, V, C, target=target, **kw)


def unmbr_ge2tb(side, op, A, Ts, C, target=None, **kw):
    return call("unmbr_ge2tb", C, side, op, A, Ts, C, target=target, **kw)


def steqr2(jobz, d, e, Z, target=None, **kw):
    """Tridiagonal QL with Z := Z * eigenvectors (jobz = Job.Vec)."""
    import numpy as np
    return np.asarray(call("steqr2", Z, jobz, list(d), list(e), Z, target=target, **kw))


def stedc_matrix(d, e, Q, target=None, **kw):
    """Tridiagonal divide and conquer into a distributed Q."""
    import numpy as np
    return np.asarray(call("stedc_mat", Q, list(d), list(e), Q, target=target, **kw))


def bdsqr_matrix(jobu, jobvt, d, e, U=None, VT=None, target=None, **kw):
    import numpy as np
    key = U if U is not None else VT
    return np.asarray(call("bdsqr_mat", key, jobu, jobvt, list(d), list(e), U, VT, target=target, **kw))


def bdsdc(d, e, **kw):
    """Bidiagonal divide and conquer on the host: (sv, u, vt) like bdsqr."""
    from .. import _slate
    return _slate.bdsdc(list(d), list(e))


def bdsdc_matrix(jobu, jobvt, d, e, U=None, VT=None, target=None, **kw):
    """Bidiagonal divide and conquer on distributed matrices, the contract of
    bdsqr_matrix: U := U U_B, VT := V_B^T VT, singular values returned."""
    import numpy as np
    key = U if U is not None else VT
    return np.asarray(call("bdsdc_mat", key, jobu, jobvt, list(d), list(e), U, VT, target=target, **kw))


def hetrd(A, target=None, **kw):
    """One-stage tridiagonal reduction of the lower triangle of a real
    symmetric / Hermitian matrix of one process: returns (d, e, T) with
    A = Q tridiag(d, e) Q^T, e signed; the reflectors stay in A, T holds the
    block-reflector factors for unmtr_hetrd."""
    import numpy as np
    d, e, T = call("hetrd", A, A, target=target, **kw)
    return np.asarray(d), np.asarray(e), T


def unmtr_hetrd(side, op, A, T, C, target=None, **kw):
    """C := op(Q) C (Side.Left) or C op(Q) (Side.Right) with Q from hetrd(A)."""
    return call("unmtr_hetrd", C, side, op, A, T, C, target=target, **kw)


def gebrd(A, target=None, **kw):
    """One-stage bidiagonal reduction of a real m x n matrix of one process,
    m >= n: returns (d, e, TQ, TP) with A = Q B P^T, B upper bidiagonal with
    diagonal d and superdiagonal e; the reflectors stay in A, TQ and TP hold
    the block-reflector factors for unmbr_gebrd."""
    import numpy as np
    d, e, TQ, TP = call("gebrd", A, A, target=target, **kw)
    return np.asarray(d), np.asarray(e), TQ, TP


def unmbr_gebrd(vect, side, op, A, T, C, target=None, **kw):
    """C := op(F) C (Side.Left) or C op(F) (Side.Right) with F = Q ("q", T =
    TQ) or F = P ("p", T = TP) from gebrd(A)."""
    from .._core import Vect
    if isinstance(vect, str):
        vect = {"q": Vect.Q, "p": Vect.P}[vect.lower()]
    return call("unmbr_gebrd", C, vect, side, op, A, T, C, target=target, **kw)
