"""QR / LQ / least squares (reference src/geqrf.cc, unmqr.cc, gelqf.cc,
unmlq.cc, gels*.cc, cholqr.cc)."""
from .._core import suffix_of
from ._wrap import call

__all__ = ["geqrf", "unmqr", "gelqf", "unmlq", "gels", "cholqr", "qr_factor", "qr_multiply_by_q",
           "lq_factor", "lq_multiply_by_q", "least_squares_solve", "gels_qr", "gels_cholqr",
           "geqp3", "unmqr_geqp3", "gelsy"]


def geqrf(A, target=None, **kw):
    """Householder QR; returns the T factors (list of matrices)."""
    return call("geqrf", A, A, target=target, **kw)


def unmqr(side, op, A, T, C, target=None, **kw):
    call("unmqr", A, side, op, A, T, C, target=target, **kw)


def gelqf(A, target=None, **kw):
    return call("gelqf", A, A, target=target, **kw)


def unmlq(side, op, A, T, C, target=None, **kw):
    call("unmlq", A, side, op, A, T, C, target=target, **kw)


def gels(A, BX, target=None, **kw):
    return call("gels", A, A, BX, target=target, **kw)


def cholqr(A, R, target=None, **kw):
    return call("cholqr", A, A, R, target=target, **kw)


def gels_qr(A, BX, target=None, **kw):
    return call("gels_qr", A, A, BX, target=target, **kw)


def gels_cholqr(A, R, BX, target=None, **kw):
    """Least squares via CholeskyQR (m >= n): A := Q, R (n x n) upper."""
    return call("gels_cholqr", A, A, R, BX, target=target, **kw)


def geqp3(A, target=None, **kw):
    """QR with column pivoting of a real m x n matrix of one process: returns
    (jpvt, T) with A P = Q R and |R_kk| non-increasing; jpvt is a 0-based int64
    array, column j of A P being column jpvt[j] of the input; R and the
    reflectors stay in A as geqrf leaves them, T holds the block-reflector
    factors for unmqr_geqp3."""
    import numpy as np
    jpvt, T = call("geqp3", A, A, target=target, **kw)
    return np.asarray(jpvt, dtype=np.int64), T


def unmqr_geqp3(side, op, A, T, C, target=None, **kw):
    """C := op(Q) C (Side.Left) or C op(Q) (Side.Right) with Q from geqp3(A)."""
    return call("unmqr_geqp3", C, side, op, A, T, C, target=target, **kw)


def gelsy(A, BX, rcond=None, target=None, **kw):
    """Minimum-norm least-squares solution for the numerical rank r = the number
    of leading k with |R_kk| > rcond |R_00| of the pivoted QR of A (the plain
    diagonal rule, not LAPACK's incremental condition estimate).  BX is
    max(m, n) x nrhs with B in its first m rows; its first n rows receive X.
    Returns r.  The default rcond is eps of the type times max(m, n)."""
    import numpy as np
    if rcond is None:
        single = suffix_of(A) in ("s", "c")
        rcond = float(np.finfo(np.float32 if single else np.float64).eps) * max(A.m, A.n, 1)
    return call("gelsy", A, A, BX, float(rcond), target=target, **kw)


qr_factor = geqrf
qr_multiply_by_q = unmqr
lq_factor = gelqf
lq_multiply_by_q = unmlq
least_squares_solve = gels
