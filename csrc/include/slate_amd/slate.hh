// Public C++ API (reference include/slate/slate.hh:43-1410).
//
// Traditional BLAS/LAPACK-named drivers taking distributed matrices and an
// Options map.  Option::Target selects Host (C++/OpenMP tile kernels) or
// Devices (gfx950 HIP kernels on this process's GPU).  Every driver is
// collective over the matrices' process grid.
#pragma once

#include "enums.hh"
#include "types.hh"
#include "exception.hh"
#include "util.hh"
#include "device.hh"
#include "comm.hh"
#include "grid.hh"
#include "matrix.hh"
#include "inproc.hh"
#include "func.hh"
#include "method.hh"
#include "matgen.hh"
#include "init.hh"
#include "eig_host.hh"
#include "debug.hh"

#include <vector>

namespace slate {

/// T factors of a QR/LQ factorization: T[0] holds one nb x nb block per
/// panel (block column k -> columns [k*nb, (k+1)*nb) of an nb x n matrix
/// replicated on the panel's process column).
template <typename T>
using TriangularFactors = std::vector<Matrix<T>>;

//------------------------------------------------------------------------------
// Level-3 BLAS
template <typename T>
void gemm(T alpha, Matrix<T> const& A, Matrix<T> const& B, T beta, Matrix<T>& C, Options const& opts = {});
template <typename T>
void gemmA(T alpha, Matrix<T> const& A, Matrix<T> const& B, T beta, Matrix<T>& C, Options const& opts = {});
template <typename T>
void gemmC(T alpha, Matrix<T> const& A, Matrix<T> const& B, T beta, Matrix<T>& C, Options const& opts = {});

template <typename T>
void hemm(Side side, T alpha, HermitianMatrix<T> const& A, Matrix<T> const& B, T beta, Matrix<T>& C,
          Options const& opts = {});
template <typename T>
void symm(Side side, T alpha, SymmetricMatrix<T> const& A, Matrix<T> const& B, T beta, Matrix<T>& C,
          Options const& opts = {});
template <typename T>
void herk(real_type<T> alpha, Matrix<T> const& A, real_type<T> beta, HermitianMatrix<T>& C, Options const& opts = {});
template <typename T>
void syrk(T alpha, Matrix<T> const& A, T beta, SymmetricMatrix<T>& C, Options const& opts = {});
template <typename T>
void her2k(T alpha, Matrix<T> const& A, Matrix<T> const& B, real_type<T> beta, HermitianMatrix<T>& C,
           Options const& opts = {});
template <typename T>
void syr2k(T alpha, Matrix<T> const& A, Matrix<T> const& B, T beta, SymmetricMatrix<T>& C, Options const& opts = {});
template <typename T>
void trmm(Side side, T alpha, TriangularMatrix<T> const& A, Matrix<T>& B, Options const& opts = {});
template <typename T>
void trsm(Side side, T alpha, TriangularMatrix<T> const& A, Matrix<T>& B, Options const& opts = {});

/// Method-specific entry points (reference slate.hh hemmA / hemmC / trsmA /
/// trsmB): the generic driver with the method option fixed.
template <typename T>
inline void hemmA(Side side, T alpha, HermitianMatrix<T> const& A, Matrix<T> const& B, T beta, Matrix<T>& C,
                  Options const& opts = {}) {
    Options o = opts;
    o[Option::MethodHemm] = int64_t(MethodHemm::HemmA);
    hemm(side, alpha, A, B, beta, C, o);
}
template <typename T>
inline void hemmC(Side side, T alpha, HermitianMatrix<T> const& A, Matrix<T> const& B, T beta, Matrix<T>& C,
                  Options const& opts = {}) {
    Options o = opts;
    o[Option::MethodHemm] = int64_t(MethodHemm::HemmC);
    hemm(side, alpha, A, B, beta, C, o);
}
template <typename T>
inline void trsmA(Side side, T alpha, TriangularMatrix<T> const& A, Matrix<T>& B, Options const& opts = {}) {
    Options o = opts;
    o[Option::MethodTrsm] = int64_t(MethodTrsm::TrsmA);
    trsm(side, alpha, A, B, o);
}
template <typename T>
inline void trsmB(Side side, T alpha, TriangularMatrix<T> const& A, Matrix<T>& B, Options const& opts = {}) {
    Options o = opts;
    o[Option::MethodTrsm] = int64_t(MethodTrsm::TrsmB);
    trsm(side, alpha, A, B, o);
}

//------------------------------------------------------------------------------
// Auxiliary
template <typename T>
void add(T alpha, Matrix<T> const& A, T beta, Matrix<T>& B, Options const& opts = {});
template <typename T>
void add(T alpha, BaseTrapezoidMatrix<T> const& A, T beta, BaseTrapezoidMatrix<T>& B, Options const& opts = {});
template <typename Ts, typename Td>
void copy(BaseMatrix<Ts> const& A, BaseMatrix<Td>& B, Options const& opts = {});
template <typename T>
void scale(real_type<T> numer, real_type<T> denom, BaseMatrix<T>& A, Options const& opts = {});
template <typename T>
void scale_row_col(Equed equed, std::vector<real_type<T>> const& R, std::vector<real_type<T>> const& C,
                   Matrix<T>& A, Options const& opts = {});
template <typename T>
void set(T offdiag, T diag, BaseMatrix<T>& A, Options const& opts = {});
/// Set each element via a lambda of global indices (reference set_lambdas.cc).
template <typename T>
void set(std::function<T(int64_t, int64_t)> const& value, BaseMatrix<T>& A, Options const& opts = {});
/// Gather the whole matrix to every rank's host array (ld = m).
template <typename T>
void gather(BaseMatrix<T> const& A, std::vector<T>& full, Options const& opts = {});
/// B = A with any source/target distributions (reference redistribute.cc).
template <typename T>
void redistribute(Matrix<T> const& A, Matrix<T>& B, Options const& opts = {});

//------------------------------------------------------------------------------
// Norms (reference norm.cc, colNorms.cc)
template <typename T>
real_type<T> norm(Norm norm, BaseMatrix<T> const& A, Options const& opts = {});
template <typename T>
void colNorms(Norm norm, Matrix<T> const& A, real_type<T>* values, Options const& opts = {});

//------------------------------------------------------------------------------
// Cholesky
template <typename T>
int64_t potrf(HermitianMatrix<T>& A, Options const& opts = {});
template <typename T>
void potrs(HermitianMatrix<T> const& A, Matrix<T>& B, Options const& opts = {});
template <typename T>
int64_t posv(HermitianMatrix<T>& A, Matrix<T>& B, Options const& opts = {});
template <typename T>
int64_t potri(HermitianMatrix<T>& A, Options const& opts = {});
template <typename T>
int64_t posv_mixed(HermitianMatrix<T>& A, Matrix<T>& B, Matrix<T>& X, int& iter, Options const& opts = {});
template <typename T>
[[deprecated("Use posv_mixed")]] inline int64_t posvMixed(HermitianMatrix<T>& A, Matrix<T>& B, Matrix<T>& X, int& iter,
                                                         Options const& opts = {}) {
    return posv_mixed(A, B, X, iter, opts);
}
template <typename T>
int64_t posv_mixed_gmres(HermitianMatrix<T>& A, Matrix<T>& B, Matrix<T>& X, int& iter, Options const& opts = {});
template <typename T>
real_type<T> pocondest(Norm in_norm, HermitianMatrix<T>& A, real_type<T> Anorm, Options const& opts = {});

//------------------------------------------------------------------------------
// LU
template <typename T>
int64_t getrf(Matrix<T>& A, Pivots& pivots, Options const& opts = {});
template <typename T>
int64_t getrf_nopiv(Matrix<T>& A, Options const& opts = {});
template <typename T>
int64_t getrf_tntpiv(Matrix<T>& A, Pivots& pivots, Options const& opts = {});
/// Exact LU row-exchange counters of this process (diagnostics / tests):
/// elements sent and rows sent (summed over column ranges) since the reset.
void lu_rowx_stats(int64_t& elems, int64_t& rows);
void lu_rowx_reset();
template <typename T>
void getrs(Matrix<T> const& A, Pivots const& pivots, Matrix<T>& B, Options const& opts = {});
template <typename T>
void getrs_nopiv(Matrix<T> const& A, Matrix<T>& B, Options const& opts = {});
template <typename T>
int64_t gesv(Matrix<T>& A, Pivots& pivots, Matrix<T>& B, Options const& opts = {});
template <typename T>
int64_t gesv_nopiv(Matrix<T>& A, Matrix<T>& B, Options const& opts = {});
template <typename T>
int64_t gesv_mixed(Matrix<T>& A, Pivots& pivots, Matrix<T>& B, Matrix<T>& X, int& iter, Options const& opts = {});
/// (reference's older camel-case name)
template <typename T>
[[deprecated("Use gesv_mixed")]] inline int64_t gesvMixed(Matrix<T>& A, Pivots& pivots, Matrix<T>& B, Matrix<T>& X,
                                                         int& iter, Options const& opts = {}) {
    return gesv_mixed(A, pivots, B, X, iter, opts);
}
template <typename T>
int64_t gesv_mixed_gmres(Matrix<T>& A, Pivots& pivots, Matrix<T>& B, Matrix<T>& X, int& iter,
                         Options const& opts = {});
template <typename T>
int64_t getri(Matrix<T>& A, Pivots const& pivots, Options const& opts = {});
template <typename T>
real_type<T> gecondest(Norm in_norm, Matrix<T>& A, real_type<T> Anorm, Options const& opts = {});
template <typename T>
int64_t trtri(TriangularMatrix<T>& A, Options const& opts = {});
template <typename T>
void trtrm(TriangularMatrix<T>& A, Options const& opts = {});
template <typename T>
real_type<T> trcondest(Norm in_norm, TriangularMatrix<T>& A, Options const& opts = {});

//------------------------------------------------------------------------------
// QR / LQ / least squares
template <typename T>
void geqrf(Matrix<T>& A, TriangularFactors<T>& T_, Options const& opts = {});
template <typename T>
void unmqr(Side side, Op op, Matrix<T> const& A, TriangularFactors<T> const& T_, Matrix<T>& C,
           Options const& opts = {});
template <typename T>
void gelqf(Matrix<T>& A, TriangularFactors<T>& T_, Options const& opts = {});
template <typename T>
void unmlq(Side side, Op op, Matrix<T> const& A, TriangularFactors<T> const& T_, Matrix<T>& C,
           Options const& opts = {});
template <typename T>
void gels(Matrix<T>& A, TriangularFactors<T>& T_, Matrix<T>& BX, Options const& opts = {});
template <typename T>
int64_t cholqr(Matrix<T>& A, Matrix<T>& R, Options const& opts = {});

//------------------------------------------------------------------------------
// Eigenvalues / SVD (host-centric, reference heev.cc / svd.cc)
template <typename T>
void heev(HermitianMatrix<T>& A, std::vector<real_type<T>>& Lambda, Matrix<T>& Z, Options const& opts = {});
/// Eigenpairs of a subset: the eigenvalues of the range (the semantics of
/// stebz: Range::All, Range::Value [vl, vu), Range::Index 1 <= il <= iu <= n)
/// ascending in Lambda, sized to their number m, which is returned, and when
/// Z is wanted (n rows, at least m columns) their orthonormal eigenvectors in
/// its first m columns, the others zero.  The reduction that
/// Option::MethodHetrd selects, stebz on the tridiagonal, stein for the
/// vectors and the back-transforms of heev on the n x m block only.  A is not
/// modified.  A Z with fewer than m columns throws Exception naming m, with
/// Lambda already filled.  Real and complex types on the two-stage reduction,
/// real types on the one-stage one.  One process, one device, block-cyclic
/// operands: anything else throws NotImplemented.
template <typename T>
int64_t heevx(HermitianMatrix<T>& A, Range range, real_type<T> vl, real_type<T> vu, int64_t il, int64_t iu,
              std::vector<real_type<T>>& Lambda, Matrix<T>& Z, Options const& opts = {});
template <typename T>
void svd(Matrix<T>& A, std::vector<real_type<T>>& Sigma, Matrix<T>& U, Matrix<T>& VT, Options const& opts = {});
/// Stage 1 of heev: Hermitian (dense general storage) -> band of width nb.
template <typename T>
void he2hb(Matrix<T>& A, std::vector<TriangularFactors<T>>& Ts, Options const& opts = {});
/// Stage 1 of svd: general (m >= n) -> upper band of width nb.
template <typename T>
void ge2tb(Matrix<T>& A, std::vector<TriangularFactors<T>>& TU, std::vector<TriangularFactors<T>>& TV,
           Options const& opts = {});
template <typename T>
void hegst(int64_t itype, HermitianMatrix<T>& A, HermitianMatrix<T> const& B, Options const& opts = {});
template <typename T>
void hegv(int64_t itype, HermitianMatrix<T>& A, HermitianMatrix<T>& B, std::vector<real_type<T>>& Lambda,
          Matrix<T>& Z, Options const& opts = {});

//------------------------------------------------------------------------------
// Band (reference gbtrf.cc, gbtrs.cc, gbsv.cc, pbtrf.cc, pbtrs.cc, pbsv.cc,
// gbmm.cc, hbmm.cc, tbsm.cc)
template <typename T>
int64_t gbtrf(BandMatrix<T>& A, Pivots& pivots, Options const& opts = {});
template <typename T>
void gbtrs(BandMatrix<T> const& A, Pivots const& pivots, Matrix<T>& B, Options const& opts = {});
template <typename T>
int64_t gbsv(BandMatrix<T>& A, Pivots& pivots, Matrix<T>& B, Options const& opts = {});
template <typename T>
int64_t pbtrf(HermitianBandMatrix<T>& A, Options const& opts = {});
template <typename T>
void pbtrs(HermitianBandMatrix<T> const& A, Matrix<T>& B, Options const& opts = {});
template <typename T>
int64_t pbsv(HermitianBandMatrix<T>& A, Matrix<T>& B, Options const& opts = {});
template <typename T>
void gbmm(T alpha, BandMatrix<T> const& A, Matrix<T> const& B, T beta, Matrix<T>& C, Options const& opts = {});
template <typename T>
void hbmm(Side side, T alpha, HermitianBandMatrix<T> const& A, Matrix<T> const& B, T beta, Matrix<T>& C,
          Options const& opts = {});
template <typename T>
void tbsm(Side side, T alpha, TriangularBandMatrix<T> const& A, Matrix<T>& B, Options const& opts = {});
/// tbsm with gbtrf's row interchanges (reference slate.hh:305-310,
/// src/tbsmPivots.cc): the interchanges of tile k are applied to
/// B(k:mt-1, :) before tile k's solve on a forward sweep (op(A) lower, the L
/// of gbtrf) or after it on a backward sweep (op(A) upper); empty pivots =
/// plain tbsm.
template <typename T>
void tbsm(Side side, T alpha, TriangularBandMatrix<T> const& A, Pivots const& pivots, Matrix<T>& B,
          Options const& opts = {});

//------------------------------------------------------------------------------
// Hermitian indefinite (reference hetrf.cc, hetrs.cc, hesv.cc); LAPACK ipiv.
template <typename T>
int64_t hetrf(HermitianMatrix<T>& A, std::vector<int64_t>& ipiv, Options const& opts = {});
template <typename T>
void hetrs(HermitianMatrix<T> const& A, std::vector<int64_t> const& ipiv, Matrix<T>& B, Options const& opts = {});
template <typename T>
int64_t hesv(HermitianMatrix<T>& A, std::vector<int64_t>& ipiv, Matrix<T>& B, Options const& opts = {});
// Aasen (reference hetrf.cc signatures): P A P^T = L T L^H, T band (kl = ku = nb)
template <typename T>
int64_t hetrf(HermitianMatrix<T>& A, Pivots& pivots, BandMatrix<T>& T_, Pivots& pivots2, Matrix<T>& H,
              Options const& opts = {});
template <typename T>
void hetrs(HermitianMatrix<T>& A, Pivots& pivots, BandMatrix<T>& T_, Pivots& pivots2, Matrix<T>& B,
           Options const& opts = {});
template <typename T>
int64_t hesv(HermitianMatrix<T>& A, Pivots& pivots, BandMatrix<T>& T_, Pivots& pivots2, Matrix<T>& H, Matrix<T>& B,
             Options const& opts = {});

/// op(A) X = B with getrf factors (op = NoTrans, Trans, ConjTrans).
template <typename T>
void getrs(Op trans, Matrix<T> const& A, Pivots const& pivots, Matrix<T>& B, Options const& opts = {});
/// Out-of-place inverse from getrf factors (reference getriOOP.cc).
template <typename T>
int64_t getri(Matrix<T>& A, Pivots const& pivots, Matrix<T>& B, Options const& opts);
/// Random butterfly transform A := U^T A V and the RBT solver (gerbt.cc, gesv_rbt.cc).
template <typename T>
void gerbt(Matrix<T>& A, int depth, uint64_t seed_u, uint64_t seed_v, Options const& opts = {});
template <typename T>
int64_t gesv_rbt(Matrix<T>& A, Matrix<T>& B, Matrix<T>& X, int& iter, Options const& opts = {});

//------------------------------------------------------------------------------
// Two-stage reduction building blocks (reference slate.hh:1050-1334).
/// Householder reflectors of a bulge-chasing stage (hb2st / tb2bd) plus the
/// diagonal phase that makes the condensed form real; replicated on every
/// rank (the reference keeps them in a distributed Matrix V).
template <typename T>
struct BandReflectors {
    host::Reflectors<T> Q;
    std::vector<T> phase;
};

/// Band Hermitian -> real symmetric tridiagonal (D, E); A = Q T Q^H with
/// Q = V.Q diag(V.phase).
template <typename T>
void hb2st(HermitianBandMatrix<T>& A, std::vector<real_type<T>>& D, std::vector<real_type<T>>& E,
           BandReflectors<T>& V, Options const& opts = {});
/// C = op(Q) C (Side::Left) or C op(Q) (Side::Right) with Q from hb2st.
template <typename T>
void unmtr_hb2st(Side side, Op op, BandReflectors<T> const& V, Matrix<T>& C, Options const& opts = {});
/// C = op(Q1) C / C op(Q1) with Q1 the he2hb reflectors (stored below the band of A).
template <typename T>
void unmtr_he2hb(Side side, Op op, Matrix<T>& A, std::vector<TriangularFactors<T>>& Ts, Matrix<T>& C,
                 Options const& opts = {});
/// Upper triangular band -> real upper bidiagonal: A = U B V^H.
template <typename T>
void tb2bd(TriangularBandMatrix<T>& A, std::vector<real_type<T>>& D, std::vector<real_type<T>>& E,
           BandReflectors<T>& U, BandReflectors<T>& V, Options const& opts = {});
/// Apply the tb2bd reflectors U or V: C = op(Q) C or C op(Q).
template <typename T>
void unmbr_tb2bd(Side side, Op op, BandReflectors<T> const& V, Matrix<T>& C, Options const& opts = {});
/// Apply the ge2tb reflectors: Side::Left with the QR factors TU (C = op(U1) C),
/// Side::Right with the LQ factors TV (C = C op(V1^H)).
template <typename T>
void unmbr_ge2tb(Side side, Op op, Matrix<T>& A, std::vector<TriangularFactors<T>>& Ts, Matrix<T>& C,
                 Options const& opts = {});

/// Tridiagonal eigenvalues only (root-free QL).
template <typename R>
void sterf(std::vector<R>& D, std::vector<R>& E, Options const& opts = {});
/// Eigenvalues of the symmetric tridiagonal (D of n, E of n - 1) by Sturm-count
/// bisection (src/stebz.cc, slate_amd/sturm.hh), ascending in W, which is
/// sized to the number found.  Range::All: all n; Range::Index: the 1-based
/// il <= k <= iu of the ascending order; Range::Value: those with
/// N(vl) < k <= N(vu), N(x) the number of eigenvalues below x, i.e. [vl, vu)
/// up to rounding at the end points.  A subset has the bits of the same
/// entries of the full set.  Accuracy is absolute, a few eps max|T_ij|.
/// Target::Devices: one kernel launch on the calling context's device (two
/// for Range::Value) and one host synchronisation, the fetch of the result;
/// host targets: the same arithmetic with OpenMP across eigenvalues.  D and E
/// are replicated host vectors: on a grid every process computes all values
/// itself.  n = 0 and n = 1 are accepted; an all-zero matrix returns zeros
/// without a launch.  Throws Exception, before any launch, on a non-finite
/// entry, on vl >= vu (Value) or on il / iu outside 1 <= il <= iu <= n (Index).
template <typename R>
void stebz(Range range, R vl, R vu, int64_t il, int64_t iu, std::vector<R> const& D, std::vector<R> const& E,
           std::vector<R>& W, Options const& opts = {});
/// Singular values of the upper bidiagonal (D of n, E of n - 1) by the same
/// bisection on its Golub-Kahan tridiagonal of order 2n, DESCENDING in S as
/// svd returns them; Range::Index counts in that order (il = 1 is the
/// largest), Range::Value keeps the values in [vl, vu).  The signs of D and E
/// do not matter.  Accuracy is relative, about (2n - 1) eps, for values above
/// sqrt(safe_min) max|B_ij|; below that floor a value is the midpoint of its
/// last interval (absolute accuracy), which is what an exact zero singular
/// value returns.  Targets, limits and refusals as for stebz.
template <typename R>
void bdsbz(Range range, R vl, R vu, int64_t il, int64_t iu, std::vector<R> const& D, std::vector<R> const& E,
           std::vector<R>& S, Options const& opts = {});
/// N(x_j), the number of eigenvalues of tridiag(D, E) below x_j, per shift.
template <typename R>
std::vector<int64_t> sturm_count(std::vector<R> const& D, std::vector<R> const& E, std::vector<R> const& x,
                                 Options const& opts = {});
/// Counters of the last stebz / bdsbz of this process (also through heev /
/// svd with the Bisection methods): order of the tridiagonal counted (2n for
/// bdsbz), values returned, trial points per step P (1 on the host), the most
/// steps any value took, kernel launches and host synchronisations (both
/// zero on the host target).  P comes from n and the device's CU count;
/// SLATE_STEBZ_POINTS in the environment (1, 2, 4 .. 64) overrides it.
struct StebzStats {
    int64_t n = 0, values = 0, points = 0, steps = 0, launches = 0, host_syncs = 0;
};
StebzStats stebz_stats();
/// Eigenvectors of the symmetric tridiagonal (D of n, E of n - 1) that belong
/// to the m eigenvalues W, ascending as stebz returns them, by inverse
/// iteration (src/stein.cc, slate_amd/stein.hh): Z becomes the n x m
/// column-major matrix of unit vectors, one column per value, the entry of
/// largest modulus positive.  Values closer than 1e-3 |T|_1 form a cluster,
/// whose vectors are orthonormalised against each other (classical
/// Gram-Schmidt applied twice) after every round; there are exactly five
/// rounds (LAPACK's MAXITS).  A vector is accepted when it passes LAPACK's
/// growth test in three of them; returns the number that were not, their
/// 1-based indices in ifail (LAPACK's ifail).  Target::Devices: the launches
/// depend on n, m and the existence of a cluster only, one host
/// synchronisation, two calls give the same bits; host targets: the same
/// arithmetic with OpenMP across vectors and clusters.  n = 0 or m = 0
/// returns at once, n = 1 returns [1], an all-zero matrix the first m unit
/// vectors, all without a launch.  Throws Exception, before any launch, on a
/// non-finite entry of D, E or W, on a W that is not ascending and on m > n.
template <typename R>
int64_t stein(std::vector<R> const& D, std::vector<R> const& E, std::vector<R> const& W, std::vector<R>& Z,
              Options const& opts = {});
template <typename R>
int64_t stein(std::vector<R> const& D, std::vector<R> const& E, std::vector<R> const& W, std::vector<R>& Z,
              std::vector<int64_t>& ifail, Options const& opts = {});
/// Counters of the last stein of this process (also through heevx): order,
/// vectors, clusters and the size of the largest, rounds run, vectors not
/// accepted, kernel launches and host synchronisations (both zero on the host
/// target).  With SLATE_STEIN_PROFILE=1 in the environment, the milliseconds
/// of the device kernels by kind (events, no extra synchronisation).
struct SteinStats {
    int64_t n = 0, values = 0, clusters = 0, largest_cluster = 0, rounds = 0, failed = 0, launches = 0,
            host_syncs = 0;
    double ms_solve = 0, ms_orth = 0, ms_transpose = 0;
};
SteinStats stein_stats();
/// Tridiagonal QL/QR; with jobz = Vec, Z := Z * (eigenvectors).
template <typename T>
void steqr2(Job jobz, std::vector<real_type<T>>& D, std::vector<real_type<T>>& E, Matrix<T>& Z,
            Options const& opts = {});
/// Tridiagonal divide and conquer: eigenvalues ascending in D, vectors in Q.
template <typename R>
void stedc(std::vector<R>& D, std::vector<R>& E, Matrix<R>& Q, Options const& opts = {});
/// D&C stages (reference stedc_solve.cc, stedc_z_vector.cc, stedc_sort.cc,
/// stedc_deflate.cc, stedc_secular.cc, stedc_merge.cc).
template <typename R>
void stedc_solve(std::vector<R>& D, std::vector<R>& E, Matrix<R>& Q, Options const& opts = {});
template <typename R>
void stedc_z_vector(Matrix<R>& Q, int64_t n1, R sgn, std::vector<R>& z, Options const& opts = {});
template <typename R>
void stedc_sort(std::vector<R>& D, std::vector<R>& z, Matrix<R>& Q, Matrix<R>& Qout, std::vector<int64_t>& perm,
                Options const& opts = {});
template <typename R>
int64_t stedc_deflate(R rho, std::vector<R>& D, std::vector<R>& z, Matrix<R>& Q, std::vector<char>& deflated,
                      Options const& opts = {});
template <typename R>
void stedc_secular(R rho, std::vector<R> const& D, std::vector<R> const& z, std::vector<R>& Lambda, Matrix<R>& U,
                   Options const& opts = {});
template <typename R>
void stedc_merge(Matrix<R>& Q, Matrix<R>& U, Matrix<R>& Qout, Options const& opts = {});
/// Bidiagonal SVD: D descending singular values; U := U Ub, VT := Vb^H VT.
template <typename T>
void bdsqr(Job jobu, Job jobvt, std::vector<real_type<T>>& D, std::vector<real_type<T>>& E, Matrix<T>& U,
           Matrix<T>& VT, Options const& opts = {});
/// Bidiagonal SVD by divide and conquer (src/bdsdc.cc), the contract of bdsqr:
/// D descending singular values, U := U Ub, VT := Vb^T VT, E destroyed.  Every
/// process runs the whole divide and conquer on local arrays (about 4 n^2
/// reals, device memory on the device target).  Accuracy is absolute
/// (eps ||B||).  Without vectors it is the values-only QR iteration.
template <typename T>
void bdsdc(Job jobu, Job jobvt, std::vector<real_type<T>>& D, std::vector<real_type<T>>& E, Matrix<T>& U,
           Matrix<T>& VT, Options const& opts = {});
/// Counters of the last divide and conquer of this process (bdsdc, or svd
/// with MethodSVD::DC): merges, merged and deflated columns in all and per
/// tree level (0 = root), launches of the three device kernels.
struct BdsdcStats {
    int64_t merges = 0, columns = 0, deflated = 0;
    int64_t launches_secular = 0, launches_zhat = 0, launches_matrix = 0;
    std::vector<int64_t> level_columns, level_deflated;
};
BdsdcStats bdsdc_stats();

/// One-stage tridiagonal reduction (src/hetrd.cc; LAPACK sytrd): A = Q T Q^T
/// with T = tridiag(D, E), E signed.  Real types, Uplo::Lower, a matrix of one
/// process on one device or the host; anything else throws NotImplemented
/// (Uplo::Upper: Exception).  The reflectors stay in A below the subdiagonal;
/// T[0] holds the 64 x 64 block-reflector factor of every panel of 64 columns
/// (panel p at column 64 p), T[1] the scalars tau.  The strict upper triangle
/// of A is not read.
template <typename T>
void hetrd(HermitianMatrix<T>& A, std::vector<real_type<T>>& D, std::vector<real_type<T>>& E,
           TriangularFactors<T>& T_, Options const& opts = {});
/// C := op(Q) C (Side::Left) or C op(Q) (Side::Right), Q = H_0 H_1 .. H_{n-2}
/// from hetrd(A, ..., T), panel by panel.
template <typename T>
void unmtr_hetrd(Side side, Op op, HermitianMatrix<T>& A, TriangularFactors<T>& T_, Matrix<T>& C,
                 Options const& opts = {});
/// Counters of the last one-stage reduction of this process (hetrd, or heev
/// with MethodHetrd::OneStage): reduced columns, panels, launches of the four
/// column kernels (zero on the host target) and host synchronisations inside
/// the reduction.  With SLATE_HETRD_PROFILE=1 in the environment the device
/// reduction also records events between its kernels and reports the device
/// milliseconds of the symv launches, the other column kernels (panel), the
/// syr2k updates and the T factors; zero otherwise.
struct HetrdStats {
    int64_t columns = 0, panels = 0, host_syncs = 0;
    int64_t launches_column = 0, launches_larfg = 0, launches_symv = 0, launches_correct = 0;
    double ms_symv = 0, ms_panel = 0, ms_syr2k = 0, ms_larft = 0;
};
HetrdStats hetrd_stats();

/// Which factor of the bidiagonal reduction unmbr_gebrd applies (LAPACK ormbr's vect).
enum class Vect : char { Q = 'Q', P = 'P' };
/// One-stage bidiagonal reduction (src/gebrd.cc; LAPACK gebrd): A = Q B P^T
/// with B upper bidiagonal, diagonal D (n) and superdiagonal E (n - 1).  Real
/// types, m >= n, a matrix of one process on one device or the host; anything
/// else throws NotImplemented.  The left reflectors stay in A below the
/// diagonal, the right ones to the right of the superdiagonal, each with its
/// unit entry stored.  TQ[0] / TP[0] hold the 64 x 64 block-reflector factor
/// of every panel of 64 columns (panel p at column 64 p), TQ[1] / TP[1] the
/// scalars tauq / taup.  The entries of A are assumed to be such that their
/// squares neither overflow nor underflow (svd scales first).
template <typename T>
void gebrd(Matrix<T>& A, std::vector<real_type<T>>& D, std::vector<real_type<T>>& E, TriangularFactors<T>& TQ,
           TriangularFactors<T>& TP, Options const& opts = {});
/// C := op(F) C (Side::Left) or C op(F) (Side::Right), F = Q = H_0 .. H_{n-1}
/// (Vect::Q, order m, T = TQ) or F = P = G_0 .. G_{n-2} (Vect::P, order n,
/// T = TP) from gebrd(A, ...): LAPACK ormbr, one larfb per panel.
template <typename T>
void unmbr_gebrd(Vect vect, Side side, Op op, Matrix<T>& A, TriangularFactors<T>& T_, Matrix<T>& C,
                 Options const& opts = {});
/// Counters of the last one-stage bidiagonal reduction of this process (gebrd,
/// or svd with MethodGebrd::OneStage): reduced columns, panels, launches of the
/// seven column kernels (zero on the host target) and host synchronisations
/// inside the reduction.  With SLATE_GEBRD_PROFILE=1 in the environment the
/// device reduction also records events between its kernels and reports the
/// device milliseconds of pass 1 (A^T u), pass 2 (A v), the other column
/// kernels (panel), the trailing GEMMs and the T factors; zero otherwise.
struct GebrdStats {
    int64_t columns = 0, panels = 0, host_syncs = 0;
    int64_t launches_column = 0, launches_larfg_u = 0, launches_pass1 = 0, launches_finish_y = 0,
            launches_larfg_v = 0, launches_pass2 = 0, launches_finish_x = 0;
    double ms_pass1 = 0, ms_pass2 = 0, ms_panel = 0, ms_gemm = 0, ms_larft = 0;
};
GebrdStats gebrd_stats();

/// QR with column pivoting (src/geqp3.cc; LAPACK geqp3): A P = Q R with
/// |R_kk| non-increasing.  Real types, any m and n, a matrix of one process on
/// one device or the host; anything else throws NotImplemented.  R is left in
/// the upper triangle / trapezoid of A, the k = min(m, n) reflectors below the
/// diagonal with their unit entries implied, as geqrf leaves them.  jpvt gets
/// n entries, 0-based: column j of A P is column jpvt[j] of the input; all
/// columns are free and the entry value of jpvt is ignored.  T[0] holds the
/// 64 x 64 block-reflector factor of every panel of 64 columns (panel p at
/// column 64 p), T[1] the scalars tau.  The entries of A are assumed to be such
/// that their squares neither overflow nor underflow (gelsy scales first).
template <typename T>
void geqp3(Matrix<T>& A, std::vector<int64_t>& jpvt, TriangularFactors<T>& T_, Options const& opts = {});
/// C := op(Q) C (Side::Left) or C op(Q) (Side::Right), Q = H_0 .. H_{k-1} of
/// order m from geqp3(A, jpvt, T): one larfb per panel.
template <typename T>
void unmqr_geqp3(Side side, Op op, Matrix<T>& A, TriangularFactors<T>& T_, Matrix<T>& C, Options const& opts = {});
/// Minimum-norm least-squares solution for a numerical rank chosen by rcond
/// (LAPACK gelsy's contract with a simpler rank rule): geqp3, the rank r = the
/// number of leading k with |R_kk| > rcond |R_00| (the plain diagonal rule, not
/// LAPACK's incremental condition estimate), C = (Q^T B)(0:r), the minimum-norm
/// solution of [R11 R12] y = C by an LQ factorization of that row block, and
/// X = P y.  BX is max(m, n) x nrhs with B in its first m rows; on exit its
/// first n rows hold X.  A is overwritten by its factorization (scaled into
/// range first when its largest entry is tiny or huge).  r returns; r = 0
/// gives X = 0.  Operands as for geqp3.
template <typename T>
int64_t gelsy(Matrix<T>& A, Matrix<T>& BX, real_type<T> rcond, Options const& opts = {});
/// Counters of the last geqp3 of this process (also through gelsy): factored
/// columns, panels, launches of each kernel kind (zero on the host target),
/// the columns whose norm was recomputed inside a panel (counted on the device
/// and fetched with the final copy) and host synchronisations inside the
/// factorization.  With SLATE_GEQP3_PROFILE=1 in the environment the device
/// factorization also records events between its kernels and reports the
/// device milliseconds of the pivot search and swap, the product A^T v, the
/// other column kernels (panel), the trailing GEMMs and the T factors; zero
/// otherwise.
struct Geqp3Stats {
    int64_t columns = 0, panels = 0, host_syncs = 0, norm_recomputes = 0;
    int64_t launches_norms = 0, launches_pivot = 0, launches_swap = 0, launches_column = 0, launches_larfg = 0,
            launches_product = 0, launches_finish = 0, launches_recompute = 0;
    double ms_pivot = 0, ms_product = 0, ms_panel = 0, ms_gemm = 0, ms_larft = 0;
};
Geqp3Stats geqp3_stats();

//------------------------------------------------------------------------------
// Real-symmetric aliases (real types only) and compatibility names.
template <typename T>
void syev(SymmetricMatrix<T>& A, std::vector<real_type<T>>& Lambda, Matrix<T>& Z, Options const& opts = {});
/// syevx: heevx for a real SymmetricMatrix.
template <typename T>
int64_t syevx(SymmetricMatrix<T>& A, Range range, real_type<T> vl, real_type<T> vu, int64_t il, int64_t iu,
              std::vector<real_type<T>>& Lambda, Matrix<T>& Z, Options const& opts = {});
template <typename T>
void sygst(int64_t itype, SymmetricMatrix<T>& A, SymmetricMatrix<T> const& B, Options const& opts = {});
template <typename T>
void sygv(int64_t itype, SymmetricMatrix<T>& A, SymmetricMatrix<T>& B, std::vector<real_type<T>>& Lambda,
          Matrix<T>& Z, Options const& opts = {});
template <typename T>
int64_t sytrf(SymmetricMatrix<T>& A, std::vector<int64_t>& ipiv, Options const& opts = {});
template <typename T>
void sytrs(SymmetricMatrix<T> const& A, std::vector<int64_t> const& ipiv, Matrix<T>& B, Options const& opts = {});
template <typename T>
int64_t sysv(SymmetricMatrix<T>& A, std::vector<int64_t>& ipiv, Matrix<T>& B, Options const& opts = {});
template <typename T>
void svd_vals(Matrix<T>& A, std::vector<real_type<T>>& Sigma, Options const& opts = {});
template <typename T>
void gesvd(Matrix<T>& A, std::vector<real_type<T>>& Sigma, Matrix<T>& U, Matrix<T>& VT, Options const& opts = {});
template <typename T>
void gels_qr(Matrix<T>& A, TriangularFactors<T>& T_, Matrix<T>& BX, Options const& opts = {});
/// Least squares via CholeskyQR (m >= n): A := Q, R upper n x n.
template <typename T>
void gels_cholqr(Matrix<T>& A, Matrix<T>& R, Matrix<T>& BX, Options const& opts = {});

//------------------------------------------------------------------------------
// Printing (reference include/slate/print.hh).  Collective; rank 0 prints a
// MATLAB-style `label = [ ... ];` block.  Options PrintVerbose (0-4, default
// 2 = edges), PrintEdgeItems (16), PrintWidth (10), PrintPrecision (4).
template <typename T>
void print(const char* label, BaseMatrix<T> const& A, Options const& opts = {});
/// Vector x[0:n:incx] (rank 0 only).
template <typename T>
void print(const char* label, int64_t n, T const* x, int64_t incx = 1, Options const& opts = {});
/// What print() writes on rank 0, as a string (empty elsewhere).
template <typename T>
std::string print_to_string(const char* label, BaseMatrix<T> const& A, Options const& opts = {});
template <typename R>
int snprintf_value(char* buf, size_t len, int width, int precision, R value);

/// Wait for all device work of this process (drivers already synchronize).
void sync();

}  // namespace slate

#include "simplified_api.hh"
