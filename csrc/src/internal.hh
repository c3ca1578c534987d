// Driver-internal helpers: distribution math over a view, panel broadcasts
// and tile exchanges.  These replace the reference's listBcast / listReduce /
// tileSend / tileRecv (BaseMatrix.hh:1762-2456) with whole-panel collectives:
// one contiguous buffer per panel per communicator instead of one message
// per tile.
#pragma once

#include "slate_amd/slate.hh"
#include "slate_amd/runtime.hh"
#include "slate_amd/trace.hh"

#include <cmath>
#include <cstdlib>
#include <functional>
#include <limits>
#include <vector>

namespace slate {
namespace internal {
/// Working precision of the mixed-precision solvers' factorization.
template <typename T> struct lower_prec { using type = T; };
template <> struct lower_prec<double> { using type = float; };
template <> struct lower_prec<std::complex<double>> { using type = std::complex<float>; };

/// GMRES-IR continuation of a mixed-precision solve (gmres.cc): each column
/// of X (the current estimate) is refined by restarted GMRES on A x = b with
/// the low-precision factors as right preconditioner (solve_lo, in place on a
/// low-precision vector); residual(R, V) computes R -= A V.  Returns true when
/// every column met the classical stopping test; iters = the largest GMRES
/// iteration count over the columns.
template <typename T>
bool gmres_refine(Matrix<T>& B, Matrix<T>& X, real_type<T> Anorm, int itermax, int& iters,
                  std::function<void(Matrix<T>&, Matrix<T>&)> const& residual,
                  std::function<void(Matrix<typename lower_prec<T>::type>&)> const& solve_lo, Options const& opts);
}  // namespace internal

namespace internal {

/// Real trailing updates C -= X Y as NT products against a transposed copy of
/// Y (the 4-wave rotated MFMA tile, measured faster than the NN 8-wave tile
/// on large shapes); SLATE_UPDATE_NT=0 keeps the NN form.
inline bool update_nt() {
    static const bool v = [] {
        const char* e = std::getenv("SLATE_UPDATE_NT");
        return e ? std::atoi(e) != 0 : true;
    }();
    return v;
}

/// Local row offset within `A`'s local block for view row-tile index i (first
/// local row whose global index is >= start of tile i).
template <typename T>
inline int64_t lrow_of(BaseMatrix<T> const& A, int64_t i) {
    auto& s = *A.storage();
    int64_t g = (i < A.mt() ? std::max<int64_t>(0, (A.row0() / s.mb + i) * s.mb - A.row0()) : A.srows());
    return g2l_ceil(A.row0() + std::min(g, A.srows()), s.mb, s.rrel(), s.grid->p()) - A.lrow_begin();
}
template <typename T>
inline int64_t lcol_of(BaseMatrix<T> const& A, int64_t j) {
    auto& s = *A.storage();
    int64_t g = (j < A.nt() ? std::max<int64_t>(0, (A.col0() / s.nb + j) * s.nb - A.col0()) : A.scols());
    return g2l_ceil(A.col0() + std::min(g, A.scols()), s.nb, s.crel(), s.grid->q()) - A.lcol_begin();
}

/// Global row/col (within view) where tile i/j starts.
template <typename T>
inline int64_t grow_of(BaseMatrix<T> const& A, int64_t i) {
    auto& s = *A.storage();
    if (i >= A.mt()) return A.srows();
    return std::max<int64_t>(0, (A.row0() / s.mb + i) * s.mb - A.row0());
}
template <typename T>
inline int64_t gcol_of(BaseMatrix<T> const& A, int64_t j) {
    auto& s = *A.storage();
    if (j >= A.nt()) return A.scols();
    return std::max<int64_t>(0, (A.col0() / s.nb + j) * s.nb - A.col0());
}

/// Dense device/host buffer sized for panels.
template <typename T>
class Work {
public:
    Work() = default;
    Work(Target t, size_t n) { resize(t, n); }
    void resize(Target t, size_t n) {
        dev_ = (t == Target::Devices);
        if (n <= n_) return;
        release();
        n_ = std::max<size_t>(n, 1);
        if (dev_) p_ = static_cast<T*>(device::malloc(n_ * sizeof(T)));
        else { h_.assign(n_, T(0)); p_ = h_.data(); }
    }
    ~Work() { release(); }
    Work(Work&& o) noexcept { *this = std::move(o); }
    Work& operator=(Work&& o) noexcept {
        release();
        p_ = o.p_; n_ = o.n_; dev_ = o.dev_; h_ = std::move(o.h_);
        if (!dev_) p_ = h_.data();
        o.p_ = nullptr; o.n_ = 0;
        return *this;
    }
    T* data() const { return p_; }
    size_t size() const { return n_; }
private:
    void release() {
        if (dev_ && p_) device::free(p_);
        p_ = nullptr; n_ = 0; h_.clear();
    }
    T* p_ = nullptr;
    size_t n_ = 0;
    bool dev_ = false;
    std::vector<T> h_;
};

/// stein after the public wrappers (stein.cc): the unit eigenvectors of
/// tridiag(D, E) for the ascending values W into Z (n x m, column-major,
/// leading dimension ldz), which is host memory, or with z_on_device (target
/// Devices only) memory of the calling context's device, where heevx goes on
/// with it.  ifail: the 1-based indices of the vectors that were not accepted.
template <typename R>
void stein_core(std::vector<R> const& D, std::vector<R> const& E, std::vector<R> const& W, R* Z, int64_t ldz,
                bool z_on_device, std::vector<int64_t>& ifail, Options const& opts);

/// Location of a target.
inline Loc loc_of(Target t) { return t == Target::Devices ? Loc::Device : Loc::Host; }

/// Normalize a HostTask/HostNest/HostBatch/Host target; Devices requires a GPU.
inline Target resolve_target(Options const& opts) {
    Target t = get_target(opts, Target::HostTask);
    if (t == Target::Devices && !device::available())
        slate_error("Target::Devices requested but no HIP device is available");
    return t;
}

/// Option::GemmPrecision as a driver on scalar type T applies it: the value is
/// checked for every type and in effect for float only.
template <typename T>
inline GemmPrecision driver_gemm_precision(Options const& opts) {
    const GemmPrecision p = lb::gemm_precision_option(opts);
    return std::is_same_v<T, float> ? p : GemmPrecision::Native;
}
/// Mixed-precision drivers on working type T: the option goes to the fp32
/// factorization; a complex working type has no bf16 path to give it to.
template <typename T>
inline void check_mixed_gemm_precision(Options const& opts, char const* name) {
    if (lb::gemm_precision_option(opts) != GemmPrecision::Native && is_complex_v<T>)
        slate_not_implemented(std::string(name) + ": Option::GemmPrecision needs a real matrix type");
}

/// Driver nesting depth on this thread.  Option::HoldLocalWorkspace = false
/// (the default, reference src/potrf.cc:42,198) frees a matrix's non-origin
/// instance -- the device copy of a host-origin matrix, i.e. SLATE's
/// workspace tiles -- when the OUTERMOST driver finishes, so composite drivers
/// (gesv = getrf + getrs, posv, gels, ...) keep it between their stages.
inline int& driver_depth() { thread_local int d = 0; return d; }
struct DriverScope {
    DriverScope() { ++driver_depth(); }
    ~DriverScope() { --driver_depth(); }
    DriverScope(DriverScope const&) = delete;
    DriverScope& operator=(DriverScope const&) = delete;
};

/// End of a driver for an output matrix: write back to the origin instance
/// (tileUpdateAllOrigin) and release the workspace instance unless held.
template <typename T>
inline void finish_origin(BaseMatrix<T> const& A, Options const& opts) {
    A.storage()->update_origin();
    if (driver_depth() <= 1 && !get_option<bool>(opts, Option::HoldLocalWorkspace, false))
        A.storage()->release_workspace();
}

/// Block-cyclic working copy of an arbitrary-distribution (lambda
/// constructor) matrix or of a view of one: the drivers' contiguous local
/// arrays need the 2-D block-cyclic layout, while the reference drivers
/// consume any layout tile by tile.  Same processes; the largest tile of A
/// becomes the uniform tile.  The copy is the tile-by-tile redistribution.
template <typename T>
Matrix<T> block_cyclic(BaseMatrix<T> const& A, Options const& opts) {
    const int64_t b = std::max<int64_t>(1, std::max(A.storage()->mb, A.storage()->nb));
    Matrix<T> B(A.m(), A.n(), b, b, A.grid());
    B.insertLocalTiles(resolve_target(opts));
    slate::copy<T, T>(A, B, opts);
    return B;
}
/// A itself, or its block-cyclic copy when A has an arbitrary distribution
template <typename T>
Matrix<T> bc_operand(BaseMatrix<T> const& A, Options const& opts) {
    return A.arbitrary_layout() ? block_cyclic(A, opts) : Matrix<T>(A);
}
/// Block-cyclic copy of B whose row tiles are those of the (block-cyclic)
/// factor F, on F's grid: the right-hand side of a solve with F's factors.
template <typename T>
Matrix<T> block_cyclic_rows_of(BaseMatrix<T> const& F, BaseMatrix<T> const& B, Options const& opts) {
    Matrix<T> Bb(B.m(), B.n(), F.mb(), F.mb(), F.grid());
    Bb.insertLocalTiles(resolve_target(opts));
    slate::copy<T, T>(B, Bb, opts);
    return Bb;
}
/// Pivots / T factors of an arbitrary-layout matrix are expressed in the
/// tiling of its block-cyclic working copy (block_cyclic(), tile size = the
/// largest tile of A), which is deterministic; the solve-side drivers (getrs,
/// getri, unmqr, unmlq) re-create that copy, so factor and solve agree.
template <typename T>
bool needs_bc(BaseMatrix<T> const& A, BaseMatrix<T> const& B) {
    return A.arbitrary_layout() || B.arbitrary_layout();
}

/// Visit every STORED local element of the NoTrans view A on the host
/// instance (dense: the whole local block; band-only storage: the stored band
/// tiles) with its view-relative global (i, j): f(i, j, T& value).
template <typename T, typename F>
void for_each_stored(BaseMatrix<T> const& A, bool write, F&& f) {
    slate_error_if_msg(A.op() != Op::NoTrans, "for_each_stored: NoTrans view required");
    auto& s = *A.storage();
    s.get(Loc::Host, write);
    const int64_t r0 = A.lrow_begin(), r1 = A.lrow_end();
    const int p = s.grid->p(), q = s.grid->q();
    for (int64_t lc = A.lcol_begin(); lc < A.lcol_end(); ++lc) {
        const int64_t gc = l2g(lc, s.nb, s.crel(), q) - A.col0();
        int64_t a = r0, b = r1;
        if (s.banded) {
            const int64_t lj = lc / s.nb;
            a = std::max(r0, s.boff[lj]);
            b = std::min(r1, s.bend[lj]);
        }
        if (b <= a) continue;
        T* col = s.local_ptr(Loc::Host, a, lc);
        for (int64_t lr = a; lr < b; ++lr) f(l2g(lr, s.mb, s.rrel(), p) - A.row0(), gc, col[lr - a]);
    }
}

/// Broadcast a contiguous buffer over `comm` from `root` (stream-ordered).
template <typename T>
inline void bcast(Comm& comm, T* buf, size_t count, int root, lb::Ctx const& c) {
    if (comm.size() == 1 || count == 0) return;
    comm.bcast(buf, count, root, c.loc(), c.stream);
}

/// Pack a strided block into a dense buffer (ld = m).
template <typename T>
inline void pack(lb::Ctx const& c, int64_t m, int64_t n, T const* A, int64_t lda, T* W) {
    lb::copy2d(c, m, n, A, lda, W, m);
}

/// Reduce info across ranks (reference internal_reduce_info.cc): min over
/// nonzero values.
int64_t reduce_info(int64_t info, Comm& comm);

/// Read a device (or host) int info.
int64_t fetch_info(Target t, int* info);

/// All-gather of per-column norms etc. helper: allreduce on host vector.
template <typename R>
inline void allreduce_host(Comm& comm, R* v, size_t n, ReduceOp op) {
    if (comm.size() == 1 || n == 0) return;
    comm.allreduce(v, v, n, scalar_type<R>(), op, Loc::Host, nullptr);
}

/// Replicated LAPACK band storage: AB(r0 + i - j, j) = A(i, j) for
/// -ku <= i - j <= kl; ldab >= r0 + kl + 1.  conj_upper: read A's upper
/// band (i < j) as the conj-transposed lower band (Hermitian band, Upper).
template <typename T>
std::vector<T> band_gather(BaseMatrix<T> const& A, int64_t kl, int64_t ku, int64_t r0, int64_t ldab,
                           bool upper_as_lower = false) {
    const int64_t n = A.n();
    std::vector<T> ab(size_t(ldab) * n, T(0));
    for_each_stored(A, false, [&](int64_t i, int64_t j, T& v) {
        if (upper_as_lower) {
            if (j >= i && j - i <= ku) ab[(r0 + j - i) + i * ldab] = slate::conj(v);   // (j, i) of the lower band
        } else if (i - j <= kl && j - i <= ku) {
            ab[(r0 + i - j) + j * ldab] = v;
        }
    });
    // every band entry is owned by exactly one rank
    Comm& w = A.grid()->world();
    if (w.size() > 1) {
        using R = real_type<T>;
        size_t mult = is_complex_v<T> ? 2 : 1;
        allreduce_host<R>(w, reinterpret_cast<R*>(ab.data()), ab.size() * mult, ReduceOp::Sum);
    }
    return ab;
}

template <typename T>
void band_scatter(BaseMatrix<T>& A, std::vector<T> const& ab, int64_t kl, int64_t ku, int64_t r0, int64_t ldab,
                  bool upper_as_lower = false) {
    for_each_stored(A, true, [&](int64_t i, int64_t j, T& v) {
        if (upper_as_lower) {
            if (j >= i && j - i <= ku) v = slate::conj(ab[(r0 + j - i) + i * ldab]);
        } else if (i - j <= kl && j - i <= ku) {
            v = ab[(r0 + i - j) + j * ldab];
        }
    });
}

/// General redistribution B = op(A) between two matrices over the same world
/// (any grids / tile sizes with equal element counts), tile by tile over p2p.
template <typename T>
void redistribute_op(BaseMatrix<T> const& A, BaseMatrix<T>& B, Target target);

/// Distributed tridiagonal eigensolvers (eig_dist.cc): divide and conquer
/// with Q on its 2-D grid, and QL with the rotations applied to each rank's
/// rows of Z.  d, e replicated; eigenvalues ascending in d.
template <typename R>
void stedc_dist(std::vector<R>& d, std::vector<R> const& e, Matrix<R>& Q, Options const& opts);
template <typename T>
int64_t steqr2_dist(std::vector<real_type<T>>& d, std::vector<real_type<T>>& e, Matrix<T>& Z, Options const& opts);

/// Bidiagonal divide and conquer on local column-major arrays of c's memory
/// (bdsdc.cc): B(D, E) = UB diag(D) VB^T, UB / VB n x n with leading
/// dimension ld, D descending.  Replicated: every caller computes all of it.
template <typename R>
void bdsdc_local(lb::Ctx const& c, std::vector<R>& D, std::vector<R> const& E, R* UB, R* VB, int64_t ld);
/// A's local entries := phase[i] * op(src)(i, j) (src real, local, op(src) of
/// A's size; phase may be empty); A a whole NoTrans matrix.
template <typename T>
void bdsdc_place(lb::Ctx const& c, Matrix<T>& A, real_type<T> const* src, int64_t lds, bool trans,
                 std::vector<T> const& phase);

/// Panel width of the one-stage reductions (hetrd.cc, gebrd.cc, geqp3.cc; what
/// they share is in reduce_common.hh, their operand checks among it); their T
/// factors are kReducePanel x kReducePanel blocks, panel p at column p * kReducePanel.
constexpr int64_t kReducePanel = 64;
constexpr int64_t kHetrdPanel = kReducePanel, kGebrdPanel = kReducePanel, kGeqp3Panel = kReducePanel;
/// One-stage tridiagonal reduction of the lower triangle of the contiguous
/// local n x n array A (c's memory): A = Q T Q^T, T = tridiag(d, e) with
/// signed e, reflectors left in A below the subdiagonal with their unit entry
/// stored, tau (n) and Tfac (kHetrdPanel x n) in c's memory, d and e on the
/// host.  One host synchronisation, at the end.  The strict upper triangle is
/// not read.
template <typename R>
void hetrd_local(lb::Ctx const& c, int64_t n, R* A, int64_t lda, std::vector<R>& d, std::vector<R>& e, R* tau,
                 R* Tfac);
/// C (mc x nc) := op(Q) C (Left) or C op(Q) (Right), Q = H_0 .. H_{n-2} of
/// hetrd_local, one lb::larfb per panel; stream-ordered on the device.
template <typename R>
void unmtr_hetrd_local(lb::Ctx const& c, Side side, Op op, int64_t n, R const* A, int64_t lda, R const* Tfac,
                       int64_t mc, int64_t nc, R* C, int64_t ldc);

/// One-stage bidiagonal reduction of the contiguous local m x n array A (c's
/// memory), m >= n: A = Q B P^T, B upper bidiagonal (d, e), left reflectors
/// left in A below the diagonal and right ones right of the superdiagonal,
/// unit entries stored; tauq, taup (n each) and TQ, TP (kGebrdPanel x n each)
/// in c's memory, d and e on the host.  One host synchronisation, at the end.
template <typename R>
void gebrd_local(lb::Ctx const& c, int64_t m, int64_t n, R* A, int64_t lda, std::vector<R>& d, std::vector<R>& e,
                 R* tauq, R* taup, R* TQ, R* TP);
/// C (mc x nc) := op(F) C (Left) or C op(F) (Right), F = Q (order m) or P
/// (order n) of gebrd_local, one lb::larfb per panel; stream-ordered on the device.
template <typename R>
void unmbr_gebrd_local(lb::Ctx const& c, Vect vect, Side side, Op op, int64_t m, int64_t n, R const* A, int64_t lda,
                       R const* Tfac, int64_t mc, int64_t nc, R* C, int64_t ldc);

/// QR with column pivoting of the contiguous local m x n array A (c's memory):
/// A P = Q R, R in the upper triangle / trapezoid, the min(m, n) reflectors
/// below the diagonal with unit entries implied; tau (min(m, n)) and Tfac
/// (kGeqp3Panel x n) in c's memory, jpvt (n, 0-based) on the host.  One host
/// synchronisation, at the end.
template <typename R>
void geqp3_local(lb::Ctx const& c, int64_t m, int64_t n, R* A, int64_t lda, std::vector<int64_t>& jpvt, R* tau,
                 R* Tfac);
/// C (mc x nc) := op(Q) C (Left) or C op(Q) (Right), Q (order m) of
/// geqp3_local, one lb::larfb per panel; stream-ordered on the device.
template <typename R>
void unmqr_geqp3_local(lb::Ctx const& c, Side side, Op op, int64_t m, int64_t n, R const* A, int64_t lda,
                       R const* Tfac, int64_t mc, int64_t nc, R* C, int64_t ldc);

/// Range guard shared by heev, svd and gelsy (reference heev.cc:73-102,
/// svd.cc:85-125): returns the factor alpha the matrix was scaled to (1 if
/// untouched) and sets `bad` when ||A||_max is NaN or Inf.  A matrix with
/// ||A||_max below sqrt(safe_min / eps) or above its reciprocal is scaled by
/// alpha / ||A||_max, so the reductions neither underflow nor overflow; the
/// caller rescales its results afterwards.
template <typename R>
R range_alpha(R anorm, bool& bad) {
    const R sml = std::numeric_limits<R>::min() / std::numeric_limits<R>::epsilon();
    const R sqrt_sml = std::sqrt(sml), sqrt_big = R(1) / sqrt_sml;
    bad = std::isnan(anorm) || std::isinf(anorm);
    if (bad) return R(1);
    if (anorm > R(0) && anorm < sqrt_sml) return sqrt_sml;
    if (anorm > sqrt_big) return sqrt_big;
    return R(1);
}

/// Apply LU pivots to the rows of B (forward: P B; backward: P^T B).
template <typename T>
void apply_pivots(Pivots const& pivots, BaseMatrix<T> const& A, Matrix<T>& B, Target target, bool forward);

}  // namespace internal
}  // namespace slate
