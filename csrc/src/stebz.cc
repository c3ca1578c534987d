// Eigenvalues of a symmetric tridiagonal (stebz) and singular values of a
// bidiagonal (bdsbz) by Sturm-count bisection: all of them, those in an
// interval, or those with given indices.  The arithmetic is
// slate_amd/sturm.hh; the device kernels are kernels/stebz.hip, the host
// twins host::sturm_counts / host::stebz_range (eig_host.cc).
//
// Both routines scale (D, E) to unit max-norm, count on (d, e^2) and scale
// the values back.  bdsbz counts on the Golub-Kahan tridiagonal of order 2n
// (zero diagonal, off-diagonals d_1, e_1, d_2, ..., d_n) and keeps its upper
// half, eigenvalues n .. 2n - 1, which are the singular values ascending.
//
// Device target: d, e^2 and the two end points of a range by value go up in
// one copy; the range by value counts at its end points (one launch), the
// refinement is one launch whatever the range and however early the values
// converge (each wave runs to its own stopping rule), and the counts, the
// values and their step numbers come back in one copy followed by the only
// host synchronisation.  launches = 1 + (range == Value), host_syncs = 1.
//
// Every eigenvalue is refined from the same start interval with the same
// number of trial points P, chosen from the order of the problem (not from
// the number of values wanted), so a subset has the bits of the same entries
// of the full set.  Two eigenvalues take the same trial points until a point
// separates them, which then bounds one from above and the other from below:
// the values come out in order without a sort.
#include "internal.hh"
#include "slate_amd/eig_host.hh"
#include "slate_amd/sturm.hh"
#include "../kernels/kernels.hh"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace slate {

namespace {

std::mutex g_stats_mu;
StebzStats g_stats;   // of the last stebz / bdsbz in this process

void publish(StebzStats const& st) {
    std::lock_guard<std::mutex> lk(g_stats_mu);
    g_stats = st;
}

/// Trial points per eigenvalue and step on the device: the largest power of
/// two that still gives every (eigenvalue, point) lane of a Range::All call
/// a lane of its own with one wave per SIMD (4 SIMDs of 64 lanes per CU): the
/// division chain of one wave keeps a SIMD's FP64 pipe busy, so more waves
/// per SIMD buy little, while idle SIMDs are free.
int choose_points(int64_t values) {
    if (const char* e = std::getenv("SLATE_STEBZ_POINTS")) {
        const int p = std::atoi(e);
        slate_error_if_msg(p < 1 || p > 64 || (p & (p - 1)) != 0, "SLATE_STEBZ_POINTS must be 1, 2, 4, 8, 16, 32 or 64");
        return p;
    }
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device::get_device()) != hipSuccess || cus <= 0)
        cus = 256;
    const int64_t lanes = int64_t(cus) * 4 * 64;
    int p = 1;
    while (p < 64 && std::max<int64_t>(values, 1) * (2 * p) <= lanes) p *= 2;
    return p;
}

/// A tridiagonal scaled to unit max-norm, ready to count on.
template <typename R>
struct Problem {
    int64_t n = 0;
    std::vector<R> d, e2;     // n and n - 1
    R scale = 1, pivmin = 0;
    sturm::Interval<R> iv;
    sturm::Stop<R> stop;
};

template <typename R>
void check_finite(std::vector<R> const& D, std::vector<R> const& E, int64_t n, char const* name) {
    slate_error_if_msg(int64_t(E.size()) < n - 1, std::string(name) + ": E has fewer than n - 1 entries");
    bool ok = true;
    for (int64_t i = 0; i < n; ++i) ok = ok && std::isfinite(D[i]);
    for (int64_t i = 0; i + 1 < n; ++i) ok = ok && std::isfinite(E[i]);
    slate_error_if_msg(!ok, std::string(name) + ": the matrix has a NaN or Inf entry");
}

template <typename R>
void check_range(Range range, R vl, R vu, int64_t il, int64_t iu, int64_t n, char const* name) {
    slate_error_if_msg(range != Range::All && range != Range::Value && range != Range::Index,
                       std::string(name) + ": range is none of Range::All, Range::Value, Range::Index");
    if (range == Range::Value)
        slate_error_if_msg(!(vl < vu), std::string(name) + ": Range::Value needs vl < vu");
    if (range == Range::Index)
        slate_error_if_msg(il < 1 || iu < il || iu > n, std::string(name) + ": Range::Index needs 1 <= il <= iu <= n");
}

template <typename R>
R max_abs(std::vector<R> const& D, std::vector<R> const& E, int64_t n) {
    R s = 0;
    for (int64_t i = 0; i < n; ++i) s = std::max(s, std::abs(D[i]));
    for (int64_t i = 0; i + 1 < n; ++i) s = std::max(s, std::abs(E[i]));
    return s;
}

/// pivmin and the start interval from the scaled d and off-diagonal e (n - 1); e2 := e^2
template <typename R>
void finish_problem(Problem<R>& p, std::vector<R> const& e) {
    p.e2.resize(e.size());
    for (size_t i = 0; i < e.size(); ++i) p.e2[i] = e[i] * e[i];
    p.pivmin = sturm::pivmin_of<R>(p.n, p.e2.data());
    p.iv = sturm::start_interval<R>(p.n, p.d.data(), e.data(), p.pivmin);
}

/// The scaled eigenvalues [k0, k1) ascending, or with by_value those that
/// sturm::wanted_of_counts(N(x0), N(x1), kmin) selects.  all_values: the
/// number of values of a Range::All call on this problem (chooses P).
template <typename R>
std::vector<R> solve(Problem<R> const& p, bool by_value, R x0, R x1, int64_t k0, int64_t k1, int64_t kmin,
                     int64_t all_values, Options const& opts, StebzStats& st) {
    const Target target = internal::resolve_target(opts);
    const int64_t n = p.n;
    st.n = n;
    std::vector<R> w;
    if (target != Target::Devices) {
        if (by_value) {
            const R x[2] = {x0, x1};
            int64_t c[2];
            host::sturm_counts<R>(n, p.d.data(), p.e2.data(), p.pivmin, 2, x, c);
            const sturm::Wanted wt = sturm::wanted_of_counts(c[0], c[1], kmin);
            k0 = wt.k0; k1 = wt.k1;
        }
        w.resize(size_t(k1 - k0));
        st.points = 1;
        st.steps = host::stebz_range<R>(n, p.d.data(), p.e2.data(), p.pivmin, p.iv.lo, p.iv.hi, p.stop.abstol,
                                        p.stop.floor, k0, k1, w.data());
        st.values = k1 - k0;
        return w;
    }
    namespace kd = slate_amd::dev;
    lb::Ctx c = lb::Ctx::device(0);
    const int P = choose_points(all_values);
    const int64_t maxv = by_value ? n - kmin : k1 - k0;
    // up: d | e2 | x0 x1 in one copy
    std::vector<R> up(size_t(2 * n + 2), R(0));
    std::copy(p.d.begin(), p.d.end(), up.begin());
    std::copy(p.e2.begin(), p.e2.end(), up.begin() + n);
    up[2 * n] = x0;
    up[2 * n + 1] = x1;
    internal::Work<R> dev_in(Target::Devices, up.size());
    // down: counts (2 int64) | values (maxv R) | steps (maxv int32) in one copy
    const size_t off_w = 2 * sizeof(int64_t), off_s = off_w + size_t(maxv) * sizeof(R);
    const size_t out_bytes = off_s + size_t(maxv) * sizeof(int32_t);
    internal::Work<unsigned char> dev_out(Target::Devices, out_bytes);
    std::vector<unsigned char> down(out_bytes, 0);
    device::memcpy_async(dev_in.data(), up.data(), up.size() * sizeof(R), c.stream);
    int64_t* dcnt = reinterpret_cast<int64_t*>(dev_out.data());
    if (by_value) {
        kd::sturm_count<R>(n, dev_in.data(), dev_in.data() + n, p.pivmin, 2, dev_in.data() + 2 * n, dcnt, c.stream);
        ++st.launches;
    }
    kd::StebzRefine<R> a;
    a.n = n;
    a.d = dev_in.data();
    a.e2 = dev_in.data() + n;
    a.lo = p.iv.lo; a.hi = p.iv.hi;
    a.pivmin = p.pivmin; a.abstol = p.stop.abstol; a.floor = p.stop.floor;
    a.k0 = k0; a.k1 = k1; a.kmin = kmin;
    a.cnt = by_value ? dcnt : nullptr;
    a.points = P;
    a.max_steps = sturm::step_cap<R>(P);
    a.w = reinterpret_cast<R*>(dev_out.data() + off_w);
    a.steps = reinterpret_cast<int32_t*>(dev_out.data() + off_s);
    if (maxv > 0) {
        kd::stebz_refine<R>(a, maxv, c.stream);
        ++st.launches;
    }
    device::memcpy_async(down.data(), dev_out.data(), out_bytes, c.stream);
    slate_hip_call(hipStreamSynchronize(c.stream));
    ++st.host_syncs;
    if (by_value) {
        int64_t cnt[2];
        std::memcpy(cnt, down.data(), sizeof(cnt));
        const sturm::Wanted wt = sturm::wanted_of_counts(cnt[0], cnt[1], kmin);
        k0 = wt.k0; k1 = wt.k1;
    }
    const int64_t m = k1 - k0;
    w.resize(size_t(m));
    if (m > 0) std::memcpy(w.data(), down.data() + off_w, size_t(m) * sizeof(R));
    int32_t most = 0;
    for (int64_t i = 0; i < m; ++i) {
        int32_t sv;
        std::memcpy(&sv, down.data() + off_s + size_t(i) * sizeof(int32_t), sizeof(sv));
        most = std::max(most, sv);
    }
    st.points = P;
    st.steps = most;
    st.values = m;
    return w;
}

}  // namespace

StebzStats stebz_stats() {
    std::lock_guard<std::mutex> lk(g_stats_mu);
    return g_stats;
}

//------------------------------------------------------------------------------
template <typename R>
void stebz(Range range, R vl, R vu, int64_t il, int64_t iu, std::vector<R> const& D, std::vector<R> const& E,
           std::vector<R>& W, Options const& opts) {
    trace::Block tb("stebz");
    const int64_t n = int64_t(D.size());
    check_finite(D, E, n, "stebz");
    check_range(range, vl, vu, il, iu, n, "stebz");
    internal::resolve_target(opts);
    StebzStats st;
    st.n = n;
    const R scale = max_abs(D, E, n);
    if (n == 0 || scale == R(0)) {
        // every eigenvalue is zero
        int64_t m = n;
        if (range == Range::Index) m = iu - il + 1;
        if (range == Range::Value) m = (vl <= R(0) && R(0) < vu) ? n : 0;
        W.assign(size_t(m), R(0));
        st.values = m;
        publish(st);
        return;
    }
    Problem<R> p;
    p.n = n;
    p.scale = scale;
    p.d.resize(n);
    std::vector<R> e(size_t(n - 1));
    for (int64_t i = 0; i < n; ++i) p.d[i] = D[i] / scale;
    for (int64_t i = 0; i + 1 < n; ++i) e[i] = E[i] / scale;
    finish_problem(p, e);
    p.stop.abstol = std::numeric_limits<R>::epsilon();   // eps max|T_ij| of the scaled matrix
    p.stop.floor = R(0);
    int64_t k0 = 0, k1 = n;
    if (range == Range::Index) { k0 = il - 1; k1 = iu; }
    W = solve<R>(p, range == Range::Value, vl / scale, vu / scale, k0, k1, 0, n, opts, st);
    for (R& x : W) x *= scale;
    publish(st);
}

template <typename R>
void bdsbz(Range range, R vl, R vu, int64_t il, int64_t iu, std::vector<R> const& D, std::vector<R> const& E,
           std::vector<R>& S, Options const& opts) {
    trace::Block tb("bdsbz");
    const int64_t n = int64_t(D.size());
    check_finite(D, E, n, "bdsbz");
    check_range(range, vl, vu, il, iu, n, "bdsbz");
    internal::resolve_target(opts);
    StebzStats st;
    st.n = 2 * n;
    const R scale = max_abs(D, E, n);
    if (n == 0 || scale == R(0)) {
        int64_t m = n;
        if (range == Range::Index) m = iu - il + 1;
        if (range == Range::Value) m = (vl <= R(0) && R(0) < vu) ? n : 0;
        S.assign(size_t(m), R(0));
        st.values = m;
        publish(st);
        return;
    }
    // Golub-Kahan: zero diagonal, off-diagonals d_1, e_1, d_2, ..., d_n
    Problem<R> p;
    p.n = 2 * n;
    p.scale = scale;
    p.d.assign(size_t(2 * n), R(0));
    std::vector<R> g(size_t(2 * n - 1));
    for (int64_t i = 0; i < n; ++i) {
        g[2 * i] = D[i] / scale;
        if (i + 1 < n) g[2 * i + 1] = E[i] / scale;
    }
    finish_problem(p, g);
    p.iv.lo = R(0);   // the upper half of the spectrum
    p.stop.abstol = R(0);
    p.stop.floor = sturm::floor_value<R>();
    // descending index j (1 = largest) is ascending eigenvalue 2n - j
    int64_t k0 = n, k1 = 2 * n;
    if (range == Range::Index) { k0 = 2 * n - iu; k1 = 2 * n - il + 1; }
    // N(x) for x <= 0 is below n by definition of the wanted half: any x < -||T|| gives 0
    const R x0 = vl <= R(0) ? R(-4) : vl / scale, x1 = vu <= R(0) ? R(-4) : vu / scale;
    S = solve<R>(p, range == Range::Value, x0, x1, k0, k1, n, n, opts, st);
    std::reverse(S.begin(), S.end());
    for (R& x : S) x *= scale;
    publish(st);
}

template <typename R>
std::vector<int64_t> sturm_count(std::vector<R> const& D, std::vector<R> const& E, std::vector<R> const& x,
                                 Options const& opts) {
    trace::Block tb("sturm_count");
    const int64_t n = int64_t(D.size()), nx = int64_t(x.size());
    check_finite(D, E, n, "sturm_count");
    for (R v : x) slate_error_if_msg(std::isnan(v), "sturm_count: a shift is NaN");
    const Target target = internal::resolve_target(opts);
    std::vector<int64_t> cnt(size_t(nx), 0);
    if (n == 0 || nx == 0) return cnt;
    const R scale = max_abs(D, E, n);
    if (scale == R(0)) {
        for (int64_t j = 0; j < nx; ++j) cnt[j] = x[j] > R(0) ? n : 0;
        return cnt;
    }
    Problem<R> p;
    p.n = n;
    p.d.resize(n);
    std::vector<R> e(size_t(n - 1));
    for (int64_t i = 0; i < n; ++i) p.d[i] = D[i] / scale;
    for (int64_t i = 0; i + 1 < n; ++i) e[i] = E[i] / scale;
    finish_problem(p, e);
    std::vector<R> xs(x.size());
    for (int64_t j = 0; j < nx; ++j) xs[j] = x[j] / scale;
    if (target != Target::Devices) {
        host::sturm_counts<R>(n, p.d.data(), p.e2.data(), p.pivmin, nx, xs.data(), cnt.data());
        return cnt;
    }
    lb::Ctx c = lb::Ctx::device(0);
    std::vector<R> up(size_t(2 * n + nx), R(0));
    std::copy(p.d.begin(), p.d.end(), up.begin());
    std::copy(p.e2.begin(), p.e2.end(), up.begin() + n);
    std::copy(xs.begin(), xs.end(), up.begin() + 2 * n);
    internal::Work<R> dev_in(Target::Devices, up.size());
    internal::Work<int64_t> dev_cnt(Target::Devices, size_t(nx));
    device::memcpy_async(dev_in.data(), up.data(), up.size() * sizeof(R), c.stream);
    slate_amd::dev::sturm_count<R>(n, dev_in.data(), dev_in.data() + n, p.pivmin, nx, dev_in.data() + 2 * n,
                                   dev_cnt.data(), c.stream);
    device::memcpy_async(cnt.data(), dev_cnt.data(), size_t(nx) * sizeof(int64_t), c.stream);
    slate_hip_call(hipStreamSynchronize(c.stream));
    return cnt;
}

#define SLATE_STEBZ_INST(R)                                                                                   \
    template void stebz<R>(Range, R, R, int64_t, int64_t, std::vector<R> const&, std::vector<R> const&,       \
                           std::vector<R>&, Options const&);                                                  \
    template void bdsbz<R>(Range, R, R, int64_t, int64_t, std::vector<R> const&, std::vector<R> const&,       \
                           std::vector<R>&, Options const&);                                                  \
    template std::vector<int64_t> sturm_count<R>(std::vector<R> const&, std::vector<R> const&,                \
                                                 std::vector<R> const&, Options const&);
SLATE_STEBZ_INST(float)
SLATE_STEBZ_INST(double)

}  // namespace slate
