// Eigenvectors of a symmetric tridiagonal for given eigenvalues by inverse
// iteration (stein).  The arithmetic is slate_amd/stein.hh; the device kernels
// are kernels/stein.hip, the host twin host::stein (eig_host.cc).
//
// The host scales (D, E, W) to unit max-norm, fixes the clusters and the
// perturbed values from W alone, and then runs exactly invit::kRounds rounds.
// Device target: d, e and the values go up in one copy, the cluster tables in
// two; every round is one stein_solve launch over all vectors and, when any
// cluster exists, one stein_orth launch with a workgroup per cluster; one
// stein_transpose launch writes Z.  Which vectors are finished is decided on
// the device and read there, so the launches depend on n, m and the
// existence of a cluster only:
//   launches = kRounds (1 + (clusters > 0)) + 1,   host_syncs = 1,
// the fetch of the acceptance flags (and of Z, when Z is host memory).
// Workspace on the device: 4 n mp reals ([row][vector]: the iterate and the
// three diagonals of U), mp = m rounded up to 64, plus O(m) per-vector state.
#include "internal.hh"
#include "reduce_common.hh"
#include "slate_amd/eig_host.hh"
#include "slate_amd/stein.hh"
#include "../kernels/kernels.hh"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace slate {

namespace {

internal::LastStats<SteinStats> g_stats;   // of the last stein in this process

enum { kSolve = 0, kOrth = 1, kTranspose = 2, kKinds = 3 };

}  // namespace

SteinStats stein_stats() { return g_stats.get(); }

namespace internal {

template <typename R>
void stein_core(std::vector<R> const& D, std::vector<R> const& E, std::vector<R> const& W, R* Z, int64_t ldz,
                bool z_on_device, std::vector<int64_t>& ifail, Options const& opts) {
    trace::Block tb("stein");
    const int64_t n = int64_t(D.size()), m = int64_t(W.size());
    const Target target = resolve_target(opts);
    slate_error_if_msg(z_on_device && target != Target::Devices, "stein: a device Z needs Target::Devices");
    slate_error_if_msg(int64_t(E.size()) < n - 1, "stein: E has fewer than n - 1 entries");
    slate_error_if_msg(m > n, "stein: more eigenvalues than the order of the matrix (m = " + std::to_string(m) +
                                  " > n = " + std::to_string(n) + ")");
    bool ok = true;
    for (int64_t i = 0; i < n; ++i) ok = ok && std::isfinite(D[i]);
    for (int64_t i = 0; i + 1 < n; ++i) ok = ok && std::isfinite(E[i]);
    slate_error_if_msg(!ok, "stein: the matrix has a NaN or Inf entry");
    for (int64_t j = 0; j < m; ++j) ok = ok && std::isfinite(W[j]);
    slate_error_if_msg(!ok, "stein: an eigenvalue is NaN or Inf");
    for (int64_t j = 1; j < m; ++j) ok = ok && W[j - 1] <= W[j];
    slate_error_if_msg(!ok, "stein: the eigenvalues W are not ascending");
    slate_error_if_msg(m > 0 && ldz < n, "stein: ldz < n");
    SteinStats st;
    st.n = n;
    st.values = m;
    ifail.clear();
    if (n == 0 || m == 0) { g_stats.set(st); return; }
    R scale = R(0);
    for (int64_t i = 0; i < n; ++i) scale = std::max(scale, std::abs(D[i]));
    for (int64_t i = 0; i + 1 < n; ++i) scale = std::max(scale, std::abs(E[i]));
    if (n == 1 || scale == R(0)) {
        // [1], or the first m unit vectors of an all-zero matrix: no launch
        std::vector<R> I(size_t(n * m), R(0));
        for (int64_t j = 0; j < m; ++j) I[j + j * n] = R(1);
        if (z_on_device) {
            lb::Ctx c = lb::Ctx::device(0);
            slate_hip_call(hipMemcpy2DAsync(Z, size_t(ldz) * sizeof(R), I.data(), size_t(n) * sizeof(R),
                                            size_t(n) * sizeof(R), size_t(m), hipMemcpyHostToDevice, c.stream));
            slate_hip_call(hipStreamSynchronize(c.stream));
            ++st.host_syncs;
        } else {
            for (int64_t j = 0; j < m; ++j) std::copy(I.begin() + j * n, I.begin() + (j + 1) * n, Z + j * ldz);
        }
        g_stats.set(st);
        return;
    }
    // d | e | w, scaled
    std::vector<R> up(size_t(2 * n - 1 + m));
    R* d = up.data();
    R* e = d + n;
    R* w = e + (n - 1);
    for (int64_t i = 0; i < n; ++i) d[i] = D[i] / scale;
    for (int64_t i = 0; i + 1 < n; ++i) e[i] = E[i] / scale;
    for (int64_t j = 0; j < m; ++j) w[j] = W[j] / scale;
    const R onenrm = invit::one_norm<R>(n, d, e);
    const invit::Clusters<R> cl = invit::find_clusters<R>(m, w, onenrm);
    const int64_t nc = int64_t(cl.first.size());
    st.clusters = nc;
    st.largest_cluster = cl.largest;
    st.rounds = invit::kRounds;
    std::vector<int32_t> done(size_t(m), 0);
    if (target != Target::Devices) {
        host::stein<R>(n, d, e, onenrm, m, w, cl.cluster.data(), nc, cl.first.data(), cl.last.data(), Z, ldz,
                       done.data());
    } else {
        namespace kd = slate_amd::dev;
        lb::Ctx c = lb::Ctx::device(0);
        StageProfile prof("SLATE_STEIN_PROFILE", kKinds, c.stream);
        const int64_t mp = (m + kd::kSteinLanes - 1) / kd::kSteinLanes * kd::kSteinLanes;
        Work<R> dev_in(Target::Devices, up.size());
        Work<R> ws(Target::Devices, size_t(4 * n * mp + 3 * mp));
        // cluster | pass | done | cpass, and first | last
        std::vector<int32_t> iup(size_t(3 * m + nc), 0);
        std::copy(cl.cluster.begin(), cl.cluster.end(), iup.begin());
        std::vector<int64_t> lup(size_t(2 * std::max<int64_t>(nc, 1)), 0);
        std::copy(cl.first.begin(), cl.first.end(), lup.begin());
        std::copy(cl.last.begin(), cl.last.end(), lup.begin() + nc);
        Work<int32_t> dev_i(Target::Devices, iup.size());
        Work<int64_t> dev_l(Target::Devices, lup.size());
        Work<R> dev_z;
        if (!z_on_device) dev_z.resize(Target::Devices, size_t(n * m));
        device::memcpy_async(dev_in.data(), up.data(), up.size() * sizeof(R), c.stream);
        device::memcpy_async(dev_i.data(), iup.data(), iup.size() * sizeof(int32_t), c.stream);
        device::memcpy_async(dev_l.data(), lup.data(), lup.size() * sizeof(int64_t), c.stream);
        kd::SteinSolve<R> a;
        a.n = n; a.m = m; a.mp = mp;
        a.d = dev_in.data();
        a.e = a.d + n;
        a.w = a.e + (n - 1);
        a.bnorm = invit::rhs_norm<R>(n, onenrm);
        a.cluster = dev_i.data();
        a.pass = dev_i.data() + m;
        a.done = dev_i.data() + 2 * m;
        a.x = ws.data();
        a.ua = a.x + n * mp;
        a.ub = a.ua + n * mp;
        a.ud = a.ub + n * mp;
        a.xmax = a.ud + n * mp;
        a.nrm = a.xmax + mp;
        a.unn = a.nrm + mp;
        kd::SteinOrth<R> o;
        o.n = n; o.mp = mp;
        o.first = dev_l.data();
        o.last = dev_l.data() + nc;
        o.x = a.x; o.xmax = a.xmax; o.nrm = a.nrm; o.unn = a.unn;
        o.cpass = dev_i.data() + 3 * m;
        o.done = a.done;
        prof.mark(StageProfile::Start);
        for (int round = 0; round < invit::kRounds; ++round) {
            a.round = round;
            kd::stein_solve<R>(a, c.stream);
            ++st.launches;
            prof.mark(kSolve);
            if (nc > 0) {
                kd::stein_orth<R>(o, nc, c.stream);
                ++st.launches;
                prof.mark(kOrth);
            }
        }
        R* zd = z_on_device ? Z : dev_z.data();
        const int64_t ldd = z_on_device ? ldz : n;
        kd::stein_transpose<R>(n, m, mp, a.x, a.xmax, a.nrm, zd, ldd, c.stream);
        ++st.launches;
        prof.mark(kTranspose);
        device::memcpy_async(done.data(), a.done, size_t(m) * sizeof(int32_t), c.stream);
        if (!z_on_device)
            slate_hip_call(hipMemcpy2DAsync(Z, size_t(ldz) * sizeof(R), zd, size_t(n) * sizeof(R), size_t(n) * sizeof(R),
                                            size_t(m), hipMemcpyDeviceToHost, c.stream));
        slate_hip_call(hipStreamSynchronize(c.stream));
        ++st.host_syncs;
        const std::vector<double> ms = prof.finish();
        st.ms_solve = ms[kSolve];
        st.ms_orth = ms[kOrth];
        st.ms_transpose = ms[kTranspose];
    }
    for (int64_t j = 0; j < m; ++j)
        if (!done[j]) ifail.push_back(j + 1);
    st.failed = int64_t(ifail.size());
    g_stats.set(st);
}

template void stein_core<float>(std::vector<float> const&, std::vector<float> const&, std::vector<float> const&,
                                float*, int64_t, bool, std::vector<int64_t>&, Options const&);
template void stein_core<double>(std::vector<double> const&, std::vector<double> const&, std::vector<double> const&,
                                 double*, int64_t, bool, std::vector<int64_t>&, Options const&);

}  // namespace internal

//------------------------------------------------------------------------------
template <typename R>
int64_t stein(std::vector<R> const& D, std::vector<R> const& E, std::vector<R> const& W, std::vector<R>& Z,
              std::vector<int64_t>& ifail, Options const& opts) {
    const int64_t n = int64_t(D.size()), m = int64_t(W.size());
    slate_error_if_msg(m > n, "stein: more eigenvalues than the order of the matrix (m = " + std::to_string(m) +
                                  " > n = " + std::to_string(n) + ")");
    Z.assign(size_t(n * m), R(0));
    internal::stein_core<R>(D, E, W, Z.data(), n, false, ifail, opts);
    return int64_t(ifail.size());
}

template <typename R>
int64_t stein(std::vector<R> const& D, std::vector<R> const& E, std::vector<R> const& W, std::vector<R>& Z,
              Options const& opts) {
    std::vector<int64_t> ifail;
    return stein<R>(D, E, W, Z, ifail, opts);
}

#define SLATE_STEIN_INST(R)                                                                                  \
    template int64_t stein<R>(std::vector<R> const&, std::vector<R> const&, std::vector<R> const&,           \
                              std::vector<R>&, std::vector<int64_t>&, Options const&);                       \
    template int64_t stein<R>(std::vector<R> const&, std::vector<R> const&, std::vector<R> const&,           \
                              std::vector<R>&, Options const&);
SLATE_STEIN_INST(float)
SLATE_STEIN_INST(double)

}  // namespace slate
