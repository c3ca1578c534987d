// Host side of one merge of the divide and conquer, shared by stedc_dist
// (eig_dist.cc) and bdsdc (bdsdc.cc): everything between the caller's
// deflation loop and its GEMMs.  Device kernels: kernels/dc_merge.hip.
#pragma once

#include "internal.hh"
#include "../kernels/kernels.hh"

#include <initializer_list>
#include <vector>

namespace slate {
namespace internal {

using slate_amd::dev::BdsdcSide;
using slate_amd::dev::DcMerge;
using slate_amd::dev::DcRotations;
using slate_amd::dev::StedcSide;

/// Rotations recorded (not applied) by a deflation loop, in application order.
struct RotationList {
    std::vector<int64_t> ab;   // pairs (a, b)
    std::vector<double> cs;    // pairs (c, s)
    int64_t count() const { return int64_t(cs.size()) / 2; }
};

/// Device vectors and column scratch, kept from merge to merge.
struct DcMergeWork {
    Work<double> dvec, dscr;
    Work<int64_t> divec;
};

/// Close-pole step of the deflation loops, on the sorted (Ds, zs): the rotation
/// of entries (last, s) that zeroes zs[last].  If it moves the two poles by no
/// more than tol it is appended to every list of `record`, the poles and z
/// are updated and true is returned: entry `last` is then deflated.
bool close_pole_rotation(std::vector<double>& Ds, std::vector<double>& zs, int64_t last, int64_t s, double tol,
                         std::initializer_list<RotationList*> record);

/// Roots (org, tau) and z-hat of the k active poles dd with weights zz,
/// znorm2 = |zz|^2; Poles is secular::LinearPoles<double> or SquaredPoles<double>.
/// Device target: dd and zz go into the device block of a merge of n entries
/// and nrot recorded rotations in all, the two kernels run there, org and tau
/// come back and zh stays on the device (the vector zh is left empty).
/// Host target: the host twin fills all three.
template <typename Poles>
void secular_solve(lb::Ctx const& c, DcMergeWork& ws, int64_t n, int64_t nrot, int64_t k, double rho,
                   std::vector<double> const& dd, std::vector<double> const& zz, double znorm2,
                   std::vector<int64_t>& org, std::vector<double>& tau, std::vector<double>& zh);

/// The descriptor of a merge whose roots secular_solve has found, and one
/// DcRotations in rot_out per list of `rots`.  Host target: the pointers of
/// the given vectors.  Device target: the vectors are uploaded next to what
/// secular_solve left in the device block.
DcMerge merge_layout(lb::Ctx const& c, DcMergeWork& ws, int64_t n, std::vector<double> const& dd,
                     std::vector<double> const& zh, std::vector<double> const& tau, std::vector<int64_t> const& org,
                     std::vector<int64_t> const& act, std::vector<int64_t> const& defl, std::vector<int64_t> const& ord,
                     std::vector<int64_t> const& inv_perm, std::initializer_list<RotationList const*> rots,
                     DcRotations* rot_out);

/// Output columns [0, ncols) of a merge matrix into M (ld ldm), asynchronous on
/// the device: the column kernel in batches whose scratch stays under a byte
/// budget, or its host twin.  Returns the number of kernel launches.
template <typename R, typename Side>
int64_t merge_columns(lb::Ctx const& c, DcMergeWork& ws, DcMerge const& mg, DcRotations const& rot, Side const& side,
                      int64_t ncols, R* M, int64_t ldm);

}  // namespace internal
}  // namespace slate
