// Core enumerations.  Semantics follow the reference's include/slate/enums.hh
// (Target :34-40, Option :63-99, NormScope :115, GridOrder :125, MOSI :138-143)
// and BLAS++/LAPACK++ enums (Op, Uplo, Diag, Side, Norm, Layout) which the
// reference takes from its blaspp submodule.
#pragma once

#include <cstdint>
#include <string>

namespace slate {

/// Location and method of computation (reference enums.hh:34-40).
/// On this framework HostTask/HostNest/HostBatch all run the C++/OpenMP host
/// kernels; Devices runs the gfx950 HIP kernels on this process's GPU.
enum class Target : char {
    Host      = 'H',
    HostTask  = 'T',
    HostNest  = 'N',
    HostBatch = 'B',
    Devices   = 'D',
};

inline bool is_host(Target t) { return t != Target::Devices; }

enum class Op     : char { NoTrans = 'N', Trans = 'T', ConjTrans = 'C' };
enum class Uplo   : char { Upper = 'U', Lower = 'L', General = 'G' };
enum class Diag   : char { NonUnit = 'N', Unit = 'U' };
enum class Side   : char { Left = 'L', Right = 'R' };
enum class Layout : char { ColMajor = 'C', RowMajor = 'R' };
enum class Norm   : char { One = '1', Two = '2', Inf = 'I', Fro = 'F', Max = 'M' };
enum class Job    : char { NoVec = 'N', Vec = 'V', AllVec = 'A', SomeVec = 'S', OverwriteVec = 'O' };
enum class Equed  : char { None = 'N', Row = 'R', Col = 'C', Both = 'B' };

/// Whether computing matrix norm, column norms, or row norms (enums.hh:115).
enum class NormScope : char { Columns = 'C', Rows = 'R', Matrix = 'M' };

/// Order to map processes to tile grid (enums.hh:125).
enum class GridOrder : char { Col = 'C', Row = 'R', Unknown = 'U' };

/// Layout conversion request (enums.hh:105).
enum class LayoutConvert : char { ColMajor = 'C', RowMajor = 'R', None = 'N' };

/// Eigenvalue method (enums.hh MethodEig).  Bisection (not in the reference):
/// values only, Sturm-count bisection (stebz) in place of sterf.
enum class MethodEig : char { QR = 'Q', DC = 'D', Bisection = 'B' };

/// Bidiagonal SVD method of svd with vectors: implicit-shift QR iteration
/// (bdsqr, default) or divide and conquer (bdsdc); Bisection: values only,
/// Sturm-count bisection on the Golub-Kahan form (bdsbz) in place of the
/// values-only QR iteration.  Not in the reference.
enum class MethodSVD : char { QR = 'Q', DC = 'D', Bisection = 'B' };

/// Which eigenvalues / singular values stebz and bdsbz compute (LAPACK's
/// range): all, those in [vl, vu), or those with index il .. iu.
enum class Range : char { All = 'A', Value = 'V', Index = 'I' };

/// Tridiagonal reduction of heev / syev / hegv / sygv: two stages (he2hb on
/// the device, the bulge chase hb2st on the host; default) or the one-stage
/// hetrd (sytrd panels, a symv per column on the device).  Not in the reference.
enum class MethodHetrd : char { TwoStage = '2', OneStage = '1' };

/// Bidiagonal reduction of svd / gesvd / svd_vals: two stages (ge2tb on the
/// device, the bulge chase tb2bd on the host; default) or the one-stage gebrd
/// (labrd panels, two matrix-vector products per column on the device).  Not
/// in the reference.
enum class MethodGebrd : char { TwoStage = '2', OneStage = '1' };

/// Arithmetic of the large device fp32 products (trailing updates) of a
/// routine: the fp32 MFMA kernels, or the split-operand bf16 MFMA kernel with
/// 1, 3 or 6 plane products per K-step (gemm_bf16s.hip).  Not in the reference.
enum class GemmPrecision : char { Native = 'N', BF16 = '1', BF16x3 = '3', BF16x6 = '6' };

/// Keys for options passed to routines (enums.hh:63-99).
enum class Option : char {
    ChunkSize,
    Lookahead,
    BlockSize,
    InnerBlocking,
    MaxPanelThreads,
    Tolerance,
    Target,
    HoldLocalWorkspace,
    Depth,
    MaxIterations,
    UseFallbackSolver,
    PivotThreshold,
    /// Mixed-precision solvers (gesv_mixed / posv_mixed): when classical
    /// refinement stalls or is projected to miss MaxIterations, continue with
    /// GMRES-IR preconditioned by the same low-precision factors before the
    /// full-precision fallback.  Not in the reference (default off: the
    /// reference semantics, classical refinement then fallback).
    EscalateGmres,
    /// GemmPrecision of the fp32 trailing updates (gemm, getrf family, potrf;
    /// the mixed solvers apply it to their low-precision factorization only).
    /// Default Native.  Not in the reference.
    GemmPrecision,

    PrintVerbose = 50,
    PrintEdgeItems,
    PrintWidth,
    PrintPrecision,

    MethodCholQR = 60,
    MethodEig,
    MethodGels,
    MethodGemm,
    MethodHemm,
    MethodLU,
    MethodTrsm,
    /// MethodSVD of svd / gesvd with vectors.  Default QR.  Not in the reference.
    MethodSVD,
    /// MethodHetrd of heev / syev / hegv / sygv.  Default TwoStage.  Not in the reference.
    MethodHetrd,
    /// MethodGebrd of svd / gesvd / svd_vals.  Default TwoStage.  Not in the reference.
    MethodGebrd,
};

const int HostNum    = -1;
const int AllDevices = -2;
const int AnyDevice  = -3;

/// Coherency state.  The reference keeps MOSI per tile instance
/// (enums.hh:138-143); here a matrix's local array has one host and one device
/// instance and the state is kept per instance at matrix granularity.
enum MOSI : short {
    Modified = 0x100,
    OnHold   = 0x1000,
    Shared   = 0x010,
    Invalid  = 0x001,
};
typedef short MOSI_State;

/// Kind of a tile buffer (reference Tile.hh:120-124).
enum class TileKind : char { Workspace = 'W', SlateOwned = 'S', UserOwned = 'U' };

//------------------------------------------------------------------------------
inline char to_char(Op v)     { return char(v); }
inline char to_char(Uplo v)   { return char(v); }
inline char to_char(Diag v)   { return char(v); }
inline char to_char(Side v)   { return char(v); }
inline char to_char(Norm v)   { return char(v); }
inline char to_char(Target v) { return char(v); }

inline Op    flip_trans(Op op, bool conj) { return op == Op::NoTrans ? (conj ? Op::ConjTrans : Op::Trans) : Op::NoTrans; }
inline Uplo  flip(Uplo u) { return u == Uplo::Lower ? Uplo::Upper : (u == Uplo::Upper ? Uplo::Lower : u); }
inline Side  flip(Side s) { return s == Side::Left ? Side::Right : Side::Left; }

const char* to_string(Target t);
const char* to_string(Op v);
const char* to_string(Uplo v);
const char* to_string(Norm v);
Target str2target(const std::string& s);
Norm   str2norm(const std::string& s);
const char* to_string(GemmPrecision p);
/// "native", "bf16", "bf16x3", "bf16x6"; anything else throws.
GemmPrecision str2gemm_precision(const std::string& s);

}  // namespace slate
