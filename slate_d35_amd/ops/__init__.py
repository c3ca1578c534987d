"""Direct access to the gfx950 kernels on torch tensors (single process).

These bypass the distributed matrix classes and call the local BLAS layer
(csrc/src/local_blas.cc) on device pointers; used by kernel numerics tests
and micro-benchmarks.  Tensors are interpreted column-major: pass the
transpose of a row-major torch tensor, or use the helpers below which take
care of layout.
"""
from __future__ import annotations

from .. import _slate

__all__ = ["have_native_ops", "gemm", "gemm_async", "gemm_lowprec", "lowprec_gemm_calls", "bdsdc_stats", "sturm_count", "stebz_stats", "stein_stats", "symv_lower", "hetrd_stats", "gebrd_stats", "geqp3_stats", "gemv_t_block", "gemv_n_block", "herk", "gemm_tri", "gemm_variant_counts", "trsm", "potrf", "getrf_panel", "geqrf_panel", "lu_sign",
           "set_queue", "queue_sync"]


def set_queue(q: int):
    """HIP queue of the calls below (0 default; 1 = the high-priority panel queue)."""
    _slate.set_ops_queue(q)


def queue_sync(q: int):
    _slate.queue_sync(q)


def have_native_ops() -> bool:
    return hasattr(_slate, "lb_gemm_d")


def _suffix(t):
    import torch
    return {torch.float32: "s", torch.float64: "d", torch.complex64: "c", torch.complex128: "z"}[t.dtype]


def _cm(t):
    """(ptr, m, n, ld) of a torch tensor viewed as a column-major matrix:
    a row-major (n x m) contiguous tensor is an m x n column-major matrix.
    Synchronizes torch's stream first: the native kernels run on the
    framework's own HIP queues."""
    import torch
    assert t.dim() == 2 and t.stride(1) == 1, "row-major contiguous rows expected"
    if t.is_cuda:
        # torch's own stream only: a device-wide synchronize would also wait
        # for work queued on the framework's queues (e.g. gemm_async)
        torch.cuda.current_stream(t.device).synchronize()
    ptr = t.data_ptr()
    if t.numel() == 0:
        # torch reports a null pointer for an empty view; pass where the view
        # lies in its allocation, as for any other operand
        ptr = t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()
    return ptr, t.shape[1], t.shape[0], t.stride(0)


def gemm(opA: str, opB: str, alpha, A, B, beta, C):
    """Column-major C = alpha op(A) op(B) + beta C on the device, where a
    row-major torch tensor X (r x c) represents the column-major c x r matrix X^T."""
    fn = getattr(_slate, f"lb_gemm_{_suffix(C)}")
    pa, ma, na, lda = _cm(A)
    pb, mb, nb, ldb = _cm(B)
    pc, mc, nc, ldc = _cm(C)
    k = na if opA == "N" else ma
    fn(opA, opB, mc, nc, k, alpha, pa, lda, pb, ldb, beta, pc, ldc)


def gemm_lowprec(mode: str, opA: str, opB: str, alpha, A, B, beta, C, uplo: str = "G"):
    """gemm on float32 tensors by the split-operand bf16 MFMA kernel: mode
    "bf16", "bf16x3" or "bf16x6" (1, 3 or 6 bf16 plane products per K-step,
    fp32 accumulation).  uplo "L" / "U" updates only that triangle of a
    square C.  Conventions of gemm."""
    import torch
    assert A.dtype == B.dtype == C.dtype == torch.float32, "float32 tensors expected"
    pa, ma, na, lda = _cm(A)
    pb, mb, nb, ldb = _cm(B)
    pc, mc, nc, ldc = _cm(C)
    k = na if opA == "N" else ma
    _slate.lb_gemm_lowprec(mode, uplo, opA, opB, mc, nc, k, float(alpha), pa, lda, pb, ldb, float(beta), pc, ldc)


def lowprec_gemm_calls() -> int:
    """Launches of the split-operand bf16 kernel in this process so far."""
    return _slate.lowprec_gemm_calls()


def bdsdc_stats() -> dict:
    """Counters of the last bidiagonal divide and conquer of this process
    (bdsdc, or svd with method_svd="dc"): merges, merged and deflated columns
    (in all and per tree level, root first) and the launches of the three
    device kernels (zero on the host target)."""
    return _slate.bdsdc_stats()


def sturm_count(d, e, x, target=None):
    """N(x_j), the number of eigenvalues of the symmetric tridiagonal (d, e)
    below each shift x_j (int64 ndarray): the raw count kernel that stebz and
    bdsbz refine with, one lane per shift on target="d", the same recurrence
    (csrc/include/slate_amd/sturm.hh) on the host targets.  float32 / float64
    after d."""
    import numpy as np
    from .._core import opts
    d = np.asarray(d)
    t = "s" if d.dtype == np.float32 else "d"
    as_list = lambda a: np.asarray(a).astype(np.float64).ravel().tolist()
    return _slate.sturm_count(t, as_list(d), as_list(e), as_list(x), opts(target))


def stein_stats() -> dict:
    """Counters of the last stein of this process (also through heevx): `n`,
    `values` (vectors), `clusters` and `largest_cluster`, `rounds` (always
    five), `failed` (vectors that never passed the growth test), `launches`
    and `host_syncs` (both zero on the host targets); with
    SLATE_STEIN_PROFILE=1 in the environment also `ms_solve`, `ms_orth` and
    `ms_transpose`, the device time by kernel."""
    from .. import _slate
    return _slate.stein_stats()


def stebz_stats() -> dict:
    """Counters of the last stebz / bdsbz of this process (also through heev /
    svd_vals with method_eig / method_svd "bisection"): `n` the order of the
    tridiagonal counted on (2n for bdsbz), `values` returned, `points` P per
    eigenvalue and step (1 on the host; chosen from n and the device's CU
    count, SLATE_STEBZ_POINTS overrides), `steps` the most any value took,
    `launches` (1, or 2 for a range by value; 0 on the host) and `host_syncs`
    (1 on the device)."""
    return _slate.stebz_stats()


def hetrd_stats() -> dict:
    """Counters of the last one-stage tridiagonal reduction of this process
    (hetrd, or heev with method_hetrd="one_stage"): `columns`, `panels`,
    `host_syncs` inside the reduction and the launches of its four column
    kernels, launches_column / _larfg / _symv / _correct (zero on the host
    target).  ms_symv / ms_panel / ms_syr2k / ms_larft are device milliseconds
    from events between the kernels, recorded only when SLATE_HETRD_PROFILE=1
    is in the environment (zero otherwise)."""
    return _slate.hetrd_stats()


def symv_lower(A, x, offset: int = 0, repeat: int = 1):
    """y = S x on the device, S the symmetric block of the column-major matrix
    A that starts at (offset, offset), read from its lower triangle only: the
    strict upper triangle is never loaded.  float32 or float64; returns y
    (order of A less offset).  Two calls give the same bits.  repeat > 1
    enqueues the same product that many times before the one synchronisation
    (timing)."""
    import torch
    pa, rows, cols, lda = _cm(A)
    m = cols - offset
    assert 0 <= offset and m >= 0 and rows >= cols and x.numel() == m and x.dtype == A.dtype and x.is_contiguous()
    if x.is_cuda:
        torch.cuda.current_stream(x.device).synchronize()
    y = torch.empty(m, dtype=A.dtype, device=A.device)
    torch.cuda.current_stream(A.device).synchronize()
    if m > 0:
        _slate.lb_symv_lower(_suffix(A), m, pa + (offset + offset * lda) * A.element_size(), lda, x.data_ptr(),
                             y.data_ptr(), repeat)
    return y


def gebrd_stats() -> dict:
    """Counters of the last one-stage bidiagonal reduction of this process
    (gebrd, or svd with method_gebrd="one_stage"): `columns`, `panels`,
    `host_syncs` inside the reduction and the launches of its seven column
    kernels, launches_column / _larfg_u / _pass1 / _finish_y / _larfg_v /
    _pass2 / _finish_x (zero on the host target).  ms_pass1 / ms_pass2 /
    ms_panel / ms_gemm / ms_larft are device milliseconds from events between
    the kernels, recorded only when SLATE_GEBRD_PROFILE=1 is in the environment
    (zero otherwise)."""
    return _slate.gebrd_stats()


def geqp3_stats() -> dict:
    """Counters of the last QR with column pivoting of this process (geqp3, or
    gelsy): `columns`, `panels`, `host_syncs` inside the factorization,
    `norm_recomputes` (the columns whose norm was recomputed inside a panel,
    counted on the device) and the launches of its kernels, launches_norms /
    _pivot / _swap / _column / _larfg / _product / _finish / _recompute (zero
    on the host target).  ms_pivot / ms_product / ms_panel / ms_gemm / ms_larft
    are device milliseconds from events between the kernels, recorded only when
    SLATE_GEQP3_PROFILE=1 is in the environment (zero otherwise)."""
    return _slate.geqp3_stats()


def _gemv_block(trans, A, x, row_offset, col_offset, repeat, use_lb):
    import torch
    pa, rows, cols, lda = _cm(A)
    mr, nc = rows - row_offset, cols - col_offset
    assert 0 <= row_offset and 0 <= col_offset and mr >= 0 and nc >= 0
    assert x.numel() == (mr if trans else nc) and x.dtype == A.dtype and x.is_contiguous()
    if x.is_cuda:
        torch.cuda.current_stream(x.device).synchronize()
    y = torch.empty(nc if trans else mr, dtype=A.dtype, device=A.device)
    torch.cuda.current_stream(A.device).synchronize()
    if mr > 0 and nc > 0:
        _slate.lb_gemv_block(_suffix(A), trans, mr, nc, pa + (row_offset + col_offset * lda) * A.element_size(), lda,
                             x.data_ptr(), y.data_ptr(), repeat, use_lb)
    else:
        y.zero_()
    return y


def gemv_t_block(A, x, row_offset: int = 0, col_offset: int = 0, repeat: int = 1, use_lb: bool = False):
    """y = B^T x on the device, B the block of the column-major matrix A that
    starts at (row_offset, col_offset) and runs to its last row and column:
    pass 1 of the one-stage bidiagonal reduction.  Nothing outside the block
    is loaded.  float32 or float64; two calls give the same bits.  repeat > 1
    enqueues the same product that many times before the one synchronisation
    (timing); use_lb=True runs lb::gemv instead (the yardstick)."""
    return _gemv_block(True, A, x, row_offset, col_offset, repeat, use_lb)


def gemv_n_block(A, x, row_offset: int = 0, col_offset: int = 0, repeat: int = 1, use_lb: bool = False):
    """y = B x on the device, B as in gemv_t_block: pass 2 of the one-stage
    bidiagonal reduction."""
    return _gemv_block(False, A, x, row_offset, col_offset, repeat, use_lb)


def gemm_async(queue: int, opA: str, opB: str, alpha, A, B, beta, C):
    """gemm launched on `queue` without waiting for it (queue_sync(queue))."""
    fn = getattr(_slate, f"lb_gemm_async_{_suffix(C)}")
    pa, ma, na, lda = _cm(A)
    pb, mb, nb, ldb = _cm(B)
    pc, mc, nc, ldc = _cm(C)
    k = na if opA == "N" else ma
    fn(queue, opA, opB, mc, nc, k, alpha, pa, lda, pb, ldb, beta, pc, ldc)


def herk(uplo: str, op: str, alpha, A, beta, C):
    fn = getattr(_slate, f"lb_herk_{_suffix(C)}")
    pa, ma, na, lda = _cm(A)
    pc, n, _, ldc = _cm(C)
    k = na if op == "N" else ma
    fn(uplo, op, n, k, alpha, pa, lda, beta, pc, ldc)


def gemm_tri(uplo: str, opA: str, opB: str, alpha, A, B, beta, C):
    """The uplo ("L" / "U") triangle of the square C = alpha op(A) op(B) + beta C;
    the other triangle is not touched.  Conventions of gemm."""
    fn = getattr(_slate, f"lb_gemm_tri_{_suffix(C)}")
    pa, ma, na, lda = _cm(A)
    pb, mb, nb, ldb = _cm(B)
    pc, n, _, ldc = _cm(C)
    k = na if opA == "N" else ma
    fn(uplo, opA, opB, n, k, alpha, pa, lda, pb, ldb, beta, pc, ldc)


def gemm_variant_counts() -> dict:
    """Launches so far in this process of each native GEMM variant, by name.
    Real kernels: <s|d>_a<m|k>_b<n|k>_<BM>x<BN>_w<waves>_<rot|plain>_<G|L|U|S>_
    <ionly|checked> (a / b: the contiguous dimension of the stored operand;
    G general, L / U triangular, S staircase store); complex kernels:
    <c|z>_<opA><opB>_64x64_w4_<G|L|U>_<full|checked>; dispatcher routes:
    splitk, splitk_tri, pack_b_nt, pack_a_tn, gemv.  Names that never launched
    may be absent."""
    return _slate.gemm_variant_counts()


def trsm(side: str, uplo: str, op: str, diag: str, alpha, A, B):
    fn = getattr(_slate, f"lb_trsm_{_suffix(B)}")
    pa, _, _, lda = _cm(A)
    pb, m, n, ldb = _cm(B)
    fn(side, uplo, op, diag, m, n, alpha, pa, lda, pb, ldb)


def potrf(uplo: str, A):
    fn = getattr(_slate, f"lb_potrf_{_suffix(A)}")
    pa, n, _, lda = _cm(A)
    return fn(uplo, n, pa, lda)


def getrf_panel(A, tournament: bool = False):
    """LU of a column-major m x n panel; returns (info, ipiv).  Partial pivoting
    per column, or tournament (CALU) pivoting per 32-column block."""
    fn = getattr(_slate, f"lb_getrf_panel_{_suffix(A)}")
    pa, m, n, lda = _cm(A)
    return fn(m, n, pa, lda, tournament)


def geqrf_panel(A):
    """Householder QR of a column-major m x n panel; returns (tau, T) as torch tensors."""
    fn = getattr(_slate, f"lb_geqrf_panel_{_suffix(A)}")
    pa, m, n, lda = _cm(A)
    return fn(m, n, pa, lda)


def lu_sign(A):
    """Sign-modified LU without pivoting of a column-major n x n block in
    place (the Householder reconstruction step of the CholeskyQR / TSQR QR
    panels, lu_dist.cc): L U = A + diag(s), s_k = the unit phase of the k-th
    pivot; returns s."""
    fn = getattr(_slate, f"lb_lu_sign_{_suffix(A)}")
    pa, m, n, lda = _cm(A)
    return fn(n, pa, lda)
