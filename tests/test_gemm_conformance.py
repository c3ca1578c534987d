"""Conformance of every native GEMM variant (gemm_mfma.hip, gemm_cplx.hip and the
dispatcher in local_blas.cc) against exact and high-precision references.

Every operand is a view into a larger NaN-filled allocation (class Mat): an
over-read shows as NaN in the result, a stray store as a changed guard element.
Exact tests use integer data, for which any correct kernel returns the reference
bit for bit; rounding tests use uniform data and an elementwise bound.  The
shapes are the smallest that reach each variant of the dispatcher, and the last
GPU test checks with the launch counters (ops.gemm_variant_counts) that the
sweep reached every name in EXPECTED_VARIANTS.

Variants the sweep leaves out on purpose:
  * the staircase 'S' store (gemm_stair_real): it needs the block-cyclic tile
    table of the distributed Cholesky update, which has its own driver tests;
  * batched launches other than those split-K makes (trtri_blocks): no raw
    entry point; they run the same instantiations as the single launches.

The harness itself is tested without a GPU: numpy's own product passes every
check, and five single mutations of it are each reported.
"""
import functools
import os

import numpy as np
import pytest

import slate_d35_amd as s

DTYPES = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
REAL_OPS = [("N", "N"), ("N", "T"), ("T", "N"), ("T", "T")]
CPLX_OPS = [(a, b) for a in "NTC" for b in "NTC"]
GUARD = 256                     # guard band: 256 columns and 256 rows around every view
ALL_LD = ("tight", "padded", "odd_ld", "odd_ptr")
ALIGNED_LD = ("tight", "padded")
# large shapes: the unaligned class alternates between its two forms over the op pairs
BIG_LD = ("tight", "padded", "unaligned")


def _cplx(t):
    return t in "cz"


def _ops(t):
    return CPLX_OPS if _cplx(t) else REAL_OPS


def _scalars(t):
    """alpha, beta that keep integer data exact; both complex ones have an imaginary part"""
    return (1 + 2j, -2 + 1j) if _cplx(t) else (0.5, -2.0)


# ---------------------------------------------------------------- operands
def _layout(rows, cls):
    """(leading dimension, element offset of the base from a 16-byte boundary)"""
    if cls == "tight":
        return max(rows, 1), 0
    if cls == "padded":
        return (rows + 15) // 16 * 16 + 16, 0
    if cls == "odd_ld":
        return rows + 3, 0
    if cls == "odd_ptr":            # aligned leading dimension, base one element off
        return (rows + 15) // 16 * 16 + 16, 1
    raise ValueError(cls)


class Mat:
    """A column-major rows x cols matrix as a view into a 1-D allocation filled
    with NaN: a guard band of 256 columns and 256 rows before and after, and the
    leading-dimension padding between the columns."""

    def __init__(self, data, cls):
        self.rows, self.cols = data.shape
        self.ld, shift = _layout(self.rows, cls)
        guard = (GUARD * self.ld + GUARD + 15) // 16 * 16
        self.lo = guard + shift
        self.hi = self.lo + self.cols * self.ld
        nan = complex(np.nan, np.nan) if np.iscomplexobj(data) else np.nan
        self.buf = np.full(self.hi + guard, nan, data.dtype)
        self.view(self.buf)[...] = data

    def view(self, buf):
        """the rows x cols matrix inside buf (this allocation, or a copy of it)"""
        return buf[self.lo:self.hi].reshape(self.cols, self.ld)[:, :self.rows].T

    def _outside(self, buf):
        pad = buf[self.lo:self.hi].reshape(self.cols, self.ld)[:, self.rows:]
        return [np.ascontiguousarray(x).view(np.uint8) for x in (buf[:self.lo], buf[self.hi:], pad)]

    def check_untouched(self, after):
        """guard bands and padding of `after` are bit-identical to the allocation's"""
        assert after.shape == self.buf.shape
        for name, x, y in zip(("guard before", "guard after", "ld padding"), self._outside(after),
                              self._outside(self.buf)):
            assert np.array_equal(x, y), f"store outside C: {name} changed"


def _op(op, x):
    return x if op == "N" else x.T if op == "T" else x.conj().T


def _stored(op, x):
    """the array as stored so that op(stored) = x"""
    return _op(op, x)


def _tri_mask(n, uplo):
    return np.tri(n, dtype=bool) if uplo == "L" else np.tri(n, dtype=bool).T


@functools.lru_cache(maxsize=4)
def _operands(t, m, n, k, data, herk=False):
    """op(A) m x k, op(B) k x n and C0 m x n: integers in [-8, 8] ("int") or
    uniform(-1, 1) ("uniform"); herk: op(B) = op(A)^H, Im C0(i,i) != 0"""
    rng = np.random.default_rng(1000003 * m + 1009 * n + k + (7 if herk else 0))

    def part(r, c):
        return rng.integers(-8, 9, (r, c)).astype(np.float64) if data == "int" else rng.uniform(-1, 1, (r, c))

    def draw(r, c):
        x = part(r, c) + 1j * part(r, c) if _cplx(t) else part(r, c)
        return x.astype(DTYPES[t])

    a, b, c0 = draw(m, k), draw(k, n), np.asfortranarray(draw(m, n))
    if herk:
        b = np.ascontiguousarray(a.conj().T)
        if _cplx(t):
            d = np.arange(m)
            c0.imag[d, d] = np.where(c0.imag[d, d] == 0, 3, c0.imag[d, d])
    for x in (a, b, c0):
        x.setflags(write=False)
    return a, b, c0


def _high(t, data):
    """reference precision: exact integer sums fit fp64; otherwise fp64 for the
    32-bit types and long double for the 64-bit ones"""
    if data == "int" or t in "sc":
        return np.complex128 if _cplx(t) else np.float64
    return np.clongdouble if _cplx(t) else np.longdouble


@functools.lru_cache(maxsize=4)
def _reference(t, m, n, k, data, alpha, beta, herk=False):
    """alpha op(A) op(B) + beta C0 in the reference precision (herk: real
    diagonal), and for uniform data scale = |alpha| |op A||op B| + |beta| |C0|"""
    a, b, c0 = _operands(t, m, n, k, data, herk)
    hp = _high(t, data)
    ah, bh, ch = a.astype(hp), b.astype(hp), c0.astype(hp)
    ref = hp(alpha) * (ah @ bh)
    if beta != 0:
        ref = ref + hp(beta) * ch
    if herk and _cplx(t):
        d = np.arange(m)
        ref.imag[d, d] = 0
    ref = np.asfortranarray(ref)
    scale = None
    if data == "uniform":
        mod = [np.abs(x).astype(np.float64) for x in (a, b, c0)]        # fp64 is ample for the bound's scale
        scale = np.asfortranarray(abs(alpha) * (mod[0] @ mod[1]) + abs(beta) * mod[2])
    return ref, scale


# ---------------------------------------------------------------- checks
def _same(x, y):
    return np.array_equal(x, y) or np.array_equal(x, y, equal_nan=True)


def _where(bad):
    idx = np.argwhere(bad)
    return f"{len(idx)} elements differ, first at {idx[:4].tolist()}"


def check_result(got, c_init, ref, scale, mode, t, k, uplo="G"):
    """mode "exact": got == ref bit for bit; "rounding": |got - ref| <= c (k + 72)
    u scale elementwise, c = 1 (real) or 2 (complex), u = 2^-24 or 2^-53: k terms
    of a dot product, up to 64 split-K partials, the alpha / beta epilogue, and
    sqrt(2) for the four-chain complex product.  A triangular store is checked
    on its triangle; the other one keeps its contents.  Returns the largest
    error / bound (0 for exact)."""
    if uplo != "G":
        mask = _tri_mask(got.shape[0], uplo)
        assert _same(got[~mask], c_init[~mask]), "store outside the triangle: " + _where(
            (got != c_init) & ~(np.isnan(got) & np.isnan(c_init)) & ~mask)
        got, ref = got[mask], ref[mask]
        scale = None if scale is None else scale[mask]
    if mode == "exact":
        assert _same(got, ref), _where(got != ref)
        return 0.0
    u = 2.0 ** -24 if t in "sc" else 2.0 ** -53
    c = 2 if _cplx(t) else 1
    err = np.abs(got.astype(ref.dtype) - ref)
    bound = c * (k + 72) * u * scale
    ratio = float(np.max(err / bound)) if err.size else 0.0
    assert not np.isnan(err).any() and np.all(err <= bound), f"max err/bound {ratio:.3f}; " + _where(~(err <= bound))
    return ratio


def run_case(kernel, t, kind, ta, tb, m, n, k, cls, mode="exact", uplo="G", beta0=False):
    """One product through `kernel` on padded views, checked against the
    reference.  kind "gemm", "gemm_tri" (triangle uplo of a square C) or "herk"
    (C = alpha op(A) op(A)^H + beta C with real alpha, beta; op = ta).  beta0:
    beta = 0 on a C filled with NaN."""
    herk = kind == "herk"
    data = "int" if mode == "exact" else "uniform"
    alpha, beta = (0.5, -2.0) if herk else _scalars(t)
    if beta0:
        beta = 0.0
    a, b, c0 = _operands(t, m, n, k, data, herk)
    ref, scale = _reference(t, m, n, k, data, alpha, beta, herk)
    c_init = c0
    if beta0:
        c_init = np.full_like(c0, complex(np.nan, np.nan) if _cplx(t) else np.nan)
    A = Mat(_stored(ta, a), cls)
    B = None if herk else Mat(_stored(tb, b), cls)
    C = Mat(c_init, cls)
    call = dict(kind=kind, ta=ta, tb=tb, alpha=alpha, beta=beta, uplo=uplo)
    after = kernel(call, A, B, C)
    try:
        C.check_untouched(after)
        return check_result(C.view(after), c_init, ref, scale, mode, t, k, uplo)
    except AssertionError as e:
        raise AssertionError(f"{t} {kind} {ta}{tb} {uplo} {(m, n, k)} {cls} beta0={beta0}: {e}") from None


# ---------------------------------------------------------------- kernels
def numpy_kernel(call, A, B, C):
    """the stand-in kernel of the CPU self-test: numpy's product in the working
    precision on the same padded views; returns the allocation of C afterwards"""
    out = C.buf.copy()
    dt = out.dtype.type
    a = A.view(A.buf)
    if call["kind"] == "herk":
        opa = _op("N" if call["ta"] == "N" else "C", a)
        opb = opa.conj().T
    else:
        opa, opb = _op(call["ta"], a), _op(call["tb"], B.view(B.buf))
    c = C.view(out)
    full = dt(call["alpha"]) * (opa @ opb)
    if call["beta"] != 0:
        full = full + dt(call["beta"]) * c
    if call["kind"] == "herk" and np.iscomplexobj(full):
        d = np.arange(full.shape[0])
        full.imag[d, d] = 0
    c[...] = full if call["uplo"] == "G" else np.where(_tri_mask(full.shape[0], call["uplo"]), full, c)
    return out


def _torch():
    import torch
    return torch


def gpu_kernel(call, A, B, C):
    """the native kernels through s.ops on device copies of the allocations"""
    torch = _torch()

    def dev(M):
        return torch.from_numpy(M.buf).cuda()

    def view(M, buf):       # row-major (cols x rows) tensor = the column-major matrix
        return buf[M.lo:M.hi].view(M.cols, M.ld)[:, :M.rows]

    tA, tC = dev(A), dev(C)
    if call["kind"] == "herk":
        s.ops.herk(call["uplo"], call["ta"], call["alpha"], view(A, tA), call["beta"], view(C, tC))
    else:
        tB = dev(B)
        if call["kind"] == "gemm":
            s.ops.gemm(call["ta"], call["tb"], call["alpha"], view(A, tA), view(B, tB), call["beta"], view(C, tC))
        else:
            s.ops.gemm_tri(call["uplo"], call["ta"], call["tb"], call["alpha"], view(A, tA), view(B, tB),
                           call["beta"], view(C, tC))
    return tC.cpu().numpy()


# ---------------------------------------------------------------- CPU self-test of the harness
SELF_SHAPES = [(130, 67, 24), (64, 64, 0), (33, 65, 17)]


@pytest.mark.parametrize("t", "sdcz")
def test_harness_accepts_reference_product(t):
    """numpy's own product in the working precision passes the exact and the
    rounding test on every layout class: the reference machinery, the data and
    the constants leave room for a correct kernel."""
    for (m, n, k) in SELF_SHAPES:
        for cls in ALL_LD:
            for ta, tb in _ops(t):
                run_case(numpy_kernel, t, "gemm", ta, tb, m, n, k, cls)
                run_case(numpy_kernel, t, "gemm", ta, tb, m, n, k, cls, beta0=True)
                r = run_case(numpy_kernel, t, "gemm", ta, tb, m, n, k, cls, mode="rounding")
                assert r <= 1.0
    for uplo in "LU":
        for op in ("N", "C"):
            run_case(numpy_kernel, t, "herk", op, op, 65, 65, 17, "padded", uplo=uplo)
            run_case(numpy_kernel, t, "herk", op, op, 65, 65, 17, "odd_ld", mode="rounding", uplo=uplo)
        run_case(numpy_kernel, t, "gemm_tri", "N", "T", 65, 65, 17, "padded", uplo=uplo)


def _mutations(t):
    """name -> (stand-in kernel with one defect, run_case arguments)"""
    alpha = _scalars(t)[0]

    def one_element(call, A, B, C):
        out = numpy_kernel(call, A, B, C)
        C.view(out)[77, 41] += 1
        return out

    def dropped_slice(call, A, B, C):         # k-slice 5 missing in the 16 x 16 block at (64, 32)
        out = numpy_kernel(call, A, B, C)
        opa, opb = _op(call["ta"], A.view(A.buf)), _op(call["tb"], B.view(B.buf))
        C.view(out)[64:80, 32:48] -= out.dtype.type(alpha) * np.outer(opa[64:80, 5], opb[5, 32:48])
        return out

    def padding_store(call, A, B, C):         # C(m, 0): the first element of the ld padding
        out = numpy_kernel(call, A, B, C)
        out[C.lo + C.rows] = 0
        return out

    def guard_store(call, A, B, C):           # one element before C(0, 0)
        out = numpy_kernel(call, A, B, C)
        out[C.lo - 1] = 0
        return out

    def swapped(call, A, B, C):
        return numpy_kernel(call, B, A, C)

    def conj_alpha(call, A, B, C):
        return numpy_kernel(dict(call, alpha=np.conj(call["alpha"])), A, B, C)

    gemm = ("gemm", "N", "T", 130, 67, 24, "padded")
    muts = {
        "one element off by 1": (one_element, gemm, {}),
        "k-slice dropped in a 16x16 block": (dropped_slice, gemm, {}),
        "k-slice dropped, uniform data": (dropped_slice, gemm, dict(mode="rounding")),
        "store into the ld padding": (padding_store, gemm, {}),
        "store into the guard band": (guard_store, ("gemm", "N", "T", 130, 67, 24, "tight"), {}),
        "triangular operands swapped": (swapped, ("gemm_tri", "N", "T", 65, 65, 17, "padded"), dict(uplo="L")),
    }
    if _cplx(t):
        muts["Im alpha negated"] = (conj_alpha, gemm, {})
        muts["triangular operands swapped (N, C)"] = (swapped, ("gemm_tri", "N", "C", 65, 65, 17, "padded"),
                                                      dict(uplo="U"))
    return muts


@pytest.mark.parametrize("t", "sdcz")
def test_harness_detects_mutations(t):
    """Each single defect planted in the stand-in kernel is reported."""
    for name, (kernel, args, kw) in _mutations(t).items():
        run_case(numpy_kernel, t, *args, **kw)            # the unmutated kernel passes the same case
        with pytest.raises(AssertionError):
            run_case(kernel, t, *args, **kw)
        print(f"{t}: detected: {name}")


def test_expected_variants_are_distinct():
    assert len(set(EXPECTED_VARIANTS)) == len(EXPECTED_VARIANTS) == 181


# ---------------------------------------------------------------- variants
# Names as launch_tile / launch_cplx / dgemm / gemm build them (ops.gemm_variant_counts).
# Read against launch_gemm: 64 x 64 tiles (4 waves) below 128 tiles of 128^2,
# any mask; 128 x 128 otherwise, where a general fp64 store with a K-contiguous
# operand takes 8 waves (rotated for TN only) and everything else 4 waves;
# 256 x 128 for large general fp32.  The default pipeline is rotated for fp64
# and plain for fp32.  Operand pairs a<m|k>_b<n|k>: NN, NT, TN, TT.
_PAIRS = ("am_bk", "am_bn", "ak_bk", "ak_bn")
_KINDS = ("checked", "ionly")
EXPECTED_VARIANTS = (
    [f"{t}_{p}_64x64_w4_{pipe}_{u}_{kind}"
     for t, pipe in (("s", "plain"), ("d", "rot")) for p in _PAIRS for u in "GLU" for kind in _KINDS]
    + [f"s_{p}_128x128_w4_plain_{u}_{kind}" for p in _PAIRS for u in "GLU" for kind in _KINDS]
    + [f"d_{p}_128x128_w4_rot_{u}_{kind}" for p in _PAIRS for u in "LU" for kind in _KINDS]
    + [f"d_{v}_G_{kind}" for v in ("am_bn_128x128_w4_rot", "am_bk_128x128_w8_plain", "ak_bk_128x128_w8_rot",
                                   "ak_bn_128x128_w8_plain") for kind in _KINDS]
    + [f"s_{p}_256x128_w8_plain_G_{kind}" for p in _PAIRS for kind in _KINDS]
    + [f"{t}_{a}{b}_64x64_w4_G_{kind}" for t in "cz" for a, b in CPLX_OPS for kind in ("checked", "full")]
    + [f"{t}_{a}{b}_64x64_w4_{u}_checked" for t in "cz" for a, b in CPLX_OPS for u in "LU"]
    + ["splitk", "splitk_tri", "pack_b_nt", "pack_a_tn", "gemv"]
)
_SEEN = set()


@pytest.fixture(autouse=True)
def _record_variants(request):
    """the variants each GPU test of this module launched, for the coverage test"""
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    before = s.ops.gemm_variant_counts()
    yield
    _SEEN.update(name for name, c in s.ops.gemm_variant_counts().items() if c > before.get(name, 0))


def _sweep(t, kind, shapes, classes, ops=None, uplos=("G",), mode="exact", beta0=False):
    worst = 0.0
    for (m, n, k) in shapes:
        for uplo in uplos:
            for i, (ta, tb) in enumerate(ops or _ops(t)):
                for cls in classes:
                    if cls == "unaligned":
                        cls = ("odd_ld", "odd_ptr")[i % 2]
                    r = run_case(gpu_kernel, t, kind, ta, tb, m, n, k, cls, mode=mode, uplo=uplo, beta0=beta0)
                    worst = max(worst, r)
    if mode == "rounding":
        print(f"{t} {kind} {shapes}: max err/bound {worst:.3f}")
    return worst


K_EDGES = (0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 48)
MN_EDGES = ((300, 257), (1, 17), (17, 1), (65, 63), (129, 16), (129, 17))
HERK_OPS = (("N", "N"), ("C", "C"))       # herk takes one op; the pair keeps _sweep's shape


# ---------------------------------------------------------------- real kernels, exact
@pytest.mark.gpu
@pytest.mark.parametrize("t", "sd")
def test_real_tile64_checked(t):
    """64 x 64 tile, bounds-checked: every edge class of m, n and k, every
    layout (n <= 16 with op(B) = N goes to gemv)."""
    _sweep(t, "gemm", [(m, n, k) for (m, n) in MN_EDGES for k in K_EDGES], ALL_LD)


@pytest.mark.gpu
@pytest.mark.parametrize("t", "sd")
def test_real_tile64_interior(t):
    _sweep(t, "gemm", [(256, 256, k) for k in (16, 32, 48)], ALIGNED_LD)


@pytest.mark.gpu
@pytest.mark.parametrize("t", "sd")
def test_real_tile128(t):
    """128 x 128 tiles (132 of them: edge tiles, a last row group of 3, a block
    count = 4 mod 8); fp64: the 4-wave rotated tile for NT, 8 waves otherwise."""
    _sweep(t, "gemm", [(1400, 1500, 24), (1400, 1500, 33)], BIG_LD)
    _sweep(t, "gemm", [(1408, 1536, 32)], ALIGNED_LD)


@pytest.mark.gpu
def test_real_tile256_checked():
    """fp32 256 x 128 tiles (m >= 512 and 512 tiles)"""
    _sweep("s", "gemm", [(4000, 4090, 24)], BIG_LD)


@pytest.mark.gpu
def test_real_tile256_interior():
    _sweep("s", "gemm", [(4096, 4096, 32)], ALIGNED_LD)


@pytest.mark.gpu
@pytest.mark.parametrize("t", "sd")
def test_real_splitk(t):
    """fewer than 128 tiles and k >= 1024: K slices of one batched launch (with
    and without a remainder chunk) and the in-order reduction"""
    _sweep(t, "gemm", [(m, n, k) for (m, n) in ((200, 96), (130, 130)) for k in (1024, 1030, 4100)],
           ("padded", "odd_ld", "odd_ptr"))


@pytest.mark.gpu
@pytest.mark.parametrize("t", "sd")
def test_real_splitk_triangular(t):
    """herk of a tall panel: split-K into scratch, then the triangle merged by geadd"""
    _sweep(t, "herk", [(300, 300, 5000)], ("padded", "odd_ld"), ops=HERK_OPS, uplos="LU")


@pytest.mark.gpu
@pytest.mark.parametrize("t", "sd")
def test_real_triangular_tile64(t):
    """triangular store on the 64 x 64 tile with A != B, all four op pairs, and herk"""
    shapes = [(n, n, k) for n in (65, 333) for k in (17, 97)]
    _sweep(t, "gemm_tri", shapes, ALL_LD, uplos="LU")
    _sweep(t, "herk", shapes, ("padded", "odd_ld"), ops=HERK_OPS, uplos="LU")
    _sweep(t, "gemm_tri", [(256, 256, 32)], ALIGNED_LD, uplos="LU")


@pytest.mark.gpu
@pytest.mark.parametrize("t", "sd")
def test_real_triangular_tile128(t):
    """136 triangle tiles of 128^2 (n >= 1921)"""
    _sweep(t, "gemm_tri", [(1930, 1930, 24)], BIG_LD, uplos="LU")
    _sweep(t, "gemm_tri", [(2048, 2048, 32)], ALIGNED_LD, uplos="LU")


@pytest.mark.gpu
def test_fp64_nn_as_nt_on_packed_b():
    """m >= 4096, n >= 1024, 256 <= k <= 2048: NT on a transposed copy of B"""
    _sweep("d", "gemm", [(4160, 1100, 256), (4160, 1100, 257)], ALL_LD, ops=[("N", "N")])


@pytest.mark.gpu
def test_fp64_nn_as_tn_on_packed_a():
    """k > 2048, m, n >= 4096: TN on a transposed copy of A; an odd slice length
    gives an unaligned packed operand, and a small SLATE_GEMM_PACK_BYTES two slices"""
    shape = [(4100, 4100, 2065)]
    _sweep("d", "gemm", shape, BIG_LD, ops=[("N", "N")])
    old = os.environ.get("SLATE_GEMM_PACK_BYTES")
    os.environ["SLATE_GEMM_PACK_BYTES"] = "1"           # slices of the minimum, 2048: 2048 + 17
    try:
        _sweep("d", "gemm", shape, ("odd_ptr",), ops=[("N", "N")])
    finally:
        if old is None:
            del os.environ["SLATE_GEMM_PACK_BYTES"]
        else:
            os.environ["SLATE_GEMM_PACK_BYTES"] = old


@pytest.mark.gpu
@pytest.mark.parametrize("t", "sd")
def test_real_gemv_boundary(t):
    """n = 16 (gemv kernels when op(B) = N) against n = 17 (MFMA tile)"""
    _sweep(t, "gemm", [(300, 16, 129), (300, 17, 129)], ALL_LD)


# ---------------------------------------------------------------- complex kernel, exact
CPLX_LD = ("tight", "padded", "odd_ld")         # alignment plays no part in launch_cplx


@pytest.mark.gpu
@pytest.mark.parametrize("t", "cz")
def test_complex_checked(t):
    """all nine op pairs with alpha and beta that have imaginary parts, every
    edge class of k against the 8-wide K-tile"""
    _sweep(t, "gemm", [(m, n, k) for (m, n) in ((130, 67), (1, 65), (65, 1)) for k in (0, 1, 7, 8, 9, 16, 17, 24)],
           CPLX_LD)


@pytest.mark.gpu
@pytest.mark.parametrize("t", "cz")
def test_complex_full(t):
    _sweep(t, "gemm", [(128, 192, k) for k in (8, 16, 24)], CPLX_LD)


@pytest.mark.gpu
@pytest.mark.parametrize("t", "cz")
def test_complex_triangular(t):
    """triangular store with A != B for every op pair, and herk (real diagonal)"""
    shapes = [(n, n, k) for n in (65, 200) for k in (9, 24)]
    _sweep(t, "gemm_tri", shapes, ("padded", "odd_ld"), uplos="LU")
    _sweep(t, "herk", shapes, CPLX_LD, ops=HERK_OPS, uplos="LU")


# ---------------------------------------------------------------- rounding
@pytest.mark.gpu
@pytest.mark.parametrize("t", "sd")
def test_rounding_real(t):
    """uniform(-1, 1) data, elementwise |err| <= (k + 72) u scale, on the 64 x 64
    tile, the 128 x 128 tiles (fp64: 4 and 8 waves, plain and rotated), the
    fp32 256 x 128 tile, split-K and the triangular store: an accumulation in
    the wrong precision, which integer data cannot show."""
    _sweep(t, "gemm", [(300, 257, 129)], ("odd_ld",), mode="rounding")
    _sweep(t, "gemm", [(1400, 1500, 33)], ("padded",), mode="rounding")
    _sweep(t, "gemm", [(200, 96, 4100)], ("padded",), mode="rounding")
    _sweep(t, "gemm_tri", [(333, 333, 97)], ("padded",), mode="rounding", uplos="LU")
    if t == "s":
        _sweep(t, "gemm", [(4000, 4090, 24)], ("padded",), ops=[("N", "N"), ("T", "T")], mode="rounding")


@pytest.mark.gpu
@pytest.mark.parametrize("t", "cz")
def test_rounding_complex(t):
    """as test_rounding_real with the factor 2 of the complex product: checked
    and full kernel, triangular store and herk"""
    _sweep(t, "gemm", [(130, 67, 24), (128, 192, 24)], ("padded",), mode="rounding")
    _sweep(t, "gemm_tri", [(200, 200, 24)], ("padded",), ops=[("N", "C"), ("C", "N"), ("T", "N")], mode="rounding",
           uplos="LU")
    _sweep(t, "herk", [(200, 200, 24)], ("padded",), ops=HERK_OPS, mode="rounding", uplos="LU")


# ---------------------------------------------------------------- semantics
@pytest.mark.gpu
@pytest.mark.parametrize("t", "sdcz")
def test_beta_zero_ignores_c(t):
    """beta == 0 on a C filled with NaN gives the exact finite product: every
    tile configuration, split-K, both complex kernels, triangular stores"""
    if _cplx(t):
        _sweep(t, "gemm", [(130, 67, 17), (128, 192, 16)], ("padded",), beta0=True)
        _sweep(t, "gemm_tri", [(65, 65, 9)], ("padded",), ops=[("N", "C"), ("C", "N")], uplos="LU", beta0=True)
        return
    shapes = [(300, 257, 33), (256, 256, 32), (1400, 1500, 24), (1408, 1536, 32), (200, 96, 1030), (300, 16, 129)]
    _sweep(t, "gemm", shapes, ("padded",), beta0=True)
    _sweep(t, "gemm_tri", [(333, 333, 17)], ("padded",), uplos="LU", beta0=True)
    _sweep(t, "herk", [(300, 300, 5000)], ("padded",), ops=HERK_OPS[:1], uplos="L", beta0=True)
    if t == "s":
        _sweep(t, "gemm", [(4000, 4090, 24), (4096, 4096, 32)], ("padded",), ops=[("N", "T"), ("T", "N")], beta0=True)


@pytest.mark.gpu
@pytest.mark.parametrize("t", "sdcz")
def test_k_zero_scales_c(t):
    """k == 0: C = beta C, whatever the tile multiples of m and n.  The empty
    operands are zero-width views of live allocations, so a kernel that loads
    from them regardless reads owned memory."""
    shapes = [(130, 67, 0), (128, 192, 0), (256, 256, 0), (64, 64, 0)]
    _sweep(t, "gemm", shapes, ("tight", "padded"))
    _sweep(t, "gemm", shapes, ("padded",), beta0=True)
    _sweep(t, "gemm_tri", [(128, 128, 0)], ("padded",), ops=_ops(t)[:2], uplos="LU")


@pytest.mark.gpu
@pytest.mark.parametrize("t", "cz")
def test_herk_diagonal_is_real(t):
    """complex herk with beta != 0 on a C whose diagonal has an imaginary part:
    Im C(i,i) == 0 exactly afterwards (as BLAS and the host target), both uplo
    and both ops."""
    n, k = 130, 24
    a, _, c0 = _operands(t, n, n, k, "int", True)
    assert np.all(c0.imag.diagonal() != 0)
    for uplo in "LU":
        for op in ("N", "C"):
            A, C = Mat(_stored(op, a), "padded"), Mat(c0, "padded")
            after = gpu_kernel(dict(kind="herk", ta=op, tb=op, alpha=0.5, beta=-2.0, uplo=uplo), A, None, C)
            got = C.view(after)
            assert np.all(got.imag.diagonal() == 0), (uplo, op, got.imag.diagonal()[:4])
            run_case(gpu_kernel, t, "herk", op, op, n, n, k, "padded", uplo=uplo)


@pytest.mark.gpu
@pytest.mark.parametrize("t", "sdcz")
def test_her2k_by_gemm_tri_pairs(t):
    """C = alpha A B^H + conj(alpha) B A^H + beta C on one triangle, as her2k
    forms it from two triangular products"""
    n, k = 200, 24
    alpha, beta = _scalars(t)
    beta = -2.0
    a, _, c0 = _operands(t, n, n, k, "int")
    b = _operands(t, n, n, k + 1, "int")[0][:, :k]
    hp = _high(t, "int")
    ah, bh = a.astype(hp), b.astype(hp)
    ref = alpha * (ah @ bh.conj().T) + np.conj(alpha) * (bh @ ah.conj().T) + beta * c0.astype(hp)
    for uplo in "LU":
        for op in ("N", "C"):
            o1, o2 = (op, "C" if op == "N" else "N")
            # op N: A, B stored n x k, C = alpha A B^H + ...; op C: stored k x n, C = alpha A^H B + ...
            A, B, C = Mat(_stored(op, a), "odd_ld"), Mat(_stored(op, b), "padded"), Mat(c0, "padded")
            mid = gpu_kernel(dict(kind="gemm_tri", ta=o1, tb=o2, alpha=alpha, beta=beta, uplo=uplo), A, B, C)
            C.check_untouched(mid)
            C2 = Mat(np.array(C.view(mid)), "padded")
            after = gpu_kernel(dict(kind="gemm_tri", ta=o1, tb=o2, alpha=np.conj(alpha), beta=1.0, uplo=uplo),
                               B, A, C2)
            C2.check_untouched(after)
            check_result(C2.view(after), c0, ref, None, "exact", t, k, uplo)


# ---------------------------------------------------------------- coverage (keep last)
@pytest.mark.gpu
def test_variant_coverage():
    """Every name in EXPECTED_VARIANTS was launched by the tests above, and they
    launched nothing the list does not name: a threshold that moves in the
    dispatcher shows here instead of silently shrinking the sweep."""
    assert _SEEN, "no launches recorded: this test checks the sweep, so it needs the whole module to run"
    missing = [v for v in EXPECTED_VARIANTS if v not in _SEEN]
    extra = sorted(_SEEN - set(EXPECTED_VARIANTS))
    assert not missing and not extra, f"not launched: {missing}; launched but not listed: {extra}"
