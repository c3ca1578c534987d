"""Option::GemmPrecision / gemm_bf16s.hip: fp32 products formed from bf16 MFMAs
on split operands (bf16: 1, bf16x3: 3, bf16x6: 6 plane products per K-step).

Kernel tests go through s.ops.gemm_lowprec (the raw kernel); driver tests
through gemm_precision=...; the host target, option parsing and the native
tester run without a GPU."""
import functools
import os
import subprocess

import numpy as np
import pytest

import slate_d35_amd as s

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "slate_tester")

MODES = ["bf16", "bf16x3", "bf16x6"]
OPS = [("N", "N"), ("N", "T"), ("T", "N"), ("T", "T")]
SHAPES = [(300, 257, 161), (128, 128, 32), (129, 127, 33), (1, 1, 1), (64, 513, 7)]
U = 2.0 ** -8          # bf16 unit roundoff used by the bounds
C_MODE = {"bf16": 2 * U + U * U, "bf16x3": 3 * U * U + 2.0 ** -22, "bf16x6": 2.0 ** -21}


def _torch():
    import torch
    return torch


def _dev(x):
    """column-major matrix x -> row-major device tensor of its transpose"""
    return _torch().from_numpy(np.array(x.T, order="C", copy=True)).cuda()


def _host(t):
    return t.cpu().numpy().T


def _stored(op, x):
    """the array as stored for op(X) = x"""
    return x if op == "N" else np.ascontiguousarray(x.T)


def _run(mode, ta, tb, alpha, opa, opb, beta, c0, uplo="G"):
    """C = alpha opa opb + beta c0 by the low-precision kernel; opa / opb are op(A) / op(B)."""
    tA, tB, tC = _dev(_stored(ta, opa)), _dev(_stored(tb, opb)), _dev(c0)
    s.ops.gemm_lowprec(mode, ta, tb, alpha, tA, tB, beta, tC, uplo=uplo)
    return _host(tC)


@functools.lru_cache(maxsize=None)
def _ints(m, n, k, lo, hi, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(lo, hi + 1, (m, k)).astype(np.float32)
    b = rng.integers(lo, hi + 1, (k, n)).astype(np.float32)
    return a, b


@functools.lru_cache(maxsize=None)
def _uniform(m, n, k, seed):
    """uniform(-1, 1) fp32 operands, C0, and the fp64 pieces of the bound"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (m, k)).astype(np.float32)
    b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    c0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    a64, b64, c64 = a.astype(np.float64), b.astype(np.float64), c0.astype(np.float64)
    alpha, beta = 0.5, -2.0
    ref = alpha * (a64 @ b64) + beta * c64
    scale = abs(alpha) * (np.abs(a64) @ np.abs(b64)) + abs(beta) * np.abs(c64)
    for x in (a, b, c0, ref, scale):
        x.setflags(write=False)
    return a, b, c0, ref, scale


# ------------------------------------------------------------------ kernel
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ta,tb", OPS)
def test_exact_layout(mode, ta, tb):
    """Integers in [-8, 8]: every term and sum is exact in bf16 and fp32, so
    every mode equals the integer product bit for bit (lane maps, transposes,
    edge tiles, the K remainder)."""
    for (m, n, k) in SHAPES:
        a, b = _ints(m, n, k, -8, 8, 11)
        c0 = np.full((m, n), np.nan, np.float32)
        got = _run(mode, ta, tb, 1.0, a, b, 0.0, c0)
        assert np.array_equal(got, a @ b), (m, n, k)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ta,tb", OPS)
def test_exact_split(mode, ta, tb):
    """A = P + Q 2^-9: the hi plane is P under RNE, so bf16 gives P B exactly
    and the split modes give A B exactly (magnitudes < 2^24 at resolution 2^-9)."""
    m, n, k = 300, 257, 161
    rng = np.random.default_rng(12)
    p = (rng.integers(1, 5, (m, k)) * rng.choice([-1, 1], (m, k))).astype(np.float64)
    q = rng.integers(-1, 2, (m, k)).astype(np.float64)
    b = rng.integers(-4, 5, (k, n)).astype(np.float64)
    a = p + q * 2.0 ** -9
    got = _run(mode, ta, tb, 1.0, a.astype(np.float32), b.astype(np.float32), 0.0, np.zeros((m, n), np.float32))
    want = (p @ b) if mode == "bf16" else (a @ b)
    assert np.array_equal(got.astype(np.float64), want)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ta,tb", OPS)
def test_error_bounds(mode, ta, tb):
    """|C - ref| <= (c_mode + (k + 4) 2^-24) (|alpha| |op A||op B| + |beta| |C0|)
    elementwise against fp64 (CPU emulation maxima at (300, 257, 161):
    2^-10.1, 2^-19.0, 2^-25.5)."""
    for (m, n, k) in SHAPES:
        a, b, c0, ref, scale = _uniform(m, n, k, 13)
        got = _run(mode, ta, tb, 0.5, a, b, -2.0, c0).astype(np.float64)
        ratio = np.abs(got - ref) / scale
        bound = C_MODE[mode] + (k + 4) * 2.0 ** -24
        print(f"{mode} {ta}{tb} {(m, n, k)}: max err/scale 2^{np.log2(max(ratio.max(), 1e-300)):.1f}, "
              f"bound 2^{np.log2(bound):.1f}")
        assert np.all(np.abs(got - ref) <= bound * scale), (m, n, k, ratio.max(), bound)


@pytest.mark.gpu
def test_modes_distinct():
    """bf16 is much worse than bf16x3 (emulation ratio 2^9), and bf16x6 is as
    good as the fp32 MFMA kernel up to the summation order."""
    m, n, k = 300, 257, 161
    a, b, c0, ref, scale = _uniform(m, n, k, 13)
    err = {}
    for mode in MODES:
        got = _run(mode, "N", "T", 0.5, a, b, -2.0, c0).astype(np.float64)
        err[mode] = (np.abs(got - ref) / scale).max()
    tA, tB, tC = _dev(a), _dev(np.ascontiguousarray(b.T)), _dev(c0)
    s.ops.gemm("N", "T", np.float32(0.5), tA, tB, np.float32(-2.0), tC)
    err["native"] = (np.abs(_host(tC).astype(np.float64) - ref) / scale).max()
    print({k_: f"2^{np.log2(v):.1f}" for k_, v in err.items()})
    assert err["bf16"] > 16 * err["bf16x3"], err
    assert err["bf16x6"] <= 4 * err["native"], err


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("n", [130, 300])
def test_triangle(mode, uplo, n):
    """uplo L / U: the other triangle of C, preset to a sentinel, is untouched
    bit for bit; the triangle itself meets the mode's bound."""
    k = 97
    a, b, _, _, _ = _uniform(n, n, k, 14)
    sentinel = np.float32(-12345.678)
    c0 = np.full((n, n), sentinel, np.float32)
    tri = np.tril(np.ones((n, n), bool)) if uplo == "L" else np.triu(np.ones((n, n), bool))
    for ta, tb in OPS:
        got = _run(mode, ta, tb, 1.0, a, b, 0.0, c0, uplo=uplo)
        assert np.array_equal(got[~tri].view(np.uint32), c0[~tri].view(np.uint32)), (ta, tb)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        bound = (C_MODE[mode] + (k + 4) * 2.0 ** -24) * (np.abs(a64) @ np.abs(b64))
        assert np.all((np.abs(got - a64 @ b64) <= bound)[tri]), (ta, tb)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_k0_and_beta0(mode):
    torch = _torch()
    m, n = 130, 70
    c0 = np.arange(m * n, dtype=np.float32).reshape(m, n) / 7
    tC = _dev(c0)
    tA = torch.zeros((0, m), dtype=torch.float32, device="cuda")   # m x 0 column-major
    tB = torch.zeros((n, 0), dtype=torch.float32, device="cuda")   # 0 x n column-major
    s.ops.gemm_lowprec(mode, "N", "N", 1.0, tA, tB, -2.0, tC)
    assert np.array_equal(_host(tC), np.float32(-2.0) * c0)
    a, b = _ints(m, n, 40, -8, 8, 15)
    got = _run(mode, "N", "N", 1.0, a, b, 0.0, np.full((m, n), np.nan, np.float32))
    assert np.all(np.isfinite(got)) and np.array_equal(got, a @ b)


# ------------------------------------------------------------------ drivers
N, NB, NRHS = 1024, 128, 3


@functools.lru_cache(maxsize=None)
def _systems():
    rng = np.random.default_rng(21)
    r = rng.uniform(-1, 1, (N, N))
    b = rng.uniform(-1, 1, (N, NRHS))
    well = 4 * np.eye(N) + r / np.sqrt(N)
    spd = r @ r.T / N + np.eye(N)
    for x in (r, b, well, spd):
        x.setflags(write=False)
    return {"rands": r, "well": well, "spd": spd, "b": b}


def _gesv_mixed(a, b, **kw):
    A, B = s.from_numpy(a, nb=NB, target="d"), s.from_numpy(b, nb=NB, target="d")
    X = s.from_numpy(np.zeros_like(b), nb=NB, target="d")
    info, _, it = s.gesv_mixed(A, B, X, target="d", **kw)
    return info, it, s.to_numpy(X)


def _backward(a, x, b):
    # the measure and tolerance of tests/test_gpu.py::test_gesv_mixed_device
    return np.linalg.norm(a @ x - b, 1) / (np.linalg.norm(a, 1) * np.linalg.norm(x, 1))


@pytest.mark.gpu
def test_gesv_mixed_bf16_well_conditioned():
    sy = _systems()
    a, b = sy["well"], sy["b"]
    c0 = s.ops.lowprec_gemm_calls()
    info0, it0, x0 = _gesv_mixed(a, b)
    assert s.ops.lowprec_gemm_calls() == c0, "the default must not reach the low-precision kernel"
    info_n, it_n, _ = _gesv_mixed(a, b, gemm_precision="native")
    assert s.ops.lowprec_gemm_calls() == c0
    assert info0 == 0 and (info_n, it_n) == (info0, it0)
    assert it0 == 2          # the fp32 factor's count before this option existed (emulation: 2)
    info, it, x = _gesv_mixed(a, b, gemm_precision="bf16")
    print(f"gesv_mixed 4I + R/sqrt(n): native iter {it0}, bf16 iter {it}")
    assert s.ops.lowprec_gemm_calls() > c0
    assert info == 0 and 0 <= it <= 10, (info, it)
    xref = np.linalg.solve(a, b)
    assert _backward(a, x, b) < 1e-15 * N
    assert np.linalg.norm(x - xref) / np.linalg.norm(xref) < 1e-15 * N


@pytest.mark.gpu
def test_gesv_mixed_bf16x3_rands():
    sy = _systems()
    a, b = sy["rands"], sy["b"]
    c0 = s.ops.lowprec_gemm_calls()
    info, it, x = _gesv_mixed(a, b, gemm_precision="bf16x3", use_fallback_solver=False)
    print(f"gesv_mixed rands bf16x3: iter {it}")
    assert s.ops.lowprec_gemm_calls() > c0
    assert info == 0 and 0 <= it <= 15, (info, it)
    assert _backward(a, x, b) < 1e-15 * N


@pytest.mark.gpu
def test_gesv_mixed_bf16x6_rands():
    sy = _systems()
    a, b = sy["rands"], sy["b"]
    info_n, it_n, _ = _gesv_mixed(a, b, gemm_precision="native", use_fallback_solver=False)
    info, it, x = _gesv_mixed(a, b, gemm_precision="bf16x6", use_fallback_solver=False)
    print(f"gesv_mixed rands: native iter {it_n}, bf16x6 iter {it}")
    assert info_n == 0 and it_n >= 0
    assert info == 0 and 0 <= it <= it_n + 1, (it, it_n)
    assert _backward(a, x, b) < 1e-15 * N


@pytest.mark.gpu
@pytest.mark.parametrize("uplo", [s.Uplo.Lower, s.Uplo.Upper])
def test_posv_mixed_bf16x3(uplo):
    sy = _systems()
    a, b = sy["spd"], sy["b"]
    A = s.HermitianMatrix(uplo, s.from_numpy(a, nb=NB, target="d"))
    B = s.from_numpy(b, nb=NB, target="d")
    X = s.from_numpy(np.zeros_like(b), nb=NB, target="d")
    c0 = s.ops.lowprec_gemm_calls()
    info, it = s.posv_mixed(A, B, X, target="d", gemm_precision="bf16x3", use_fallback_solver=False)
    print(f"posv_mixed bf16x3: iter {it}")
    assert s.ops.lowprec_gemm_calls() > c0
    assert info == 0 and it >= 0, (info, it)
    assert _backward(a, s.to_numpy(X), b) < 1e-15 * N


def _lu_residual(fn, a, **kw):
    A = s.from_numpy(a, nb=NB, target="d")
    info, piv = fn(A, target="d", **kw)
    assert info == 0
    f = s.to_numpy(A).astype(np.float64)
    n = a.shape[0]
    L, Uf = np.tril(f, -1) + np.eye(n), np.triu(f)
    ip = [kk * NB + ti * NB + off for kk, pv in enumerate(piv) for (ti, off) in pv]
    pa = a.astype(np.float64)
    for j, p_ in enumerate(ip):
        pa[[j, p_]] = pa[[p_, j]]
    return np.linalg.norm(pa - L @ Uf) / np.linalg.norm(pa)


@pytest.mark.gpu
@pytest.mark.parametrize("routine", ["getrf", "getrf_tntpiv"])
def test_getrf_float32_bf16x6(routine):
    a = _systems()["rands"].astype(np.float32)
    fn = getattr(s, routine)
    c0 = s.ops.lowprec_gemm_calls()
    r_native = _lu_residual(fn, a, gemm_precision="native")
    assert s.ops.lowprec_gemm_calls() == c0
    r_x6 = _lu_residual(fn, a, gemm_precision="bf16x6")
    assert s.ops.lowprec_gemm_calls() > c0
    print(f"{routine}: |PA - LU|/|A| native {r_native:.3e}, bf16x6 {r_x6:.3e}")
    assert r_x6 <= 2 * r_native, (r_x6, r_native)


@pytest.mark.gpu
def test_gemm_driver_float32_bf16x6():
    from helpers import relerr, rnd, tol
    m, n, k = 400, 300, 200
    a, b, c = rnd(m, k, np.float32, 1), rnd(k, n, np.float32, 2), rnd(m, n, np.float32, 3)
    A, B, C = (s.from_numpy(x, nb=NB, target="d") for x in (a, b, c))
    c0 = s.ops.lowprec_gemm_calls()
    s.gemm(np.float32(1.5), A, B, np.float32(0.5), C, target="d", gemm_precision="bf16x6")
    assert s.ops.lowprec_gemm_calls() > c0
    ref = 1.5 * a.astype(np.float64) @ b.astype(np.float64) + 0.5 * c.astype(np.float64)
    assert relerr(s.to_numpy(C), ref) < tol(np.float32)


@pytest.mark.gpu
def test_gesv_mixed_complex_rejects_option():
    n = 256
    rng = np.random.default_rng(5)
    a = rng.uniform(-1, 1, (n, n)) + 1j * rng.uniform(-1, 1, (n, n)) + 4 * np.eye(n)
    b = rng.uniform(-1, 1, (n, 1)) + 0j
    A, B = s.from_numpy(a, nb=NB, target="d"), s.from_numpy(b, nb=NB, target="d")
    X = s.from_numpy(np.zeros_like(b), nb=NB, target="d")
    with pytest.raises(Exception, match="GemmPrecision"):
        s.gesv_mixed(A, B, X, target="d", gemm_precision="bf16x3")


# ------------------------------------------------------------------ no GPU
def test_host_target_ignores_option():
    """target="h": the option changes nothing, bit for bit (float32 gemm and getrf)."""
    from helpers import rnd
    m, n, k, nb = 300, 260, 200, 128
    a, b, c = rnd(m, k, np.float32, 1), rnd(k, n, np.float32, 2), rnd(m, n, np.float32, 3)
    out = []
    for kw in ({}, {"gemm_precision": "bf16"}):
        A, B, C = (s.from_numpy(x, nb=nb) for x in (a, b, c))
        s.gemm(np.float32(1.5), A, B, np.float32(0.5), C, target="h", **kw)
        out.append(s.to_numpy(C))
    assert np.array_equal(out[0], out[1])
    sq = rnd(m, m, np.float32, 4)
    out = []
    for kw in ({}, {"gemm_precision": "bf16"}):
        A = s.from_numpy(sq, nb=nb)
        info, piv = s.getrf(A, target="h", **kw)
        out.append((info, piv, s.to_numpy(A)))
    assert out[0][0] == out[1][0] == 0 and out[0][1] == out[1][1]
    assert np.array_equal(out[0][2], out[1][2])


def test_option_parsing():
    from helpers import rnd
    a = rnd(40, 40, np.float32, 1)
    for name in ("native", "bf16", "bf16x3", "bf16x6"):
        A, B, C = (s.from_numpy(a, nb=16) for _ in range(3))
        s.gemm(np.float32(1), A, B, np.float32(0), C, target="h", gemm_precision=name)
    A, B, C = (s.from_numpy(a, nb=16) for _ in range(3))
    with pytest.raises(Exception, match="gemm precision"):
        s.gemm(np.float32(1), A, B, np.float32(0), C, target="h", gemm_precision="fp8")
    with pytest.raises(Exception, match="GemmPrecision"):
        s.gemm(np.float32(1), A, B, np.float32(0), C, target="h", gemm_precision=7)


def test_native_tester_option():
    r = subprocess.run(["make", "tester"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([EXE, "--gemm-precision", "bf16x3", "gesv_mixed", "--dim", "256", "--target", "h"],
                       capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", SLATE_COMM="host",
                                OMP_NUM_THREADS="2"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "all tests passed" in out, out[-3000:]
    assert "bf16x3" in out, out[-3000:]
    r = subprocess.run([EXE, "--gemm-precision", "fp8", "gesv_mixed", "--dim", "64", "--target", "h"],
                       capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", SLATE_COMM="host"))
    assert r.returncode != 0
