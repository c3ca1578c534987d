"""Bidiagonal divide and conquer (csrc/src/bdsdc.cc, host target): bdsdc
against numpy on every size class and on the hard spectra, the sqre = 1 leaf,
svd with method_svd="dc" against numpy and the QR path, a 2 x 2 grid, the
native tester, and bit-for-bit stedc and bdsdc results across the secular.hh
and dc_merge refactors."""
import hashlib
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import slate_d35_amd as s
from helpers import rnd
from bdsdc_cases import KINDS, bidiagonal, check

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")


def svd_tol(dt):
    """test_eig.py's tol(): its svd tests' bound on values and on relerr."""
    return 1e-3 if dt in (np.float32, np.complex64) else 1e-10


@pytest.fixture
def leaf8():
    """SLATE_BDSDC_LEAF is read at every call."""
    old = os.environ.get("SLATE_BDSDC_LEAF")
    os.environ["SLATE_BDSDC_LEAF"] = "8"
    yield
    if old is None:
        os.environ.pop("SLATE_BDSDC_LEAF", None)
    else:
        os.environ["SLATE_BDSDC_LEAF"] = old


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 129, 257, 600])
def test_bdsdc_sizes(n):
    d, e, ref = bidiagonal("random", n)
    sv, u, vt = s.bdsdc(d, e)
    check(d, e, ref, sv, u, vt)
    st = s.ops.bdsdc_stats()
    assert (st["merges"] > 0) == (n > 64)
    assert st["launches_secular"] == st["launches_zhat"] == st["launches_matrix"] == 0   # host twins


@pytest.mark.parametrize("kind", KINDS)
def test_bdsdc_kinds(kind):
    d, e, ref = bidiagonal(kind, 600)
    sv, u, vt = s.bdsdc(d, e)
    check(d, e, ref, sv, u, vt)
    st = s.ops.bdsdc_stats()
    assert st["columns"] == sum(st["level_columns"]) and st["deflated"] == sum(st["level_deflated"])
    if kind == "cluster":
        assert st["deflated"] > 0
    if kind == "zerodiag":
        assert sv[-1] <= 1e-13 * 600 * ref.max()


@pytest.mark.parametrize("scale", [1e150, 1e-150])
def test_bdsdc_scaling(scale):
    d, e, ref = bidiagonal("random", 600, scale)
    sv, u, vt = s.bdsdc(d, e)
    check(d, e, ref, sv, u, vt)


def test_bdsdc_small_leaf(leaf8):
    d, e, ref = bidiagonal("random", 100)
    sv, u, vt = s.bdsdc(d, e)
    check(d, e, ref, sv, u, vt)
    assert s.ops.bdsdc_stats()["merges"] >= 7


@pytest.mark.parametrize("zero_at", [None, 0, 2, 3])
def test_bdsdc_sqre1_leaf(leaf8, zero_at):
    """n = leaf + 1: one merge whose left child (rows 0..3, columns 0..4) is
    exactly one sqre = 1 leaf -- the extra column is chased away by Givens
    rotations from the right -- also with a zero on that leaf's diagonal."""
    rng = np.random.default_rng(5)
    d, e = rng.standard_normal(9), rng.standard_normal(8)
    if zero_at is not None:
        d[zero_at] = 0.0
    ref = np.linalg.svd(np.diag(d) + np.diag(e, 1), compute_uv=False)
    sv, u, vt = s.bdsdc(d, e)
    check(d, e, ref, sv, u, vt)
    assert s.ops.bdsdc_stats()["merges"] == 1


def test_bdsdc_matrix_host():
    """bdsdc_matrix keeps bdsqr_matrix's contract: U := U U_B with a
    rectangular U, VT := V_B^T VT; float32 data; the values-only call."""
    n, m, nb = 130, 170, 32
    d, e, ref = bidiagonal("random", n)
    U0, VT0 = s.from_numpy(np.eye(n), nb=nb), s.from_numpy(np.eye(n), nb=nb)
    sv = s.bdsdc_matrix(s.Job.Vec, s.Job.Vec, d, e, U0, VT0)
    u0, vt0 = s.to_numpy(U0), s.to_numpy(VT0)
    check(d, e, ref, sv, u0, vt0)
    q, w = rnd(m, n, np.float64, 3), rnd(n, n, np.float64, 4)
    U, VT = s.from_numpy(q, nb=nb), s.from_numpy(w, nb=nb)
    sv2 = s.bdsdc_matrix(s.Job.Vec, s.Job.Vec, d, e, U, VT)
    assert np.array_equal(sv2, sv)
    # two roundings of an inner product of length n: ours and numpy's
    eps = np.finfo(np.float64).eps
    assert np.linalg.norm(s.to_numpy(U) - q @ u0) <= 2 * n * eps * np.linalg.norm(q) * np.linalg.norm(u0)
    assert np.linalg.norm(s.to_numpy(VT) - vt0 @ w) <= 2 * n * eps * np.linalg.norm(vt0) * np.linalg.norm(w)
    assert np.abs(s.bdsdc_matrix(s.Job.NoVec, s.Job.NoVec, d, e) - ref).max() <= 1e-13 * n * ref.max()
    Uf = s.from_numpy(np.eye(n, dtype=np.float32), nb=nb)
    VTf = s.from_numpy(np.eye(n, dtype=np.float32), nb=nb)
    svf = s.bdsdc_matrix(s.Job.Vec, s.Job.Vec, d.astype(np.float32), e.astype(np.float32), Uf, VTf)
    d32, e32 = d.astype(np.float32).astype(np.float64), e.astype(np.float32).astype(np.float64)
    ref32 = np.linalg.svd(np.diag(d32) + np.diag(e32, 1), compute_uv=False)
    check(d32, e32, ref32, svf, s.to_numpy(Uf), s.to_numpy(VTf),
          factor=float(np.finfo(np.float32).eps / np.finfo(np.float64).eps))


@pytest.mark.parametrize("nb", [16, 32])
@pytest.mark.parametrize("dt", [np.float64, np.complex128])
@pytest.mark.parametrize("mn", [(96, 96), (150, 110), (110, 150), (300, 40)])
def test_svd_method_dc(mn, dt, nb):
    m, n = mn
    k = min(m, n)
    a = rnd(m, n, dt, 9)
    ref = np.linalg.svd(a, compute_uv=False)
    out = {}
    for method in ("dc", "qr"):
        A = s.from_numpy(a, nb=nb)
        U = s.from_numpy(np.zeros((m, k), dt), nb=nb)
        VT = s.from_numpy(np.zeros((k, n), dt), nb=nb)
        sv = s.svd(A, U, VT, method_svd=method)
        u, vt = s.to_numpy(U), s.to_numpy(VT)
        assert np.allclose(sv, ref, atol=svd_tol(dt) * ref.max()), method
        assert np.linalg.norm(u @ np.diag(sv) @ vt - a) / (np.linalg.norm(a) * k) < svd_tol(dt), method
        assert np.linalg.norm(u.conj().T @ u - np.eye(k)) / k < svd_tol(dt), method
        assert np.linalg.norm(vt @ vt.conj().T - np.eye(k)) / k < svd_tol(dt), method
        out[method] = sv
    assert np.allclose(out["dc"], out["qr"], atol=svd_tol(dt) * ref.max())
    assert s.ops.bdsdc_stats()["merges"] > 0 or k <= 64


def test_method_svd_option():
    assert s.MethodSVD.QR != s.MethodSVD.DC
    a = rnd(40, 40, np.float64, 2)
    with pytest.raises(Exception, match="method_svd"):
        s.svd(s.from_numpy(a, nb=16), method_svd="jacobi")
    # values only: the option is accepted and the QR values-only path runs
    sv = s.svd(s.from_numpy(a, nb=16), method_svd="dc")
    assert np.allclose(sv, np.linalg.svd(a, compute_uv=False), atol=1e-10 * sv.max())


def _free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_bdsdc_grid_2x2():
    """Replicated compute on a 2 x 2 grid: every rank keeps its own part."""
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "2")
    env["SLATE_TRANSPORT"] = "host"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=4",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(HERE, "bdsdc_worker.py"), "2", "2", "h"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "BDSDC_DIST_OK" in out, out[-4000:]


def test_native_tester_bdsdc():
    """The native tester's bdsdc routine (r_bdsqr's check with divide and
    conquer) and svd --method-svd dc, real and complex."""
    r = subprocess.run(["make", "tester"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    port = _free_port()
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               SLATE_MASTER_PORT=str(port), SLATE_COMM="host", OMP_NUM_THREADS="2")
    r = subprocess.run([os.path.join(ROOT, "bin", "slate_tester"), "bdsdc,svd", "--method-svd", "dc", "--type", "d,z",
                        "--dim", "150,140x110x110", "--nb", "32", "--target", "h"], env=env, capture_output=True,
                       text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "all tests passed" in out, out[-4000:]
    assert out.count("pass") >= 8 and out.count("method_svd=dc") == 4, out[-4000:]


def test_python_tester_method_svd(capsys):
    from slate_d35_amd import tester
    rc = tester.main(["svd", "--method-svd", "dc", "--dim", "150x110x110", "--nb", "32", "--type", "d,z", "--target", "h"])
    out = capsys.readouterr().out
    assert rc == 0 and "all tests passed" in out, out
    assert out.count("method_svd=dc") == 2, out
    assert s.ops.bdsdc_stats()["merges"] > 0


# ---- the stedc path after the secular.hh refactor: bit for bit
def _stedc_input(kind, n=500):
    rng = np.random.default_rng(7)
    if kind == "toeplitz":
        return np.full(n, 2.0), np.full(n - 1, -1.0)
    if kind == "wilkinson":
        m = (n - 1) // 2
        return np.abs(np.arange(-m, n - m, dtype=float)), np.ones(n - 1)
    if kind == "graded":
        return np.logspace(0, -15, n), np.logspace(0, -15, n - 1) * 0.1
    if kind == "cluster":
        d = np.ones(n)
        d[::7] = 1 + 1e-12
        return d, np.full(n - 1, 1e-9)
    d, e = rng.standard_normal(n), rng.standard_normal(n - 1)
    e[::5] = 1e-14
    return d, e


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


@pytest.mark.parametrize("kind", ["toeplitz", "wilkinson", "graded", "cluster", "tinyoff"])
def test_stedc_bitwise_unchanged(kind):
    """The five test_stedc_secular_hard inputs: eigenvalues of s.stedc and of
    s.stedc_matrix, and the Q that stedc_matrix writes (its SHA-256 and every
    25th row; all of Q is 2 MB), captured before secular.hh got root_core."""
    g = lambda name: np.load(os.path.join(GOLDEN, f"stedc_{kind}_{name}.npy"))  # noqa: E731
    d, e = _stedc_input(kind)
    w, z = s.stedc(d, e)
    assert np.array_equal(np.asarray(w), g("w"))
    assert np.array_equal(_sha(np.asarray(z)), g("z_sha256"))
    Q = s.from_numpy(np.zeros((500, 500)), nb=64)
    w2 = np.asarray(s.stedc_matrix(d, e, Q))
    q = s.to_numpy(Q)
    assert np.array_equal(w2, g("w_matrix"))
    assert np.array_equal(q[::25], g("q_rows"))
    assert np.array_equal(_sha(q), g("q_sha256"))


# ---- the host bdsdc path after the merge moved to dc_merge: bit for bit
BDSDC_PINNED = {"random": ("random", 600), "cluster": ("cluster", 600), "zerodiag": ("zerodiag", 600),
                "tiny": ("tiny", 600), "graded": ("graded", 257), "leaf8": ("random", 100),
                "float32": ("random", 130)}


def _bdsdc_pinned(case):
    """(sv, u, vt) of one pinned case: s.bdsdc, with SLATE_BDSDC_LEAF=8 for
    leaf8, and float32 identities through bdsdc_matrix (nb = 32) for float32."""
    kind, n = BDSDC_PINNED[case]
    d, e, _ = bidiagonal(kind, n)
    if case == "float32":
        U, VT = (s.from_numpy(np.eye(n, dtype=np.float32), nb=32) for _ in range(2))
        sv = s.bdsdc_matrix(s.Job.Vec, s.Job.Vec, d.astype(np.float32), e.astype(np.float32), U, VT)
        return np.asarray(sv), s.to_numpy(U), s.to_numpy(VT)
    old = os.environ.get("SLATE_BDSDC_LEAF")
    if case == "leaf8":
        os.environ["SLATE_BDSDC_LEAF"] = "8"
    try:
        sv, u, vt = s.bdsdc(d, e)
    finally:
        if case == "leaf8":
            os.environ.pop("SLATE_BDSDC_LEAF")
            if old is not None:
                os.environ["SLATE_BDSDC_LEAF"] = old
    return np.asarray(sv), np.asarray(u), np.asarray(vt)


@pytest.mark.parametrize("case", list(BDSDC_PINNED))
def test_bdsdc_bitwise_unchanged(case):
    """Singular values (whole), and U and VT (SHA-256 and every 25th row) of
    the host-target bdsdc, captured before the merge of stedc_dist and bdsdc
    became one (dc_merge.cc).  The outputs do not depend on the thread count."""
    g = lambda name: np.load(os.path.join(GOLDEN, f"bdsdc_{case}_{name}.npy"))  # noqa: E731
    sv, u, vt = _bdsdc_pinned(case)
    assert np.array_equal(sv, g("sv"))
    assert np.array_equal(u[::25], g("u_rows"))
    assert np.array_equal(vt[::25], g("vt_rows"))
    assert np.array_equal(_sha(u), g("u_sha256"))
    assert np.array_equal(_sha(vt), g("vt_sha256"))
