"""Inverse iteration on the host target (csrc/include/slate_amd/stein.hh,
host::stein, csrc/src/stein.cc) and heevx / syevx on it: stein on every case
of stein_cases.py within the bounds derived from LAPACK's own error, the
refusals, heevx with both reductions, the 1 x 2 grid refusal, the C entry
points and both testers.  The cases and their bounds are in stein_cases.py,
shared with test_stein_gpu.py."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import slate_d35_amd as s
import stein_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "slate_d35_amd")
TG = "h"


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("case,n,kw", C.CASES, ids=C.CASE_IDS)
def test_stein(case, n, kw, dt):
    C.check_stein_case(case, n, kw, dt, TG)


def test_stein_small_and_empty():
    C.check_stein_small(TG)


def test_stein_refusals():
    C.check_stein_refusals(TG)


def test_host_stats():
    d, e = C.tridiagonal("random", "float64", 65)
    s.stein(d, e, s.stebz(d, e, target=TG), target=TG)
    st = s.ops.stein_stats()
    assert st["launches"] == 0 and st["host_syncs"] == 0 and st["rounds"] == 5 and st["values"] == 65, st


def test_lapack_table():
    """LAPACK's stebz + stein on the same inputs must not exceed twice what
    TABLE records for it: the guard of the constants the bounds come from."""
    sl = pytest.importorskip("scipy.linalg")
    worst = {}
    for case, n, kw in C.CASES:
        for dt in (np.float64, np.float32):
            d, e = C.tridiagonal(case, np.dtype(dt).name, n)
            stebz, stein = sl.get_lapack_funcs(("stebz", "stein"), dtype=dt)
            rng = 2 if kw else 0
            m, w, iblock, isplit, info = stebz(d, e, rng, 0.0, 0.0, kw.get("il", 1), kw.get("iu", len(d)),
                                               0.0, "B")
            assert info == 0
            z, info = stein(d, e, w[:m], iblock, isplit)
            assert info == 0
            r, o = C.measures(d, e, w[:m], z, dt)
            k = (case, np.dtype(dt).name)
            worst[k] = tuple(max(x, y) for x, y in zip(worst.get(k, (0.0, 0.0)), (r, o)))
    for (case, dtname), (r, o) in sorted(worst.items()):
        r64, r32, o64, o32 = C.TABLE[case]
        rr, oo = (r32, o32) if dtname == "float32" else (r64, o64)
        print(f"LAPACK {case} {dtname}: r {r:.3f} (recorded {rr}) o {o:.3f} (recorded {oo})")
        assert r <= 2 * rr and o <= 2 * oo, (case, dtname, r, rr, o, oo)


@pytest.mark.parametrize("mh", ["two_stage", "one_stage"])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", [130, 257])
def test_heevx(n, dt, mh):
    C.check_heevx(n, dt, mh, TG)


def test_heevx_complex_two_stage():
    C.check_heevx(130, np.complex128, "two_stage", TG)


def test_heevx_leaves_a_and_syevx():
    C.check_heevx_unmodified(TG)


def test_heevx_refusals():
    C.check_heevx_refusals(TG)


def _free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_heevx_grid_of_two_refused():
    """A 1 x 2 host grid: heevx raises NotImplemented naming the grid; heev still runs."""
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "2")
    env["SLATE_TRANSPORT"] = "host"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(HERE, "stein_worker.py"), "1", "2", "h"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "HEEVX_REFUSED_OK" in out, out[-4000:]


C_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include "slate_amd/c_api.h"
int main(void) {
    enum { N = 10, M = 4 };
    double d[N], e[N - 1], w[N], z[(N + 2) * M];
    int64_t nf = -1, nfailed = -1, ifail[M];
    for (int i = 0; i < N; ++i) d[i] = 2;
    for (int i = 0; i + 1 < N; ++i) e[i] = -1;
    slate_Options o[1] = {{slate_Option_Target, 'H', 0.0}};
    if (slate_stebz_r64('I', 0, 0, 2, 5, N, d, e, &nf, w, 1, o) != 0 || nf != M) return 1;
    if (slate_stein_r64(N, d, e, M, w, z, N + 2, &nfailed, ifail, 1, o) != 0 || nfailed != 0) return 2;
    if (slate_stein_r64(N, d, e, M, w, z, N + 2, 0, 0, 1, o) != 0) return 3;
    /* residual and orthogonality of the four vectors of (-1, 2, -1) */
    double res = 0, orth = 0;
    for (int j = 0; j < M; ++j) {
        const double* x = z + j * (N + 2);
        for (int i = 0; i < N; ++i) {
            double t = 2 * x[i] - (i > 0 ? x[i - 1] : 0) - (i + 1 < N ? x[i + 1] : 0) - w[j] * x[i];
            res = fmax(res, fabs(t));
        }
        for (int k = 0; k <= j; ++k) {
            double dot = 0;
            for (int i = 0; i < N; ++i) dot += x[i] * z[k * (N + 2) + i];
            orth = fmax(orth, fabs(dot - (k == j)));
        }
    }
    double wbad[2] = {1.0, 0.5};
    int refused = slate_stein_r64(N, d, e, 2, wbad, z, N + 2, &nfailed, ifail, 1, o);
    printf("stein res %.3e orth %.3e refused %d (%s)\n", res, orth, refused, slate_last_error());
    /* eigenpairs 2 .. 5 of the dense (-1, 2, -1) */
    const int64_t n = 40, nb = 16, il = 2, iu = 5;
    double *A = calloc(n * n, sizeof(double)), *Z = calloc(n * 6, sizeof(double)), L[40];
    for (int64_t i = 0; i < n; ++i) { A[i + i * n] = 2; if (i + 1 < n) A[i + 1 + i * n] = A[i + (i + 1) * n] = -1; }
    slate_Matrix_r64 As = slate_Matrix_create_fromLAPACK_r64(n, n, A, n, nb);
    slate_Matrix_r64 Zs = slate_Matrix_create_fromLAPACK_r64(n, 6, Z, n, nb);
    int64_t m = -1;
    int rc = slate_hermitian_eig_range_r64('L', As, 'I', 0, 0, il, iu, &m, L, Zs, 1, o);
    double lerr = 0, zres = 0, ztail = 0;
    const double pi = 3.14159265358979323846;
    for (int64_t k = 0; k < m; ++k) {
        lerr = fmax(lerr, fabs(L[k] - (2 - 2 * cos((il + k) * pi / (n + 1)))));
        for (int64_t i = 0; i < n; ++i) {
            const double* x = Z + k * n;
            zres = fmax(zres, fabs(2 * x[i] - (i > 0 ? x[i - 1] : 0) - (i + 1 < n ? x[i + 1] : 0) - L[k] * x[i]));
        }
    }
    for (int64_t i = 4 * n; i < 6 * n; ++i) ztail = fmax(ztail, fabs(Z[i]));
    int64_t m2 = -1;
    int rc2 = slate_hermitian_eig_range_r64('L', As, 'V', 0.0, 0.1, 0, 0, &m2, L, 0, 1, o);
    slate_Matrix_destroy_r64(As);
    slate_Matrix_destroy_r64(Zs);
    printf("eig_range rc %d m %d lerr %.3e zres %.3e ztail %.3e rc2 %d m2 %d\n", rc, (int)m, lerr, zres, ztail, rc2,
           (int)m2);
    return (res <= 1e-13 && orth <= 1e-13 && refused == -1 && rc == 0 && m == 4 && lerr <= 1e-13 && zres <= 1e-12 &&
            ztail == 0 && rc2 == 0 && m2 == 4) ? 0 : 5;
}
"""


def test_c_api(tmp_path):
    src, exe = tmp_path / "stein_c.c", tmp_path / "stein_c"
    src.write_text(C_SRC)
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT}/csrc/include", str(src), f"-L{PKG}", "-lslate_amd",
                    f"-Wl,-rpath,{PKG}", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "not ascending" in r.stdout, r.stdout
    f90 = open(os.path.join(ROOT, "csrc", "api", "slate_c_api.f90")).read()
    for name in ("slate_stein_r32", "slate_stein_r64", "slate_hermitian_eig_range_r32", "slate_hermitian_eig_range_r64",
                 "slate_hermitian_eig_range_c32", "slate_hermitian_eig_range_c64",
                 "integer(c_int64_t) :: ifail(*)"):
        assert name in f90, name


def run_native_tester(target):
    r = subprocess.run(["make", "tester"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    port = _free_port()
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               SLATE_MASTER_PORT=str(port), SLATE_COMM="host", OMP_NUM_THREADS="2")
    for mh in ("two_stage", "one_stage"):
        r = subprocess.run([os.path.join(ROOT, "bin", "slate_tester"), "stein,heevx", "--method-hetrd", mh, "--type",
                            "s,d", "--dim", "300", "--nb", "64", "--target", target], env=env, capture_output=True,
                           text=True, timeout=600)
        out = r.stdout + r.stderr
        assert r.returncode == 0 and "all tests passed" in out, out[-4000:]
        assert out.count("pass") >= 4, out[-4000:]


def test_native_tester():
    run_native_tester("h")


def test_python_tester(capsys):
    from slate_d35_amd import tester
    rc = tester.main(["stein", "heevx", "--dim", "300", "--nb", "64", "--type", "s,d", "--target", "h"])
    out = capsys.readouterr().out
    assert rc == 0 and "all tests passed" in out, out
    assert s.ops.stein_stats()["n"] == 300 and s.ops.stein_stats()["failed"] == 0
