"""Sturm-count bisection on the host target (csrc/include/slate_amd/sturm.hh,
host::sturm_counts / host::stebz_range, csrc/src/stebz.cc): the count, stebz
and bdsbz with every range, the refusals, heev / svd_vals / sygv with the
bisection methods, the C entry points and both testers.  The cases and their
bounds are in stebz_cases.py, shared with test_stebz_gpu.py."""
import os
import socket
import subprocess

import numpy as np
import pytest

import slate_d35_amd as s
import stebz_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "slate_d35_amd")
TG = "h"


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", C.SIZES)
def test_sturm_count_exact(n, dt):
    C.check_sturm_count(n, dt, TG)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", C.SIZES)
def test_stebz_random(n, dt):
    C.check_stebz_random(n, dt, TG)


@pytest.mark.parametrize("n", C.SIZES[1:])
def test_stebz_laplacian_closed_form(n):
    C.check_stebz_laplacian(n, TG)


def test_stebz_wilkinson():
    C.check_stebz_wilkinson(TG)


def test_stebz_direct_sum_repeated():
    C.check_stebz_direct_sum(TG)


def test_stebz_all_zero_and_empty():
    C.check_stebz_zero(TG)


def test_stebz_scaled():
    C.check_stebz_scaled(TG)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", C.SIZES)
def test_ranges(n, dt):
    C.check_ranges(n, dt, TG)


def test_refusals():
    C.check_refusals(TG)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", C.SIZES)
def test_bdsbz_random(n, dt):
    C.check_bdsbz_random(n, dt, TG)


@pytest.mark.parametrize("n", C.SIZES)
def test_bdsbz_ones_closed_form(n):
    C.check_bdsbz_ones(n, TG)


def test_bdsbz_zero_entry():
    C.check_bdsbz_zero_entry(TG)


def test_bdsbz_graded_float32():
    C.check_bdsbz_graded(TG)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", [130, 257])
def test_heev_bisection(n, dt):
    C.check_heev_bisection(n, dt, TG)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", [130, 257])
def test_svd_vals_bisection(n, dt):
    C.check_svd_vals_bisection(n, dt, TG)


def test_sygv_bisection():
    C.check_sygv_bisection(TG)


def test_host_stats():
    d, e, _ = C.random_tri(65, "float64")
    s.stebz(d, e, target=TG)
    st = s.ops.stebz_stats()
    assert st == dict(n=65, values=65, points=1, steps=st["steps"], launches=0, host_syncs=0)
    assert 1 <= st["steps"] <= 70   # log2(start interval / (2 eps)) for a unit max-norm matrix


C_SRC = r"""
#include <stdio.h>
#include <math.h>
#include "slate_amd/c_api.h"
int main(void) {
    enum { N = 10 };
    double d[N], e[N - 1], w[N], sv[N];
    float df[N], ef[N - 1], wf[N];
    int64_t nf = -1;
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < N; ++i) { d[i] = 2; df[i] = 2; }
    for (int i = 0; i + 1 < N; ++i) { e[i] = -1; ef[i] = -1; }
    slate_Options o[1] = {{slate_Option_Target, 'H', 0.0}};
    if (slate_stebz_r64('A', 0, 0, 0, 0, N, d, e, &nf, w, 1, o) != 0 || nf != N) return 1;
    double err = 0;
    for (int k = 1; k <= N; ++k) err = fmax(err, fabs(w[k - 1] - (2 - 2 * cos(k * pi / (N + 1)))));
    if (slate_stebz_r64('I', 0, 0, 2, 4, N, d, e, &nf, sv, 1, o) != 0 || nf != 3 || sv[0] != w[1] || sv[2] != w[3])
        return 2;
    if (slate_stebz_r32('V', 0.5f, 2.5f, 0, 0, N, df, ef, &nf, wf, 1, o) != 0 || nf != 4) return 3;
    for (int i = 0; i + 1 < N; ++i) e[i] = 1;
    for (int i = 0; i < N; ++i) d[i] = 1;
    if (slate_bdsbz_r64('A', 0, 0, 0, 0, N, d, e, &nf, sv, 0, 0) != 0 || nf != N) return 4;
    double errs = 0;
    for (int k = 1; k <= N; ++k) errs = fmax(errs, fabs(sv[k - 1] - 2 * cos(k * pi / (2 * N + 1))));
    int refused = slate_stebz_r64('V', 1.0, 1.0, 0, 0, N, d, e, &nf, w, 0, 0);
    printf("err %.3e errs %.3e refused %d (%s)\n", err, errs, refused, slate_last_error());
    printf("constants %d %d %d %d\n", slate_MethodSVD_Bisection, slate_MethodEig_QR, slate_MethodEig_DC,
           slate_MethodEig_Bisection);
    return (err <= 1e-14 && errs <= 1e-14 && refused == -1) ? 0 : 5;
}
"""


def test_c_api(tmp_path):
    src, exe = tmp_path / "stebz_c.c", tmp_path / "stebz_c"
    src.write_text(C_SRC)
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT}/csrc/include", str(src), f"-L{PKG}", "-lslate_amd",
                    f"-Wl,-rpath,{PKG}", "-lm", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "constants 66 81 68 66" in r.stdout and "vl < vu" in r.stdout, r.stdout
    f90 = open(os.path.join(ROOT, "csrc", "api", "slate_c_api.f90")).read()
    for name in ("slate_MethodEig_Bisection = 66", "slate_MethodEig_QR = 81", "slate_MethodEig_DC = 68",
                 "slate_MethodSVD_Bisection = 66", "slate_stebz_r64", "slate_bdsbz_r32"):
        assert name in f90, name


def _free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def run_native_tester(target):
    r = subprocess.run(["make", "tester"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    port = _free_port()
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               SLATE_MASTER_PORT=str(port), SLATE_COMM="host", OMP_NUM_THREADS="2")
    r = subprocess.run([os.path.join(ROOT, "bin", "slate_tester"), "stebz,bdsbz,heev_vals,svd_vals", "--method-eig",
                        "bisection", "--method-svd", "bisection", "--type", "s,d", "--dim", "300", "--nb", "64",
                        "--target", target], env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "all tests passed" in out, out[-4000:]
    assert out.count("pass") >= 8, out[-4000:]
    assert out.count("method_eig=bisection") == 2 and out.count("method_svd=bisection") == 2, out[-4000:]


def test_native_tester():
    run_native_tester("h")


def test_python_tester(capsys):
    from slate_d35_amd import tester
    rc = tester.main(["stebz", "bdsbz", "heev_vals", "svd_vals", "--method-eig", "bisection", "--method-svd",
                      "bisection", "--dim", "300", "--nb", "64", "--type", "s,d", "--target", "h"])
    out = capsys.readouterr().out
    assert rc == 0 and "all tests passed" in out, out
    assert out.count("method_eig=bisection") == 2 and out.count("method_svd=bisection") == 2, out
    assert s.ops.stebz_stats()["values"] == 300
