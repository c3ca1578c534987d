"""Child process of test_stebz_gpu.py: SLATE_STEBZ_POINTS is read when the
library chooses P, so each P gets a fresh process.  Runs the shared cases of
stebz_cases.py on the device for a few sizes and prints the P in effect."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import slate_d35_amd as s  # noqa: E402
import stebz_cases as C  # noqa: E402


def main():
    want = int(os.environ["SLATE_STEBZ_POINTS"])
    for dt in (np.float64, np.float32):
        for n in (2, 65, 257, 1000):
            C.check_stebz_random(n, dt, "d")
            st = s.ops.stebz_stats()
            assert st["points"] == want and st["launches"] == 1 and st["host_syncs"] == 1, st
            C.check_ranges(n, dt, "d")
            C.check_bdsbz_random(n, dt, "d")
    C.check_stebz_laplacian(1000, "d")
    C.check_stebz_wilkinson("d")
    C.check_stebz_direct_sum("d")
    C.check_bdsbz_ones(257, "d")
    C.check_bdsbz_zero_entry("d")
    C.check_bdsbz_graded("d")
    print(f"STEBZ_WORKER_OK points={want}")


if __name__ == "__main__":
    main()
