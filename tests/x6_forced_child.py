"""Body of the forced half of tests/test_conv_x6_exact_gpu.py.  The library reads BG_CONV_X6_FORCE into a process-wide static, so the
geometries off the bf16x6 dispatch table can only run the split kernel in a process STARTED with it set: that test starts this file
once.  Runs x6_cases.ROUTE_CASES (three recipes each), MUST_NOT_RUN, EPI_CASES, STATS_CASES, PRECISION_CASES and SCALING_CASES as the
check_* functions of that test define them, stops at the first failure (an exception), prints one "[x6 precision]" line per
precision case and a last line that ends in "ok"."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import x6_cases as X


def main():
    import test_conv_x6_exact_gpu as T
    t0 = time.time()
    for bwd, shape, k, _ in X.ROUTE_CASES:
        T.check_case(bwd, shape, k)
    for bwd, shape, k in X.MUST_NOT_RUN:
        T.check_case(bwd, shape, k, expect=False)
    t1 = time.time()
    print("outputs with a nonzero reference that differ from it, per recipe:", T.INEXACT, flush=True)
    assert T.INEXACT["pieces"] == 0
    for case in X.EPI_CASES:
        T.check_epilogues(*case)
    for case in X.STATS_CASES:
        T.check_statistics(*case)
    t2 = time.time()
    for case in X.PRECISION_CASES:
        T.check_precision(*case)
    for case in X.SCALING_CASES:
        T.check_scaling(*case)
    t3 = time.time()
    print(f"{len(X.ROUTE_CASES)} route cases x {len(X.RECIPES)} recipes + {len(X.MUST_NOT_RUN)} that must not run {t1 - t0:.1f} s, "
          f"{len(X.EPI_CASES)} epilogue x 7 + {len(X.STATS_CASES)} statistics cases {t2 - t1:.1f} s, "
          f"{len(X.PRECISION_CASES)} precision + {len(X.SCALING_CASES)} scaling cases {t3 - t2:.1f} s: ok")


if __name__ == "__main__":
    assert os.environ.get("BG_CONV_X6_FORCE") == "1", "start this file with BG_CONV_X6_FORCE=1 in the environment"
    main()
