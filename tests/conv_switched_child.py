"""Body of the tests of the once-read conv switches.  The library reads BG_NO_C16, BG_NO_ROWS, BG_WGRAD_NO_STRIP, BG_WGRAD_NO_TC and
BG_WGRAD_NO_TG into process-wide statics, so the fallbacks they expose can only run in a process STARTED with them set:
tests/test_conv_cases_cpu.py starts this file with `plan` (the restated planners against the library's host-only queries, no GPU) and
tests/test_conv_exact_gpu.py with `gpu` (conv_cases.SWITCHED_ROUTES / SWITCHED_WGRAD on exact data, as the tests of that file run
theirs).  Prints one line that ends in "ok"; any failure is an exception."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np

import conv_cases as CC


def plan():
    from blurred_gan_amd import _lib
    from test_conv_cases_cpu import _sweep
    lib = _lib.load()
    shapes = [c[0] for c in CC.ROUTE_CASES] + [c[0] for c in CC.WGRAD_CASES] + _sweep(1500, 7)
    modes = set()
    for (B, H, W, Ci, Co, s) in shapes:
        pl = CC.plan_wgrad(B, H, W, Ci, Co, s)
        modes.add(pl["mode"])
        assert lib.bg_conv2d_bwd_filter_workspace_bytes(B, H, W, Ci, Co, 5, s) == pl["ws_bytes"], (B, H, W, Ci, Co, s, pl)
        for bwd in (0, 1):
            assert lib.bg_conv2d_splitk_workspace_bytes(bwd, B, H, W, Ci, Co, 5, s) == CC.splitk_workspace_bytes(bwd, B, H, W, Ci, Co, 5, s)
            assert CC.route(bwd, B, H, W, Ci, Co, s)["family"] not in (CC.C16, CC.RS, CC.RG)
    assert modes == {0, 1, 2, 3, 4, 5, 10, 11, 12, 20, 21, 22}, modes
    for bwd, shape, family in CC.SWITCHED_ROUTES:
        assert CC.route(bwd, *shape)["family"] == family, (bwd, shape, CC.route(bwd, *shape)["family"])
    for shape, mode in CC.SWITCHED_WGRAD:
        assert CC.plan_wgrad(*shape)["mode"] == mode, (shape, CC.plan_wgrad(*shape)["mode"])
    print(f"{len(shapes)} geometries, {len(CC.SWITCHED_ROUTES)} + {len(CC.SWITCHED_WGRAD)} cases: plan ok")


def gpu():
    import test_conv_exact_gpu as T
    for bwd, shape, family in CC.SWITCHED_ROUTES:
        for recipe in ("dense", "decode"):
            act, w = (CC.make_dgrad if bwd else CC.make_fwd)(shape, recipe)
            ref = CC.ref_dgrad(act, w, shape[5], shape[1:3]) if bwd else CC.ref_fwd(act, w, shape[5])
            out, d = T.run_route(bwd, shape, act, w)                      # asserts the launch names, the tile, the guard bands
            assert d["family"] == family, (bwd, shape, d["family"])
            assert np.array_equal(out, ref), f"{d['names'][0]} {CC.case_id(shape)} [{recipe}]: {CC.describe_wrong(out, ref, shape[3], recipe, bwd)}"
    for shape, mode in CC.SWITCHED_WGRAD:
        assert CC.plan_wgrad(*shape)["mode"] == mode
        for recipe in ("dense", "decode"):
            x, dy, pix = CC.make_wgrad(shape, recipe)
            ref = CC.ref_wgrad(x, dy, shape[5])
            dw = T.run_wgrad(shape, x, dy)
            assert np.array_equal(dw, ref), f"filter gradient {CC.case_id(shape)} mode {mode} [{recipe}]: " + \
                (CC.decode_wgrad(dw, ref, pix, shape) if recipe == "decode" else f"{int((dw != ref).sum())} of {ref.size} wrong")
    print(f"{len(CC.SWITCHED_ROUTES)} + {len(CC.SWITCHED_WGRAD)} cases: gpu ok")


if __name__ == "__main__":
    assert CC.OFF == set(CC.SWITCHED_ENV), "start this file with conv_cases.SWITCHED_ENV in the environment"
    {"plan": plan, "gpu": gpu}[sys.argv[1]]()
