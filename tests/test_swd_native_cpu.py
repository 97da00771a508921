"""CPU tests of the native SWD metric (csrc/swd.hip, swd_native.py): the new entries are declared, exported and bound; argument
errors are statuses returned before anything is launched; the Python surface refuses what it cannot take; the demos know the
two flags; and the ISA of the kernels: no spills, no private segment, no fused multiply-add in the bit-exact pyramid / ingest."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

NEW = ["bg_swd_ingest_f32", "bg_pyr_down_f32", "bg_pyr_up_f32", "bg_swd_gather_f32", "bg_swd_standardize_workspace_bytes",
       "bg_swd_standardize_f32", "bg_sort_rows_f32", "bg_abs_diff_mean_workspace_bytes", "bg_abs_diff_mean_f32"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge._load_build_module().build_lib(verbose=False)
    from blurred_gan_amd import _lib
    return _lib.load()


def test_new_symbols_declared_exported_bound_and_abi_unchanged(lib):
    from blurred_gan_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "bgan.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in bgan.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.bg_version() == 5 and _lib.ABI_VERSION == 5
    for wrapper in ("swd_ingest", "pyr_down", "pyr_up", "swd_gather", "swd_standardize", "sort_rows", "abs_diff_mean"):
        assert callable(getattr(ops, wrapper))
    import __graft_entry__ as ge
    assert "swd.hip" in ge._load_build_module().SOURCES


def test_argument_errors_are_statuses(lib):
    """Host buffers stand in for device memory: a refused call returns before it would touch them."""
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    OK_NULL, SHAPE, WS = -6, -1, -5
    # null pointers
    assert lib.bg_swd_ingest_f32(None, p, 1, 16, 16, 3, 1, 1.0, 0.0, None) == OK_NULL
    assert b"bg_swd_ingest_f32" in lib.bg_last_error()
    assert lib.bg_pyr_down_f32(p, None, 1, 16, 16, None) == OK_NULL
    assert lib.bg_pyr_up_f32(None, None, p, 1, 8, 8, None) == OK_NULL
    assert lib.bg_swd_gather_f32(p, None, p, p, 1, 16, 16, 7, 4, None) == OK_NULL
    assert lib.bg_swd_standardize_f32(None, 4, 7, None, p, 1 << 20, None) == OK_NULL
    assert lib.bg_sort_rows_f32(None, 1, 8, None) == OK_NULL
    assert lib.bg_abs_diff_mean_f32(p, None, 8, 1, p, p, 1 << 20, None) == OK_NULL
    # shapes
    assert lib.bg_swd_ingest_f32(p, p, 1, 16, 16, 2, 1, 1.0, 0.0, None) == SHAPE            # C = 2
    assert b"C=2" in lib.bg_last_error()
    assert lib.bg_swd_ingest_f32(p, p, 1, 16, 16, 4, 0, 1.0, 0.0, None) == SHAPE
    assert lib.bg_pyr_down_f32(p, p, 1, 2, 16, None) == SHAPE                               # H = 2
    assert lib.bg_pyr_down_f32(p, p, 1, 16, 2, None) == SHAPE
    assert lib.bg_pyr_up_f32(p, None, p, 1, 1, 8, None) == SHAPE                            # h = 1
    assert lib.bg_swd_gather_f32(p, p, p, p, 1, 16, 16, 6, 4, None) == SHAPE                # even nhood
    assert lib.bg_swd_gather_f32(p, p, p, p, 1, 16, 5, 7, 4, None) == SHAPE                 # nhood > min(H, W)
    assert lib.bg_swd_standardize_f32(p, 4, 4, None, p, 1 << 20, None) == SHAPE
    assert lib.bg_sort_rows_f32(p, 1, 0, None) == SHAPE                                     # n = 0
    assert lib.bg_sort_rows_f32(p, 0, 8, None) == SHAPE
    assert lib.bg_sort_rows_f32(p, 1, (1 << 24) + 1, None) == SHAPE
    assert lib.bg_sort_rows_f32(p, 1 << 16, 1 << 15, None) == SHAPE                         # rows * n = 2^31
    assert lib.bg_abs_diff_mean_f32(p, p, 0, 1, p, p, 1 << 20, None) == SHAPE
    assert lib.bg_abs_diff_mean_f32(p, p, 8, 0, p, p, 1 << 20, None) == SHAPE
    # workspaces: the query is a pure host function, a short or missing one is refused
    need = lib.bg_swd_standardize_workspace_bytes(640, 7)
    assert need > 0 and lib.bg_swd_standardize_workspace_bytes(0, 7) == 0
    assert lib.bg_swd_standardize_f32(p, 640, 7, None, p, need - 1, None) == WS
    assert lib.bg_swd_standardize_f32(p, 640, 7, None, None, need, None) == WS
    need = lib.bg_abs_diff_mean_workspace_bytes(128 * 2048, 4)
    assert need >= 4 * 8 and lib.bg_abs_diff_mean_workspace_bytes(0, 4) == 0
    assert lib.bg_abs_diff_mean_f32(p, p, 128 * 2048, 4, p, p, need - 1, None) == WS
    assert b"workspace" in lib.bg_last_error()
    # alignment: floats on 4 bytes, doubles on 8
    assert lib.bg_sort_rows_f32(p + 2, 1, 8, None) == -2
    assert lib.bg_abs_diff_mean_f32(p, p, 8, 1, p + 4, p, 1 << 20, None) == -2


def test_native_metric_refuses_host_arrays():
    from blurred_gan_amd import metrics
    import torch
    m = metrics.SWDMetric(native=True, seed=0)
    x = np.zeros((2, 3, 16, 16), np.float32)
    with pytest.raises(TypeError):
        m.update_state(x, x)
    with pytest.raises(TypeError):
        m.update_state(torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16))         # a CPU tensor is no better
    with pytest.raises(ValueError):
        metrics.SWDMetric(native=True, data_format="CHWN")
    with pytest.raises(ValueError):
        metrics.SWDMetric(data_format="NHWC")                                          # belongs to the native path
    d = metrics.SWDMetric()                                                            # the default object is what it was
    assert (d.native, d.on_device, d.data_format) == (False, False, "NCHW")


def test_callback_without_preprocessing_needs_native():
    from blurred_gan_amd import callbacks
    with pytest.raises(ValueError, match="native"):
        callbacks.SWDMetricCallback(None)
    cb = callbacks.SWDMetricCallback(None, native=True, seed=1)
    m = cb.metric
    assert m.native and (m.data_format, m.scale, m.shift) == ("NHWC", 127.5, 127.5)
    x = object()
    assert cb.image_preprocessing_fn(x) is x
    fn = lambda images: images
    cb2 = callbacks.SWDMetricCallback(fn, native=True)
    assert cb2.image_preprocessing_fn is fn and cb2.metric.native and cb2.metric.data_format == "NCHW"
    assert not callbacks.SWDMetricCallback(fn).metric.native


def test_api_native_switch_defaults_off():
    from blurred_gan_amd import sliced_wasserstein as sw
    assert sw.API((4, 32, 32, 3), seed=1).native is False and sw.API((4, 32, 32, 3), seed=1, native=True).native is True


def test_native_module_refuses_an_active_program(monkeypatch):
    from blurred_gan_amd import program, swd_native
    monkeypatch.setattr(program, "active", lambda: object())
    for call in (lambda: swd_native.ingest(None), lambda: swd_native.pyr_down(None), lambda: swd_native.finalize_descriptors([]),
                 lambda: swd_native.level_distances([], [], 4, 128, None)):
        with pytest.raises(RuntimeError, match="step program"):
            call()


@pytest.mark.parametrize("demo", ["demo_mnist", "demo_celeba"])
def test_demo_parsers_know_the_swd_flags(demo):
    import importlib
    mod = importlib.import_module(demo)
    args = mod.make_parser().parse_args([])
    assert args.swd_every_n_examples == 0 and args.swd_samples == 1000
    args = mod.make_parser().parse_args(["--swd-every-n-examples", "50000", "--swd-samples", "64"])
    assert (args.swd_every_n_examples, args.swd_samples) == (50000, 64)
    assert "50000" in mod.make_parser().format_help()


def test_swd_kernels_do_not_spill_and_the_exact_ones_do_not_fuse(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "swd.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-w", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "blurred-gan_amd", "csrc", "swd.hip"), "-o", str(out)], check=True)
    isa = out.read_text()
    seen = set()
    for m in re.finditer(r"\.name:\s+(\S*_kernel\S*)\n(.*?)\.wavefront_size", isa, flags=re.S):
        seen.add(m.group(1))
        for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            v = re.search(r"\." + key + r":\s+(\d+)", m.group(2))
            assert v and int(v.group(1)) == 0, (m.group(1), key)
    for stem in ("swd_ingest_kernel", "pyr_down_kernel", "pyr_up_kernel", "swd_gather_kernel", "swd_stats_kernel",
                 "swd_stats_final_kernel", "swd_standardize_apply_kernel", "sort_chunk_kernel", "sort_global_kernel", "abs_diff_partial_kernel",
                 "abs_diff_final_kernel"):
        assert any(stem in n for n in seen), stem
    exact = [n for n in seen if any(s in n for s in ("swd_ingest_kernel", "pyr_down_kernel", "pyr_up_kernel"))]
    assert len(exact) == 6 + 2 + 2, exact          # ingest: 3 layouts x {4, 1}; pyr_down, pyr_up: {4, 1}
    for name in exact:
        body = re.search(r"^" + re.escape(name) + r":(.*?)s_endpgm", isa, flags=re.S | re.M).group(1)
        assert "v_fma_f32" not in body and "v_fmac_f32" not in body and "v_pk_fma_f32" not in body, name
    for name in seen:                              # the wide bodies really move 16 bytes
        if re.search(r"(pyr_down_kernel|pyr_up_kernel|swd_gather_kernel|sort_global_kernel)ILi4E", name):
            body = re.search(r"^" + re.escape(name) + r":(.*?)s_endpgm", isa, flags=re.S | re.M).group(1)
            assert "global_store_dwordx4" in body, name
