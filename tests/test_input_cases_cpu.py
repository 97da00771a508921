"""What the case list of the input pipeline's kernel tests (tests/input_cases.py) reaches, proved from arithmetic on the list alone: no
GPU, no kernel.  The launch constants the list restates are checked against the text of csrc/input.hip, csrc/misc.hip and the grid cap both take from csrc/common.h, so the list
cannot drift from the launches unnoticed; the two oracles alone decide that no geometry needs a yardstick wider than the dense kernel's
atol."""
import os
import re

import numpy as np
import pytest

import input_cases as IC
from helpers import YARDSTICK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blurred-gan_amd", "csrc")


class Facts:
    """The situations one case puts a kernel in, from its numbers alone."""

    def __init__(self, c):
        self.name, self.N, self.B, (self.Hs, self.Ws), (self.Hd, self.Wd), self.C, self.idx, self.flip = c
        self.P = self.Hd * self.Wd
        self.n_pix = self.B * self.P
        self.vec = self.C in IC.VEC_C
        self.n_grp = self.n_pix // 4 if self.vec else 0
        self.tail = self.n_pix % 4 if self.vec else 0
        # the units of the grid-stride loop and the workgroups it is given
        self.units = -(-self.n_pix // 4) if self.vec else self.n_pix
        self.blocks = max(1, min(-(-self.units // IC.THREADS), IC.MAX_BLOCKS))
        self.loop_units = self.n_grp if self.vec else self.n_pix
        self.trips = -(-self.loop_units // (self.blocks * IC.THREADS))
        first = 4 * np.arange(self.n_grp, dtype=np.int64)                    # first and last pixel of every group
        last = first + 3
        self.row_crossings = int(((first // self.Wd != last // self.Wd) & (first // self.P == last // self.P)).sum())
        cross = np.nonzero(first // self.P != last // self.P)[0]
        self.sample_crossings = [(int(g), int(first[g] // self.P), int(last[g] // self.P)) for g in cross]
        self.down = self.Hs > self.Hd and self.Ws > self.Wd
        self.up = self.Hs < self.Hd and self.Ws < self.Wd
        dyadic = lambda a, b: (max(a, b) % min(a, b) == 0) and ((max(a, b) // min(a, b)) & (max(a, b) // min(a, b) - 1)) == 0
        self.non_dyadic = not dyadic(self.Hs, self.Hd) or not dyadic(self.Ws, self.Wd)

    def crossing_changes_image_and_flag(self, first_group=0):
        return any(self.idx[a] != self.idx[b] and bool(self.flip[a]) != bool(self.flip[b])
                   for g, a, b in self.sample_crossings if g >= first_group)


FACTS = [Facts(c) for c in IC.CASES]


def some(pred):
    return [f.name for f in FACTS if pred(f)]


# ------------------------------------------------------------------ the list against the launches
def test_the_restated_launch_constants_are_the_sources():
    for path in ("input.hip", "misc.hip"):
        text = open(os.path.join(CSRC, path)).read()
        assert re.search(r"constexpr int kT = (\d+);", text).group(1) == str(IC.THREADS), path
        # either file's grid_for is bg::grid_cap (common.h) with its own kT: one workgroup per kT units, at most MAX_BLOCKS of them
        assert re.search(r"inline unsigned grid_for\(size_t n[^)]*\) \{ return bg::grid_cap\(n, kT(, per_thread)?\); \}", text), path
    grid = re.search(r"inline unsigned grid_cap\(size_t n, int threads, int per_thread = 1\) \{\s*return [^;]*?, (\d+) \* (\d+)\)\);",
                     open(os.path.join(CSRC, "common.h")).read())
    assert grid and int(grid.group(1)) * int(grid.group(2)) == IC.MAX_BLOCKS
    assert grid.group(0).count("threads") == 2 and "cdiv(n, (size_t)threads * per_thread)" in grid.group(0)
    text = open(os.path.join(CSRC, "input.hip")).read()
    # the channel counts of the four-pixel kernel, the units its grid is sized by, and the dense kernel's: one float per lane
    assert tuple(int(c) for c in re.findall(r"case (\d+): bg::launch\(u8_gather_resize_vec_kernel<\1>", text)) == IC.VEC_C
    assert "const dim3 grid(grid_for(bg::cdiv(n_pix, 4))), block(kT);" in text and "u8_gather_resize_any_kernel, dim3(grid_for(n_pix))" in text
    assert "u8_normalize_resize_kernel, dim3(grid_for(total)), dim3(kT)" in open(os.path.join(CSRC, "misc.hip")).read()
    assert IC.CAPACITY == IC.THREADS * IC.MAX_BLOCKS == 524288


def test_cases_are_well_formed_and_inside_the_contract():
    assert len({f.name for f in FACTS}) == len(FACTS)
    for f in FACTS:
        assert len(f.idx) == f.B == len(f.flip) and all(0 <= i < f.N for i in f.idx) and set(f.flip) <= {0, 1}, f.name
        assert {0, f.N - 1} <= set(f.idx) or (f.B == 1 and f.idx == [f.N - 1] and f.N > 1), f.name     # both ends of the dataset
        assert f.Hs * f.Ws * f.C < 2 ** 31 and f.P < 2 ** 31, f.name                 # the entry point's contract
        assert f.N <= 8, f.name                                                      # constant_images' distinct bytes
        if f.B > 1:
            assert any(a != b for a, b in zip(f.flip, f.flip[1:])), f.name           # flags differ between neighbours
        if f.B > 2:
            assert f.idx != sorted(f.idx), f.name
    assert some(lambda f: f.B > f.N)
    assert some(lambda f: len(set(f.idx)) < f.B and any(a == b for a, b in zip(f.idx, f.idx[1:])) and any(a != b for a, b in zip(f.idx, f.idx[1:])))


# ------------------------------------------------------------------ what the list reaches
@pytest.mark.parametrize("C", IC.VEC_C)
def test_four_pixel_kernel_situations_per_channel_count(C):
    mine = [f for f in FACTS if f.C == C]
    pick = lambda pred: [f.name for f in mine if pred(f)]
    assert pick(lambda f: f.down) and pick(lambda f: f.up), "a true downscale and a true upscale"
    assert pick(lambda f: (f.down or f.up) and f.non_dyadic)
    assert not pick(lambda f: (f.Hs, f.Ws) == (f.Hd, f.Wd))
    for tail in range(4):
        assert pick(lambda f: f.n_grp > 0 and f.tail == tail), f"a tail of {tail} behind at least one group"
    assert pick(lambda f: f.n_pix < 4 and f.n_grp == 0 and f.tail == f.n_pix), "the tail alone"
    assert pick(lambda f: f.Wd % 4 != 0 and f.row_crossings > 0), "a group over a row end"
    assert pick(lambda f: f.P % 4 != 0 and f.crossing_changes_image_and_flag()), "a group over a sample end, image and flag changing"
    # a group over a sample end between two samples of the SAME image too (the pointer is taken again, to the same place)
    assert pick(lambda f: any(f.idx[a] == f.idx[b] for _, a, b in f.sample_crossings))


def test_the_one_pixel_kernel_runs_at_two_other_channel_counts():
    assert some(lambda f: f.C == 2) and some(lambda f: f.C == 5)
    assert {f.C for f in FACTS} - set(IC.VEC_C) == {2, 5}


def test_degenerate_taps_and_mirrors():
    assert some(lambda f: f.Hs == 1 and f.Hd > 1) and some(lambda f: f.Ws == 1 and f.Wd > 1)
    assert some(lambda f: f.Hd == 1 and f.Hs > 1) and some(lambda f: f.Wd == 1 and f.Ws > 1)
    for f in FACTS:
        if f.Hs == 1:
            _, lo, hi = IC.taps(f.Hd, 1)
            assert not lo.any() and not hi.any()
    mirrored = lambda f: any(f.flip)
    assert some(lambda f: mirrored(f) and f.Wd % 2 == 1 and f.Wd > 1) and some(lambda f: mirrored(f) and f.Wd % 2 == 0)
    assert some(lambda f: mirrored(f) and f.Wd == 1)


def test_an_upscale_clamps_both_taps_at_both_ends():
    def clamps(n_out, n_in):
        pos, lo, hi = IC.taps(n_out, n_in)
        return n_out > n_in and pos[0] < 0 and lo[0] == 0 and np.ceil(pos[-1]) > n_in - 1 and hi[-1] == n_in - 1
    for C in IC.VEC_C:
        assert [f.name for f in FACTS if f.C == C and clamps(f.Wd, f.Ws) and clamps(f.Hd, f.Hs)], C


def test_second_trips_with_ragged_ends():
    vec = [f for f in FACTS if f.vec and f.trips >= 2]
    anyc = [f for f in FACTS if not f.vec and f.trips >= 2]
    assert vec and anyc
    for f in vec + anyc:
        assert f.blocks == IC.MAX_BLOCKS and f.loop_units > IC.CAPACITY and f.loop_units % IC.CAPACITY % IC.THREADS != 0, f.name
    # the four-pixel kernel: a tail behind a second trip, a second trip that starts mid-sample, and a sample end inside a group of the
    # second trip with image and flag changing
    assert [f.name for f in vec if f.tail == 3]
    assert [f.name for f in vec if (4 * IC.CAPACITY) % f.P != 0]
    assert [f.name for f in vec if f.crossing_changes_image_and_flag(first_group=IC.CAPACITY)]
    t = IC.case("c1_second_trip")
    assert (t[2] * 255 * 257, t[2] * 255 * 257 // 4) == (2162655, 540663) and IC.case("c2_second_trip")[2] * 255 * 257 == 589815
    # the smallest batches that qualify at this output size
    assert (t[2] - 1) * 65535 // 4 <= IC.CAPACITY and (IC.case("c2_second_trip")[2] - 1) * 65535 <= IC.CAPACITY
    # the dense kernel's own case: past the capacity, ragged
    _, B, _, (Hd, Wd), C = IC.DENSE_CASE
    total = B * Hd * Wd * C
    assert IC.CAPACITY < total < 2 * IC.CAPACITY and (total - IC.CAPACITY) % IC.THREADS != 0
    # every other case stays small
    assert all(f.n_pix * f.C <= 4096 for f in FACTS if f.trips < 2)


# ------------------------------------------------------------------ the tolerance the GPU test will apply
def test_no_geometry_needs_a_yardstick_above_the_dense_kernels_atol():
    """On the two oracles alone: where the float32 oracle does not meet the point rule itself the bound is YARDSTICK x its largest
    deviation, and that may not exceed IC.YARDSTICK_CAP.  A cap on the choice of geometries and bytes, not a measurement."""
    names = [f.name for f in FACTS]
    for name in names:
        _, _, _, rule, dev32 = IC.case_references(name)
        print(f"{name}: float32 oracle max|dev| {dev32:.3e}, rule {rule}")
        assert rule == "point" or YARDSTICK * dev32 <= IC.YARDSTICK_CAP, (name, dev32)
    _, B, src_hw, dst_hw, C = IC.DENSE_CASE
    rule, _, dev32 = IC.tolerance(*IC.references(IC.data(IC.DENSE_CASE[0], B, *src_hw, C), dst_hw))
    print(f"{IC.DENSE_CASE[0]}: float32 oracle max|dev| {dev32:.3e}, rule {rule}")
    assert rule == "point" or YARDSTICK * dev32 <= IC.YARDSTICK_CAP


def test_constant_images_have_distinct_bytes():
    src, v = IC.constant_images(8, 2, 3, 4)
    assert len(set(v.tolist())) == 8 and (src == v[:, None, None, None]).all()
    want = (v.astype(np.float32) - np.float32(127.5)) / np.float32(127.5)
    assert len(set(want.tolist())) == 8
