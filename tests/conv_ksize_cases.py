"""Case tables of the fp32 conv family at kernel sizes 3 and 1, on the exact integer data, the float64 reference and the restated host
dispatch of tests/conv_cases.py (every function there takes k).  tests/test_conv_ksize_cases_cpu.py proves the tables on the CPU --
exact in float32, on the claimed route, the cell union equal to a written-out set, the planners equal to the library's host-only
queries at k = 1 and 3 -- and tests/test_conv_ksize_exact_gpu.py runs them through the harness of tests/test_conv_exact_gpu.py.

A case shape is (B, H, W, Cin, Cout, stride, k) on the conv's input side.  The cells are those of conv_cases.route_cells /
wgrad_cells plus the ones only a kernel size other than 5 has (route_cells / wgrad_cells below): a data-gradient phase with no tap
(k = 1, stride 2), a merged phase pair of which one phase, or both, is tapless, split-K over one tap, the SAME pads (0, 1) and (1, 1)
of k = 3 stride 2, thin row kernels at 5 thin channels, conv_thin_n_mfma with 15 and with 16 live columns, the tap-sorted filter
gradient with 9 taps and with 1, and every 5x5-only fast path stepping aside.

Shapes start from the table of tests/test_conv_ksize_gpu.py, whose route claims were made on the GPU, cut to the smallest that still
reach the cell.  Sizes: nothing is above the tap-grouped step-aside shape 128 x 32 x 32 x 16 -> 16 (2 097 152 elements a side), and
only the four merged-phase data gradients are otherwise above a million elements (1.05 M and 1.31 M of dx): launch_igemm merges
phases only when one phase alone has more than 256 M tiles of 128 rows, i.e. more than 32 768 pixels per phase and 131 072 pixels of
dx, and the gather-GEMM needs N = Cin >= 8 -- 8 channels is the least.  Their forward (8 -> 16 channels: conv_direct) is not listed;
a direction whose family is None is not run."""
import conv_cases as CC

IG, RS, RG = CC.IG, CC.RS, CC.RG
TNM, TKM, TNPA, TNP, TN, TK, DI = ("conv_thin_n_mfma", "conv_thin_k_mfma", "conv_thin_n_patch_all", "conv_thin_n_patch", "conv_thin_n",
                                   "conv_thin_k", "conv_direct")


def k3s2_pads(H, W):
    """SAME pads (top, left) of a 3x3 stride-2 conv: 0 on an even extent (the one padding row is at the far end), 1 on an odd one."""
    return CC.same_pads(H, 3, 2)[1], CC.same_pads(W, 3, 2)[1]


def route_cells(bwd, d, shape):
    """conv_cases.route_cells plus the cells of a kernel size other than 5."""
    B, H, W, Ci, Co, s, k = shape
    c = set(CC.route_cells(bwd, d, B))
    f, way = d["family"], "dgrad" if bwd else "fwd"
    p = CC.gather_params(bwd, B, H, W, Ci, Co, k, s)
    nt = [len(g["taps"]) for g in p["ph"]]
    if k == 3 and s == 2:
        c.add("k3s2:pad%d%d" % k3s2_pads(H, W))
    if min(nt) == 0:
        c.add(f"{f[5:]}:empty_phases")
    if f == "conv_igemm":
        if d["ks"] > 1:
            c.add(f"igemm:splitk:{max(nt)}tap:{way}")
        if d["sorted"]:
            skipped = any(CC._live(p, g, ay, ax) < len(g["taps"]) for g in p["ph"] for ay in range(g["Ha"]) for ax in range(g["Wa"]))
            c.add(f"igemm:pos_major:k{k}:" + ("padding_skipped" if skipped else "no_padding_tap"))
        if min(nt) == 0:
            c.add(f"igemm:empty_phases:{d['BM']}x{d['BN']}")
        if d["pmerge"] == 2:
            c.add(f"igemm:pmerge2:k{k}:" + ("pos_major" if d["sorted"] else "image_major"))
            if CC.tapless_groups(p, 2):
                c.add("igemm:pmerge2:tapless_pair")
        if d["odd_phases"]:
            c.add(f"igemm:odd_map_phases:{H}x{W}")
    elif f == "conv_rows":
        c |= {f"rows:thin{d['N']}", f"rows:{way}:s{s}"}
    elif f == "conv_rows_thin_k":
        thin = Co if bwd else Ci
        c |= {f"rowsg:thin{thin}", f"rowsg:{way}:s{s}"}
        if (W * thin) % 4:
            c.add("rowsg:scalar_staging")
    elif f == "conv_thin_n_mfma":
        c |= {f"thin_n_mfma:k{k}:n{p['N']}", f"thin_n_mfma:ck{p['Ck']}"}
    elif f == "conv_thin_n_patch_all":
        c.add(f"patch_all:live_phases{sum(1 for n in nt if n)}")
    elif f == "conv_direct":
        c.add(f"direct:k{k}")
    return c


def wgrad_cells(pl, shape):
    """conv_cases.wgrad_cells plus the kernel size of every mode, the tap count of the tap-sorted order and the wide-row fall-back."""
    B, H, W, Ci, Co, s, k = shape
    c = set(CC.wgrad_cells(pl, B, s)) | {f"k{k}:mode{pl['mode']}"}
    if pl["tap_sorted"]:
        c.add(f"tap_sorted:{k * k}tap")
    # a geometry the row-MFMA kernels (modes 31 / 30) take by every condition of plan_wgrad but the 64 KB of LDS their rows need
    thin_ci = k == 3 and k * Ci <= 16 and Ci <= 4 and Co in (16, 32, 64) and pl["Wo"] % 4 == 0
    thin_co = k == 3 and k * Co <= 16 and Co <= 4 and Ci in (16, 32) and W % 4 == 0 and s == 1
    if (thin_ci and pl["mode"] in (10, 11)) or (thin_co and pl["mode"] in (20, 21)):
        c.add(f"wide_row:mode{pl['mode']}")
    return c


# (shape, forward family, forward cells, data-gradient family, data-gradient cells); a family of None: that direction is not run
ROUTE_CASES = [
    # ---- gather-GEMM: both tiles, both K steps, ragged M and N
    ((2, 8, 8, 32, 32, 2, 3), IG, {"igemm:128x32:bk16", "igemm:ragged_m", "k3s2:pad00"}, IG, {"igemm:128x32:bk16", "igemm:pmerge1"}),
    ((3, 8, 8, 32, 64, 1, 3), IG, {"igemm:64x64:bk16"}, IG, {"igemm:128x32:bk16"}),
    ((2, 16, 16, 64, 128, 2, 3), IG, {"igemm:64x64:bk16"}, IG, {"igemm:64x64:bk32", "igemm:pmerge1"}),
    ((2, 8, 8, 128, 32, 1, 3), IG, {"igemm:128x32:bk32", "igemm:splitk2"}, IG, {"igemm:64x64:bk16"}),
    ((3, 9, 7, 48, 24, 2, 3), IG, {"igemm:n24of32", "igemm:ragged_m", "k3s2:pad11"}, DI, {"direct:k3"}),   # dy has 24 channels: no 16-channel K step
    # ---- split-K: nine taps both ways; split forward and unsplit back (the one-tap phase has 16 K steps); ONE tap of 1024 channels
    ((5, 2, 2, 256, 512, 1, 3), IG, {"igemm:splitk4", "igemm:splitk:9tap:fwd"}, IG, {"igemm:splitk8", "igemm:splitk:9tap:dgrad"}),
    ((5, 2, 2, 256, 512, 2, 3), IG, {"igemm:splitk4", "igemm:splitk:9tap:fwd"}, IG, {"igemm:64x64:bk32", "igemm:ragged_m"}),
    ((130, 4, 4, 128, 256, 2, 3), IG, {"igemm:splitk2", "igemm:ragged_m"}, IG, {"igemm:64x64:bk32", "igemm:ragged_m"}),   # 520 rows
    ((5, 2, 2, 1024, 64, 1, 1), IG, {"igemm:splitk2", "igemm:splitk:1tap:fwd"}, IG, {"igemm:64x64:bk16"}),
    # ---- odd maps at k = 3 stride 2: pads (1, 1) and four phases of different extents
    ((3, 7, 7, 32, 48, 2, 3), IG, {"igemm:n48of64", "igemm:ragged_m", "k3s2:pad11"}, IG, {"igemm:odd_map_phases:7x7", "igemm:odd_map_phases"}),
    ((3, 9, 7, 32, 48, 2, 3), IG, {"igemm:n48of64", "k3s2:pad11"}, IG, {"igemm:odd_map_phases:9x7"}),
    # ---- position-major tiles (B a multiple of the tile, <= 64 positions): padding taps skipped at k = 3, none to skip at k = 1
    ((128, 4, 4, 64, 64, 1, 3), IG, {"igemm:pos_major:k3:padding_skipped", "igemm:m_fast0"}, IG, {"igemm:pos_major:k3:padding_skipped", "igemm:m_fast0"}),
    ((128, 8, 8, 32, 128, 2, 3), IG, {"igemm:pos_major:k3:padding_skipped", "igemm:m_fast1", "k3s2:pad00"},
     IG, {"igemm:pos_major:k3:padding_skipped", "igemm:128x32:bk32"}),
    ((128, 4, 4, 64, 64, 1, 1), IG, {"igemm:pos_major:k1:no_padding_tap"}, IG, {"igemm:pos_major:k1:no_padding_tap"}),
    # ---- k = 1 stride 2: the data gradient has ONE tap, in phase (0, 0); the other three phases store zeros over the NaN
    ((128, 8, 8, 32, 64, 2, 1), IG, {"igemm:pos_major:k1:no_padding_tap"}, IG, {"igemm:empty_phases:128x32", "igemm:pos_major:k1:no_padding_tap"}),
    ((3, 6, 6, 64, 32, 2, 1), IG, {"igemm:128x32:bk16"}, IG, {"igemm:empty_phases:64x64", "igemm:pmerge1"}),
    ((3, 7, 9, 32, 64, 2, 1), IG, {"igemm:64x64:bk16"}, IG, {"igemm:empty_phases:128x32", "igemm:odd_map_phases:7x9"}),
    # ---- phases merged in pairs (see the size note above); at k = 1 the pair (1, 2) has no tap at all
    ((640, 16, 16, 8, 16, 2, 3), None, set(), IG, {"igemm:pmerge2:k3:pos_major", "igemm:pmerge2"}),
    ((513, 16, 16, 8, 16, 2, 3), None, set(), IG, {"igemm:pmerge2:k3:image_major", "igemm:ragged_m"}),
    ((640, 16, 16, 8, 16, 2, 1), None, set(), IG, {"igemm:pmerge2:k1:pos_major", "igemm:pmerge2:tapless_pair"}),
    ((513, 16, 16, 8, 16, 2, 1), None, set(), IG, {"igemm:pmerge2:k1:image_major", "igemm:pmerge2:tapless_pair", "igemm:empty_phases:128x32"}),
    # ---- row kernels at k = 3: scatter form on the thin OUTPUT side, gather form on the thin CONTRACTION side
    ((5, 40, 16, 16, 5, 1, 3), RS, {"rows:fwd:w16", "rows:ipw4", "rows:ipw4:short_last", "rows:ragged_strip", "rows:thin5", "rows:fwd:s1"},   # strips 32 + 8
     RG, {"rowsg:dgrad", "rowsg:tg1", "rowsg:nt1", "rowsg:thin5", "rowsg:dgrad:s1", "rowsg:ragged_strip"}),
    ((3, 20, 32, 32, 3, 1, 3), RS, {"rows:fwd:w32", "rows:ipw2", "rows:ipw2:short_last", "rows:thin3"}, RG, {"rowsg:tg2", "rowsg:nt2", "rowsg:thin3"}),
    ((2, 36, 64, 64, 4, 1, 3), RS, {"rows:fwd:w64", "rows:ipw1", "rows:ragged_strip", "rows:thin4"}, RG, {"rowsg:tg4", "rowsg:nt4", "rowsg:thin4"}),
    ((2, 20, 128, 16, 1, 1, 3), RS, {"rows:fwd:w128", "rows:ipw1", "rows:thin1"}, RG, {"rowsg:dgrad", "rowsg:tg4", "rowsg:thin1"}),
    ((5, 32, 32, 3, 32, 2, 3), RG, {"rowsg:fwd", "rowsg:fwd:s2", "rowsg:tg1", "rowsg:nt2", "k3s2:pad00"}, RS, {"rows:dgrad:w16", "rows:ipw4:short_last", "rows:dgrad:s2"}),
    ((3, 40, 64, 5, 16, 2, 3), RG, {"rowsg:fwd", "rowsg:tg2", "rowsg:nt1", "rowsg:thin5", "rowsg:ragged_strip"},
     RS, {"rows:dgrad:w32", "rows:ipw2:short_last", "rows:ragged_strip", "rows:thin5"}),
    ((2, 44, 128, 4, 64, 2, 3), RG, {"rowsg:fwd", "rowsg:tg4", "rowsg:nt4", "rowsg:thin4"}, RS, {"rows:dgrad:w64", "rows:ragged_strip", "rows:thin4"}),
    ((2, 24, 256, 3, 16, 2, 3), RG, {"rowsg:fwd", "rowsg:tg4"}, RS, {"rows:dgrad:w128", "rows:ragged_strip"}),
    ((2, 18, 16, 1, 16, 1, 3), RG, {"rowsg:fwd:s1", "rowsg:thin1", "rowsg:ragged_strip"}, RS, {"rows:dgrad:w16", "rows:dgrad:s1", "rows:thin1"}),
    ((3, 31, 31, 3, 32, 2, 3), RG, {"rowsg:scalar_staging", "k3s2:pad11"}, RS, {"rows:dgrad:w16", "rows:ragged_strip"}),   # 93 floats a row
    ((2, 33, 32, 3, 64, 1, 3), RG, {"rowsg:fwd:s1", "rowsg:nt4", "rowsg:ragged_strip"}, RS, {"rows:dgrad:w32", "rows:ragged_strip"}),   # strips 16 + 16 + 1 / 32 + 1
    ((2, 20, 24, 2, 32, 1, 3), TKM, {"thin_k_mfma:nt1"}, TNP, {"thin_n_patch"}),            # 24-pixel rows: both row kernels decline
    # ---- the families behind the row kernels
    ((2, 12, 20, 16, 5, 1, 3), TNM, {"thin_n_mfma:k3:n5"}, DI, {"direct:k3"}),              # N = 5 at k = 3: 15 of 16 MFMA columns
    ((2, 9, 11, 48, 3, 1, 3), TNM, {"thin_n_mfma:ck48"}, TKM, {"thin_k_mfma:nt2"}),         # 48 channels in three chunks
    ((2, 9, 11, 20, 12, 1, 1), TNM, {"thin_n_mfma:k1:n12"}, DI, {"direct:k1"}),
    ((2, 8, 8, 24, 16, 1, 1), TNM, {"thin_n_mfma:k1:n16"}, IG, {"igemm:n24of32"}),          # all 16 columns
    ((2, 8, 8, 3, 16, 1, 1), TKM, {"thin_k_mfma:nt1"}, TNM, {"thin_n_mfma:k1:n3"}),         # a 1x1 stride-1 data gradient IS a forward rectangle
    ((3, 14, 14, 1, 64, 2, 3), TKM, {"thin_k_mfma:nt2"}, TNPA, {"patch_all:live_phases4", "patch_all:ck64", "patch_all:n1"}),
    ((3, 14, 14, 4, 32, 2, 1), TKM, {"thin_k_mfma:nt1"}, TNPA, {"patch_all:live_phases1", "thin_n_patch_all:empty_phases", "patch_all:n4"}),
    ((2, 14, 14, 16, 1, 2, 3), TNP, {"thin_n_patch"}, TKM, {"thin_k_mfma:nt1"}),
    ((2, 14, 14, 64, 1, 2, 3), TN, {"thin_n"}, TKM, {"thin_k_mfma:nt2"}),                   # the stride-2 patch of 64 channels is past 150 KB
    ((2, 9, 7, 128, 3, 2, 3), TN, {"thin_n"}, TK, {"thin_k"}),
    ((2, 9, 7, 3, 96, 2, 3), TK, {"thin_k"}, TN, {"thin_n"}),
    ((2, 9, 7, 20, 12, 2, 3), DI, {"direct:k3"}, DI, {"direct:k3"}),
    ((2, 9, 7, 20, 12, 2, 1), DI, {"direct:k1"}, DI, {"direct:k1", "direct:empty_phases"}),
    ((3, 8, 8, 32, 3, 2, 1), TNP, {"thin_n_patch"}, TKM, {"thin_k_mfma:empty_phases"}),            # empty phases on the thin kernels
    ((2, 9, 7, 3, 8, 2, 1), TKM, {"thin_k_mfma:nt1"}, TN, {"thin_n:empty_phases"}),
    ((2, 9, 7, 128, 3, 2, 1), TN, {"thin_n"}, TK, {"thin_k:empty_phases"}),
    # ---- the shapes of the 5x5-only row-staged 16-channel kernels (conv_c16_*): the gather-GEMM takes them
    ((3, 64, 64, 16, 32, 2, 3), IG, {"igemm:128x32:bk16"}, IG, {"igemm:128x32:bk16", "igemm:pmerge1"}),
    ((2, 128, 128, 16, 32, 2, 3), IG, {"igemm:128x32:bk16"}, IG, {"igemm:128x32:bk16", "igemm:pmerge1"}),
    # ---- production geometry, 3x3 stride 1: the tiny_k3 stacks (2x2x32 -> 32 transposed, 8x8x16 -> 3 image conv), the convs after
    # its two upsamples (4x4x32 -> 16, 8x8x16 -> 16) and the first and last upsample-then-conv stages of the 64x64 generator
    ((4, 2, 2, 32, 32, 1, 3), IG, {"igemm:128x32:bk16"}, IG, {"igemm:128x32:bk16"}),
    ((4, 8, 8, 16, 3, 1, 3), TNM, {"thin_n_mfma:k3:n3"}, TKM, {"thin_k_mfma:nt1"}),
    ((4, 4, 4, 32, 16, 1, 3), IG, {"igemm:128x32:bk16"}, IG, {"igemm:128x32:bk16"}),
    ((4, 8, 8, 16, 16, 1, 3), IG, {"igemm:128x32:bk16"}, IG, {"igemm:128x32:bk16"}),
    ((2, 8, 8, 512, 256, 1, 3), IG, {"igemm:64x64:bk32", "igemm:splitk8"}, IG, {"igemm:64x64:bk32", "igemm:splitk4"}),
    ((2, 64, 64, 64, 32, 1, 3), IG, {"igemm:128x32:bk16"}, IG, {"igemm:64x64:bk16"}),
]
C16_SHAPES = [(3, 64, 64, 16, 32, 2, 3), (2, 128, 128, 16, 32, 2, 3)]
PRODUCTION = [(4, 2, 2, 32, 32, 1, 3), (4, 8, 8, 16, 3, 1, 3), (4, 4, 4, 32, 16, 1, 3), (4, 8, 8, 16, 16, 1, 3), (2, 8, 8, 512, 256, 1, 3),
              (2, 64, 64, 64, 32, 1, 3)]

# (shape, mode, slabs the planner reports (1 = none), cells).  k k Cin <= 36 for a thin side of at most 4 channels, so the thin
# modes 12 and 22 (more than 96 rows of taps x channels) cannot be reached below k = 5, and the row-MFMA modes 30 / 31 take k = 3 only
WGRAD_CASES = [
    ((2, 7, 7, 96, 96, 1, 3), 1, 1, {"mode1:pow2_0", "k3:mode1"}), ((2, 4, 4, 128, 256, 2, 3), 1, 1, {"mode1:pow2_1"}),
    ((128, 4, 4, 96, 96, 1, 3), 1, 8, {"mode1:pow2_2", "tap_sorted:9tap"}), ((130, 4, 4, 128, 256, 2, 3), 1, 4, {"mode1:pow2_1", "reduce:float4"}),
    ((3, 6, 6, 128, 128, 1, 1), 1, 1, {"k1:mode1", "mode1:pow2_0"}),
    ((2, 7, 9, 48, 48, 1, 3), 2, 1, {"mode2:pow2_0", "k3:mode2"}), ((2, 16, 16, 64, 128, 2, 3), 2, 1, {"mode2:pow2_1"}),
    ((128, 4, 4, 64, 64, 1, 3), 2, 8, {"mode2:pow2_2", "tap_sorted:9tap"}), ((128, 4, 4, 64, 64, 1, 1), 2, 8, {"mode2:pow2_2", "tap_sorted:1tap"}),
    ((5, 2, 2, 1024, 64, 1, 1), 2, 1, {"k1:mode2", "mode2:pow2_1"}),
    ((3, 9, 7, 48, 24, 2, 3), 3, 1, {"mode3:pow2_0", "k3:mode3"}), ((2, 16, 16, 64, 32, 2, 3), 3, 1, {"mode3:pow2_1"}),
    ((128, 8, 8, 64, 32, 2, 3), 3, 4, {"mode3:pow2_2", "tap_sorted:9tap"}), ((3, 6, 6, 64, 32, 2, 1), 3, 1, {"k1:mode3", "mode3:pow2_0"}),
    ((3, 9, 7, 32, 48, 2, 3), 4, 1, {"mode4:pow2_0", "k3:mode4"}), ((3, 8, 8, 32, 64, 1, 3), 4, 1, {"mode4:pow2_1"}),
    ((128, 8, 8, 32, 64, 2, 3), 4, 4, {"mode4:pow2_2", "tap_sorted:9tap"}), ((128, 8, 8, 32, 64, 2, 1), 4, 4, {"k1:mode4", "tap_sorted:1tap"}),
    ((2, 7, 9, 16, 16, 1, 3), 5, 1, {"mode5:pow2_0", "k3:mode5"}), ((2, 8, 8, 32, 32, 2, 3), 5, 1, {"mode5:pow2_1"}),
    ((128, 4, 4, 32, 32, 2, 3), 5, 1, {"mode5:pow2_2", "tap_sorted:9tap"}), ((128, 4, 4, 32, 32, 2, 1), 5, 1, {"k1:mode5", "tap_sorted:1tap"}),
    ((2, 8, 8, 16, 16, 1, 1), 5, 1, {"k1:mode5", "mode5:pow2_1"}),
    ((3, 14, 14, 1, 64, 2, 3), 10, 1, {"mode10", "k3:mode10"}), ((2, 8, 8, 3, 16, 1, 1), 10, 1, {"k1:mode10"}),
    ((2, 10, 14, 4, 32, 2, 3), 11, 1, {"mode11", "k3:mode11"}),
    # rows too wide for the row-MFMA kernels' 64 KB of LDS (thin-Ci: > 227 pixels of 4 channels at stride 1, > 310 of RGB at stride 2;
    # thin-Co: > 298 of 32 -> 3): the plan falls back to the generic thin kernels; half as wide, each is on mode 31 / 30
    ((1, 8, 256, 4, 32, 1, 3), 11, 8, {"wide_row:mode11", "reduce:float4"}), ((1, 8, 320, 3, 32, 2, 3), 10, 2, {"wide_row:mode10"}),
    ((1, 8, 320, 32, 3, 1, 3), 20, 10, {"wide_row:mode20"}),
    ((2, 9, 11, 48, 3, 1, 3), 20, 1, {"mode20", "k3:mode20"}), ((3, 20, 12, 48, 3, 1, 3), 20, 3, {"mode20", "reduce:float4"}),
    ((2, 9, 11, 48, 3, 1, 1), 20, 1, {"k1:mode20"}),
    ((2, 36, 64, 64, 4, 1, 3), 21, 18, {"mode21", "k3:mode21"}),            # 64 channels: the thin-Co row kernel declines
    ((2, 20, 128, 16, 1, 1, 3), 30, 4, {"mode30:mt1", "k3:mode30"}), ((3, 20, 32, 32, 3, 1, 3), 30, 6, {"mode30:mt2"}),
    ((2, 18, 16, 1, 16, 1, 3), 31, 4, {"mode31:nt1", "mode31:rb16", "k3:mode31"}), ((5, 32, 32, 3, 32, 2, 3), 31, 10, {"mode31:nt2", "mode31:rb8"}),
    ((2, 44, 128, 4, 64, 2, 3), 31, 6, {"mode31:nt4", "mode31:rb8"}), ((3, 31, 31, 3, 32, 2, 3), 31, 6, {"mode31:nt2"}),
    ((8, 128, 32, 3, 32, 2, 3), 31, 64, {"mode31:nt2", "reduce:tall"}),
    ((2, 9, 7, 20, 12, 2, 3), 0, 1, {"mode0", "k3:mode0"}), ((3, 20, 20, 3, 5, 1, 3), 0, 5, {"mode0", "reduce:scalar"}),
    ((5, 40, 16, 16, 5, 1, 3), 0, 13, {"mode0", "reduce:float4"}),           # 5 thin channels: neither thin family
    ((2, 9, 7, 20, 12, 2, 1), 0, 1, {"k1:mode0"}),
    # ---- the shapes of the 5x5-only filter gradients on the generic modes: c16 (mode 32), strip-resident at Wo = 8 / 16 / 32 (mode 33),
    # tap-grouped at M = 131 072 (mode 7)
    ((3, 64, 64, 16, 32, 2, 3), 5, 6, {"mode5:pow2_1"}), ((2, 128, 128, 16, 32, 2, 3), 5, 16, {"mode5:pow2_1"}),
    ((3, 16, 16, 32, 64, 2, 3), 4, 1, {"mode4:pow2_1"}), ((2, 32, 32, 64, 128, 2, 3), 2, 4, {"mode2:pow2_1"}),
    ((2, 64, 64, 32, 64, 2, 3), 4, 8, {"mode4:pow2_1"}), ((128, 32, 32, 16, 16, 1, 3), 5, 54, {"mode5:pow2_1", "reduce:float4"}),
    # ---- production geometry
    ((2, 64, 64, 64, 32, 1, 3), 3, 32, {"mode3:pow2_1", "reduce:float4"}), ((4, 8, 8, 16, 3, 1, 3), 30, 4, {"mode30:mt1"}),
]
# shape -> (the 5x5-only mode the same geometry is on at k = 5, the generic mode at k = 3)
STEP_ASIDE_WGRAD = {(3, 64, 64, 16, 32, 2, 3): (32, 5), (2, 128, 128, 16, 32, 2, 3): (32, 5), (3, 16, 16, 32, 64, 2, 3): (33, 4),
                    (2, 32, 32, 64, 128, 2, 3): (33, 2), (2, 64, 64, 32, 64, 2, 3): (33, 4), (128, 32, 32, 16, 16, 1, 3): (7, 5)}
WIDE_ROWS = {(1, 8, 256, 4, 32, 1, 3): (11, 31), (1, 8, 320, 3, 32, 2, 3): (10, 31), (1, 8, 320, 32, 3, 1, 3): (20, 30)}   # -> (mode, at W / 2)

# epilogues, one case per kernel family with its own epilogue code: (data gradient?, shape)
EPI_CASES = [
    (0, (2, 8, 8, 32, 32, 2, 3)), (1, (2, 8, 8, 32, 32, 2, 3)), (0, (3, 8, 8, 32, 64, 1, 3)),    # gather-GEMM float4 epilogue, both tiles
    (0, (5, 2, 2, 1024, 64, 1, 1)),                                                             # ... applied by the split-K reduce
    (1, (3, 6, 6, 64, 32, 2, 1)), (1, (128, 8, 8, 32, 64, 2, 1)),                               # ... on phases with no tap: epilogue(0)
    (0, (5, 40, 16, 16, 5, 1, 3)), (1, (5, 32, 32, 3, 32, 2, 3)), (0, (2, 20, 128, 16, 1, 1, 3)),   # scatter rows (64- and 128-pixel workgroups)
    (0, (5, 32, 32, 3, 32, 2, 3)), (1, (5, 40, 16, 16, 5, 1, 3)),                               # gather rows
    (0, (2, 12, 20, 16, 5, 1, 3)), (0, (2, 8, 8, 24, 16, 1, 1)), (1, (3, 14, 14, 1, 64, 2, 3)), (1, (3, 14, 14, 4, 32, 2, 1)),
    (0, (2, 14, 14, 16, 1, 2, 3)), (0, (2, 14, 14, 64, 1, 2, 3)), (0, (3, 14, 14, 1, 64, 2, 3)), (0, (2, 9, 7, 3, 96, 2, 3)),
    (0, (2, 9, 7, 20, 12, 2, 3)), (1, (2, 9, 7, 20, 12, 2, 1)),                                 # thin and direct kernels
]

# statistics epilogue of the gather-GEMM: position-major at k = 3, a merged pair with no tap at k = 1 (its rows are exact zeros), both
# tiles with unmerged empty phases, phases of different extents
STATS_CASES = [(0, (128, 4, 4, 64, 64, 1, 3)), (1, (513, 16, 16, 8, 16, 2, 1)), (1, (3, 6, 6, 64, 32, 2, 1)), (1, (3, 7, 9, 32, 64, 2, 1)),
               (1, (2, 8, 8, 32, 32, 2, 3)), (1, (3, 7, 7, 32, 48, 2, 3)), (0, (3, 8, 8, 32, 64, 1, 3))]

# isolation (a NaN image; two runs): one case per launch name, and one per filter-gradient kernel for the two runs
ISOLATION_ROUTES = [(0, (2, 8, 8, 32, 32, 2, 3)), (1, (5, 2, 2, 256, 512, 1, 3)), (0, (128, 4, 4, 64, 64, 1, 3)), (1, (128, 8, 8, 32, 64, 2, 1)),
                    (0, (5, 40, 16, 16, 5, 1, 3)), (1, (5, 32, 32, 3, 32, 2, 3)), (0, (5, 32, 32, 3, 32, 2, 3)), (1, (5, 40, 16, 16, 5, 1, 3)),
                    (0, (2, 12, 20, 16, 5, 1, 3)), (1, (2, 8, 8, 3, 16, 1, 1)), (0, (3, 14, 14, 1, 64, 2, 3)), (1, (2, 14, 14, 16, 1, 2, 3)),
                    (1, (3, 14, 14, 4, 32, 2, 1)), (0, (2, 14, 14, 16, 1, 2, 3)), (1, (2, 20, 24, 2, 32, 1, 3)), (0, (2, 14, 14, 64, 1, 2, 3)),
                    (1, (2, 9, 7, 3, 8, 2, 1)), (0, (2, 9, 7, 3, 96, 2, 3)), (1, (2, 9, 7, 128, 3, 2, 1)), (0, (2, 9, 7, 20, 12, 2, 3)),
                    (1, (2, 9, 7, 20, 12, 2, 1))]
ISOLATION_WGRAD = [(128, 4, 4, 64, 64, 1, 3), (128, 4, 4, 64, 64, 1, 1), (130, 4, 4, 128, 256, 2, 3), (3, 14, 14, 1, 64, 2, 3),
                   (3, 20, 12, 48, 3, 1, 3), (3, 20, 32, 32, 3, 1, 3), (5, 32, 32, 3, 32, 2, 3), (3, 20, 20, 3, 5, 1, 3)]
