"""CPU: the case table of tests/spectral_cases.py held to its claims through the library's own route query -- every case has the
properties it is listed for, the table as a whole covers the branches it was written to reach, and the integer recipe of the
sigma-only test is exact for the reason it gives."""
import numpy as np
import pytest

from blurred_gan_amd import ops
import spectral_cases as SC


def _described():
    return [(c, SC.describe(c, ops.spectral.route(c["K"], c["N"], c["taps"]))) for c in SC.CASES]


def test_case_ids_are_unique_and_the_table_has_thirteen_cases():
    assert len(set(SC.IDS)) == len(SC.IDS) == 13
    assert max(c["K"] * c["N"] for c in SC.CASES) * 4 < 1.2e6          # the largest matrix: 1.1 MB


@pytest.mark.parametrize("case", SC.CASES, ids=SC.IDS)
def test_case_has_its_claimed_properties(case):
    d = SC.describe(case, ops.spectral.route(case["K"], case["N"], case["taps"]))
    assert case["K"] % case["taps"] == 0
    for k, v in case["claims"].items():
        assert d[k] == v, f"{SC.case_id(case)}: {k} claimed {v!r}, the library's route gives {d[k]!r}"
    # nothing derived is left unclaimed (midrow exists only where there is a second unit to start anywhere)
    assert set(d) == set(case["claims"]), (SC.case_id(case), set(d) ^ set(case["claims"]))


def test_the_table_covers_what_it_was_written_for():
    described = _described()
    assert SC.coverage(described) == SC.COVER
    # the check can fail: without the wide cases exactly their entries go missing
    fewer = SC.coverage([(c, d) for c, d in described if d["route"] != "wide"])
    lost = {k for k in SC.COVER if fewer[k] != SC.COVER[k]}
    assert lost == {"wide_vecs", "wide_partial_second_sweep", "wide_last_strip_one_row", "scale_T", "finish", "finish_p8_nonzero"}
    # the issue's reading of the existing cases: every multi-unit dot / apply case there is a multiple of a unit
    for K, N in ((100, 8192), (6400, 512), (12800, 512)):
        assert (K * N) % SC.EW_ELEMS == 0 and ops.spectral.route(K, N)["ew_units"] > 1


def test_workspace_regions_follow_from_the_route():
    """[pass_units][N] | [pass_units] | [ew_units], each padded to 4 floats: what the guard band behind the workspace relies on."""
    pad = lambda n: -(-n // 4) * 4
    for c in SC.CASES:
        r = ops.spectral.route(c["K"], c["N"], c["taps"])
        assert r["ws_floats"] == pad(r["pass_units"] * c["N"]) + pad(r["pass_units"]) + pad(r["ew_units"]), SC.case_id(c)


@pytest.mark.parametrize("case", SC.CASES, ids=SC.IDS)
def test_integer_recipe_is_exact_in_any_order(case):
    W, u, v, want = SC.exact_data(case)
    K, N = case["K"], case["N"]
    assert W.dtype == u.dtype == v.dtype == np.float32 and W.shape == (K, N)
    assert np.abs(W).max() == 3 and np.abs(u).max() <= 2 and np.abs(v).max() <= 2 and np.array_equal(W, np.round(W))
    assert 12 * K * N < 1 << 24
    # the sum of the terms' magnitudes bounds every partial sum in every order
    mag = int(np.abs(v).astype(np.int64) @ (np.abs(W).astype(np.int64) @ np.abs(u).astype(np.int64)))
    assert mag <= 12 * K * N and abs(want) <= mag
    # float32 numpy, row sums first or column sums first, gives the integer
    assert float((v * (W @ u)).sum(dtype=np.float32)) == float(want) == float(((v @ W) * u).sum(dtype=np.float32))
    # the data can tell: every row adds a positive integer (rows dropped, however many, lower the sum; v still has both signs),
    # and the last four columns together count
    rows = v.astype(np.int64) * (W.astype(np.int64) @ u.astype(np.int64))
    assert (rows > 0).all() and rows.sum() == want and v.min() < 0 < v.max()
    cols = (v.astype(np.int64) @ W.astype(np.int64)) * u.astype(np.int64)
    assert cols[-4:].any() and want != 0
