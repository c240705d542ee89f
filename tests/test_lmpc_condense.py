"""The condensing of a controller -- H, the rows of G, Hinv, the dual Hessian Y, the ADMM step sizes, Kinv -- against the 60-digit truths of
tests/golden/condense_truth_*.npz within the bound of tests/condense_ref.py, on the host: LmpcController::condense through
LMPC(..., device=-1) and debug_get, for every family the device kernel is held to in tests/test_lmpc_condense_gpu.py and
tests/test_emu_condense.py.  Also: the numpy restatement the bound's constant comes from stays an eighth below it, the check notices two
small defects, and a truth assembled from channels is the dense truth of the same controller."""
import numpy as np
import pytest

import condense_ref as R


@pytest.mark.parametrize("name", R.FAMILIES)
def test_host_set_up_against_the_truth(name):
    ctrls = R.host_controllers(name)                       # (holds the host's layout of rows, bounds and boxes to condense_ref.layout)
    R.check_family(name, [R.arrays_of(c.debug_get) for c in ctrls], " (host)")
    for c, (ctl, lay, tr) in zip(ctrls, R.family(name)):
        # the cost from the multipliers only where the inverse inverts: never for a regularised Hessian
        assert int(c.debug_get("flags")[0]) == R.restate(ctl, lay)["cost_direct"] and (not tr["reg"] or int(c.debug_get("flags")[0]) == 1)


@pytest.mark.parametrize("name", R.FAMILIES)
def test_restatement_stays_an_eighth_below_the_bound(name):
    gots = [R.restate(ctl, lay) for ctl, lay, tr in R.family(name)]
    R.check_family(name, gots, " (restatement, against C / 8)", c=R.C_BOUND / 8)
    assert all(g["regularised"] == tr["reg"] for g, (_, _, tr) in zip(gots, R.family(name)))


def test_conditions_of_the_families():
    for name in R.FAMILIES:
        for ctl, lay, tr in R.family(name):
            assert tr["reg"] == (name == "cond_regularised")
            if not tr["reg"]:
                assert R.relative_bound(tr, lay) <= 1e-6, name
    kappa = [tr["lam"][1] / tr["lam"][0] for _, _, tr in R.family("cond_chain")]
    assert min(kappa) >= 5e5 and max(kappa) <= 2e6                      # about 1e6
    for ctl, lay, tr in R.family("cond_regularised"):
        zero = [q for q in range(lay["nz"]) if not tr["H"][q].any() and not tr["H"][:, q].any()]
        assert zero and all(np.isfinite(lay["lw"][q]) and tr["rho_b"][q] == R.RHO_MIN for q in zero)      # (1e-8 max diag H on Hinv's diagonal: the clip's lower end)
    # the shapes the kernel's forms switch at (lmpc_condense_lds: LDS up to NP = 96 where P and Q fit; the scratch form behind)
    dims = {name: R.pad_dims(R.family(name)[0][1])[:2] for name in R.EDGES}
    assert dims["edge_lds96"][0] == 96 and dims["edge_big98"][0] == 98 and 81 <= dims["edge_bytes84"][0] <= 96 and dims["edge_bytes84"][1] >= 97
    forms = {name: R.condense_lds(*R.family(name)[0][0]["dims"][:1], R.family(name)[0][0]["dims"][2], *dims[name]) for name in R.EDGES}
    assert [forms[n][1] for n in R.EDGES] == [False, True, True] and all(f[0] <= R.LDS_LIMIT - 64 for f in forms.values()), forms
    assert all(not R.condense_lds(c["dims"][0], c["dims"][2], l["nz"], len(l["kind"]))[1] for n in R.FAMILIES if n not in R.EDGES for c, l, _ in R.family(n))
    eq_box = [lay for _, lay, _ in R.family("rows_mg1") if (lay["lw"] == lay["uw"]).any()]
    eq_row = [lay for _, lay, _ in R.family("features") if (lay["lo"] == lay["hi"]).any()]
    assert len(eq_box) == R.K and len(eq_row) == R.K                       # the 1e3 of an equality, on a box and on a row
    for ctl, lay, tr in R.family("features"):
        nx, nu, ny, ph, ch = ctl["dims"]
        assert ch < ph and nx == 17 and (ctl["DUW"] > 0).all() and "P" in ctl and set(lay["kind"]) == {0, 1, 2, 3}
        assert len(set(lay["soft"][lay["soft"] > 0])) == 2
    softs = [tuple(sorted(set(lay["soft"]))) for _, lay, _ in R.family("features")]
    assert len(set(softs)) == R.K


def _one_defect_fails(name, k, spoil):
    fam = R.family(name)
    gots = [R.restate(ctl, lay) for ctl, lay, tr in fam]
    R.check_family(name, gots, " (restatement)")
    spoil(gots[k], fam[k])
    with pytest.raises(AssertionError):
        R.check_family(name, gots, " (restatement with a defect)")


def test_a_small_error_in_an_off_diagonal_tile_of_h_is_noticed():
    def spoil(got, member):
        nz, mg, ldz, ldg, ldy = R.pad_dims(member[1])
        H = got["H"].reshape(ldz, ldz)
        assert nz > 16
        H[2, 16] += 1e3 * R.U * np.abs(H).max()
    _one_defect_fails("shape_nz17", 1, spoil)


def test_a_dropped_cross_term_of_an_increment_weight_is_noticed():
    def spoil(got, member):
        ctl, lay, tr = member
        got.update(R.restate(ctl, lay, drop_cross_term=True))
    _one_defect_fails("features", 2, spoil)
    _one_defect_fails("rows_mg0", 0, spoil)


def test_channel_assembly_is_the_dense_truth():
    """two channels, nz = 8: the interleaved small truths against the 60-digit truth of the combined controller"""
    (ctl, lay, tr), = R.family("assembly_nz8")
    dense_ctl, dense = R.record("assembly_nz8.dense")
    assert ctl["dims"] == dense_ctl["dims"] == (4, 2, 2, 4, 4) and lay["nz"] == 8
    for k in ("A", "B", "C", "OW", "UW", "DUW", "xmin", "xmax", "dumin", "dumax", "umin", "umax"):
        assert np.array_equal(ctl[k], dense_ctl[k]), k
    for k in ("H", "G", "Hinv", "GH", "GHG", "Kinv", "rho_b", "rho_g"):
        a, b = tr[k], dense[k]
        assert a.shape == b.shape and (a != 0).sum() < a.size or a.ndim == 1, k
        # each side is a 60-digit number rounded once: equal, but for a tie between two doubles
        assert np.abs(a - b).max() <= R.U * np.abs(b).max(), (k, np.abs(a - b).max())
        assert np.array_equal(a == 0, np.abs(b) <= 1e-40 * np.abs(b).max()), k           # the zeros of the interleaving are zeros of the dense truth
    assert abs(tr["lam"][1] / tr["lam"][0] - dense["lam"][1] / dense["lam"][0]) <= 1e-9 * dense["lam"][1] / dense["lam"][0]
