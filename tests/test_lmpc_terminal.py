"""The terminal cost on the host: the condensed Hessian against an independent numpy condensing, the no-op statements byte for
byte, every refusal of the setter, the exported symbol, the LQR identity on the yardstick itself (tests/terminal_ref.py) -- which pins the
yardstick and the weight-column convention before any GPU run --, the recorded yardstick results, and the banks' all-or-none rule where it can
be reached without a device (LMPCHetero's needs one: tests/test_lmpc_terminal_gpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import rate_ref as RR
import terminal_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("H", "Kinv", "Gr", "Gc", "Y", "lw", "uw", "rho_b", "lg0", "ug0", "rho_g", "g_soft", "dims", "MA0", "MA1", "Ym", "MA0p", "MA1p", "Ymp",
         "flags", "dims_maps", "g_refrow", "g_step", "g_kind", "g_comp", "slo", "shi", "ws_limit", "terminal")


def _host(sp, terminal=True):
    from libmpc_amd import LMPC
    return TR.configure(LMPC(*sp["dims"], device=-1), sp, terminal=terminal)


def _hessian(c):
    d = c.debug_get("dims")
    nz, ldz = int(d[0]), int(d[2])
    return c.debug_get("H").reshape(ldz, ldz)[:nz, :nz]


def test_the_symbol_is_exported_and_declared():
    from libmpc_amd import _capi
    assert "mpcx_lmpc_set_terminal_cost" in _capi.EXPORTS and _capi.lib().mpcx_lmpc_set_terminal_cost is not None
    header = open(os.path.join(ROOT, "include", "mpcx.h")).read()
    assert "int mpcx_lmpc_set_terminal_cost(mpcx_lmpc_t h, const double *P, const double *xT, const double *Tx);" in header
    import pympcxx
    assert hasattr(pympcxx.LMPC, "setTerminalCost")
    assert "setTerminalCost" in open(os.path.join(ROOT, "include", "mpcx", "LMPC.hpp")).read()


@pytest.mark.parametrize("case", ["full", "blocked nx=17", "lqr", "integrator"])
def test_condensed_hessian_is_the_numpy_condensing_plus_the_terminal_block(case):
    sp = {"full": TR.full_feature_terminal, "blocked nx=17": lambda: TR.condense_spec(17, 3, 2, 9, 4, 900),
          "lqr": lambda: TR.lqr_spec("stable", 5)[0], "integrator": TR.integrator_constrained}[case]()
    Hn, S = TR.condensed_hessian(sp)
    H = _hessian(_host(sp))
    assert np.abs(H - Hn).max() <= 1e-12 * np.abs(Hn).max()
    # ... and the term is S' P S on top of the controller without it
    H0 = _hessian(_host(sp, terminal=False))
    T = S.T @ sp["P"] @ S
    assert np.abs(T).max() >= 1e-3 * np.abs(Hn).max()
    assert np.abs((H - H0) - T).max() <= 1e-12 * np.abs(Hn).max()
    assert np.array_equal(H, H.T)


def test_never_set_set_to_null_and_set_then_removed_condense_to_the_same_bytes():
    for sp in (TR.full_feature_terminal(), TR.integrator_constrained()):
        never = _host(sp, terminal=False)
        null = _host(sp, terminal=False)
        assert null.setTerminalCost(None)
        back = _host(sp)
        assert back.debug_get("terminal").size == TR.condensed_hessian(sp)[1].shape[0] * (sp["dims"][0] + 1 + sp["dims"][3] + sp["dims"][2])
        assert back.setTerminalCost(None)
        with_term = _host(sp)
        differs = 0
        for name in NAMES:
            a = never.debug_get(name)
            for other in (null, back):
                b = other.debug_get(name)
                assert a.tobytes() == b.tobytes(), name
            differs += a.tobytes() != with_term.debug_get(name).tobytes()
        assert never.debug_get("terminal").size == 0
        assert differs >= 5                       # (the comparison can tell: H, Kinv, Y, the maps and the stored block change with the term)


def test_stored_block_is_p_symmetrised_then_xt_then_tx():
    sp = TR.full_feature_terminal()
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    c = _host(sp, terminal=False)
    P = sp["P"].copy()
    P[0, 1] += 4e-11 * np.abs(P).max()            # below the symmetry threshold: taken, and symmetrised
    assert c.setTerminalCost(P, sp["xT"], sp["Tx"])
    t = c.debug_get("terminal")
    assert t.size == nx * nx + nx + nx * (ny + ndu)
    Ps = t[:nx * nx].reshape(nx, nx).T
    assert np.array_equal(Ps, Ps.T) and np.array_equal(Ps, 0.5 * (P + P.T))
    assert np.array_equal(t[nx * nx:nx * nx + nx], sp["xT"])
    assert np.array_equal(t[nx * nx + nx:].reshape(ny + ndu, nx).T, sp["Tx"])
    # null xT and Tx are zeros
    assert c.setTerminalCost(sp["P"])
    assert not c.debug_get("terminal")[nx * nx:].any()


def test_every_refusal_stores_nothing():
    from libmpc_amd import _capi
    sp = TR.full_feature_terminal()
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    c = _host(sp)
    before = {n: c.debug_get(n).tobytes() for n in ("H", "terminal", "MA0")}
    P, xT, Tx = sp["P"], sp["xT"], sp["Tx"]

    def refused(Pm, x=None, T=None, word=""):
        assert c.setTerminalCost(Pm, x, T) is False
        assert word in _capi.lib().mpcx_last_error().decode()
        for n, b in before.items():
            assert c.debug_get(n).tobytes() == b, n

    bad = P.copy(); bad[1, 1] = np.nan
    refused(bad, word="NaN or infinite")
    bad = P.copy(); bad[0, 2] = bad[2, 0] = np.inf
    refused(bad, word="NaN or infinite")
    x = xT.copy(); x[0] = np.inf
    refused(P, x, Tx, word="xT")
    T = Tx.copy(); T[1, 0] = np.nan
    refused(P, xT, T, word="Tx")
    bad = P.copy(); bad[0, 1] += 1e-9 * np.abs(P).max()
    refused(bad, xT, Tx, word="not symmetric")
    w, V = np.linalg.eigh(P)
    bad = P - 1e-9 * np.abs(P).max() * np.outer(V[:, 0], V[:, 0])         # the zero eigenvalue of the rank-deficient P pushed below the threshold
    refused(0.5 * (bad + bad.T), xT, Tx, word="not positive semidefinite")
    refused(-np.eye(nx), word="not positive semidefinite")
    # the semidefinite P itself (smallest eigenvalue 0 to rounding) and a slightly indefinite one inside the threshold are taken
    assert abs(w[0]) <= 1e-12 * w[-1]
    assert c.setTerminalCost(P - 1e-12 * np.abs(P).max() * np.outer(V[:, 0], V[:, 0]))
    # a null handle
    assert _capi.lib().mpcx_lmpc_set_terminal_cost(None, None, None, None) == _capi.E_INVALID
    # shapes are checked before the call
    with pytest.raises(ValueError):
        c.setTerminalCost(np.eye(nx + 1))
    with pytest.raises(ValueError):
        c.setTerminalCost(P, xT, np.zeros((nx, ny)))


@pytest.mark.parametrize("name,ph", [("integrator", 3), ("integrator", 10), ("stable", 5), ("unstable", 2)])
def test_lqr_identity_on_the_yardstick(name, ph):
    """With P the Riccati solution of (A, B, C' W C, R) the horizon's cost is the infinite one: the yardstick's first move is -K x0 and its cost
    0.5 x0' P x0, whatever ph.  Conditions: no weight on the output of the predicted step ph (the internal column ph of wOutput, user column
    ph - 1), none on the increments, lastU = 0, zero references, ch >= ph - 1, no bound."""
    sp, Q, R = TR.lqr_spec(name, ph)
    P, K = sp["P"], sp["K"]
    A, B = sp["A"], sp["B"]
    assert np.abs(A.T @ P @ A - A.T @ P @ B @ K + Q - P).max() <= 1e-10 * np.abs(P).max()
    if name == "unstable":
        assert abs(max(abs(np.linalg.eigvals(A))) - 1.2) <= 1e-12
    assert max(abs(np.linalg.eigvals(A - B @ K))) < 1.0
    nx, nu = sp["dims"][:2]
    x0 = np.random.default_rng(5).normal(size=(16, nx)); u0 = np.zeros((16, nu))
    ref = TR.solve_batch(sp, x0, u0)
    assert (ref["status"] == 0).all() and (ref["polished"] == 1).all()
    cmd = -x0 @ K.T
    cost = 0.5 * np.einsum("bi,ij,bj->b", x0, P, x0)
    assert (np.abs(ref["cmd"] - cmd).max(axis=1) / np.maximum(np.abs(cmd).max(axis=1), 1e-12)).max() <= 1e-9
    assert (np.abs(ref["cost"] - cost) / np.maximum(1.0, cost)).max() <= 1e-9
    # the product's Hessian of the same controller is the Riccati recursion's: its unconstrained first move is -K x0 too (host arrays only)
    c = _host(sp)
    d = c.debug_get("dims"); nz, ldz = int(d[0]), int(d[2])
    H = c.debug_get("H").reshape(ldz, ldz)[:nz, :nz]
    Hn, S = TR.condensed_hessian(sp)
    assert np.abs(H - Hn).max() <= 1e-12 * np.abs(Hn).max()


def test_lqr_terminal_cost_needs_a_positive_input_weight_and_a_model():
    from libmpc_amd import LMPC, MpcxError
    c = LMPC(2, 1, 0, 1, 5, 5, device=-1)
    with pytest.raises(MpcxError):
        c.lqr_terminal_cost()
    sp = RR.integrator_spec(5)
    sp["UW"] = np.zeros((1, 5))
    RR.configure(c, sp)
    with pytest.raises(ValueError, match="positive input weight"):
        c.lqr_terminal_cost(step=0)
    with pytest.raises(ValueError, match="not a column"):
        c.lqr_terminal_cost(step=5)
    # the weights the helper reads are the ones given, matrix form and slice form
    sp = RR.integrator_spec(5)
    RR.configure(c, sp)
    A, B, Q, R = c._lqr_problem(1)
    assert np.array_equal(Q, sp["C"].T @ np.diag(sp["OW"][:, 1]) @ sp["C"]) and np.array_equal(R, np.diag(sp["UW"][:, 1]))
    assert c.setObjectiveWeights([3.0], [0.5], [0.0], (2, 4))
    assert c._lqr_problem(2)[3][0, 0] == 0.5 and c._lqr_problem(3)[2][0, 0] == 3.0 and c._lqr_problem(1)[3][0, 0] == sp["UW"][0, 1]


def test_recorded_yardstick_results_are_the_yardstick():
    g = np.load(os.path.join(ROOT, "tests", "golden", "terminal_oracle.npz"))
    sp = TR.full_feature_terminal()
    x0, u0, yconst, ystep, dmeas = TR.full_feature_batch(24)
    assert np.array_equal(g["fullc_x0"], x0) and np.array_equal(g["fulls_x0"], x0) and np.array_equal(g["fullc_u0"], u0)
    for prefix in ("fullc_", "fulls_", "fulls1_"):
        assert (g[prefix + "polished"] == 1).mean() >= 0.75, prefix           # at most a quarter of a batch unpolished
    pb = TR.builder(sp)
    for b in (0, 1):
        one = TR.solve_one(pb, sp, x0[b], u0[b], yconst[b])
        assert np.allclose(one["cmd"], g["fullc_cmd"][b], rtol=1e-12, atol=1e-14) and abs(one["cost"] - g["fullc_cost"][b]) <= 1e-12 * max(1.0, abs(one["cost"]))
        one = TR.solve_one(pb, sp, x0[b], u0[b], ystep[b], dmeas[b])
        assert np.allclose(one["cmd"], g["fulls_cmd"][b], rtol=1e-12, atol=1e-14)
    # the term matters in these cases: without it the first move differs by ten times the tolerance the GPU tests compare at, and more
    no = TR.solve_one(RR.builder(sp), {k: v for k, v in sp.items() if k not in ("P", "xT", "Tx")}, x0[0], u0[0], yconst[0])
    assert np.abs(no["cmd"] - g["fullc_cmd"][0]).max() >= 10 * 1e-5 * np.abs(g["fullc_cmd"][0]).max()


def test_bank_of_single_handles_takes_the_term_in_every_controller_or_in_none():
    """LMPCBank's rule is checked before it touches the device; LMPCHetero's create asks for a device first (tests/test_lmpc_terminal_gpu.py)"""
    from libmpc_amd import LMPCBank
    sp = TR.integrator_constrained()
    with pytest.raises(ValueError, match="terminal cost in every controller or in none"):
        LMPCBank([_host(sp), _host(sp, terminal=False)])
    took_back = _host(sp)
    assert took_back.setTerminalCost(None)
    with pytest.raises(ValueError, match="terminal cost in every controller or in none"):
        LMPCBank([_host(sp), took_back])
