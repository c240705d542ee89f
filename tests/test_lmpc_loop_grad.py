"""The backward pass of the closed loop on the host: the reference of tests/loop_grad_ref.py against central differences of its own
forward loop, the restatement over the kernels' formulas against that reference on every case of the GPU tests (the figure the kernels' one tolerance
derives from), what the GPU tests need of the cases' seeds, and the C ABI where it can be reached without a device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import loop_grad_ref as G
import model_sens_ref as Mo
import param_sens_ref as P
import sens_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _arrays(fam):
    from libmpc_amd import LMPC
    sp = G.family(fam)[0]
    c = S.configure(LMPC(*sp["dims"], device=-1), sp)
    a = Mo.arrays(c)
    a["Cq"] = P.arrays(c)["Cq"]
    return a


@functools.lru_cache(maxsize=None)
def _restatement(name):
    """worst disagreement of the restatement with the truth over the usable instances of a case"""
    R = G.reference(name)
    a = _arrays(G.CASES[name][0])
    worst = 0.0
    for b in np.nonzero(R["usable"])[0]:
        worst = max(worst, G.compare(R["grad"][b], G.restate_one(R, a, b, R["fwd"][b])))
    return worst


@pytest.mark.parametrize("name", G.CASES)
def test_cases_stay_within_the_cap_and_have_the_active_sets_asked_for(name):
    """decided from the truth alone, before any GPU run"""
    R = G.reference(name)
    assert R["n"] - int(R["usable"].sum()) <= G.SKIP_CAP * R["n"], (name, R["usable"])
    assert R["nonempty"] == (name != "smallest")
    if name == "full":
        assert R["changes"]
    for B in G.BATCHES.get(name, ()):            # ... and so do the batches made of them
        of = np.arange(B) % R["n"]
        assert (~R["usable"][of]).sum() <= G.SKIP_CAP * B


def test_cases_cover_the_axes():
    fams = {c[0] for c in G.CASES.values()}
    assert {"smallest", "full", "blocked", "soft", "refs", "ndu2", "nx33", "nx32", "nu_gt_nx"} <= fams
    assert {c[2] for c in G.CASES.values()} >= {1, 2, 5}
    assert {c[3] for c in G.CASES.values()} == {"own", "other", "batch"} and {c[4] for c in G.CASES.values()} == {"instance", "preview"}
    assert {c[5] for c in G.CASES.values()} == {True, False}
    assert {1, 63, 64, 65} <= {b for bs in G.BATCHES.values() for b in bs}
    for fam, (nx, nu, ny) in (("nx33", (33, 1, 1)), ("nx32", (32, 1, 1)), ("nu_gt_nx", (2, 3, 3))):
        d = G.family(fam)[0]["dims"]
        assert (d[0], d[1], d[3]) == (nx, nu, ny) and 65 in G.BATCHES[fam] and G.CASES[fam][3] == "batch"


@pytest.mark.parametrize("name", G.CASES)
def test_restatement_agrees_with_the_truth(name):
    worst = _restatement(name)
    print(f"{name}: restatement worst {worst:.2e}")
    assert worst <= G.RESTATEMENT_WORST


def test_the_recorded_figure_is_the_measured_one():
    """measured <= recorded <= 2 x measured (the convention of qp_truth); KERNEL_TOL derives from it and from nothing else"""
    measured = max(_restatement(name) for name in G.CASES)
    print(f"restatement worst over the cases: {measured:.3e}, recorded {G.RESTATEMENT_WORST:.3e}")
    assert measured <= G.RESTATEMENT_WORST <= 2.0 * measured
    assert G.KERNEL_TOL == max(8.0 * G.RESTATEMENT_WORST, 1e-12)


def test_reference_agrees_with_central_differences_of_its_own_loop():
    """Within a piece (the same active sets at every tick of both perturbed runs) the loop is affine in x0, u0, yref and the noise, so a central
    difference carries rounding only; in a plant entry it is a polynomial of degree <= ticks, so the truncation term is h^2 / 6 times a third
    derivative.  With L = sum |seed . trajectory| the loss's magnitude: a loss evaluation is a chain of a few hundred float64 operations per
    entry, each relative 2^-52, say <= 1e3 eps L in all; the difference of two of them over 2h gives 1e3 eps L / h, and the third derivative of a
    degree-`ticks` polynomial with coefficients of the order of L is at most ticks^3 L.  h = 1e-5: bound = 1e3 eps L / h + ticks^3 L h^2 / 6
    ~ 2.3e-8 L.  A direction that leaves the piece is left out; most must stay."""
    name = "full_other"
    R = G.reference(name)
    I, pb = R, R["pb"]
    sp = R["sp"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    h, eps, T = 1e-5, 2.0 ** -52, R["ticks"]
    kind, Ap, Bp, Bdp = R["plant"]
    tried = kept = 0
    worst = 0.0
    rg = np.random.default_rng(3)
    for b in np.nonzero(R["usable"])[0][:3]:
        f0, g = R["fwd"][b], R["grad"][b]
        L = float(np.abs(R["seed_x"][:, b] * f0["x"]).sum() + np.abs(R["seed_u"][:, b] * f0["u"]).sum())
        bound = 1e3 * eps * L / h + T ** 3 * L * h * h / 6.0

        def diff(**kw):
            p = {k: v[0] for k, v in kw.items()}; m = {k: v[1] for k, v in kw.items()}
            fp, fm = G.forward_one(I, pb, b, **p), G.forward_one(I, pb, b, **m)
            same = all(np.array_equal(f["act"], f0["act"]) for f in (fp, fm))
            return (G.loss_of(I, b, fp) - G.loss_of(I, b, fm)) / (2 * h), same
        checks = []
        dx, du, dy = rg.normal(size=nx), rg.normal(size=nu), rg.normal(size=ny)
        dw = rg.normal(size=(T, nx))
        checks.append((diff(x0=(R["x0"][b] + h * dx, R["x0"][b] - h * dx)), g["d_x0"] @ dx))
        checks.append((diff(u0=(R["u0"][b] + h * du, R["u0"][b] - h * du)), g["d_u0"] @ du))
        checks.append((diff(yshift=(h * dy, -h * dy)), g["d_yref"] @ dy))
        checks.append((diff(noise=(R["noise"][:, b] + h * dw, R["noise"][:, b] - h * dw)), (g["d_noise"] * dw).sum()))
        for M, n, idx in ((Ap, "d_plant_A", 0), (Bp, "d_plant_B", 1), (Bdp, "d_plant_Bd", 2)):
            if not M.size:
                continue
            i, j = rg.integers(M.shape[0]), rg.integers(M.shape[1])
            E = np.zeros_like(M); E[i, j] = h
            pl = lambda s: tuple(Q + s * E if q == idx else Q for q, Q in enumerate((Ap, Bp, Bdp)))
            checks.append((diff(plant=(pl(1.0), pl(-1.0))), g[n][i, j]))
        for (fd, same), an in checks:
            tried += 1
            if same:
                kept += 1
                worst = max(worst, abs(fd - an) / bound)
    print(f"central differences: worst error / bound {worst:.2e}, {kept} of {tried} directions stayed within their piece")
    assert kept >= 0.7 * tried and worst <= 1.0


def test_abi_without_a_device():
    from libmpc_amd import _capi
    lib = _capi.lib()
    header = open(os.path.join(ROOT, "include", "mpcx.h")).read()
    for n in ("mpcx_lmpc_loop_grad_create", "mpcx_lmpc_loop_grad_run", "mpcx_lmpc_loop_grad_destroy", "mpcx_lmpc_loop_grad_desc_size"):
        assert n in _capi.EXPORTS and getattr(lib, n) is not None and n + "(" in header
    assert C.sizeof(_capi.LoopGradDesc) == lib.mpcx_lmpc_loop_grad_desc_size()
    d, h = _capi.LoopGradDesc(), C.c_void_p()
    assert lib.mpcx_lmpc_loop_grad_create(None, C.byref(d), None, C.byref(h)) == _capi.E_INVALID
    assert lib.mpcx_lmpc_loop_grad_run(None, None) == _capi.E_INVALID and lib.mpcx_lmpc_loop_grad_destroy(None) == _capi.OK
    import libmpc_amd
    assert callable(libmpc_amd.lmpc_closed_loop) and hasattr(libmpc_amd.LMPC, "make_loop_gradient") and hasattr(libmpc_amd, "LoopGradientResult")
