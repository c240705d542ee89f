"""The begin, adjoint and finish kernels of the closed loop's backward pass (libmpc_amd/csrc/lmpc_loop_grad.hip), their own source stepped through
the SIMT emulator of tests/emu/ on the CPU in both lane orders: guards behind every output and behind the launch's LDS.  The per-tick vector-Jacobian
products come from the reference (tests/loop_grad_ref.py), the packed plant block is built here in the order lmpc_loop.hip documents, and every
output is held to loop_grad_ref.KERNEL_TOL.  This is where a missing barrier in the transposed products shows without a GPU.  Built with clang++,
as tests/test_emu_sens.py is."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import loop_grad_ref as G

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
PAD, GUARD, GUARD_I = 64, -7.25e300, -77


def _clangxx():
    for c in (shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not installed")
    out = str(tmp_path_factory.mktemp("emu_loop_grad") / "run_loop_grad")
    subprocess.run([cxx, "-O1", "-std=c++20", "-I" + EMU, "-w", "-o", out, os.path.join(EMU, "run_loop_grad.cpp"), os.path.join(EMU, "hipemu_switch.S")], check=True)
    return out


def pack_plants(Ap, Bp, Bdp, ipw):
    """[B, nx, .] -> the packed plant block: tile t, term j, instance q of the tile, row i at ((t terms + j) ipw + q) nx + i, the last tile's padding zero"""
    B, nx = Ap.shape[0], Ap.shape[1]
    cols = np.concatenate([Ap, Bp, Bdp], axis=2)                                  # [B, nx, terms]: term j is column j
    terms = cols.shape[2]
    tiles = (B + ipw - 1) // ipw
    out = np.zeros((tiles, terms, ipw, nx))
    for b in range(B):
        out[b // ipw, :, b % ipw, :] = cols[b].T
    return out.ravel()


def run(exe, name, B, plants, order):
    R = G.reference(name)
    T = G.tiled(R, B)
    of = T["of"]
    assert R["usable"][of].all()
    nx, nu, ndu, ny, ph, ch = R["sp"]["dims"]
    ticks = R["ticks"]
    kind, Ap, Bp, Bdp = T["plant"]
    if kind != "batch":
        Ap, Bp, Bdp = (np.broadcast_to(m, (B,) + m.shape) for m in (Ap, Bp, Bdp))
    if plants:
        plant = pack_plants(Ap, Bp, Bdp, 64 // nx if nx < 64 else 1)
    else:
        assert kind != "batch"
        plant = np.concatenate([m[0].ravel() for m in (Ap, Bp, Bdp)])            # row-major each
    tx = np.stack([R["fwd"][b]["x"] for b in of], axis=1); tu = np.stack([R["fwd"][b]["u"] for b in of], axis=1)
    d = np.stack([np.stack([G.tick_refs(R, b, k)[1][:, 0] for b in of]) for k in range(ticks)]) if ndu else np.zeros((ticks, B, 0))
    parts = [[nx, nu, ndu, ny, ph, B, ticks, int(plants), 1, 1], plant, tx, tu, T["u0"], d, T["seed_x"], T["seed_u"]]
    for k in range(ticks - 1, -1, -1):
        for i in (1, 2, 3):
            parts.append(np.stack([R["fwd"][b]["vjp"][k][i] for b in of]))
        parts.append(np.zeros(B))
    inp = " ".join(repr(float(v)) for v in np.concatenate([np.asarray(p, float).ravel() for p in parts])) + "\n"
    r = subprocess.run([exe], input=inp, capture_output=True, text=True, env=dict(os.environ, HIPEMU_ORDER=order), timeout=600)
    assert r.returncode == 0, r.stderr[:2000]
    o = json.loads(r.stdout)
    assert o["tick"] == -1 and o["after"] == -1
    npl = nx + nu + ndu
    shapes = dict(d_x0=(B, nx), d_u0=(B, nu), d_yref=(B, ny), d_noise=(ticks, B, nx), d_plant=(B, npl, nx), x=(B, nx), u=(B, nu), lam=(B, nx), mu=(B, nu))
    out = {}
    for n, shp in shapes.items():
        v = np.array(o[n], float)
        cnt = int(np.prod(shp))
        assert v.size == cnt + PAD and (v[cnt:] == GUARD).all(), n
        out[n] = v[:cnt].reshape(shp)
    out["c"] = np.array(o["c"], float).reshape(ticks, B, nu)
    f = np.array(o["flags"])
    assert (f[B:] == GUARD_I).all() and (f[:B] == 0).all()
    return R, T, out, o


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name,B", [("full_batch", 65), ("nx33", 3), ("nu_gt_nx", 65)])
def test_the_per_instance_form_matches_the_truth(exe, name, B, order):
    R, T, out, _ = run(exe, name, B, True, order)
    of = T["of"]
    nx, nu = R["sp"]["dims"][0], R["sp"]["dims"][1]
    truth, use = G.stacked(R, of, G.PER_INSTANCE + G.PLANT)
    got = dict(d_x0=out["d_x0"], d_u0=out["d_u0"], d_yref=out["d_yref"], d_noise=out["d_noise"])
    pt = np.swapaxes(out["d_plant"], 1, 2)                                        # [B, nx, terms]
    got.update(d_plant_A=pt[:, :, :nx], d_plant_B=pt[:, :, nx:nx + nu], d_plant_Bd=pt[:, :, nx + nu:])
    worst = 0.0
    for n, t in truth.items():
        ax = tuple(a for a in range(t.ndim) if a != (1 if n == "d_noise" else 0))
        worst = max(worst, float((np.abs(got[n] - t) / np.maximum(1.0, np.abs(t).max(axis=ax, keepdims=True))).max()))
    # c_k as each replay read it, and what the last replay staged: the inputs of tick 0's solve
    c = np.stack([np.stack([R["fwd"][b]["vjp"][k][0] for b in of]) for k in range(R["ticks"])])
    worst = max(worst, float(np.abs(out["c"] - c).max() / max(1.0, np.abs(c).max())))
    print(f"{name} B={B} {order}: worst error / bound {worst:.2e} / {G.KERNEL_TOL:.2e}")
    assert worst <= G.KERNEL_TOL
    assert np.array_equal(out["x"], T["x0"]) and np.array_equal(out["u"], T["u0"])
    assert np.array_equal(out["lam"], out["d_x0"]) and np.array_equal(out["mu"], out["d_u0"])


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_the_two_forms_agree_bit_for_bit(exe, order):
    """one plant for the batch through the uniform kernels, the packed block filled with it through the per-instance ones"""
    a = run(exe, "full_other", 65, False, order)[3]
    b = run(exe, "full_other", 65, True, order)[3]
    for n in ("d_x0", "d_u0", "d_yref", "d_noise", "d_plant", "c", "x", "u"):
        assert a[n] == b[n], n
