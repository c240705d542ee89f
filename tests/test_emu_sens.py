"""The sensitivity kernel's own source (libmpc_amd/csrc/lmpc_sens.hip) stepped through the SIMT emulator of tests/emu/ on the CPU: both lane
orders, guards behind every output and behind the LDS limit, the LDS limit as an argument.  Model arrays come from a host-only handle, active
sets from the oracle, and the results are held to the KKT system of the reference QP (tests/sens_ref.py) within sens_ref.KERNEL_TOL.  Built with
clang++, as tests/test_emu_condense.py is: the LMPC kernels' helpers name the components of a two-double vector."""
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import sens_ref as S

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
PAD, GUARD, GUARD_I = 64, -7.25e300, -77
LDS = 160 * 1024


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
    out = str(tmp_path_factory.mktemp("emu_sens") / "run_sens")
    subprocess.run([cxx, "-O1", "-std=c++20", "-I" + EMU, "-w", "-o", out, os.path.join(EMU, "run_sens.cpp"), os.path.join(EMU, "hipemu_switch.S")], check=True)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    return S.reference(name)


@functools.lru_cache(maxsize=None)
def host(name):
    from libmpc_amd import LMPC
    sp = reference(name)["sp"]
    return S.configure(LMPC(*sp["dims"], device=-1), sp)


def run(exe, c, al, au, status=None, seed_cmd=None, seed_input=None, want=(1, 1, 1, 1), order="forward", limit=LDS):
    """-> dict(rc, d_x0, d_u0, d_yref [B, (nu,) n], flags [B]) with the guards checked; outputs not asked for come back as None"""
    a = S.arrays(c)
    B = len(al)
    words = c.info()["active_words"]
    jac = seed_cmd is None and seed_input is None
    n_soft = int(np.count_nonzero(c.debug_get("g_soft")))
    head = [a["nx"], a["nu"], a["ny"], a["ph"], a["nz"], a["mg"], a["ldz"], a["ldg"], a["ldy"], a["rowsF"], a["kin"], a["nxp"], a["nup"], a["nyp"],
            int(c.debug_get("dims_maps")[5]), words, n_soft, B, int(jac), int(status is not None), int(seed_cmd is not None), int(seed_input is not None),
            *want, len(a["boxrow_ref"])]
    bits = lambda f: S.pack_bits(np.asarray(f).astype(bool), words).view(np.uint32).astype(float).ravel()
    parts = [head, c.debug_get("Y"), c.debug_get("MF1"), a["g_refrow"][:a["mg"]], a["boxrow_ptr"][:a["nz"] + 1], a["boxrow_ref"], a["blk"], bits(al), bits(au)]
    parts += [p for p in (status, seed_cmd, seed_input) if p is not None]
    inp = " ".join(repr(float(v)) for v in np.concatenate([np.asarray(p, float).ravel() for p in parts])) + "\n"
    r = subprocess.run([exe, str(limit)], input=inp, capture_output=True, text=True, env=dict(os.environ, HIPEMU_ORDER=order), timeout=600)
    assert r.returncode == 0, r.stderr[:2000]
    o = json.loads(r.stdout)
    R = a["nu"] if jac else 1
    out = {"rc": o["rc"]}
    for (name, n), asked in zip((("d_x0", a["nx"]), ("d_u0", a["nu"]), ("d_yref", a["ny"])), want):
        v = np.array(o[name], float)
        cnt = B * R * n
        assert v.size == cnt + PAD and (v[cnt:] == GUARD).all(), name
        assert asked or (v == GUARD).all(), name                    # an output that was not asked for is not written anywhere
        out[name] = v[:cnt].reshape((B, R, n) if jac else (B, n)) if asked and o["rc"] == 0 else None
    f = np.array(o["flags"])
    assert (f[B:] == GUARD_I).all() and (want[3] or (f == GUARD_I).all())
    out["flags"] = f[:B]
    return out


def _pad(act, words):
    act = np.asarray(act).astype(bool)
    out = np.zeros((act.shape[0], 32 * words), bool)
    out[:, :act.shape[1]] = act
    return out


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name", ["smallest", "nz15", "nz16", "nz17", "full", "soft", "blocked"])
def test_jacobians_match_the_kkt_system(exe, name, order):
    R = reference(name)
    c = host(name)
    words = c.info()["active_words"]
    res = R["res"]
    o = run(exe, c, _pad(res["active_lower"], words), _pad(res["active_upper"], words), status=res["status"], order=order)
    assert o["rc"] == 0
    J = np.concatenate([o["d_x0"], o["d_u0"], o["d_yref"]], axis=-1)
    use = [b for b in range(len(J)) if R["jac"][b] is not None]
    assert (o["flags"][use] == 0).all()
    worst = max(np.abs(J[b] - R["jac"][b]["cmd"]).max() / max(1.0, np.abs(R["jac"][b]["cmd"]).max()) for b in use)
    print(f"{name} ({order}): worst error / bound {worst:.2e} / {S.KERNEL_TOL:.2e}")
    assert worst <= S.KERNEL_TOL


def test_vjp_null_outputs_flags_and_a_small_lds_limit(exe):
    R = reference("full")
    c = host("full")
    words = c.info()["active_words"]
    res = R["res"]
    al, au = _pad(res["active_lower"], words)[:19], _pad(res["active_upper"], words)[:19]
    B, nu, ph = 19, c.nu, c.ph
    status = res["status"][:B].copy()
    status[5] = 2                                                   # not solved: flag 1, NaN
    d = R["pb"].d
    al[7] = False; au[7] = False
    al[7, d.neq + d.na + c.nx] = True; au[7, d.neq + d.off_du] = True          # box row and step-0 rate row of input 0: parallel, flag 2
    rg = np.random.default_rng(3)
    sc, sq = rg.normal(size=(B, nu)), rg.normal(size=(B, ph + 1, nu))
    jac = run(exe, c, al, au, status=status)
    J = np.concatenate([jac["d_x0"], jac["d_u0"], jac["d_yref"]], axis=-1)
    assert jac["flags"][5] == 1 and jac["flags"][7] == 2 and np.isnan(J[5]).all() and np.isnan(J[7]).all()
    good = [b for b in range(B) if b not in (5, 7) and R["jac"][b] is not None]
    assert (jac["flags"][good] == 0).all()
    for order in ("forward", "reverse"):
        v = run(exe, c, al, au, status=status, seed_cmd=sc, seed_input=sq, order=order)
        g = np.concatenate([v["d_x0"], v["d_u0"], v["d_yref"]], axis=-1)
        assert np.array_equal(v["flags"], jac["flags"])
        for b in good:
            ref = np.einsum("r,rc->c", sc[b], R["jac"][b]["cmd"]) + np.einsum("ir,irc->c", sq[b], R["jac"][b]["input"])
            bound = S.KERNEL_TOL * max(1.0, np.abs(R["jac"][b]["input"]).max()) * (np.abs(sc[b]).sum() + np.abs(sq[b]).sum())
            assert np.abs(g[b] - ref).max() <= bound, b
    # outputs that are not asked for: the others keep their bits
    part = run(exe, c, al, au, status=status, want=(0, 1, 0, 0))
    assert part["d_u0"].tobytes() == jac["d_u0"].tobytes()
    # an LDS limit that holds working sets of a few rows only: the larger ones get flag 3 and NaN, the others keep their bits
    a = S.arrays(c)
    small = run(exe, c, al, au, status=status, limit=8 * 1024)
    assert small["rc"] == 0
    sizes = np.array([len(S.working_set(a, al[b] | au[b])) for b in range(B)])
    three = small["flags"] == 3
    assert three.any() and (~three).sum() >= 3 and sizes[three].min() > sizes[~three & (small["flags"] == 0)].max()
    Js = np.concatenate([small["d_x0"], small["d_u0"], small["d_yref"]], axis=-1)
    assert np.isnan(Js[three]).all()
    keep = small["flags"] == 0
    assert Js[keep].tobytes() == J[keep].tobytes()
