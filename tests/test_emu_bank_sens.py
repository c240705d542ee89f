"""The bank sensitivity kernel's own source (libmpc_amd/csrc/lmpc_bank_sens.hip) stepped through the SIMT emulator of tests/emu/ on the CPU: both
lane orders, guards behind every output and behind the LDS limit, the LDS limit as an argument.  The model arrays of the K controllers come from
host-only handles, the instance -> controller map is shuffled, active sets come from the oracle, and the results are held to the KKT system of each
instance's own reference QP (tests/bank_sens_ref.py) within bank_sens_ref.BANK_KERNEL_TOL.  Built with clang++, as tests/test_emu_sens.py is."""
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import bank_sens_ref as BR
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
    out = str(tmp_path_factory.mktemp("emu_bank_sens") / "run_bank_sens")
    subprocess.run([cxx, "-O1", "-std=c++20", "-I" + EMU, "-w", "-o", out, os.path.join(EMU, "run_bank_sens.cpp"), os.path.join(EMU, "hipemu_switch.S")], check=True)
    return out


@functools.lru_cache(maxsize=None)
def hosts(name):
    from libmpc_amd import LMPC
    return [BR.configure(LMPC(*sp["dims"], device=-1), sp) for sp in BR.reference(name)["specs"]]


def run(exe, ctl, model, al, au, status=None, seed_cmd=None, seed_input=None, want=(1, 1, 1, 1), order="forward", limit=LDS):
    """-> dict(rc, d_x0, d_u0, d_yref [B, (nu,) n], flags [B]) with the guards checked; outputs not asked for come back as None.  model: the
    controller of every instance, or None (instance b = controller b)"""
    arrs = [BR.arrays(c) for c in ctl]
    a = arrs[0]
    B = len(al)
    words = ctl[0].info()["active_words"]
    jac = seed_cmd is None and seed_input is None
    n_soft = int(np.count_nonzero(ctl[0].debug_get("g_soft")))
    mg = a["mg"]
    head = [a["nx"], a["nu"], a["ny"], a["ph"], a["nz"], mg, a["ldz"], a["ldg"], a["ldy"], words, n_soft, int(a["terminal"] is not None),
            len(a["terminal_raw"]), a["nc"], len(ctl), B, int(jac), int(model is not None), int(status is not None), int(seed_cmd is not None),
            int(seed_input is not None), *want, len(a["boxrow_ref"])]
    bits = lambda f: S.pack_bits(np.asarray(f).astype(bool), words).view(np.uint32).astype(float).ravel()
    parts = [head, a["g_kind"][:mg], a["g_step"][:mg], a["g_comp"][:mg], a["g_refrow"][:mg], a["boxrow_ptr"][:a["nz"] + 1], a["boxrow_ref"], a["blk"]]
    for c, ak in zip(ctl, arrs):
        nx, nu, ny = a["nx"], a["nu"], a["ny"]
        parts += [c.debug_get("Y"), c.debug_get("model")[:nx * nx + nx * nu + ny * nx], c.debug_get("wOutput"), ak["terminal_raw"], c.debug_get("wDeltaU"),
                  ak["scalar"], ak["sU"]]
    parts += [p for p in (model,) if p is not None] + [bits(al), bits(au)]
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
@pytest.mark.parametrize("name", ["smallest", "nz16", "nz17", "full", "soft", "blocked"])
def test_jacobians_match_the_kkt_system_of_each_instance(exe, name, order):
    R = BR.reference(name)
    ctl = hosts(name)
    words = ctl[0].info()["active_words"]
    o = run(exe, ctl, R["model"], _pad(R["active_lower"], words), _pad(R["active_upper"], words), status=R["status"], order=order)
    assert o["rc"] == 0
    J = np.concatenate([o["d_x0"], o["d_u0"], o["d_yref"]], axis=-1)
    use = [b for b in range(len(J)) if R["jac"][b] is not None]
    assert len(use) >= (1.0 - BR.SKIP_CAP) * len(J)
    assert (o["flags"][use] == 0).all()
    worst = max(BR.error(J[b], R["jac"][b]["cmd"]) for b in use)
    print(f"{name} ({order}): worst error / bound {worst:.2e} / {BR.BANK_KERNEL_TOL:.2e}")
    assert worst <= BR.BANK_KERNEL_TOL


def test_every_instance_its_own_controller(exe):
    """no instance -> controller map: instance b is controller b"""
    R = BR.reference("nz16")
    ctl = hosts("nz16")
    words = ctl[0].info()["active_words"]
    pick = np.array([int(np.nonzero(R["model"] == k)[0][0]) for k in range(len(ctl))])
    o = run(exe, ctl, None, _pad(R["active_lower"], words)[pick], _pad(R["active_upper"], words)[pick], status=R["status"][pick])
    assert o["rc"] == 0 and (o["flags"] == 0).all()
    J = np.concatenate([o["d_x0"], o["d_u0"], o["d_yref"]], axis=-1)
    assert max(BR.error(J[k], R["jac"][b]["cmd"]) for k, b in enumerate(pick)) <= BR.BANK_KERNEL_TOL


def test_vjp_null_outputs_flags_and_a_small_lds_limit(exe):
    R = BR.reference("full")
    ctl = hosts("full")
    words = ctl[0].info()["active_words"]
    B, nu, ph = 19, ctl[0].nu, ctl[0].ph
    al, au = _pad(R["active_lower"], words)[:B], _pad(R["active_upper"], words)[:B]
    model = R["model"][:B]
    status = R["status"][:B].copy()
    status[5] = 2                                                   # not solved: flag 1, NaN
    d = R["pbs"][0].d
    al[7] = False; au[7] = False
    al[7, d.neq + d.na + ctl[0].nx] = True; au[7, d.neq + d.off_du] = True          # box row and step-0 rate row of input 0: parallel, flag 2
    rg = np.random.default_rng(3)
    sc, sq = rg.normal(size=(B, nu)), rg.normal(size=(B, ph + 1, nu))
    jac = run(exe, ctl, model, al, au, status=status)
    J = np.concatenate([jac["d_x0"], jac["d_u0"], jac["d_yref"]], axis=-1)
    assert jac["flags"][5] == 1 and jac["flags"][7] == 2 and np.isnan(J[5]).all() and np.isnan(J[7]).all()
    good = [b for b in range(B) if b not in (5, 7) and R["jac"][b] is not None]
    assert (jac["flags"][good] == 0).all()
    for order in ("forward", "reverse"):
        for kw in (dict(seed_cmd=sc, seed_input=sq), dict(seed_cmd=sc), dict(seed_input=sq)):
            v = run(exe, ctl, model, al, au, status=status, order=order, **kw)
            g = np.concatenate([v["d_x0"], v["d_u0"], v["d_yref"]], axis=-1)
            assert np.array_equal(v["flags"], jac["flags"])
            for b in good:
                ref, mass = 0.0, 0.0
                if "seed_cmd" in kw:
                    ref = ref + np.einsum("r,rc->c", sc[b], R["jac"][b]["cmd"]); mass += np.abs(sc[b]).sum()
                if "seed_input" in kw:
                    ref = ref + np.einsum("ir,irc->c", sq[b], R["jac"][b]["input"]); mass += np.abs(sq[b]).sum()
                bound = BR.BANK_KERNEL_TOL * max(1.0, np.abs(R["jac"][b]["input"]).max()) * mass
                assert np.abs(g[b] - ref).max() <= bound, b
    # outputs that are not asked for: the others keep their bits
    part = run(exe, ctl, model, al, au, status=status, want=(0, 1, 0, 0))
    assert part["d_u0"].tobytes() == jac["d_u0"].tobytes()
    # an LDS limit that holds working sets of a few rows only: the larger ones get flag 3 and NaN, the others keep their bits
    a = BR.arrays(ctl[0])
    small = run(exe, ctl, model, al, au, status=status, limit=1696)
    assert small["rc"] == 0
    sizes = np.array([len(S.working_set(a, al[b] | au[b])) for b in range(B)])
    three = small["flags"] == 3
    assert three.any() and (~three).sum() >= 3 and sizes[three].min() > sizes[~three & (small["flags"] == 0)].max()
    Js = np.concatenate([small["d_x0"], small["d_u0"], small["d_yref"]], axis=-1)
    assert np.isnan(Js[three]).all()
    keep = small["flags"] == 0
    assert Js[keep].tobytes() == J[keep].tobytes()
    # not even one row fits: the launch is refused and writes nothing
    none = run(exe, ctl, model, al, au, status=status, limit=512)
    assert none["rc"] == -2 and (none["flags"] == GUARD_I).all()
