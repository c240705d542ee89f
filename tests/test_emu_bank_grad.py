"""The bank gradient kernels' own source (libmpc_amd/csrc/lmpc_bank_grad.hip) stepped through the SIMT emulator of tests/emu/ on the CPU: both
lane orders, guards behind every output, behind flags and n_used and behind the LDS limit, the LDS limit as an argument, the per-instance outputs
and the per-controller sums.  The model arrays of the K controllers come from host-only handles, the instance -> controller map is shuffled,
active sets and optima come from the oracle, and the results are held to the truth of each instance's own controller (tests/bank_grad_ref.py)
within bank_grad_ref.BANK_GRAD_KERNEL_TOL.  Built with clang++, as tests/test_emu_bank_sens.py is."""
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import bank_grad_ref as G
import sens_ref as S
from libmpc_amd.bank import group_by_model

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
PAD, GUARD, GUARD_I = 64, -7.25e300, -77
LDS = 160 * 1024
D_OUTS = ("d_oweight", "d_uweight", "d_duweight", "d_lower", "d_upper", "d_A", "d_B", "d_C", "d_Bd", "d_Dd")
C_OUTS = tuple("c" + n[1:] for n in D_OUTS)
KEYS = G.PARAM + G.MODEL                                           # the truth's names, in the order of D_OUTS
ALL, WEIGHTS, BOUNDS, MODEL = (1,) * 10, (1, 1, 1) + (0,) * 7, (0, 0, 0, 1, 1) + (0,) * 5, (0,) * 5 + (1,) * 5


def wave_len(cap, nx, nu, ny, ph, nz, model=True):
    """doubles of a wavefront's LDS slice for working sets of up to cap rows: bank_grad_wave_len of lmpc_bank_grad.hip, restated"""
    even = (nz + 1) & ~1
    n = max(cap * (cap + 1) // 2 + cap, 2 * ph * nx if model else 0) + 5 * cap + (ph + 2) // 2 + nx * (nx + nu) + ny * nx + 2 * even + (ph + 1) * nx + ph * ny
    return n + ((ph + 1) * (nx + nu) + even + ph * nu + 3 * nx + ph * ny if model else 0)


FULL = (4, 2, 2, 10, 20)                                           # nx, nu, ny, ph, nz of the full family
SMALL_LDS = 8 * wave_len(3, *FULL)                                 # one wavefront's slice for working sets of up to three rows
TINY_LDS = 8 * (wave_len(1, *FULL) - 1)                            # not one row


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
    out = str(tmp_path_factory.mktemp("emu_bank_grad") / "run_bank_grad")
    subprocess.run([cxx, "-O1", "-std=c++20", "-I" + EMU, "-w", "-o", out, os.path.join(EMU, "run_bank_grad.cpp"), os.path.join(EMU, "hipemu_switch.S")], check=True)
    return out


@functools.lru_cache(maxsize=None)
def hosts(name):
    from libmpc_amd import LMPC
    return [G.configure(LMPC(*sp["dims"], device=-1), sp) for sp in G.reference(name)["specs"]]


def _pad(act, words):
    act = np.asarray(act).astype(bool)
    out = np.zeros((act.shape[0], 32 * words), bool)
    out[:, :act.shape[1]] = act
    return out


def problem(name, pick=None):
    """the inputs of a family as the runner takes them (instances `pick`: all)"""
    R = G.reference(name)
    ctl = hosts(name)
    words = ctl[0].info()["active_words"]
    pick = np.arange(len(R["model"])) if pick is None else np.asarray(pick)
    return dict(ctl=ctl, specs=R["specs"], model=R["model"][pick].copy(), al=_pad(R["active_lower"], words)[pick], au=_pad(R["active_upper"], words)[pick],
                status=R["status"][pick].copy(), seed_cmd=R["seed_cmd"][pick], seed_input=R["seed_input"][pick], u0=R["u0"][pick],
                seq_state=R["seq_state"][pick], seq_output=R["seq_output"][pick], seq_input=R["input"][pick], yref=R["yref"][pick])


def run(exe, pr, want=ALL, flags=True, sums=(0,) * 10, n_used=False, groups=None, order="forward", limit=LDS, status=True, seed_cmd=True,
        seed_input=True, model=True, seq_state=True):
    """-> dict(rc, d_* [B, rows, cols] (bounds [B, m_ref]), flags [B], c_* [K, ..], n_used [K]) with the guards checked; outputs not asked for come
    back as None.  groups: (order, offsets) of the per-controller sums"""
    ctl = pr["ctl"]
    arrs = [G.arrays(c) for c in ctl]
    a = arrs[0]
    B, K = len(pr["al"]), len(ctl)
    nx, nu, ndu, ny, ph, ldg = a["nx"], a["nu"], a["ndu"], a["ny"], a["ph"], a["ldg"]
    words, m = ctl[0].info()["active_words"], a["m_rows"]
    n_soft = int(np.count_nonzero(ctl[0].debug_get("g_soft")))
    flag_word = (2 if a["terminal"] is not None else 0) | (a["nc"] << 2)
    head = [nx, nu, ndu, ny, ph, a["nz"], a["mg"], a["ldz"], ldg, a["ldy"], words, n_soft, m, flag_word, K, B, *want, int(flags), *sums, int(n_used)]
    bits = lambda f: S.pack_bits(np.asarray(f).astype(bool), words).view(np.uint32).astype(float).ravel()
    pad = lambda v: np.concatenate([np.asarray(v, float), np.zeros(ldg)])[:ldg]
    parts = [pad(a["g_kind"]), pad(a["g_step"]), pad(a["g_comp"]), pad(a["g_refrow"]), a["boxrow_ptr"][:a["nz"] + 1], a["boxrow_ref"], a["blk"]]
    for c, ak, sp in zip(ctl, arrs, pr["specs"]):
        uref, duref, dmeas = G.own_references(sp)
        parts += [c.debug_get("Y"), c.debug_get("model"), np.concatenate([c.debug_get("wOutput"), ak["terminal_raw"]]), c.debug_get("wU"), c.debug_get("wDeltaU"),
                  ak["scalar"], ak["sU"], np.concatenate([np.zeros(ldg), pad(ak["g_soft"])]), pad(ak["lg0"]), pad(ak["ug0"]),
                  np.asarray(sp["yref"]).T, np.asarray(uref).T, np.asarray(duref).T, np.asarray(dmeas).T]
    opt = lambda v, on: np.asarray(v, float) if on else np.zeros(0)
    parts += [opt(pr["model"], model), bits(pr["al"]), bits(pr["au"]), opt(pr["status"], status), opt(pr["seed_cmd"], seed_cmd), opt(pr["seed_input"], seed_input),
              pr["u0"], opt(pr["seq_state"], seq_state), pr["seq_output"], pr["seq_input"], pr["yref"]]
    parts += [np.zeros(0), np.zeros(0)] if groups is None else [np.asarray(groups[0], float), np.asarray(groups[1], float)]
    fin = lambda v: np.where(np.isfinite(v), v, np.sign(v) * 1e300)                     # (infinite bounds: never read, the rows they belong to are hard)
    flat = [np.asarray(head, float)]
    for v in parts:
        v = fin(np.asarray(v, float).ravel())
        flat += [np.array([float(len(v))]), v]
    inp = " ".join(repr(float(v)) for v in np.concatenate(flat)) + "\n"
    r = subprocess.run([exe, str(limit)], input=inp, capture_output=True, text=True, env=dict(os.environ, HIPEMU_ORDER=order), timeout=600)
    assert r.returncode == 0, r.stderr[:2000]
    o = json.loads(r.stdout)
    out = {"rc": o["rc"]}
    shapes = ((ph, ny), (ph, nu), (ph, nu), (m,), (m,), (nx, nx), (nu, nx), (nx, ny), (ndu, nx), (ndu, ny))       # column-major: [columns, rows]
    for names, lead, asked_all in ((D_OUTS, B, want), (C_OUTS, K, sums)):
        for name, shp, asked in zip(names, shapes, asked_all):
            v = np.array(o[name], float)
            cnt = int(np.prod((lead,) + shp))
            assert v.size == cnt + PAD and (v[cnt:] == GUARD).all(), name
            assert asked or (v == GUARD).all(), name                # an output that was not asked for is not written anywhere
            out[name] = None
            if asked and o["rc"] == 0:
                w = v[:cnt].reshape((lead,) + shp)
                out[name] = np.swapaxes(w, -1, -2) if len(shp) == 2 else w
    f = np.array(o["flags"])
    assert (f[B:] == GUARD_I).all() and (flags or (f == GUARD_I).all())
    out["flags"] = f[:B]
    nu_ = np.array(o["n_used"])
    assert (nu_[K:] == GUARD_I).all() and (n_used or (nu_ == GUARD_I).all())
    out["n_used"] = nu_[:K]
    return out


def _g(o, b, names=D_OUTS):
    return {k: o[n][b] for k, n in zip(KEYS, names) if o[n] is not None}


def _worst(name, R, pr, o, use):
    arrs = [G.arrays(c) for c in pr["ctl"]]
    ep = em = 0.0
    for b in use:
        p, m = G.compare(arrs[pr["model"][b]], R["truth"][b], _g(o, b), blocked=name == "blocked")
        ep, em = max(ep, p), max(em, m)
    return ep, em


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name", G.FAMILIES)
def test_gradients_match_the_truth_of_each_instance(exe, name, order):
    R = G.reference(name)
    pr = problem(name)
    o = run(exe, pr, order=order)
    assert o["rc"] == 0
    B = len(pr["al"])
    use = [b for b in range(B) if R["truth"][b] is not None]
    assert B - len(use) <= G.SKIP_CAP * B
    assert (o["flags"][use] == 0).all()
    ep, em = _worst(name, R, pr, o, use)
    print(f"{name} ({order}): worst error of the parameter / the model outputs / bound {ep:.2e} / {em:.2e} / {G.BANK_GRAD_KERNEL_TOL:.2e}")
    assert max(ep, em) <= G.BANK_GRAD_KERNEL_TOL


def test_every_instance_its_own_controller(exe):
    """no instance -> controller map: instance b is controller b"""
    R = G.reference("nz16")
    pick = np.array([int(np.nonzero(R["model"] == k)[0][0]) for k in range(len(R["specs"]))])
    pr = problem("nz16", pick)
    ident = run(exe, pr)                                            # model = [0, 1, .. K - 1]
    none = run(exe, pr, model=False)
    assert none["rc"] == 0 and (none["flags"] == 0).all()
    for n in D_OUTS:
        assert none[n].tobytes() == ident[n].tobytes(), n
    pr["model"] = np.arange(len(pick))
    ep, em = _worst("nz16", dict(truth=[R["truth"][b] for b in pick]), pr, none, range(len(pick)))
    assert max(ep, em) <= G.BANK_GRAD_KERNEL_TOL


def test_subsets_flags_sums_and_a_small_lds_limit(exe):
    R = G.reference("full")
    B = 19
    pr = problem("full", np.arange(B))
    ctl = pr["ctl"]
    K = len(ctl)
    d = R["truths"][0].param.pb.d
    pr["status"][5] = 2                                             # not solved: flag 1, NaN
    pr["al"][7] = False; pr["au"][7] = False
    pr["al"][7, d.neq + d.na + ctl[0].nx] = True; pr["au"][7, d.neq + d.off_du] = True          # box row and step-0 rate row of input 0: parallel, flag 2
    pr["model"][9] = K                                              # a model index outside the bank: flag 1, NaN
    per = run(exe, pr)
    assert per["rc"] == 0 and per["flags"][5] == 1 and per["flags"][7] == 2 and per["flags"][9] == 1
    for n in D_OUTS:
        assert np.isnan(per[n][[5, 7, 9]]).all(), n
    good = [b for b in range(B) if b not in (5, 7, 9) and R["truth"][b] is not None]
    assert (per["flags"][good] == 0).all()
    ep, em = _worst("full", R, pr, per, good)
    assert max(ep, em) <= G.BANK_GRAD_KERNEL_TOL
    # a seed on cmd alone and on the sequence alone add up to both (the map is linear in the seed)
    one, two = run(exe, pr, seed_input=False), run(exe, pr, seed_cmd=False)
    for n in D_OUTS:
        assert np.abs(one[n][good] + two[n][good] - per[n][good]).max() <= 1e-12 * max(1.0, np.abs(per[n][good]).max()), n
    # each output subset: the outputs asked for keep their bits, the others are written nowhere (run() checks that); without a model output
    # the sequence of states may be missing
    for want, kw in ((WEIGHTS, dict(seq_state=False)), (BOUNDS, dict(seq_state=False)), (MODEL, {}), ((0, 1, 0, 0, 1, 0, 1, 0, 0, 1), dict(flags=False))):
        part = run(exe, pr, want=want, **kw)
        assert part["rc"] == 0
        for n, asked in zip(D_OUTS, want):
            assert part[n] is None if not asked else part[n].tobytes() == per[n].tobytes(), n
    # the per-controller sums: the instances of a controller in the order of group_by_model, the flagged ones left out
    member = pr["model"].copy(); member[9] = 0                      # (the instance with the foreign index is listed under a controller: it is flagged, so it adds nothing)
    grp = group_by_model(member, K)
    used = per["flags"] == 0
    for order in ("forward", "reverse"):
        red = run(exe, pr, sums=ALL, n_used=True, groups=grp, order=order)
        assert red["rc"] == 0 and np.array_equal(red["flags"], per["flags"])
        for dn, cn in zip(D_OUTS, C_OUTS):
            assert red[dn].tobytes() == per[dn].tobytes()
            ref, cnt = G.group_sums(np.where(used.reshape((-1,) + (1,) * (per[dn].ndim - 1)), per[dn], 0.0), per["flags"], *grp)
            mass, _ = G.group_sums(np.abs(np.where(used.reshape((-1,) + (1,) * (per[dn].ndim - 1)), per[dn], 0.0)), per["flags"], *grp)
            assert np.array_equal(red["n_used"], cnt)
            for k in range(K):
                assert (np.abs(red[cn][k] - ref[k]) <= max(cnt[k], 1) * 2.0 ** -52 * mass[k]).all(), (cn, k)
        if order == "forward":
            first = red
        else:
            assert all(red[n].tobytes() == first[n].tobytes() for n in C_OUTS)      # the order of the lanes does not enter the sums
    part = run(exe, pr, want=(1, 0, 0, 0, 1, 0, 1, 0, 0, 0), sums=(1, 0, 0, 0, 0, 0, 1, 0, 0, 0), groups=grp, flags=False)      # no flags: the rows tell who counts
    assert part["c_oweight"].tobytes() == first["c_oweight"].tobytes() and part["c_B"].tobytes() == first["c_B"].tobytes()
    part = run(exe, pr, want=BOUNDS, sums=(0,) * 10, n_used=True, groups=grp, flags=False, seq_state=False)
    assert np.array_equal(part["n_used"], first["n_used"])
    # an LDS limit that holds working sets of a few rows only: the larger ones get flag 3 and NaN, the others keep their bits
    a = G.arrays(ctl[0])
    small = run(exe, pr, limit=SMALL_LDS, sums=ALL, n_used=True, groups=grp)
    assert small["rc"] == 0
    sizes = np.array([len(S.working_set(a, pr["al"][b] | pr["au"][b])) for b in range(B)])
    three = small["flags"] == 3
    assert three.any() and (~three).sum() >= 3 and sizes[three].min() > sizes[~three & (small["flags"] == 0)].max()
    keep = small["flags"] == 0
    for n in D_OUTS:
        assert np.isnan(small[n][three]).all() and small[n][keep].tobytes() == per[n][keep].tobytes(), n
    assert small["n_used"].sum() == keep.sum()
    # not even one row fits: the launch is refused and writes nothing
    none = run(exe, pr, limit=TINY_LDS)
    assert none["rc"] == -2 and (none["flags"] == GUARD_I).all()
