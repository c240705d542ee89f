"""The model-sensitivity kernels' own source (libmpc_amd/csrc/lmpc_model_sens.hip) stepped through the SIMT emulator of tests/emu/ on the CPU:
both lane orders, guards behind every output, behind the partials buffer and behind the LDS limit, the LDS limit as an argument, the per-instance
and the reduced form.  Model arrays come from a host-only handle, active sets and optima from the oracle, and the results are held to the truth
of tests/model_sens_ref.py (the KKT system of the reference QP) within model_sens_ref.KERNEL_TOL.  Built with clang++, as tests/test_emu_sens.py is."""
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import model_sens_ref as Mo
import sens_ref as S

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
PAD, GUARD, GUARD_I = 64, -7.25e300, -77
LDS = 160 * 1024
SMALL_LDS = 19 * 1024            # the full family's shared operands and working sets of up to nine rows
OUTS = ("d_A", "d_B", "d_C", "d_Bd", "d_Dd")


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
    out = str(tmp_path_factory.mktemp("emu_model_sens") / "run_model_sens")
    subprocess.run([cxx, "-O1", "-std=c++20", "-I" + EMU, "-w", "-o", out, os.path.join(EMU, "run_model_sens.cpp"), os.path.join(EMU, "hipemu_switch.S")], check=True)
    return out


@functools.lru_cache(maxsize=None)
def host(name):
    from libmpc_amd import LMPC
    sp = Mo.reference(name)["sp"]
    return S.configure(LMPC(*sp["dims"], device=-1), sp)


def _pad(act, words):
    act = np.asarray(act).astype(bool)
    out = np.zeros((act.shape[0], 32 * words), bool)
    out[:, :act.shape[1]] = act
    return out


def problem(name, B=None):
    """the inputs of a family as the runner takes them: active sets, status, seeds, the oracle's optimum rolled out, per-step references"""
    R = Mo.reference(name)
    c = host(name)
    sp, res = R["sp"], R["res"]
    nx, nu, ndu, ny, ph, ch = sp["dims"]
    B = len(R["x0"]) if B is None else B
    words = c.info()["active_words"]
    tile = lambda m: np.tile(np.asarray(m, float).T[None], (B, 1, 1))
    seqs = [Mo.rollout(sp, R["x0"][b], res["input"][b]) for b in range(B)]
    return dict(c=c, al=_pad(res["active_lower"], words)[:B], au=_pad(res["active_upper"], words)[:B], status=res["status"][:B].copy(),
                seed_cmd=R["seed_cmd"][:B], seed_input=R["seed_input"][:B], u0=R["u0"][:B],
                seq_state=np.stack([s[0] for s in seqs]), seq_output=np.stack([s[1] for s in seqs]), seq_input=res["input"][:B],
                yref=np.tile(R["yref"][:B, None, :], (1, ph, 1)), uref=tile(sp["uref"]), duref=tile(sp["duref"]),
                dmeas=tile(sp.get("dmeas", np.zeros((ndu, ph)))))


def run(exe, pr, reduce=False, want=(1,) * 7, order="forward", limit=LDS, status=True, seed_cmd=True, seed_input=True):
    """-> dict(rc, d_A [B, nx, nx] ..., flags [B], n_used) with the guards checked; outputs not asked for come back as None.  Reduced: the same
    without the leading B"""
    c = pr["c"]
    a = Mo.arrays(c)
    B = len(pr["al"])
    nx, nu, ndu, ny, ph = a["nx"], a["nu"], a["ndu"], a["ny"], a["ph"]
    words, m = c.info()["active_words"], a["m_rows"]
    soft = c.debug_get("g_soft")
    n_soft = int(np.count_nonzero(soft))
    term = c.debug_get("terminal")
    flag_word = (2 if len(term) else 0) | (a["nc"] << 2)
    head = [nx, nu, ndu, ny, ph, a["nz"], a["mg"], a["ldz"], a["ldg"], a["ldy"], int(c.debug_get("dims_maps")[5]), words, n_soft, m, flag_word,
            B, int(reduce), *want]
    bits = lambda f: S.pack_bits(np.asarray(f).astype(bool), words).view(np.uint32).astype(float).ravel()
    model = c.debug_get("model")
    nA, nB, nC = nx * nx, nx * nu, ny * nx
    pad = lambda v: np.concatenate([np.asarray(v, float), np.zeros(a["ldg"] - len(v))])[:a["ldg"]]
    arrs = [c.debug_get("Y"), c.debug_get("Xq"), model[:nA], model[nA:nA + nB], model[nA + nB:nA + nB + nC],
            np.concatenate([c.debug_get("wOutput"), term]), c.debug_get("wU"), c.debug_get("wDeltaU"), c.debug_get("scalar"), c.debug_get("sU"),
            np.concatenate([np.zeros(a["ldg"]), pad(soft)]), pad(c.debug_get("lg0")), pad(c.debug_get("ug0")),
            pad(a["g_kind"]), pad(a["g_step"]), pad(a["g_comp"]), pad(a["g_refrow"]), a["boxrow_ptr"][:a["nz"] + 1], a["boxrow_ref"], a["blk"],
            bits(pr["al"]), bits(pr["au"])]
    arrs += [pr[k] if on else np.zeros(0) for k, on in (("status", status), ("seed_cmd", seed_cmd), ("seed_input", seed_input))]
    arrs += [pr[k] for k in ("u0", "seq_state", "seq_output", "seq_input", "yref", "uref", "duref", "dmeas")]
    fin = lambda v: np.where(np.isfinite(v), v, np.sign(v) * 1e300)                     # (infinite bounds: never read, the rows they belong to are hard)
    flat = [np.asarray(head, float)]
    for v in arrs:
        v = fin(np.asarray(v, float).ravel())
        flat += [np.array([float(len(v))]), v]
    inp = " ".join(repr(float(v)) for v in np.concatenate(flat)) + "\n"
    r = subprocess.run([exe, str(limit)], input=inp, capture_output=True, text=True, env=dict(os.environ, HIPEMU_ORDER=order), timeout=600)
    assert r.returncode == 0, r.stderr[:2000]
    o = json.loads(r.stdout)
    lead = () if reduce else (B,)
    out = {"rc": o["rc"]}
    shapes = ((nx, nx), (nu, nx), (nx, ny), (ndu, nx), (ndu, ny))                      # column-major: [columns, rows]
    for name, shp, asked in zip(OUTS, shapes, want):
        v = np.array(o[name], float)
        cnt = int(np.prod(lead + shp))
        assert v.size == cnt + PAD and (v[cnt:] == GUARD).all(), name
        assert asked or (v == GUARD).all(), name                    # an output that was not asked for is not written anywhere
        out[name] = None
        if asked and o["rc"] == 0:
            out[name] = np.swapaxes(v[:cnt].reshape(lead + shp), -1, -2)
    f = np.array(o["flags"])
    assert (f[B:] == GUARD_I).all() and (want[5] or (f == GUARD_I).all())
    out["flags"] = f[:B]
    nu_ = np.array(o["n_used"])
    assert (nu_[1:] == GUARD_I).all() and ((want[6] and reduce) or nu_[0] == GUARD_I)
    out["n_used"] = int(nu_[0])
    return out


def _g(o, b):
    return {k: o[n][b] for k, n in zip(Mo.MODEL, OUTS)}


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name", Mo.FAMILIES)
def test_gradients_match_the_truth(exe, name, order):
    R = Mo.reference(name)
    pr = problem(name)
    o = run(exe, pr, order=order)
    assert o["rc"] == 0
    use = [b for b in range(len(pr["al"])) if R["truth"][b] is not None]
    assert len(pr["al"]) - len(use) <= Mo.SKIP_CAP * len(pr["al"])
    assert (o["flags"][use] == 0).all()
    worst = max(Mo.compare(R["truth"][b], _g(o, b)) for b in use)
    print(f"{name} ({order}): worst error / bound {worst:.2e} / {Mo.KERNEL_TOL:.2e}")
    assert worst <= Mo.KERNEL_TOL


def test_reduced_form_flags_null_outputs_and_a_small_lds_limit(exe):
    R = Mo.reference("full")
    B = 19                                                          # two workgroups, the second partly filled
    pr = problem("full", B)
    c = pr["c"]
    a = Mo.arrays(c)
    d = R["tr"].pb.d
    pr["status"][5] = 2                                             # not solved: flag 1, NaN
    pr["al"][7] = False; pr["au"][7] = False
    pr["al"][7, d.neq + d.na + c.nx] = True; pr["au"][7, d.neq + d.off_du] = True          # box row and step-0 rate row of input 0: parallel, flag 2
    per = run(exe, pr)
    assert per["rc"] == 0 and per["flags"][5] == 1 and per["flags"][7] == 2
    for n in OUTS:
        assert np.isnan(per[n][5]).all() and np.isnan(per[n][7]).all()
    good = [b for b in range(B) if b not in (5, 7) and R["truth"][b] is not None]
    assert (per["flags"][good] == 0).all()
    for b in good:
        assert Mo.compare(R["truth"][b], _g(per, b)) <= Mo.KERNEL_TOL, b
    # a seed on cmd alone and on the sequence alone add up to both (the map is linear in the seed)
    one = run(exe, pr, seed_input=False)
    two = run(exe, pr, seed_cmd=False)
    for n in OUTS:
        s = one[n][good] + two[n][good]
        assert np.abs(s - per[n][good]).max() <= 1e-12 * max(1.0, np.abs(per[n][good]).max())
    used = per["flags"] == 0
    for order in ("forward", "reverse"):
        red = run(exe, pr, reduce=True, order=order)
        assert red["rc"] == 0 and red["n_used"] == used.sum() and np.array_equal(red["flags"], per["flags"])
        for n in OUTS:
            ref = per[n][used].sum(axis=0)
            bound = B * 2.0 ** -52 * np.abs(per[n][used]).sum(axis=0)
            assert (np.abs(red[n] - ref) <= bound).all(), n
        if order == "forward":
            first = red
        else:
            assert all(red[n].tobytes() == first[n].tobytes() for n in OUTS)      # the order of the lanes does not enter the sums
    # outputs that are not asked for: the others keep their bits
    part = run(exe, pr, want=(0, 1, 0, 0, 1, 0, 0))
    assert part["d_B"].tobytes() == per["d_B"].tobytes() and part["d_Dd"].tobytes() == per["d_Dd"].tobytes()
    part = run(exe, pr, reduce=True, want=(1, 0, 0, 1, 0, 0, 1))
    assert part["n_used"] == used.sum() and part["d_A"].tobytes() == first["d_A"].tobytes() and part["d_Bd"].tobytes() == first["d_Bd"].tobytes()
    part = run(exe, pr, reduce=True, want=(0, 1, 0, 0, 0, 0, 0))      # d_B alone: null destinations on both sides of it, no count
    assert part["d_B"].tobytes() == first["d_B"].tobytes()
    # an LDS limit that holds working sets of a few rows only: the larger ones get flag 3 and NaN, the others keep their bits
    small = run(exe, pr, limit=SMALL_LDS)
    assert small["rc"] == 0
    sizes = np.array([len(S.working_set(a, pr["al"][b] | pr["au"][b])) for b in range(B)])
    three = small["flags"] == 3
    assert three.any() and (~three).sum() >= 3 and sizes[three].min() > sizes[~three & (small["flags"] == 0)].max()
    keep = small["flags"] == 0
    for n in OUTS:
        assert np.isnan(small[n][three]).all() and small[n][keep].tobytes() == per[n][keep].tobytes()
    sred = run(exe, pr, reduce=True, limit=SMALL_LDS)
    assert sred["n_used"] == keep.sum()
    # a limit below the shared operands: the launch is refused, nothing is written
    none = run(exe, pr, limit=4 * 1024)
    assert none["rc"] == -2 and (none["flags"] == GUARD_I).all()

