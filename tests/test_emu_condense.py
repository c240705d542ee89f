"""The bank's condensing kernel (libmpc_amd/csrc/lmpc_hetero.hip: lmpc_condense_launch and lmpc_condense_models in both forms, compiled
unchanged) stepped through on the host by the lock-step interpreter of tests/emu (TEST INFRASTRUCTURE, see tests/emu/hip/hip_runtime.h), against
the 60-digit truths of tests/golden/condense_truth_*.npz and within the bound of tests/condense_ref.py, in both orders in which the
interpreter may run the lanes of a wavefront.  No GPU, nothing of libmpcx.so but the O(n) arrays a host-only controller lays out.  In one of
the two orders a matrix that is read before every lane has finished writing it (a missing barrier) gives other numbers; a store by a lane that
owns no entry lands in the guards behind the output arrays, the kernel's LDS plan or its scratch block.  The program is built with clang++: the
helpers of the LMPC kernels name the components of a two-double vector, which g++'s vector extension does not have."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import condense_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
PAD, GUARD = 64, -7.25e300


def _clangxx():
    for c in (shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and os.path.exists(c):
            return c
    return None


def _build(tmp, name, defines=()):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not installed")
    exe = str(tmp / name)
    subprocess.run([cxx, "-O1", "-std=c++20", "-I" + EMU, "-w", *defines, "-o", exe, os.path.join(EMU, "run_condense.cpp"),
                    os.path.join(EMU, "hipemu_switch.S")], check=True)
    return exe


def _numbers(c, ctl, lay):
    """one controller's part of the runner's input: the O(n) arrays as the host-only controller `c` lays them out"""
    nx, nu, ny, ph, ch = ctl["dims"]
    nz, mg, ldz, ldg, ldy = (int(v) for v in c.debug_get("dims")[:5])
    term = c.debug_get("terminal")
    assert (term.size > 0) == ("P" in ctl) and (term.size == 0 or term.size == nx * nx + nx + nx * ny)
    cm = lambda a: np.asarray(a, float).T.ravel()
    wy, wu = c.debug_get("wOutput"), c.debug_get("wU")
    assert wy.size == (ph + 1) * ny and wu.size == (ph + 1) * nu
    parts = [[nx, nu, ny, ph, nz, mg, ldz, ldg, ldy, 1 | (2 if term.size else 0), 0.1, R.SIGMA],
             cm(ctl["A"]), cm(ctl["B"]), cm(ctl["C"]), wy, term, wu, cm(ctl["DUW"]), ctl.get("sX", np.zeros(nx)), ctl.get("sU", np.zeros(nu)), lay["blk"]]
    parts += [c.debug_get(k) for k in ("g_kind", "g_step", "g_comp", "lw", "uw", "lg0", "ug0", "g_soft")]
    assert [len(p) for p in parts[-8:]] == [ldg] * 3 + [ldz] * 2 + [ldg] * 3
    return np.concatenate([np.asarray(p, float).ravel() for p in parts])


def _run(exe, ctrls, members, order="forward"):
    """-> (the runner's JSON, [arrays of controller k as debug_get returns them]); the guards checked"""
    inp = " ".join(repr(float(v)) for v in np.concatenate([_numbers(c, ctl, lay) for c, (ctl, lay, _) in zip(ctrls, members)])) + "\n"
    r = subprocess.run([exe, str(len(ctrls))], input=inp, capture_output=True, text=True, env=dict(os.environ, HIPEMU_ORDER=order), timeout=600)
    assert r.returncode == 0, r.stderr[:2000]
    o = json.loads(r.stdout)
    assert o["rc"] == 0
    gots = []
    for c, oc in zip(ctrls, o["controllers"]):
        nz, mg, ldz, ldg, ldy = (int(v) for v in c.debug_get("dims")[:5])
        got = {}
        for name, cnt in (("H", ldz * ldz), ("Kinv", ldz * ldz), ("Gr", ldg * ldz), ("Gc", ldz * ldg), ("Y", ldy * ldy), ("rho_b", ldz), ("rho_g", 2 * ldg)):
            a = np.array(oc[name])
            assert a.size == cnt + PAD and (a[cnt:] == GUARD).all(), name       # nothing behind the array: no lane without an entry stores anything
            got[name] = a[:cnt]
        assert np.array_equal(got["rho_g"][ldg:], c.debug_get("g_soft"))         # the soft entries behind the step sizes: read, never written
        got["rho_g"] = got["rho_g"][:ldg]
        assert oc["cond_status"] == 0
        got["cost_direct"] = oc["cost_direct"]
        gots.append(got)
    return o, gots


@pytest.fixture(scope="module")
def runner(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("emu"), "run_condense")


@pytest.fixture(scope="module")
def runner_one_workgroup(tmp_path_factory):
    """the launcher's grids capped at one workgroup: it condenses every controller of the call, one behind the other"""
    return _build(tmp_path_factory.mktemp("emu1"), "run_condense_1", ("-DMPCX_CONDENSE_GRID_LDS=1", "-DMPCX_CONDENSE_GRID_BIG=1"))


_hosts = {}


def _family(name):
    if name not in _hosts:
        _hosts[name] = R.host_controllers(name)
    return _hosts[name], R.family(name)


def _check(exe, name, order, big):
    ctrls, fam = _family(name)
    o, gots = _run(exe, ctrls, fam, order)
    assert (o["big"] > 0) == big, (name, o["lds"], o["big"])
    R.check_family(name, gots, " (emulator, %s)" % order)
    for got, c, (ctl, lay, tr) in zip(gots, ctrls, fam):
        assert got["cost_direct"] == int(c.debug_get("flags")[0]) and (not tr["reg"] or got["cost_direct"] == 1)
        # the padding stays as the host lays it out: zeros, and ones behind the rows' step sizes
        for n, mask in R.written(lay).items():
            assert (got[n][~mask] == (1.0 if n == "rho_g" else 0.0)).all(), (name, n)
    return gots


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name", [n for n in R.SHAPE + R.ROWS + R.FEATURES + R.CONDITIONING])
def test_family_against_the_truth(runner, name, order):
    _check(runner, name, order, big=False)


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name,big", [("edge_lds96", False), ("edge_big98", True), ("edge_bytes84", True)])
def test_form_edges_against_the_truth(runner, name, big, order):
    """nz = 96, the last LDS shape with all six accumulators of wavefront 0 in use; the first scratch shape; the scratch form by bytes (each takes
    about a second: both orders)"""
    _check(runner, name, order, big)


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name,big", [("features", False), ("rows_mg17", False), ("cond_regularised", False), ("edge_big98", True)])
def test_one_workgroup_condenses_the_whole_family(runner, runner_one_workgroup, name, big, order):
    """the grid-stride loop: with one workgroup for four controllers every buffer of the kernel -- P, Q, the roll-out's blocks, the step sizes,
    the flags, the scratch block -- is used again behind another controller, and every array has the bits of a workgroup of its own"""
    ctrls, fam = _family(name)
    o1, one = _run(runner_one_workgroup, ctrls, fam, order)
    o4, own = _run(runner, ctrls, fam, order)
    assert (o1["big"] > 0) == big
    for a, b in zip(one, own):
        for n in R.ARRAYS:
            assert np.array_equal(a[n].view(np.uint64), b[n].view(np.uint64)), (name, n)
        assert a["cost_direct"] == b["cost_direct"]
    R.check_family(name, one, " (emulator, one workgroup, %s)" % order)
