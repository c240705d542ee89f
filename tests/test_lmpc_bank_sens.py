"""Sensitivities of a solved batch of a bank on the host: the numpy restatement of the kernel's formula, which reads no composed
map, against sens_ref.condensed_jacobian (which does: this settles the signs) and against the KKT system of each instance's own reference QP on
every family of the GPU tests -- the figure the kernel's tolerance derives from --, the share of usable instances, and the C ABI and the Python
front-ends where they can be reached without a device."""
import ctypes as C
import functools

import numpy as np
import pytest

import bank_sens_ref as BR
import sens_ref as S


@functools.lru_cache(maxsize=None)
def arrays(name):
    from libmpc_amd import LMPC
    return [BR.arrays(BR.configure(LMPC(*sp["dims"], device=-1), sp)) for sp in BR.reference(name)["specs"]]


def test_families_share_their_structure_and_differ_in_their_data():
    for name in BR.FAMILIES:
        arrs = arrays(name)
        assert len(arrs) == (4 if name == "smallest" else 8)
        a0 = arrs[0]
        for a in arrs[1:]:
            for k in ("nz", "mg", "ldz", "ldg", "ldy"):
                assert a[k] == a0[k], (name, k)
            for k in ("g_kind", "g_step", "g_comp", "g_refrow", "boxrow_ptr", "boxrow_ref", "blk"):
                assert np.array_equal(a[k], a0[k]), (name, k)
            assert np.array_equal(a["g_soft"] > 0, a0["g_soft"] > 0) and (a["terminal"] is None) == (a0["terminal"] is None)
            assert not np.array_equal(a["Y"], a0["Y"]) and not np.array_equal(a["A"], a0["A"])
        R = BR.reference(name)
        assert sorted(np.bincount(R["model"])) == [BR.PER_CONTROLLER] * len(arrs) and not np.array_equal(R["model"], np.sort(R["model"]))


@pytest.mark.parametrize("name", BR.FAMILIES)
def test_restatement_agrees_with_the_condensed_formula(name):
    """the same Jacobian from MF1 (4.8) and from the roll-out: the signs, and the d_u0 / d_yref terms.  Rounding apart they are one number, so
    the bound is the restatement's own against the truth"""
    R = BR.reference(name)
    worst = 0.0
    for b, k in enumerate(R["model"]):
        a = arrays(name)[k]
        J = BR.rollout_jacobian(a, R["active_lower"][b], R["active_upper"][b])
        Jc = S.condensed_jacobian(a, R["active_lower"][b], R["active_upper"][b])
        assert J["dependent"] == Jc["dependent"] and J["n"] == Jc["n"]
        if not Jc["dependent"]:
            worst = max(worst, BR.error(J["input"], Jc["input"]))
    print(f"{name}: roll-out against the composed map {worst:.2e}")
    assert worst <= BR.BANK_RESTATEMENT_WORST


@pytest.mark.parametrize("name", BR.FAMILIES)
def test_restatement_agrees_with_the_kkt_system(name):
    R = BR.reference(name)
    use = [b for b in range(len(R["model"])) if R["jac"][b] is not None]
    print(f"{name}: {len(use)} of {len(R['model'])} instances usable")
    assert len(use) >= (1.0 - BR.SKIP_CAP) * len(R["model"])
    worst = 0.0
    for b in use:
        J = BR.rollout_jacobian(arrays(name)[R["model"][b]], R["active_lower"][b], R["active_upper"][b])
        assert not J["dependent"]
        worst = max(worst, BR.error(J["cmd"], R["jac"][b]["cmd"]), BR.error(J["input"], R["jac"][b]["input"]))
    print(f"{name}: worst error of the restatement {worst:.2e} (committed {BR.BANK_RESTATEMENT_WORST:.2e})")
    assert worst <= BR.BANK_RESTATEMENT_WORST


def test_tolerance_is_the_restatements():
    assert BR.BANK_KERNEL_TOL == max(8.0 * BR.BANK_RESTATEMENT_WORST, 1e-12) and BR.SKIP_CAP == S.SKIP_CAP == 0.10


def test_a_parallel_pair_is_reported_dependent():
    R = BR.reference("full")
    a = arrays("full")[0]
    d = R["pbs"][0].d
    al = np.zeros(R["active_lower"].shape[1], bool); au = al.copy()
    al[d.neq + d.na + a["nx"]] = True; au[d.neq + d.off_du] = True            # box row and step-0 rate row of input 0
    J = BR.rollout_jacobian(a, al, au)
    assert J["dependent"] and J["n"] == 2 and np.isnan(J["cmd"]).all()


def test_abi_symbol_and_argument_errors():
    from libmpc_amd import _capi
    assert "mpcx_lmpc_hetero_sensitivity_batch" in _capi.EXPORTS
    lib = _capi.lib()
    f = lib.mpcx_lmpc_hetero_sensitivity_batch
    d = _capi.Sens()
    d.batch = 2
    assert f(None, C.byref(d), None, None) == _capi.E_INVALID and "null bank" in lib.mpcx_last_error().decode()
    assert lib.mpcx_lmpc_sens_size() == C.sizeof(_capi.Sens)                  # the descriptor is the single-controller one, unchanged


def test_without_a_device_the_front_ends_raise():
    """LMPCHetero's new methods and lmpc_cmd on a bank refuse as every device call does; run on an object that has only the dimensions"""
    import libmpc_amd
    from libmpc_amd import LMPCHetero, MpcxError
    het = LMPCHetero.__new__(LMPCHetero)
    het.nx, het.nu, het.ny, het.ndu, het.ph, het.device, het._h, het.count, het.active_words, het.m_ref = 3, 2, 2, 0, 6, -1, None, 4, 2, 40
    al = np.zeros((4, 2), np.int32)
    for call in (lambda: het.sensitivityBatch(al, al), lambda: het.make_sensitivity(al, al, model=np.arange(4)),
                 lambda: het.optimizeBatch(np.zeros((4, 3)), np.zeros((4, 2)), sensitivities=True),
                 lambda: libmpc_amd.lmpc_cmd(het, np.zeros((4, 3)), np.zeros((4, 2)), model=np.arange(4))):
        with pytest.raises(MpcxError) as e:
            call()
        assert e.value.code == libmpc_amd._capi.E_DEVICE
    from libmpc_amd import LMPC
    with pytest.raises((ValueError, MpcxError)):                            # model= belongs to a bank
        libmpc_amd.lmpc_cmd(LMPC(3, 2, 0, 2, 6, 6, device=-1), np.zeros((4, 3)), np.zeros((4, 2)), model=np.arange(4))
