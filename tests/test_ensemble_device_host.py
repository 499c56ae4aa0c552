"""The device route of ensemble evaluation (include/qgd_ensemble.h, DeviceProblem.set_ensemble / eval_ensemble, ``route=``;
DESIGN.md section 4m) without a device: the two entry points are declared, exported and bound with the header's argument
counts, refuse a NULL handle like every other entry point, the Python layer refuses an unknown route before a handle is asked
for, EnsembleResult keeps its five positional arguments, and the arrays set_ensemble uploads are member_problem's operators."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qgd_set_ensemble", "qgd_eval_ensemble")


def _prototypes():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "qgd_ensemble.h")).read(), flags=re.S)
    return {name: [a for a in args.split(",") if a.strip()]
            for name, args in re.findall(r"^\s*int\s+(qgd_[a-z_]+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)}


def test_the_entry_points_are_declared_exported_and_bound_as_declared(qgd):
    protos = _prototypes()
    assert set(protos) == set(NAMES)
    qgd_h = open(os.path.join(ROOT, "include", "qgd.h")).read()
    assert '#include "qgd_ensemble.h"' in qgd_h
    assert not any(n in qgd_h for n in NAMES) and not any(n in qgd._lib.EXPORTS for n in NAMES)      # (those two lists are pinned elsewhere)
    lib = qgd._lib.lib()
    for name in NAMES:
        fn = getattr(lib, name)                                        # exported: ctypes raises AttributeError otherwise
        assert len(fn.argtypes) == len(protos[name]), name
    assert len(lib.qgd_set_ensemble.argtypes) == 7 and len(lib.qgd_eval_ensemble.argtypes) == 9
    unit = open(os.path.join(ROOT, "quantumgatedesign.jl_amd", "csrc", "qgd_host_ensemble.cpp")).read()
    for name in NAMES:
        body = re.search(r"^int " + name + r"\(.*?\)\s*\{\n(.*?)^\}", unit, re.M | re.S).group(1)
        assert re.search(r"\bENTER\(h\b", body), name
    assert "hipSetDevice" not in unit and "stream_dead" not in unit


def test_both_refuse_a_null_handle(qgd):
    lib = qgd._lib.lib()
    A = qgd._lib.QGD_ERR_ARGUMENT
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.qgd_set_ensemble(None, 0, None, None, None, None, None) == A
    assert lib.qgd_set_ensemble(None, 2, p, p, p, p, p) == A
    assert lib.qgd_set_ensemble(None, -1, p, p, p, p, p) == A
    assert lib.qgd_eval_ensemble(None, None, 0, 0, None, None, None, None, None) == A
    assert lib.qgd_eval_ensemble(None, p, 3, 1, p, p, p, p, p) == A
    assert lib.qgd_eval_ensemble(None, p, 3, 0, None, p, None, None, None) == A
    assert not any(buf)


def _cnot2_ensemble(qgd, K=3, scale=True):
    prob, target = qgd.cnot2_problem(nsteps=7, tf=7.0)
    rng = np.random.default_rng(5)
    N = prob.N_tot_levels
    r = 0.1 * rng.standard_normal((K, N, N))
    ens = qgd.Ensemble(prob.system_sym[None] + (r + r.transpose(0, 2, 1)), prob.system_asym[None] + (r - r.transpose(0, 2, 1)),
                       1.0 + 0.05 * rng.standard_normal((K, prob.N_operators)) if scale else None, [0.2, 0.5, 0.3][:K])
    return prob, target, ens


def test_route_is_checked_before_a_handle_is_asked_for(qgd, monkeypatch):
    prob, target, ens = _cnot2_ensemble(qgd)
    ctrl = [qgd.GeneralBSplineControl(2, 6, prob.tf) for _ in range(prob.N_operators)]
    pcof = np.zeros(qgd.get_number_of_control_parameters(ctrl))

    def no_handle(*a, **k):
        raise AssertionError("a handle was asked for")
    monkeypatch.setattr(sys.modules[qgd.__name__ + ".evolution"], "device_problem", no_handle)
    for bad in ("host", "Device", None, 1, ""):
        with pytest.raises(ValueError, match="route must be"):
            qgd.eval_ensemble(prob, ctrl, pcof, target, ens, route=bad)
        with pytest.raises(ValueError, match="route must be"):
            qgd.discrete_adjoint_ensemble(prob, ctrl, pcof, target, ens, route=bad)
        with pytest.raises(ValueError, match="route must be"):
            qgd.EnsembleObjective(prob, ctrl, target, ens, 2, "Infidelity", route=bad)
    # the refusals that needed no device before still come first, on every route
    for route in ("auto", "device", "loop"):
        with pytest.raises(ValueError, match="pcof must have shape"):
            qgd.eval_ensemble(prob, ctrl, pcof[:-1], target, ens, route=route)
        with pytest.raises(ValueError, match="target"):
            qgd.discrete_adjoint_ensemble(prob, ctrl, pcof, None, ens, route=route)
        with pytest.raises(AssertionError, match="a handle was asked for"):      # valid arguments get as far as the handle
            qgd.eval_ensemble(prob, ctrl, pcof, target, ens, route=route)
    assert qgd.EnsembleObjective(prob, ctrl, target, ens, 2, "Infidelity").route == "auto"


def test_ensemble_result_keeps_its_positional_arguments(qgd):
    g, mg, mo = np.ones(3), np.ones((2, 3)), np.ones((2, 3))
    r = qgd.EnsembleResult(g, 0.5, 0.25, mg, mo)
    assert r.route == "loop" and tuple(r) == (g, 0.5, 0.25) and r.member_grads is mg and r.member_out3 is mo
    assert qgd.EnsembleResult(g, 0.5, 0.25, None, None, route="device").route == "device"
    with pytest.raises(TypeError):
        qgd.EnsembleResult(g, 0.5, 0.25, mg, mo, "device")              # (the new field is keyword-only)


@pytest.mark.parametrize("scale", [True, False])
def test_the_uploaded_arrays_are_the_operators_of_member_problem(qgd, scale):
    prob, _, ens = _cnot2_ensemble(qgd, scale=scale)
    ss, sa, so, ao, w = ens.device_arrays(prob)
    K, N, n_ops = ens.K, prob.N_tot_levels, prob.N_operators
    assert ss.shape == sa.shape == (K, N, N) and so.shape == ao.shape == (K, n_ops, N, N) and w.shape == (K,)
    for a in (ss, sa, so, ao, w):
        assert a.dtype == np.float64 and a.flags.c_contiguous
    assert np.array_equal(w, ens.effective_weights())
    for k in range(K):
        mp = ens.member_problem(prob, k)
        # every matrix is stored transposed: the column-major bytes the library reads, as for qgd_create
        assert ss[k].tobytes() == np.asfortranarray(mp.system_sym, dtype=np.float64).tobytes(order="F")
        assert sa[k].tobytes() == np.asfortranarray(mp.system_asym, dtype=np.float64).tobytes(order="F")
        for o in range(n_ops):
            assert np.array_equal(so[k, o].T, mp.sym_operators[o]) and np.array_equal(ao[k, o].T, mp.asym_operators[o])
            assert so[k, o].tobytes() == np.asfortranarray(mp.sym_operators[o], dtype=np.float64).tobytes(order="F")
    assert np.array_equal(qgd.Ensemble(ens.system_sym, ens.system_asym).device_arrays(prob)[4], np.full(K, 1.0 / K))
    with pytest.raises(ValueError, match="op_scale"):
        qgd.Ensemble(ens.system_sym, ens.system_asym, np.ones((K, n_ops + 1))).operator_arrays(prob.sym_operators, prob.asym_operators)
