"""The Python layer of eval_dense_pushforward without a device: what DeviceProblem.eval_dense_pushforward's argument helpers and
the functional form refuse before the library is touched, that the library exports the entry point from a header of its own and
answers a NULL handle like every other one, and that the Julia shim calls it as the header declares it (in the manner of
tests/test_pushforward_host.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qgd_eval_dense_pushforward"


def _header():
    return open(os.path.join(ROOT, "include", "qgd_dense_pushforward.h")).read()


def test_the_entry_point_is_declared_in_a_header_of_its_own(qgd):
    assert set(re.findall(r"\b(qgd_[a-z_]+)\s*\(", _header())) == {NAME}
    qgd_h = open(os.path.join(ROOT, "include", "qgd.h")).read()
    assert qgd_h.count('#include "qgd_dense_pushforward.h"') == 1
    assert NAME not in qgd_h and NAME not in qgd._lib.EXPORTS
    # the grid-point header stays pinned to its one name
    assert set(re.findall(r"\b(qgd_[a-z_]+)\s*\(", open(os.path.join(ROOT, "include", "qgd_pushforward.h")).read())) == {"qgd_eval_pushforward"}


def test_the_body_enters_through_the_prologue():
    unit = open(os.path.join(ROOT, "quantumgatedesign.jl_amd", "csrc", "qgd_host_pushforward.cpp")).read()
    body = re.search(r"^int " + NAME + r"\(.*?\)\s*\{\n(.*?)^\}", unit, re.M | re.S).group(1)
    assert re.search(r"\bENTER\(h\b", body) and "hipSetDevice" not in unit and "stream_dead" not in unit
    # nothing is launched, allocated or read off the handle's grid in front of it
    front = body[:re.search(r"\bENTER\(h\b", body).start()]
    assert not re.search(r"\b(hip[A-Z]\w*|qgdk_\w+|pool_ensure|pushforward)\s*\(", front), front


def test_the_symbol_is_exported_and_refuses_a_null_handle(qgd):
    lib = qgd._lib.lib()
    fn = getattr(lib, NAME)
    assert len(fn.argtypes) == 15
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    A = qgd._lib.QGD_ERR_ARGUMENT
    assert fn(None, None, 0, 0, 0, None, 0, None, None, None, 0, None, None, None, 0) == A
    assert fn(None, p, 1, 1, 2, p, 1, p, p, p, 1, p, p, p, 1) == A
    assert fn(None, p, 1, 0, 0, p, 1, p, None, None, 0, None, None, None, 0) == A
    assert not any(buf)
    assert hasattr(qgd, "eval_dense_pushforward") and hasattr(qgd.DeviceProblem, "eval_dense_pushforward")


def test_the_functional_form_refuses_before_a_handle_is_made(qgd, monkeypatch):
    prob, _ = qgd.cnot2_problem(nsteps=7, tf=7.0)
    ctrl = [qgd.GeneralBSplineControl(2, 6, prob.tf) for _ in range(prob.N_operators)]
    pcof = np.zeros(qgd.get_number_of_control_parameters(ctrl))
    Nn = prob.N_tot_levels
    v = np.ones(len(pcof))

    def no_handle(*a, **k):
        raise AssertionError("a handle was asked for")
    import sys
    monkeypatch.setattr(sys.modules[qgd.__name__ + ".evolution"], "device_problem", no_handle)
    f = qgd.eval_dense_pushforward
    for bad in (0, -1, 2.5, True, "2", None):
        with pytest.raises(ValueError, match="refine"):
            f(prob, ctrl, pcof, v, refine=bad)
    with pytest.raises(ValueError, match="output must be"):
        f(prob, ctrl, pcof, v, output="history")
    with pytest.raises(ValueError, match="observables go with"):
        f(prob, ctrl, pcof, v, output="expectations")
    with pytest.raises(ValueError, match="observables go with"):
        f(prob, ctrl, pcof, v, output="states", observables=np.eye(Nn))
    with pytest.raises(ValueError, match="level_map goes with"):
        f(prob, ctrl, pcof, v, output="states", level_map=np.ones((1, Nn)))
    with pytest.raises(ValueError, match="level_map"):
        f(prob, ctrl, pcof, v, output="populations", level_map=np.ones((1, Nn + 1)))
    with pytest.raises(ValueError, match="Hermitian"):
        f(prob, ctrl, pcof, v, output="expectations", observables=np.triu(np.ones((Nn, Nn))))
    with pytest.raises(ValueError, match="shape"):
        f(prob, ctrl, pcof, v[:-1])
    with pytest.raises(ValueError, match="shape"):
        f(prob, ctrl, pcof, np.ones((2, len(pcof))))
    with pytest.raises(ValueError, match="no direction"):
        f(prob, ctrl, pcof, np.ones((len(pcof), 0)))
    with pytest.raises(ValueError, match="real"):
        f(prob, ctrl, pcof, v.astype(complex))
    with pytest.raises(ValueError, match="finite"):
        f(prob, ctrl, pcof, np.full(len(pcof), np.nan))
    with pytest.raises(ValueError, match="finite"):
        f(prob, ctrl, pcof, np.array([[0.0, np.inf]] * len(pcof)))
    for kw in (dict(), dict(output="populations", level_map=np.ones((2, Nn))), dict(output="expectations", observables=np.eye(Nn)),
               dict(refine=1), dict(refine=3.0)):
        with pytest.raises(AssertionError, match="a handle was asked for"):      # valid arguments get as far as the handle
            f(prob, ctrl, pcof, v, **kw)


class _NoLibrary:
    """stands where the handle's library would: any call is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError(f"the library was called: {name}")


def test_the_method_refuses_before_the_library_is_called(qgd):
    """DeviceProblem.eval_dense_pushforward on an object that has no handle: its checks come first"""
    dp = object.__new__(qgd.DeviceProblem)
    dp.N, dp.c, dp.nsteps, dp.n_pcof, dp.h, dp.lib = 4, 4, 7, 5, None, _NoLibrary()
    v = np.ones(5)
    m = dp.eval_dense_pushforward
    with pytest.raises(ValueError, match="refine"):
        m(0, None, v, states=True)
    with pytest.raises(ValueError, match="shape"):
        m(2, None, np.ones(6), states=True)
    with pytest.raises(ValueError, match="finite"):
        m(2, None, np.array([0.0, np.nan, 0.0, 0.0, 0.0]), states=True)
    with pytest.raises(ValueError, match="at least one of"):
        m(2, None, v)
    with pytest.raises(ValueError, match="level_map"):
        m(2, None, v, level_map=np.ones((2, 5)))
    with pytest.raises(ValueError, match="Hermitian"):
        m(2, None, v, observables=np.triu(np.ones((4, 4))))


def test_julia_shim_call_matches_the_header():
    """The shim has never run (no Julia in the image): its call of the entry point is parsed and compared with the prototype in
    include/qgd_dense_pushforward.h, argument by argument."""
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    ret, args = re.search(r"^\s*(\w+)\s+" + NAME + r"\s*\(([^)]*)\)\s*;", hdr, flags=re.M).groups()
    cargs = [" ".join(a.split()).rsplit(" ", 1)[0].strip() + (" *" if "*" in a else "") for a in args.split(",")]
    cargs = [a.replace("* *", "*") for a in cargs]
    jl = open(os.path.join(ROOT, "julia", "QuantumGateDesignHIP.jl")).read()
    jret, jargs = re.search(r"ccall\(qgd_eval_dense_pushforward_ptr\(\),\s*(\w+),\s*\(((?:[^()]|\{[^}]*\})*)\)", jl, flags=re.S).groups()
    jargs = [a.strip() for a in " ".join(jargs.split()).split(",") if a.strip()]
    table = {"Cint": {"int", "int32_t"}, "Int32": {"int32_t", "int"}, "Ptr{Cvoid}": {"qgd_handle"}, "Ptr{Float64}": {"double *", "const double *"}}
    assert ret == "int" and ret in table[jret]
    assert len(jargs) == len(cargs) == 15, (jargs, cargs)
    for ja, ca in zip(jargs, cargs):
        assert ca in table[ja], (ja, ca)
    assert ":" + NAME + ")" in jl and "function hip_eval_dense_pushforward" in jl
    assert "(:" + NAME + ", libqgd)" not in jl      # (tests/test_host.py: those calls are the entry points of qgd.h)
