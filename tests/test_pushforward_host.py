"""The Python layer of eval_pushforward without a device: how pushforward_directions hands the directions on, what it and the
functional eval_pushforward refuse before the library is touched, and that the library exports the entry point and answers a
NULL handle like every other one (tests/test_host_prologue.py asks that of the entry points of qgd.h)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP = 5


def test_directions_are_handed_on_as_the_library_takes_them(qgd):
    rng = np.random.default_rng(0)
    v = rng.standard_normal(NP)
    cols, single = qgd.pushforward_directions(v, NP)
    assert single and cols.shape == (NP, 1) and cols.dtype == np.float64 and cols.flags.f_contiguous
    assert np.array_equal(cols[:, 0], v)
    V = rng.standard_normal((NP, 3))                      # C-ordered
    cols, single = qgd.pushforward_directions(V, NP)
    assert not single and cols.shape == (NP, 3) and cols.flags.f_contiguous and np.array_equal(cols, V)
    # column-major: direction j is the contiguous run j * n_pcof .. of the buffer the library reads
    assert np.array_equal(np.frombuffer(cols.tobytes(order="A")).reshape(3, NP), V.T)
    cols, single = qgd.pushforward_directions(np.arange(NP), NP)      # integers are converted, not refused
    assert single and cols.dtype == np.float64 and np.array_equal(cols[:, 0], np.arange(NP))
    cols, single = qgd.pushforward_directions([[1], [2], [3], [4], [5]], NP)      # one direction given as a column keeps its axis
    assert not single and cols.shape == (NP, 1)


@pytest.mark.parametrize("v,match", [
    (np.zeros(NP + 1), "shape"),
    (np.zeros((NP + 1, 2)), "shape"),
    (np.zeros((2, NP)), "shape"),                         # directions in rows
    (np.zeros((NP, 2, 1)), "shape"),
    (np.float64(1.0), "shape"),
    (np.zeros((NP, 0)), "no direction"),
    (np.zeros(NP, dtype=complex), "real"),
    (np.zeros(NP, dtype=bool), "real"),
    (np.full(NP, "a"), "real"),
    (np.array([0.0, 1.0, np.nan, 0.0, 0.0]), "finite"),
    (np.array([[0.0, np.inf]] * NP), "finite"),
])
def test_directions_refusals(qgd, v, match):
    with pytest.raises(ValueError, match=match):
        qgd.pushforward_directions(v, NP)


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
    with pytest.raises(ValueError, match="saveEveryNsteps"):
        qgd.eval_pushforward(prob, ctrl, pcof, v, saveEveryNsteps=0)
    with pytest.raises(ValueError, match="output must be"):
        qgd.eval_pushforward(prob, ctrl, pcof, v, output="history")
    with pytest.raises(ValueError, match="observables go with"):
        qgd.eval_pushforward(prob, ctrl, pcof, v, output="expectations")
    with pytest.raises(ValueError, match="observables go with"):
        qgd.eval_pushforward(prob, ctrl, pcof, v, output="states", observables=np.eye(Nn))
    with pytest.raises(ValueError, match="level_map goes with"):
        qgd.eval_pushforward(prob, ctrl, pcof, v, output="states", level_map=np.ones((1, Nn)))
    with pytest.raises(ValueError, match="level_map"):
        qgd.eval_pushforward(prob, ctrl, pcof, v, output="populations", level_map=np.ones((1, Nn + 1)))
    with pytest.raises(ValueError, match="Hermitian"):
        qgd.eval_pushforward(prob, ctrl, pcof, v, output="expectations", observables=np.triu(np.ones((Nn, Nn))))
    with pytest.raises(ValueError, match="shape"):
        qgd.eval_pushforward(prob, ctrl, pcof, v[:-1])
    with pytest.raises(ValueError, match="finite"):
        qgd.eval_pushforward(prob, ctrl, pcof, np.full(len(pcof), np.nan))
    for kw in (dict(), dict(output="populations", level_map=np.ones((2, Nn))), dict(output="expectations", observables=np.eye(Nn))):
        with pytest.raises(AssertionError, match="a handle was asked for"):      # valid arguments get as far as the handle
            qgd.eval_pushforward(prob, ctrl, pcof, v, saveEveryNsteps=3, **kw)


def test_the_entry_point_is_declared_exported_and_refuses_a_null_handle(qgd):
    hdr = open(os.path.join(ROOT, "include", "qgd_pushforward.h")).read()
    assert set(re.findall(r"\b(qgd_[a-z_]+)\s*\(", hdr)) == {"qgd_eval_pushforward"}
    assert '#include "qgd_pushforward.h"' in open(os.path.join(ROOT, "include", "qgd.h")).read()
    unit = open(os.path.join(ROOT, "quantumgatedesign.jl_amd", "csrc", "qgd_host_pushforward.cpp")).read()
    body = re.search(r"^int qgd_eval_pushforward\(.*?\)\s*\{\n(.*?)^\}", unit, re.M | re.S).group(1)
    assert re.search(r"\bENTER\(h\b", body) and "hipSetDevice" not in unit and "stream_dead" not in unit
    lib = qgd._lib.lib()
    fn = lib.qgd_eval_pushforward
    assert len(fn.argtypes) == 14
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    A = qgd._lib.QGD_ERR_ARGUMENT
    assert fn(None, None, 0, 0, None, 0, None, None, None, 0, None, None, None, 0) == A
    assert fn(None, p, 1, 1, p, 1, p, p, p, 1, p, p, p, 1) == A
    assert not any(buf)
    for name in ("eval_pushforward", "pushforward_directions"):
        assert hasattr(qgd, name)


def test_julia_shim_call_matches_the_header():
    """The shim has never run (no Julia in the image): its call of qgd_eval_pushforward is parsed and compared with the prototype
    in include/qgd_pushforward.h, argument by argument, as tests/test_host.py does for the entry points of qgd.h."""
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "qgd_pushforward.h")).read(), flags=re.S)
    ret, args = re.search(r"^\s*(\w+)\s+qgd_eval_pushforward\s*\(([^)]*)\)\s*;", hdr, flags=re.M).groups()
    cargs = [" ".join(a.split()).rsplit(" ", 1)[0].strip() + (" *" if "*" in a else "") for a in args.split(",")]
    cargs = [a.replace("* *", "*") for a in cargs]
    jl = open(os.path.join(ROOT, "julia", "QuantumGateDesignHIP.jl")).read()
    jret, jargs = re.search(r"ccall\(qgd_eval_pushforward_ptr\(\),\s*(\w+),\s*\(((?:[^()]|\{[^}]*\})*)\)", jl, flags=re.S).groups()
    jargs = [a.strip() for a in " ".join(jargs.split()).split(",") if a.strip()]
    table = {"Cint": {"int", "int32_t"}, "Int32": {"int32_t", "int"}, "Ptr{Cvoid}": {"qgd_handle"}, "Ptr{Float64}": {"double *", "const double *"}}
    assert ret == "int" and ret in table[jret]
    assert len(jargs) == len(cargs) == 14, (jargs, cargs)
    for ja, ca in zip(jargs, cargs):
        assert ca in table[ja], (ja, ca)
    assert ":qgd_eval_pushforward)" in jl and "hip_eval_pushforward" in jl
