"""CPU tests of the host side: B-splines against the reference's own Fortran (golden
fixture generated from oracle/_ref), controls, problem constructors, validation, and that
the C-ABI library loads and exports every symbol include/qgd.h declares."""
import ctypes as C
import math
import os
import sys
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "bspline_bsplvd.npz"))


def test_bspline_oracle_vs_reference_fortran_golden(orc):
    """oracle de Boor evaluation == pppack bsplvd_ output (fixture from the compiled reference)."""
    for deg, nb, x, nd, val in zip(GOLD["degree"], GOLD["n_basis"], GOLD["x"], GOLD["nderiv"], GOLD["values"]):
        k = deg + 1
        first, out = orc.bspline_basis_derivs(int(deg), int(nb), float(x), int(nd))
        ref = val[:k, :nd].T                       # [d, i]
        scale = np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))
        assert np.abs(out - ref).max() <= 1e-12 * scale.max(), (deg, nb, x)
        assert np.all(np.abs(out - ref) <= 2e-13 * scale), (deg, nb, x)


def test_bspline_host_vs_reference_fortran_golden(qgd):
    """the package's numpy B-spline basis == pppack bsplvd_ output."""
    for deg, nb, x, left, nd, val in zip(GOLD["degree"], GOLD["n_basis"], GOLD["x"], GOLD["left"], GOLD["nderiv"], GOLD["values"]):
        k = deg + 1
        B = qgd.bspline_basis_derivatives(int(deg), int(nb), np.array([x]), int(nd) - 1)[0]   # [d, n_basis]
        first = int(left) - k
        ref = val[:k, :nd].T
        got = B[:, first:first + k]
        scale = np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))
        assert np.all(np.abs(got - ref) <= 1e-11 * scale), (deg, nb, x)
        mask = np.ones(nb, bool); mask[first:first + k] = False
        assert not mask.any() or np.abs(B[:, mask]).max() == 0.0


def test_bspline_oracle_vs_live_reference_fortran(orc):
    """Same check against the compiled reference routine at further random points (seed 9, all k derivatives).  Where
    oracle/_ref is built the routine is called live, and must also reproduce the stored fixture
    tests/golden/bspline_bsplvd_live.npz (made by tests/golden/make_bspline_golden.py); elsewhere the fixture stands in."""
    so = os.path.join(ROOT, "oracle", "_ref", "bspline_lib.so")
    lib = C.CDLL(so) if os.path.exists(so) else None
    live = np.load(os.path.join(ROOT, "tests", "golden", "bspline_bsplvd_live.npz"))
    rng = np.random.default_rng(9)
    i = 0
    for deg, nb in [(2, 10), (4, 9), (16, 20)]:
        k = deg + 1; nk = nb + k; nd = nk - 2 * (k - 1)
        knots = np.concatenate([np.zeros(k - 1), np.linspace(0, 1, nd), np.ones(k - 1)])
        for x in rng.random(20):
            left = min(int(np.floor(x * (nd - 1) + k)), nk - k)
            assert (live["degree"][i], live["n_basis"][i], live["x"][i], live["left"][i]) == (deg, nb, x, left), i
            stored = live["values"][i][:k, :k]
            i += 1
            out = stored
            if lib is not None:
                a = np.zeros((k, k), order="F"); out = np.zeros((k, k), order="F")
                i64 = lambda v: C.byref(C.c_int64(v))
                lib.bsplvd_(knots.ctypes.data_as(C.c_void_p), i64(k), C.byref(C.c_double(x)), i64(left),
                            a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), i64(k))
                assert np.all(np.abs(stored - out) <= 1e-14 * np.maximum(1.0, np.abs(out).max(axis=0, keepdims=True)))
            _, got = orc.bspline_basis_derivs(deg, nb, float(x), k)
            scale = np.maximum(1.0, np.abs(out.T).max(axis=1, keepdims=True))
            assert np.all(np.abs(got - out.T) <= 1e-12 * scale)
    assert i == len(live["x"])


def _controls(qgd):
    tf = 3.0
    return [qgd.GRAPEControl(5, tf), qgd.FortranBSplineControl(2, 10, tf), qgd.GeneralBSplineControl(3, 7, tf),
            qgd.FortranBSplineControl(16, 20, tf),
            qgd.CarrierControl(qgd.FortranBSplineControl(4, 8, tf), [-2.0, 0.0, 1.5])]


def test_controls_host_vs_oracle(qgd, orc):
    """fill_p_vec!/fill_q_vec! tables and eval_grad_*_derivative! of the package == oracle."""
    rng = np.random.default_rng(11)
    for ctrl in _controls(qgd):
        pcof = rng.standard_normal(ctrl.N_coeff)
        for t in np.concatenate([[0.0, ctrl.tf, ctrl.tf / 2], rng.random(5) * ctrl.tf]):
            for q in (False, True):
                ref = orc.fill_p_vec(ctrl, float(t), pcof, 6, q=q)
                got = np.zeros(6)
                (ctrl.fill_q_vec if q else ctrl.fill_p_vec)(got, t, pcof)
                assert np.abs(got - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max()), (type(ctrl).__name__, t, q)
                for d in range(4):
                    gref = orc.eval_grad_derivative(ctrl, float(t), pcof, d, q=q)
                    ggot = (ctrl.eval_grad_q_derivative if q else ctrl.eval_grad_p_derivative)(t, pcof, d)
                    assert np.abs(ggot - gref).max() <= 1e-11 * max(1.0, np.abs(gref).max())


def test_control_derivatives_vs_finite_differences(qgd):
    """test/ControlFunctionTests/test_control_derivatives.jl:26-27,90: >=95% of sample times
    within 50*(1e-15)^(2/3) of a central difference of the next-lower derivative."""
    rng = np.random.default_rng(12)
    tol = 50 * (1e-15) ** (2 / 3)
    h = 1e-5
    for ctrl in _controls(qgd)[1:]:
        pcof = rng.standard_normal(ctrl.N_coeff)
        ts = 0.05 * ctrl.tf + 0.9 * ctrl.tf * rng.random(200)
        for d in range(1, 3):
            ok = 0
            for t in ts:
                fd = (ctrl.eval_p_derivative(t + h, pcof, d - 1) - ctrl.eval_p_derivative(t - h, pcof, d - 1)) / (2 * h)
                an = ctrl.eval_p_derivative(t, pcof, d)
                ok += abs(fd - an) <= tol * max(1.0, abs(an)) * 1e3
            assert ok >= 0.95 * len(ts), (type(ctrl).__name__, d, ok)


def test_control_basis_is_table(qgd):
    """G @ pcof reproduces fill_p_mat!/fill_q_mat! (Control.jl:125-149) on the stepper's grid."""
    rng = np.random.default_rng(13)
    ctrls = _controls(qgd)[:3]
    nsteps, tf, m = 12, 3.0, 3
    pcof = rng.standard_normal(qgd.get_number_of_control_parameters(ctrls))
    Gp, Gq, off = qgd.control_basis(ctrls, nsteps, tf, m)
    for n in (0, 5, 12):
        t = n * (tf / nsteps)
        pm = qgd.fill_p_mat(np.zeros((m + 1, 3)), ctrls, t, pcof)
        qm = qgd.fill_q_mat(np.zeros((m + 1, 3)), ctrls, t, pcof)
        for k, c in enumerate(ctrls):
            sl = pcof[off[k]:off[k] + c.N_coeff]
            assert np.abs(Gp[k][n] @ sl - pm[:, k]).max() < 1e-12
            assert np.abs(Gq[k][n] @ sl - qm[:, k]).max() < 1e-12


def test_guard_projector_doc_examples(qgd):
    """multi_qudit_systems.jl:291-314."""
    g = qgd.guard_projector([3], [2])
    assert np.array_equal(np.diag(g), [0, 0, 1, 0, 0, 1]) and np.count_nonzero(g) == 2
    g = qgd.guard_projector([2, 2], [2, 1])
    assert np.array_equal(np.diag(g), [0, 0, 1, 1, 0, 0, 1, 1]) and np.count_nonzero(g) == 4


def test_dispersive_problem_structure(qgd):
    prob, target = qgd.cnot3_problem(nsteps=10, tf=10.0)
    assert (prob.N_tot_levels, prob.N_initial_conditions, prob.N_operators, prob.N_ess_levels) == (64, 8, 3, 8)
    # initial conditions: essential basis states in bit-string order, last subsystem fastest
    idx = [np.argmax(prob.u0[:, c]) for c in range(8)]
    assert idx == [a * 16 + b * 4 + s for a in (0, 1) for b in (0, 1) for s in (0, 1)]
    # system Hamiltonian is real diagonal in the rotating frame; operators are a +- a'
    assert np.count_nonzero(prob.system_asym) == 0
    assert np.count_nonzero(prob.system_sym - np.diag(np.diag(prob.system_sym))) == 0
    a = qgd.lowering_operators_system((4, 4, 4))[1]
    assert np.array_equal(prob.sym_operators[1], a + a.T) and np.array_equal(prob.asym_operators[1], a - a.T)
    # CNOT on (a,b): |1 0 s> <-> |1 1 s>
    t = np.real(target)
    col = {(a, b, s): a * 4 + b * 2 + s for a in (0, 1) for b in (0, 1) for s in (0, 1)}
    row = lambda a, b, s: a * 16 + b * 4 + s
    assert t[row(1, 1, 0), col[(1, 0, 0)]] == 1 and t[row(1, 0, 1), col[(1, 1, 1)]] == 1
    assert t[row(0, 1, 1), col[(0, 1, 1)]] == 1
    assert np.allclose(t.T @ t, np.eye(8))
    # guard projector kills essential levels only
    W = prob.guard_subspace_projector
    assert np.trace(W) == 2 * (64 - 8)


def test_schrodinger_prob_validation(qgd):
    """Constructor checks of SchrodingerProb.jl:73-154 (ArgumentError -> ValueError)."""
    S = np.array([[1.0, 2.0], [2.0, 0.0]]); K = np.array([[0.0, 1.0], [-1.0, 0.0]]); Z = np.zeros((2, 2))
    ok = qgd.SchrodingerProb(S, K, [S], [K], np.eye(2), Z, None, 1.0, 10, 2)
    assert ok.real_system_size == 4 and ok.guard_subspace_projector.shape == (4, 4)
    with pytest.raises(ValueError, match="not symmetric"):
        qgd.SchrodingerProb(K, K, [S], [K], np.eye(2), Z, None, 1.0, 10, 2)
    with pytest.raises(ValueError, match="not anti-symmetric"):
        qgd.SchrodingerProb(S, S, [S], [K], np.eye(2), Z, None, 1.0, 10, 2)
    with pytest.raises(ValueError, match="Anti-symmetric operator 1"):
        qgd.SchrodingerProb(S, K, [S], [S], np.eye(2), Z, None, 1.0, 10, 2)
    with pytest.raises(ValueError, match="essential levels"):
        qgd.SchrodingerProb(S, K, [S], [K], np.eye(2), Z, None, 1.0, 10, 3)
    with pytest.raises(ValueError, match="Guard subspace projector size"):
        qgd.SchrodingerProb(S, K, [S], [K], np.eye(2), Z, np.zeros((2, 2)), 1.0, 10, 2)
    with pytest.raises(ValueError, match="Hermitian"):
        qgd.SchrodingerProb.from_hamiltonian(np.array([[0, 1], [2, 0]]), [S], [K], np.eye(2), 1.0, 10, 2)


def test_c_abi_exports_match_header(qgd):
    """libqgd_hip.so loads without a GPU and exports every function include/qgd.h declares."""
    hdr = open(os.path.join(ROOT, "include", "qgd.h")).read()
    declared = set(re.findall(r"\b(qgd_[a-z_]+)\s*\(", hdr))
    assert declared == set(qgd._lib.EXPORTS), declared ^ set(qgd._lib.EXPORTS)
    lib = qgd._lib.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.qgd_abi_version() == 2


def test_no_silent_cpu_fallback(qgd):
    """Without a GPU the compute entry points fail loudly (QGD_ERR_NO_DEVICE); on a GPU box this
    test only checks the argument validation of qgd_create."""
    import torch
    prob, _ = qgd.cnot2_problem(nsteps=4, tf=4.0)
    if torch.cuda.device_count() == 0:
        with pytest.raises(qgd._lib.QGDError) as ei:
            qgd.DeviceProblem(prob, 4)
        assert ei.value.code == qgd._lib.QGD_ERR_NO_DEVICE
    with pytest.raises(qgd._lib.QGDError) as ei:
        qgd.DeviceProblem(prob, 3)          # odd order: ArgumentError before any device work
    assert ei.value.code == qgd._lib.QGD_ERR_ARGUMENT


def test_c_consumer_compiles_against_the_header(tmp_path):
    """tests/c_consumer/rabi_consumer.c is C99 compiled with -Wall -Wextra -Werror against include/qgd.h and linked to
    libqgd_hip.so.  Without a GPU it must get as far as the SchrodingerProb validation (which needs no device) and
    then stop with the library's no-device error (exit code 3) -- never compute on the CPU."""
    import subprocess
    import torch
    from test_gpu_boundary import build_c_consumer
    exe = build_c_consumer(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if torch.cuda.device_count() == 0:
        assert res.returncode == 3, res.stdout + res.stderr
        assert "no HIP device" in res.stderr
    else:
        assert res.returncode == 0 and "C_CONSUMER_OK" in res.stdout, res.stdout + res.stderr


def test_bench_refuses_more_gpus_than_visible():
    """`python bench.py --gpus N` started bare must launch N ranks or fail loudly -- never print a 1-GPU number."""
    import subprocess
    import torch
    n = torch.cuda.device_count() + 1 if torch.cuda.device_count() else 2
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n)], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode != 0 and "refusing" in res.stderr and "metric" not in res.stdout


def test_oracle_is_not_imported_by_the_package(qgd):
    """The product must not reach the oracle (tier rule 3)."""
    pkg = os.path.join(ROOT, "quantumgatedesign.jl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("# oracle-free", ""), os.path.join(dirpath, f)


def test_richardson_and_history_io(qgd, tmp_path):
    """Richardson extrapolation (src/Tests/test_convergence.jl:233-250) on a manufactured error model,
    and the npz round trips of the convergence dictionaries and of OptimizationHistory
    (src/ipopt_optimal_control.jl:74-104)."""
    exact = np.linspace(1.0, 2.0, 7)
    err = np.cos(np.arange(7))
    order, h = 4, 0.1
    A_2h = exact + err * (2 * h) ** order
    A_h = exact + err * h ** order
    assert np.allclose(qgd.richardson_extrap_sol(A_h, A_2h, order), exact, atol=1e-15)
    est = qgd.richardson_extrap_rel_err(A_h, A_2h, order)
    assert abs(est - np.linalg.norm(A_h - exact) / np.linalg.norm(exact)) < 1e-12
    ret = {"Order 4 (QGD)": dict(order=4, nsteps=[10, 20], step_sizes=[0.1, 0.05], elapsed_times=[1.0, 2.0],
                                 histories=[np.ones((2, 3, 1), complex), 2j * np.ones((2, 3, 1))],
                                 richardson_errors=[float("nan"), 1e-3])}
    qgd.save_histories(ret, tmp_path / "conv.npz")
    back = qgd.load_histories(tmp_path / "conv.npz")
    assert back["Order 4 (QGD)"]["nsteps"] == [10, 20]
    assert np.array_equal(back["Order 4 (QGD)"]["histories"][1], ret["Order 4 (QGD)"]["histories"][1])
    h = qgd.OptimizationHistory()
    for i in range(3):
        h.iter_count.append(i); h.ipopt_obj_value.append(1.0 / (i + 1)); h.wall_time.append(0.1 * i)
        h.pcof.append(np.full(4, i, float)); h.grad_pcof.append(np.full(4, -i, float))
        h.analytic_obj_value.append(1.0 / (i + 1)); h.infidelity.append(0.5 / (i + 1))
        h.guard_penalty.append(0.0); h.ridge_penalty.append(0.01 * i)
    h.write(tmp_path / "opt.npz")
    g = qgd.read_optimization_history(tmp_path / "opt.npz")
    assert len(g) == 3 and np.array_equal(g.pcof[2], h.pcof[2]) and g.infidelity == h.infidelity


def test_jld2_files(qgd, tmp_path):
    """the result files in the reference's format.  ``.jld2`` names go through libhdf5 (jld2io): a
    valid HDF5 file of the 1.8 generation (superblock 2) behind the 512-byte JLD2 user block, the nine keys of
    write(obj::OptimizationHistory, filename) (src/ipopt_optimal_control.jl:74-86) with the HDF5 types JLD2 gives
    Vector{Int64}, Vector{Float64} and Vector{Vector{Float64}} (object references), the Setup group of :223-241, complex
    matrices as {re, im} compounds with Julia's (column-major) dimension order -- checked with h5dump where the image
    has it, and read back."""
    import shutil
    import subprocess
    jl = qgd.jld2io
    if not jl.available():
        pytest.skip("no libhdf5 in this image")
    h = qgd.OptimizationHistory()
    for i in range(3):
        h.iter_count.append(i); h.ipopt_obj_value.append(1.0 / (i + 1)); h.wall_time.append(0.1 * i)
        h.pcof.append(np.full(4, i, float)); h.grad_pcof.append(np.full(4, -i, float))
        h.analytic_obj_value.append(1.0 / (i + 1)); h.infidelity.append(0.5 / (i + 1))
        h.guard_penalty.append(0.0); h.ridge_penalty.append(0.01 * i)
    target = np.arange(6).reshape(3, 2) * (1 + 0.5j)
    f = tmp_path / "opt.jld2"
    h.write(f, dict(order=8, ridge_penalty_strength=1e-2, target=target, note="swap gate"))
    raw = open(f, "rb").read(600)
    assert raw.startswith(b"HDF5-based Julia Data Format, version ") and raw[512:520] == b"\x89HDF\r\n\x1a\n" and raw[520] == 2
    g = qgd.read_optimization_history(f)
    assert g.iter_count == [0, 1, 2] and g.infidelity == h.infidelity and np.array_equal(g.grad_pcof[2], h.grad_pcof[2])
    d = jl.load(f)
    assert d["Setup"]["order"] == 8 and d["Setup"]["note"] == "swap gate" and np.array_equal(d["Setup"]["target"], target)
    dump = shutil.which("h5dump") or "/opt/conda/bin/h5dump"
    if os.path.exists(dump):
        txt = subprocess.run([dump, "-H", str(f)], capture_output=True, text=True, check=True).stdout
        one = " ".join(txt.split())
        assert 'DATASET "iter_count" { DATATYPE H5T_STD_I64LE DATASPACE SIMPLE { ( 3 ) / ( 3 ) }' in one
        assert 'DATASET "pcof" { DATATYPE H5T_REFERENCE { H5T_STD_REF_OBJECT } DATASPACE SIMPLE { ( 3 ) / ( 3 ) }' in one
        # a 3 x 2 Julia matrix: HDF5 dimensions reversed
        assert 'DATASET "target" { DATATYPE H5T_COMPOUND { H5T_IEEE_F64LE "re"; H5T_IEEE_F64LE "im"; } DATASPACE SIMPLE { ( 2, 3 )' in one
    # the convergence dictionaries (src/Tests/test_convergence.jl:60-81)
    ret = {"Order 4 (QGD)": dict(order=4, nsteps=[10, 20], step_sizes=[0.1, 0.05], elapsed_times=[1.0, 2.0],
                                 histories=[np.random.default_rng(0).random((4, 3, 5, 2)), np.ones((4, 3, 5, 2))],
                                 richardson_errors=[float("nan"), 1e-3])}
    qgd.save_histories(ret, tmp_path / "conv.jld2")
    back = qgd.load_histories(tmp_path / "conv.jld2")["Order 4 (QGD)"]
    assert back["nsteps"] == [10, 20] and back["order"] == 4 and np.isnan(back["richardson_errors"][0])
    assert np.array_equal(back["histories"][0], ret["Order 4 (QGD)"]["histories"][0])
    with pytest.raises(TypeError):
        jl.save(tmp_path / "bad.jld2", dict(x=None))


def _quad_piece_sum(D1, tf, coeffs, t):
    """bspline2 (src/Controls/bspline_control.jl:139-165), restated term by term for one time."""
    dtknot = tf / (D1 - 2); width = 3 * dtknot
    tc = dtknot * (np.arange(1, D1 + 1) - 1.5)
    k = min(max(3, int(np.ceil(t / dtknot + 2))), D1)
    tau = lambda kk: (t - tc[kk - 1]) / width
    return (coeffs[k - 1] * (9 / 8 + 4.5 * tau(k) + 4.5 * tau(k) ** 2) + coeffs[k - 2] * (0.75 - 9 * tau(k - 1) ** 2)
            + coeffs[k - 3] * (9 / 8 - 4.5 * tau(k - 2) + 4.5 * tau(k - 2) ** 2))


def test_legacy_control_families(qgd):
    """Control families of SURVEY row f3: hard-coded quadratic B-spline, the Juqbox bcarrier2 layout
    (= carrier waves over it), piecewise monomials, trigonometric and zero controls.  Checks the
    reference's own control tests (test/ControlTests/test_control_derivatives.jl:26-27,111-124): every
    stored derivative is the time derivative of the one below it, and values match the formulas."""
    rng = np.random.default_rng(8)
    tf, D1 = 7.0, 9
    b2 = qgd.BSpline2Control(D1, tf)
    pc = rng.standard_normal(b2.N_coeff)
    ts = np.linspace(0.0, tf, 41)
    for t in ts:
        assert abs(b2.eval_p(t, pc) - _quad_piece_sum(D1, tf, pc[:D1], t)) < 1e-14
        assert abs(b2.eval_q(t, pc) - _quad_piece_sum(D1, tf, pc[D1:], t)) < 1e-14
    assert np.allclose(b2.grad_tables(ts[1:-1], 0)[0][:, 0, :D1].sum(axis=1), 1.0)      # partition of unity
    assert np.all(b2.grad_tables(ts, 4)[0][:, 3:] == 0.0)                                 # quadratic pieces
    with pytest.raises(ValueError):
        qgd.BSpline2Control(2, tf)
    # bcarrier2 (bspline_backend.jl:783-848): p = sum_f b1 cos(w t) - b2 sin(w t), q = sum_f b1 sin + b2 cos
    omega = [0.0, 1.3, -2.1]
    bc = qgd.BSplineControl(tf, D1, omega)
    pcc = rng.standard_normal(bc.N_coeff)
    assert bc.N_coeff == 2 * D1 * len(omega)
    for t in ts[::5]:
        p = q = 0.0
        for f, w in enumerate(omega):
            o1 = f * 2 * D1
            f1 = _quad_piece_sum(D1, tf, pcc[o1:o1 + D1], t); f2 = _quad_piece_sum(D1, tf, pcc[o1 + D1:o1 + 2 * D1], t)
            p += f1 * np.cos(w * t) - f2 * np.sin(w * t); q += f1 * np.sin(w * t) + f2 * np.cos(w * t)
        assert abs(bc.eval_p(t, pcc) - p) < 1e-13 and abs(bc.eval_q(t, pcc) - q) < 1e-13
    families = [b2, bc, qgd.GeneralGRAPEControl(4, tf, 3), qgd.SinCosControl(tf, frequency=1.7), qgd.SinControl(tf, 0.6),
                qgd.CosControl(tf, 2.2), qgd.SingleSymCosControl(tf, 1.1), qgd.ZeroControl(3, tf)]
    h = 1e-6
    for ctrl in families:
        pc = rng.standard_normal(ctrl.N_coeff)
        for t in (0.31, 2.47, 5.9):          # away from knots / region boundaries
            for d in range(3):
                for ev in (ctrl.eval_p_derivative, ctrl.eval_q_derivative):
                    fd = (ev(t + h, pc, d) - ev(t - h, pc, d)) / (2 * h)
                    assert abs(fd - ev(t, pc, d + 1)) <= 2e-7 * max(1.0, abs(fd)), (type(ctrl).__name__, t, d)
    g = qgd.GeneralGRAPEControl(4, 8.0, 2)
    assert abs(g.eval_p(5.0, np.arange(8.0)) - 2.0 * 0.5 ** 2) < 1e-15                   # region 2, local_t = 0.5
    s = qgd.SinCosControl(3.0, frequency=2.0)
    assert abs(s.eval_p(0.4, [1.5, 0.7]) - 1.5 * np.sin(0.8)) < 1e-15 and abs(s.eval_q(0.4, [1.5, 0.7]) - 0.7 * np.cos(0.8)) < 1e-15
    assert qgd.ZeroControl(5, 1.0).eval_p(0.3, np.ones(5)) == 0.0


def test_hermite_control(qgd):
    """HermiteControl (src/Controls/hermite_control.jl): the interpolant reproduces the data at the points
    (test/ControlFunctionTests/hermite_control_points.jl), equals scipy's Hermite interpolant, is
    C^m across points, and its stored derivatives are consistent (test_control_derivatives.jl:187)."""
    from scipy.interpolate import BPoly
    rng = np.random.default_rng(15)
    tf, npts, m = 3.0, 5, 2
    for scaling in ("Taylor", "Derivative", "Heuristic"):
        hc = qgd.HermiteControl(npts, tf, m, scaling)
        pc = rng.standard_normal(hc.N_coeff)
        assert hc.N_coeff == npts * (m + 1) * 2
        data = pc[:hc.N_coeff // 2].reshape(npts, m + 1)          # [point, derivative order]
        dt = tf / (npts - 1)
        for i in range(npts):
            for j in range(m + 1):
                taylor = hc.eval_p_derivative(min(i * dt, tf), pc, j) * dt ** j / math.factorial(j)
                assert abs(taylor - data[i, j] * hc.scaling[j]) < 1e-11, (scaling, i, j)
    hc = qgd.HermiteControl(npts, tf, m, "Derivative")             # parameters are the derivatives themselves
    pc = rng.standard_normal(hc.N_coeff)
    half = hc.N_coeff // 2
    xi = np.linspace(0, tf, npts)
    ref_p = BPoly.from_derivatives(xi, pc[:half].reshape(npts, m + 1))
    ref_q = BPoly.from_derivatives(xi, pc[half:].reshape(npts, m + 1))
    for t in np.linspace(0.01, tf - 0.01, 23):
        for d in range(4):
            assert abs(hc.eval_p_derivative(t, pc, d) - ref_p.derivative(d)(t) if d else hc.eval_p(t, pc) - ref_p(t)) < 1e-9
            assert abs(hc.eval_q_derivative(t, pc, d) - (ref_q.derivative(d)(t) if d else ref_q(t))) < 1e-9
    assert hc.eval_p_derivative(1.0, pc, 2 * m + 2) == 0.0        # degree 2m+1 pieces
    car = qgd.HermiteCarrierControl(4, tf, 1, [0.0, 2.3], "Taylor")
    assert car.N_coeff == 2 * 4 * 2 * 2
    pcc = rng.standard_normal(car.N_coeff)
    h = 1e-6
    for t in (0.37, 1.9):
        for d in range(3):
            fd = (car.eval_q_derivative(t + h, pcc, d) - car.eval_q_derivative(t - h, pcc, d)) / (2 * h)
            assert abs(fd - car.eval_q_derivative(t, pcc, d + 1)) <= 1e-6 * max(1.0, abs(fd))


def test_more_problem_constructors(qgd):
    """JaynesCummingsProblem, rotating_frame_qubit, dahlquist_problem (src/ProblemConstructors/)."""
    sizes, ess = (3, 2), (2, 2)
    kerr = np.array([[0.2, 0.01], [0.01, 0.3]]); jc = np.array([[0.0, 0.05], [0.05, 0.0]])
    p = qgd.JaynesCummingsProblem(sizes, ess, [4.1, 4.8], 4.0, kerr, jc, 10.0, 20)
    H = p.system_sym + 1j * p.system_asym                      # H = S + iK is Hermitian
    assert np.allclose(H, H.conj().T) and p.N_tot_levels == 6 and p.N_ess_levels == 4
    low = qgd.lowering_operators_system(sizes)
    n0 = low[0].T @ low[0]; n1 = low[1].T @ low[1]
    want = (0.1 * n0 + 0.8 * n1 - 0.1 * low[0].T @ low[0].T @ low[0] @ low[0] - 0.15 * low[1].T @ low[1].T @ low[1] @ low[1]
            - 0.01 * n1 @ n0 + 0.05 * (low[0].T @ low[1] + low[0] @ low[1].T))
    assert np.allclose(H, want)
    q = qgd.rotating_frame_qubit(2, 1, tf=3.0, nsteps=30, detuning_frequency=0.5, self_kerr_coefficient=0.2)
    assert q.N_tot_levels == 3 and np.allclose(np.diag(q.system_sym), [0.0, np.pi, 2 * np.pi - 0.2 * 2 * np.pi])
    assert np.allclose(q.sym_operators[0], q.sym_operators[0].T) and np.allclose(q.asym_operators[0], -q.asym_operators[0].T)
    d = qgd.dahlquist_problem(2.0j, initial_condition=1.0 + 0.5j, with_control=True)
    assert d.N_tot_levels == 1 and d.system_sym[0, 0] == -2.0 and d.N_operators == 1 and d.v0[0, 0] == 0.5
    with pytest.raises(ValueError):
        qgd.dahlquist_problem(1.0 + 1.0j)


def _header_prototypes():
    """{name: (return type, [argument types])} of every function include/qgd.h declares, and {struct: [(type, field)]}."""
    import re
    src = open(os.path.join(ROOT, "include", "qgd.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S):
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            base = re.match(r"((?:const\s+)?\w+)\s+(.*)", decl)
            for part in base.group(2).split(","):
                part = part.strip()
                fields.append((base.group(1) + (" *" if part.startswith("*") else ""), part.lstrip("* ")))
        structs[name] = fields
    protos = {}
    for ret, name, args in re.findall(r"^\s*((?:const\s+)?\w+\s*\*?)\s*(qgd_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        al = []
        for a in args.split(","):
            a = " ".join(a.split())
            if a in ("void", ""):
                continue
            m = re.match(r"((?:const\s+)?\w+)\s*((?:\*\s*(?:const\s*)?)*)\s*\w*(\[\w*\])?$", a)
            assert m, (name, a)
            stars = m.group(2).count("*") + (1 if m.group(3) else 0)
            al.append(m.group(1) + (" " + "*" * stars if stars else ""))
        protos[name] = (" ".join(ret.split()).replace(" *", "*").replace("*", " *"), al)
    return protos, structs


def test_julia_shim_signatures_match_header():
    """julia/QuantumGateDesignHIP.jl has never run (no Julia in the image): every `ccall` of the shim is parsed here and compared
    with the prototype in include/qgd.h -- symbol, return type, number of arguments and each argument's C type -- and the two
    `struct`s the shim passes by reference field by field with their C declarations (same order, same widths)."""
    import re
    protos, structs = _header_prototypes()
    jl = open(os.path.join(ROOT, "julia", "QuantumGateDesignHIP.jl")).read()
    jl = "\n".join(line.split("#")[0] if "ccall" not in line.split("#")[0] and "#" in line else line for line in jl.splitlines())

    def ctype(j):        # Julia ccall type -> the C types it may stand for
        j = j.strip()
        table = {"Cint": {"int", "int32_t"}, "Int32": {"int32_t", "int"}, "Int64": {"int64_t"}, "Clonglong": {"int64_t"},
                 "Float64": {"double"}, "Cdouble": {"double"}, "Csize_t": {"size_t"}, "Cstring": {"const char *"}, "Cvoid": {"void"},
                 "Ptr{Cvoid}": {"qgd_handle", "void *", "const void *"}, "Ptr{Float64}": {"double *", "const double *"},
                 "Ptr{Cdouble}": {"double *", "const double *"}, "Ptr{Int32}": {"int32_t *", "const int32_t *"},
                 "Ptr{Int64}": {"int64_t *", "const int64_t *"}, "Ptr{UInt8}": {"void *", "const void *", "uint8_t *", "const uint8_t *", "unsigned char *"},
                 "Ref{Ptr{Cvoid}}": {"qgd_handle *"}, "Ref{ProblemDesc}": {"const qgd_problem_desc *"},
                 "Ref{CSC}": {"const qgd_csc *"}, "Ptr{CSC}": {"const qgd_csc *"}, "Ptr{Ptr{Float64}}": {"const double **", "double **"}}
        assert j in table, f"unmapped Julia type {j!r}"
        return table[j]

    calls = re.findall(r"ccall\(\(:(\w+),\s*libqgd\),\s*([\w{}]+),\s*\(((?:[^()]|\{[^}]*\})*)\)", jl, flags=re.S)
    assert len(calls) >= 23
    seen = set()
    for name, ret, args in calls:
        assert name in protos, f"the shim calls {name}, which include/qgd.h does not declare"
        cret, cargs = protos[name]
        assert cret in ctype(ret), (name, ret, cret)
        jargs = [a for a in re.split(r",\s*(?![^{]*\})", " ".join(args.split())) if a.strip()]
        assert len(jargs) == len(cargs), (name, jargs, cargs)
        for ja, ca in zip(jargs, cargs):
            assert ca in ctype(ja), (name, ja, ca)
        seen.add(name)
    # the evaluation entry points, the constructors and the multi-GPU calls are all bound
    assert {"qgd_create", "qgd_create_csc", "qgd_destroy", "qgd_set_control_basis", "qgd_eval_forward", "qgd_discrete_adjoint",
            "qgd_eval_grad_forced", "qgd_comm_unique_id", "qgd_comm_init_rccl", "qgd_get_partition"} <= seen
    width = {"Int32": "int32_t", "Int64": "int64_t", "Float64": "double", "Ptr{Float64}": "const double *", "Ptr{Int64}": "const int64_t *"}
    for jname, cname in (("ProblemDesc", "qgd_problem_desc"), ("CSC", "qgd_csc")):
        body = re.search(r"^struct\s+" + jname + r"\b(.*?)^end", jl, flags=re.S | re.M).group(1)
        jf = [(f, t) for f, t in re.findall(r"(\w+)::([\w{}]+)", body)]
        cf = structs[cname]
        assert [f for f, _ in jf] == [f for _, f in cf], (jname, jf, cf)
        for (f, jt), (ct, _) in zip(jf, cf):
            assert width[jt] == ct, (jname, f, jt, ct)
