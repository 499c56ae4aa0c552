"""The Python layer of eval_pullback without a device: what pullback_cotangents (and through it DeviceProblem.eval_pullback and
the functional eval_pullback) refuses before the library is touched, and how it hands the arrays on."""
import numpy as np
import pytest

N, SLOTS, C = 3, 5, 2


def _good(rng):
    O = rng.standard_normal((2, N, N)) + 1j * rng.standard_normal((2, N, N))
    return dict(states_bar=rng.standard_normal((2 * N, SLOTS, C)), populations_bar=rng.standard_normal((4, SLOTS, C)),
                level_map=rng.standard_normal((4, N)), expectations_bar=rng.standard_normal((2, SLOTS, C)),
                observables=O + np.conj(np.transpose(O, (0, 2, 1))))


def test_arrays_are_handed_on_as_the_library_takes_them(qgd):
    a = _good(np.random.default_rng(0))
    sb, pb, lm, eb, re, im = qgd.pullback_cotangents(N, SLOTS, C, **a)
    for x, shape in ((sb, (2 * N, SLOTS, C)), (pb, (4, SLOTS, C)), (lm, (4, N)), (eb, (2, SLOTS, C)), (re, (N, N, 2)), (im, (N, N, 2))):
        assert x.dtype == np.float64 and x.flags.f_contiguous and x.shape == shape
    assert np.array_equal(sb, a["states_bar"]) and np.array_equal(pb, a["populations_bar"]) and np.array_equal(lm, a["level_map"])
    assert np.array_equal(re[:, :, 1], a["observables"][1].real) and np.array_equal(im[:, :, 1], a["observables"][1].imag)
    # parts that were not given stay None; a C-ordered or integer array is converted, not refused
    sb, pb, lm, eb, re, im = qgd.pullback_cotangents(N, SLOTS, C, populations_bar=np.ones((N, SLOTS, C), dtype=np.int64))
    assert sb is None and lm is None and eb is None and re is None and im is None
    assert pb.dtype == np.float64 and pb.flags.f_contiguous and pb.shape == (N, SLOTS, C)
    # real observables: no imaginary planes
    _, _, _, _, re, im = qgd.pullback_cotangents(N, SLOTS, C, expectations_bar=np.ones((1, SLOTS, C)), observables=np.eye(N))
    assert re.shape == (N, N, 1) and im is None


def test_complex_states_bar_is_split_as_complex_to_real_does(qgd):
    rng = np.random.default_rng(1)
    z = rng.standard_normal((N, SLOTS, C)) + 1j * rng.standard_normal((N, SLOTS, C))
    sb = qgd.pullback_cotangents(N, SLOTS, C, states_bar=z)[0]
    assert sb.shape == (2 * N, SLOTS, C) and sb.dtype == np.float64 and sb.flags.f_contiguous
    assert np.array_equal(sb[:N], z.real) and np.array_equal(sb[N:], z.imag)
    for col in range(C):
        assert np.array_equal(sb[:, :, col], qgd.complex_to_real(z[:, :, col]))
    # <states_bar, states> of the real form is Re <z, psi> of the complex one
    psi = rng.standard_normal((N, SLOTS, C)) + 1j * rng.standard_normal((N, SLOTS, C))
    w = np.concatenate([psi.real, psi.imag])
    assert abs(np.sum(sb * w) - np.sum(np.conj(z) * psi).real) <= 1e-13


@pytest.mark.parametrize("change,match", [
    (dict(states_bar=None, populations_bar=None, level_map=None, expectations_bar=None, observables=None), "at least one"),
    (dict(states_bar=np.zeros((N, SLOTS, C))), "states_bar"),                         # real with N rows
    (dict(states_bar=np.zeros((2 * N, SLOTS, C), dtype=complex)), "states_bar"),      # complex with 2N rows
    (dict(states_bar=np.zeros((2 * N, SLOTS + 1, C))), "states_bar"),
    (dict(states_bar=np.zeros((2 * N, SLOTS))), "states_bar"),
    (dict(states_bar=np.zeros((2 * N, SLOTS, C), dtype=bool)), "numeric"),
    (dict(states_bar=np.full((2 * N, SLOTS, C), "a")), "numeric"),
    (dict(populations_bar=np.zeros((N, SLOTS, C))), "populations_bar"),               # 4 groups in the map
    (dict(populations_bar=np.zeros((4, SLOTS, C), dtype=complex)), "real"),
    (dict(populations_bar=np.zeros((4, SLOTS, C + 1))), "populations_bar"),
    (dict(level_map=np.zeros((4, N + 1))), "level_map"),
    (dict(level_map=np.zeros((0, N))), "level_map"),
    (dict(level_map=np.zeros((4, N), dtype=complex)), "level_map"),
    (dict(level_map=np.zeros(N)), "level_map"),
    (dict(populations_bar=None), "without populations_bar"),
    (dict(expectations_bar=None), "go together"),
    (dict(observables=None), "go together"),
    (dict(expectations_bar=np.zeros((3, SLOTS, C))), "expectations_bar"),             # two observables
    (dict(expectations_bar=np.zeros((2, SLOTS, C), dtype=complex)), "real"),
    (dict(observables=np.triu(np.ones((N, N)))), "Hermitian"),
    (dict(observables=1j * np.eye(N)), "Hermitian"),
    (dict(observables=np.eye(N + 1)), "observables"),
])
def test_refusals(qgd, change, match):
    a = _good(np.random.default_rng(2))
    a.update(change)
    if "observables" in change and change["observables"] is not None and np.ndim(change["observables"]) == 2:
        a["expectations_bar"] = np.zeros((1, SLOTS, C))
    with pytest.raises(ValueError, match=match):
        qgd.pullback_cotangents(N, SLOTS, C, **a)


def test_the_functional_form_refuses_before_a_handle_is_made(qgd, monkeypatch):
    prob, _ = qgd.cnot2_problem(nsteps=7, tf=7.0)
    ctrl = [qgd.GeneralBSplineControl(2, 6, prob.tf) for _ in range(prob.N_operators)]
    pcof = np.zeros(qgd.get_number_of_control_parameters(ctrl))
    Nn, c = prob.N_tot_levels, prob.N_initial_conditions

    def no_handle(*a, **k):
        raise AssertionError("a handle was asked for")
    import sys
    monkeypatch.setattr(sys.modules[qgd.__name__ + ".evolution"], "device_problem", no_handle)
    with pytest.raises(ValueError, match="saveEveryNsteps"):
        qgd.eval_pullback(prob, ctrl, pcof, saveEveryNsteps=0, states_bar=np.zeros((2 * Nn, 8, c)))
    with pytest.raises(ValueError, match="at least one"):
        qgd.eval_pullback(prob, ctrl, pcof)
    with pytest.raises(ValueError, match="states_bar"):      # 1 + 7 // 3 = 3 slots
        qgd.eval_pullback(prob, ctrl, pcof, saveEveryNsteps=3, states_bar=np.zeros((2 * Nn, 8, c)))
    with pytest.raises(ValueError, match="Hermitian"):
        qgd.eval_pullback(prob, ctrl, pcof, expectations_bar=np.zeros((1, 8, c)), observables=np.triu(np.ones((Nn, Nn))))
    with pytest.raises(AssertionError, match="a handle was asked for"):      # valid arguments get as far as the handle
        qgd.eval_pullback(prob, ctrl, pcof, saveEveryNsteps=3, states_bar=np.zeros((2 * Nn, 3, c)))
