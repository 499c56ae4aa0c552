"""CPU test of what the six trajectory-output entry points refuse from their arguments alone (csrc/qgd_host.h: OutputSelection,
selection_refusals): with a NULL handle fail() leaves its message where qgd_last_error(NULL) reads it, so every refusal made in
front of the prologue runs here without a device -- its code, its exact message and its place in the order of the checks (a
call that passes them all ends at the prologue's "null handle")."""
import ctypes as C

import pytest

NULL_HANDLE = "null handle"
NULL_ARGUMENT = "null argument"
MAP = "a level map needs n_groups >= 1"
REFINE = "refine must be >= 1 and 1 + nsteps * refine fit a 32-bit integer"


def _pullback(p, states_bar=None, pop_bar=None, level_map=None, n_groups=0, expect_bar=None, obs_re=None, obs_im=None, n_obs=0, grad=None):
    return "qgd_eval_pullback", (None, p, 1, 0, states_bar, pop_bar, level_map, n_groups, expect_bar, obs_re, obs_im, n_obs, grad)


def _dense_pullback(p, refine=2, states_bar=None, pop_bar=None, level_map=None, n_groups=0, expect_bar=None, obs_re=None, obs_im=None, n_obs=0, grad=None):
    return "qgd_eval_dense_pullback", (None, p, 1, 0, refine, states_bar, pop_bar, level_map, n_groups, expect_bar, obs_re, obs_im, n_obs, grad)


def _pushforward(p, v=None, n_vec=1, states_dot=None, pop_dot=None, level_map=None, n_groups=0, expect_dot=None, obs_re=None, obs_im=None, n_obs=0):
    return "qgd_eval_pushforward", (None, p, 1, 0, v, n_vec, states_dot, pop_dot, level_map, n_groups, expect_dot, obs_re, obs_im, n_obs)


def _dense(p, refine=2, kind=0, level_map=None, n_groups=0, obs_re=None, obs_im=None, n_obs=0):
    return "qgd_eval_dense", (None, p, 1, 0, refine, kind, level_map, n_groups, obs_re, obs_im, n_obs, p, p)


def _populations(p, level_map=None, n_groups=0):
    return "qgd_eval_populations", (None, p, 1, 0, level_map, n_groups, p, p)


def _expectations(p, obs_re=None, obs_im=None, n_obs=0):
    return "qgd_eval_expectations", (None, p, 1, 0, obs_re, obs_im, n_obs, p, p)


def _rows(p):
    return [
        (_pullback(p, states_bar=p), NULL_ARGUMENT),
        (_pullback(p, grad=p), "qgd_eval_pullback needs at least one of states_bar, pop_bar, expect_bar"),
        (_pullback(p, states_bar=p, level_map=p, grad=p), MAP),
        (_pullback(p, expect_bar=p, n_obs=1, grad=p), "expect_bar needs obs_re and n_obs >= 1"),
        (_pullback(p, states_bar=p, grad=p), NULL_HANDLE),
        (_dense_pullback(p, refine=0, states_bar=p, grad=p), REFINE),
        (_dense_pullback(p, refine=0, states_bar=p), NULL_ARGUMENT),
        (_dense_pullback(p, refine=2, grad=p), "qgd_eval_dense_pullback needs at least one of states_bar, pop_bar, expect_bar"),
        (_pushforward(p, states_dot=p), NULL_ARGUMENT),
        (_pushforward(p, v=p, n_vec=0, states_dot=p), "qgd_eval_pushforward needs at least one direction"),
        (_pushforward(p, v=p), "qgd_eval_pushforward needs at least one of states_dot, pop_dot, expect_dot"),
        (_pushforward(p, v=p, states_dot=p, level_map=p), MAP),
        (_pushforward(p, v=p, expect_dot=p, obs_re=p), "expect_dot needs obs_re and n_obs >= 1"),
        (_dense(p, refine=0), REFINE),
        (_dense(p, kind=7), "unknown kind of dense output"),
        (_dense(p, kind=1, level_map=p), MAP),
        (_dense(p, kind=0, level_map=p), NULL_HANDLE),      # (the map is not looked at)
        (_dense(p, kind=2, n_obs=1), "qgd_eval_dense needs obs_re and n_obs >= 1 for expectation values"),
        (_populations(p, level_map=p), MAP),
        (_populations(p), NULL_HANDLE),
        (_expectations(p, n_obs=1), "qgd_eval_expectations needs obs_re and n_obs >= 1"),
        (_expectations(p, obs_re=p, n_obs=0), "qgd_eval_expectations needs obs_re and n_obs >= 1"),
        (_expectations(p, obs_re=p, n_obs=1), NULL_HANDLE),
    ]


N_ROWS = len(_rows(None))


@pytest.mark.parametrize("row", range(N_ROWS))
def test_refusals_from_the_arguments_alone(qgd, row):
    lib = qgd._lib.lib()
    buf = (C.c_double * 64)()
    (name, args), message = _rows(C.cast(buf, C.c_void_p))[row]
    assert getattr(lib, name)(*args) == qgd._lib.QGD_ERR_ARGUMENT, name
    assert lib.qgd_last_error(None).decode() == message, name
    assert not any(buf), name      # nothing was written


def test_the_pushforward_takes_fourteen_arguments(qgd):
    assert len(qgd._lib.lib().qgd_eval_pushforward.argtypes) == 14
