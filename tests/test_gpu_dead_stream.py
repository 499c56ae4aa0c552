"""GPU test of a handle whose stream is dead (qgd_host.h: stream_dead -- a communicator had to be leaked with its collective
still on the stream): every entry point that touches the device refuses with QGD_ERR_COMM in the prologue, before a HIP call
could wait for that stream; the host-only setters and getters keep working.  Nothing is made to hang: the flag is set by
the tests' hook on a healthy handle, and cleared again before the handle is closed.  The problem is cnot2 -- on the library's
defaults the small-problem path, whose evaluations never pass forward_begin."""
import ctypes as C

import numpy as np
import pytest

import cases
import qgd_hooks

pytestmark = pytest.mark.gpu


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _calls(qgd, prob, ctrl, pcof, order, small):
    """name -> arguments behind the handle, valid for cnot2_case at this order: the calls a dead handle refuses, and the
    host-only ones (with qgd_comm_destroy, which has nothing to do without a communicator) that it still answers."""
    L = qgd._lib
    N, c, n_ops, m, nsteps = prob.N_tot_levels, prob.N_initial_conditions, prob.N_operators, order // 2, prob.nsteps
    nt, npc, refine, pts = nsteps + 1, len(pcof), 2, 1 + 2 * nsteps
    # valid arguments for every call: what a healthy handle would accept (and, for the setters, act on)
    pc = np.ascontiguousarray(pcof, dtype=np.float64)
    grad, out3, hess, v, hv = np.zeros(npc), np.zeros(3), np.zeros((npc, npc)), np.ones(npc), np.zeros(npc)
    forcing = np.zeros((2 * N, nt, c), order="F")
    states, pops, expect = (np.zeros((r, nt, c), order="F") for r in (2 * N, N, 1))
    dense, sbar, sbar_dense = (np.zeros((2 * N, p, c), order="F") for p in (pts, nt, pts))
    obs_re = np.asfortranarray(np.eye(N).reshape(N, N, 1))
    term, lam = np.zeros((2 * N, c), order="F"), np.zeros((2 * N, m + 1, nt, c), order="F")
    w_in, w_out = np.ones((2 * N, c), order="F"), np.zeros((2 * N, c), order="F")
    other_target = np.asfortranarray(np.ones((2 * N, c)))
    Gp, Gq, _ = qgd.controls.control_basis(qgd.controls.as_control_list(ctrl), 20, 20.0, m)      # (a basis for ANOTHER grid)
    nco = np.array([k.N_coeff for k in ctrl], dtype=np.int32)
    gp = (C.c_void_p * n_ops)(*[_vp(g) for g in Gp])
    gq = (C.c_void_p * n_ops)(*[_vp(g) for g in Gq])
    tab_p, tab_q = (np.zeros((m + 1, n_ops, nt), order="F") for _ in range(2))
    one, needed, n_phases = np.zeros(1), C.c_size_t(), C.c_int32()
    dev_ptr, sz = C.c_void_p(), [C.c_size_t() for _ in range(3)]
    part, plan, path3, info3 = np.zeros(8, np.int32), np.zeros(4, np.int64), np.zeros(3, np.int32), np.zeros(3, np.int32)
    pinned = np.zeros(512)
    uid = np.zeros(L.QGD_UNIQUE_ID_BYTES, np.uint8)
    refused = {
        "qgd_eval_forward": (_vp(pc), npc, None, _vp(out3)),
        "qgd_discrete_adjoint": (_vp(pc), npc, 0, _vp(grad), None, None, None, _vp(out3)),
        "qgd_eval_batch": (_vp(pc), 1, npc, _vp(grad), _vp(out3), None),
        "qgd_eval_forward_forced": (_vp(pc), npc, _vp(forcing), None, _vp(out3)),
        "qgd_eval_states": (_vp(pc), npc, None, _vp(states), _vp(out3)),
        "qgd_eval_populations": (_vp(pc), npc, 0, None, 0, _vp(pops), _vp(out3)),
        "qgd_eval_expectations": (_vp(pc), npc, 0, _vp(obs_re), None, 1, _vp(expect), _vp(out3)),
        "qgd_eval_dense": (_vp(pc), npc, 0, refine, 0, None, 0, None, None, 0, _vp(dense), _vp(out3)),
        "qgd_eval_adjoint": (_vp(pc), npc, _vp(term), None, _vp(lam)),
        "qgd_apply_hamiltonian": (0, 0, 0, _vp(w_in), _vp(w_out)),
        "qgd_get_intermediate": (b"small_path", _vp(one), 1, C.byref(needed)),
        "qgd_exchange_buffer": (0, C.byref(dev_ptr), C.byref(sz[0]), C.byref(sz[1]), C.byref(sz[2])),
        "qgd_dist_forward_begin": (_vp(pc), npc),
        "qgd_dist_forward_end": (),
        "qgd_dist_adjoint_begin": (),
        "qgd_dist_adjoint_end": (),
        "qgd_dist_finish": (_vp(grad), _vp(out3)),
        "qgd_cols_forward": (_vp(pc), npc),
        "qgd_cols_adjoint": (0,),
        "qgd_eval_grad_forced": (_vp(pc), npc, _vp(grad)),
        "qgd_eval_hessian": (_vp(pc), npc, _vp(hess), _vp(grad)),
        "qgd_eval_hessian_vec": (_vp(pc), npc, _vp(v), 1, _vp(hv), _vp(grad)),
        "qgd_eval_pullback": (_vp(pc), npc, 0, _vp(sbar), None, None, 0, None, None, None, 0, _vp(grad)),
        "qgd_eval_dense_pullback": (_vp(pc), npc, 0, refine, _vp(sbar_dense), None, None, 0, None, None, None, 0, _vp(grad)),
        "qgd_set_nsteps": (20, 20.0),
        "qgd_set_target": (_vp(other_target),),
        "qgd_set_control_basis": (_vp(nco), gp, gq),
        "qgd_set_control_tables": (_vp(tab_p), _vp(tab_q)),
        "qgd_set_partition": (0, 1),
        "qgd_get_partition": (_vp(part),),
        "qgd_set_stream": (None,),
        "qgd_register_host_buffer": (_vp(pinned), pinned.nbytes),
        "qgd_unregister_host_buffer": (_vp(pinned),),
        "qgd_set_memory_budget": (0,),
        "qgd_get_memory_plan": (_vp(plan),),
        "qgd_get_timings": (None, None, 0, C.byref(n_phases)),
        "qgd_comm_init_rccl": (_vp(uid), 0, 1, L.QGD_SHARD_TIME),
    }
    # (qgd_abi_version and qgd_comm_unique_id take no handle; qgd_last_error is read after every refusal below)
    host_only = {
        "qgd_set_cost_type": (0,),
        "qgd_set_operator_path": (0,),
        "qgd_get_operator_path": (_vp(path3),),
        "qgd_set_small_path": (1 if small else 0,),
        "qgd_set_lambda_derivatives": (0,),
        "qgd_set_save_every": (1,),
        "qgd_set_timing": (0, None),
        "qgd_set_comm_timeout": (30000.0,),
        "qgd_comm_info": (_vp(info3),),
        "qgd_comm_destroy": (),      # (its own handling: no communicator is left, nothing to do)
    }
    elsewhere = {"qgd_create", "qgd_create_csc", "qgd_destroy", "qgd_abi_version", "qgd_comm_unique_id", "qgd_last_error"}
    assert set(refused) | set(host_only) | elsewhere == set(L.EXPORTS)
    outputs = (grad, out3, part, plan, info3, path3)
    return refused, host_only, outputs, dict(locals())      # (the last: whatever the pointers point to stays alive with it)


def test_dead_stream_refuses_every_device_entry_point(qgd, _small_path_mode):
    L = qgd._lib
    prob, ctrl, pcof, target = cases.cnot2_case(qgd)
    order = 4
    dp = qgd.DeviceProblem(prob, order)
    dp.set_controls(ctrl)
    dp.set_target(target)
    g0, s0 = dp.discrete_adjoint(pcof)
    small0 = bool(dp.small_path_taken())
    assert small0 == (_small_path_mode == "default")
    lib, h = dp.lib, dp.h
    refused, host_only, (grad, out3, part, plan, info3, path3), _alive = _calls(qgd, prob, ctrl, pcof, order, small0)
    qgd_hooks.stream_dead(dp, True)
    try:
        for name, args in refused.items():
            assert getattr(lib, name)(h, *args) == L.QGD_ERR_COMM, name
            assert b"leaked" in lib.qgd_last_error(h), name
        for name, args in host_only.items():
            assert getattr(lib, name)(h, *args) == L.QGD_OK, name
        assert lib.qgd_abi_version() == 2
        assert list(info3[:2]) == [-1, 0] and path3[0] in (1, 2)
    finally:
        qgd_hooks.stream_dead(dp, False)      # (qgd_destroy takes its normal path and frees the device memory)
    try:
        g1, s1 = dp.discrete_adjoint(pcof)      # the refused setters changed nothing: the same grid, basis and target, the same bits
        assert np.array_equal(g1, g0) and np.array_equal(np.asarray(s1), np.asarray(s0))
        assert bool(dp.small_path_taken()) == small0
        assert not grad.any() and not out3.any() and not part.any() and not plan.any()      # no refused call wrote an output
    finally:
        dp.close()
