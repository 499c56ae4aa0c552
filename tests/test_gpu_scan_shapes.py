"""GPU test of the blocked scan's launch plan (csrc/qgd_k_chain.hip, the host block): every branch of the code that
builds the chain launches, at the smallest grids that reach it.

Grids (plan_scan / plan_windows of qgd_host_alloc.cpp, one handle): 8 steps -- one block; 24 -- 8 blocks of 3 steps, one
level; 30 -- 10 blocks, 4 super-blocks of 3 (suffix products on for the compiled sizes); 150 -- 28 blocks of 6 steps
(sub-block history on), 7 super-blocks of 4.  Problems: cases.synthetic_case with a diagonal guard projector, order 4,
4 columns, as N = 4 (Np = 16: the compiled-size chains, one launch per sweep half), N = 72 (Np = 80: the dense chains,
one launch per scan level) and N = 72 on the generic chain kernel.  Each as one handle and as two in-process ranks of a
time partition (the window chains, the exchange slots of y_N)."""
import numpy as np
import pytest

import cases
import proto_hessian as ph
import proto_propagator as pp

pytestmark = pytest.mark.gpu

ORDER, COLS = 4, 4
FLAVOURS = {"compiled": (4, ""), "dense": (72, ""), "generic": (72, "chain_generic")}


def _problem(qgd, N, nsteps):
    prob, ctrl, pcof, target = cases.synthetic_case(qgd, N=N, c=COLS, n_ops=2, nsteps=nsteps, tf=0.05 * nsteps, seed=N + nsteps)
    prob.guard_subspace_projector = np.asfortranarray(np.diag(np.random.default_rng(N).random(2 * N)))
    return prob, ctrl, pcof, target


def _handle(qgd, prob, ctrl, target):
    dp = qgd.DeviceProblem(prob, ORDER)
    dp.set_small_path(False)                  # N = 4 would take the four-launch path of qgd_k_tiny.hip, which has no scan
    dp.set_controls(ctrl); dp.set_target(target)
    return dp


@pytest.mark.parametrize("nsteps", [8, 24, 30, 150])
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_scan_shapes_one_handle_and_two_ranks(qgd, flavour, nsteps, monkeypatch):
    import torch
    N, paths = FLAVOURS[flavour]
    monkeypatch.setenv("QGD_PATHS", paths)
    prob, ctrl, pcof, target = _problem(qgd, N, nsteps)
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, ORDER // 2)
    ref = pp.evaluate(prob, Gp, Gq, off, pcof, target, ORDER)
    href, gs = pp.history_real(ref["ws"]), np.abs(ref["grad"]).max()
    dp = _handle(qgd, prob, ctrl, target)
    try:
        hist = np.zeros(dp._hist_shape(), order="F")
        grad, out3 = dp.discrete_adjoint(pcof, False, hist)
        out3 = np.asarray(out3).copy()
        if N == 4:
            assert not dp.front_path_taken() and not dp.small_path_taken()
    finally:
        dp.close()
    e_state = np.abs(hist[:, 0] - href[:, 0]).max() / np.abs(href[:, 0]).max()
    e_hist = np.abs(hist - href).max() / np.abs(href).max()
    e_grad = np.abs(grad - ref["grad"]).max() / gs
    print(f"{flavour} {nsteps} steps: states {e_state:.2e}, history {e_hist:.2e}, gradient {e_grad:.2e} (relative)")
    assert e_state <= 1e-10 and e_hist <= 1e-10
    assert e_grad <= 1e-10
    assert out3[2] > 0                        # the guard penalty is part of the case
    stream = torch.cuda.current_stream().cuda_stream
    backs = [qgd.DeviceBackend(prob, ORDER, ctrl, target, r, 2, device=0, stream=stream) for r in range(2)]
    try:
        for b in backs:
            b.dp.set_small_path(False)
        results = qgd.LocalGroup(backs).discrete_adjoint(pcof)
        if N == 4:
            assert not any(b.dp.front_path_taken() or b.dp.small_path_taken() for b in backs)
    finally:
        for b in backs:
            b.close()
    for rank, (g, o) in enumerate(results):
        e_g = np.abs(g - grad).max() / np.abs(grad).max()
        print(f"  rank {rank} of 2 against one handle: gradient {e_g:.2e}, out3 {np.abs(np.asarray(o) / out3 - 1).max():.2e}")
        assert np.abs(g - ref["grad"]).max() <= 1e-10 * gs
        assert e_g <= 1e-11
        assert np.allclose(o, out3, rtol=1e-12, atol=0)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_scan_shapes_forced_gradient(qgd, flavour, monkeypatch):
    """The forced sweeps (qgdk_forced_chains) on the two-level grid: adjoint == forced, the reference's parity contract."""
    N, paths = FLAVOURS[flavour]
    monkeypatch.setenv("QGD_PATHS", paths)
    prob, ctrl, pcof, target = _problem(qgd, N, 30)
    dp = _handle(qgd, prob, ctrl, target)
    try:
        g_adj, _ = dp.discrete_adjoint(pcof)
        g_forced = dp.eval_grad_forced(pcof)
    finally:
        dp.close()
    err = np.abs(g_forced - g_adj).max() / np.abs(g_adj).max()
    print(f"{flavour}: forced against adjoint gradient {err:.2e}")
    assert err <= 1e-12


def test_scan_shapes_hessian_vector_product(qgd):
    """The second-order adjoint sweep starts from y_N copied to every start of the scan (qgdk_copy_yN_to_starts): N = 4 on
    the two-level grid against the numpy statement of the Hessian, at the bound of tests/test_gpu_hvp.py."""
    prob, ctrl, pcof, target = _problem(qgd, 4, 30)
    Gp, Gq, off = qgd.control_basis(ctrl, prob.nsteps, prob.tf, ORDER // 2)
    H0 = ph.hessian(prob, Gp, Gq, off, pcof, target, ORDER)
    v = np.random.default_rng(11).standard_normal(len(pcof))
    dp = _handle(qgd, prob, ctrl, target)
    try:
        hv = dp.eval_hessian_vec(pcof, v)
    finally:
        dp.close()
    err, bound = np.abs(hv - H0 @ v).max(), 1e-11 * np.abs(H0).max() * np.abs(v).sum()
    print(f"max|hv - H0 v| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
