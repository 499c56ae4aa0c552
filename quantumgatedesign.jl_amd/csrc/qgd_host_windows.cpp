// qgd_host_windows.cpp -- host side of the C ABI (include/qgd.h), time grids in bounded memory (qgd_set_memory_budget): window entry, the windowed forward and adjoint passes, the forced sweep's buffers.
#include "qgd_host.h"

namespace qgdh {


// ---------------------------------------------------------------------------
// Bounded-memory time grid.  The per-time-point matrices (D, L, R, L^-1, P: ~330 KB per step at cnot3, 18 MB at N = 256)
// of a long grid do not have to be resident together: the grid is cut into chunks_eff windows that use the SAME
// buffers one after the other.  Forward pass, windows in order: build -> inverse -> block products -> history of the
// window from the state the previous window ended in; only that state (one panel per window) is kept.  Adjoint pass,
// windows in reverse: the window's matrices and forward history are formed again from its stored start state (unless
// they are the ones still in the buffers), then the adjoint scan of the window from the y the next window ended in,
// lambda, and the window's share of the gradient, which k_contract ADDS to grad.  Cost: build + inverse + forward
// history once more for all windows but one.  The reference keeps O(nsteps) state history but no matrices at all
// (matrix-free GMRES); its low-order runs with 10^4 .. 10^6 steps (examples/cnot3_optimize_gate.sb:27-40) are what
// this mode is for.
// ---------------------------------------------------------------------------


// qgd_set_control_tables on a windowed grid: the window's slice of the caller's tables goes to the device before the
// window's matrices are built (with pcof the tables kernel forms them from the basis, which covers the whole grid)
static int window_tables(qgd_handle h)
{
    qgdk_ctx &k = h->k;
    const size_t per = (size_t)(k.m + 1) * k.n_ops, cnt = (size_t)k.nt * per, off = (size_t)k.n_off * per;
    if (h->tab_p_host.size() < off + cnt) return fail(h, QGD_ERR_STATE, "no control tables: call qgd_set_control_tables or pass pcof");
    double *tmp = nullptr;
    HIP_TRY(h, hipMalloc((void **)&tmp, 2 * cnt * sizeof(double) + 64));
    hipError_t e1 = hipMemcpyAsync(tmp, h->tab_p_host.data() + off, cnt * sizeof(double), hipMemcpyHostToDevice, k.stream);
    hipError_t e2 = hipMemcpyAsync(tmp + cnt, h->tab_q_host.data() + off, cnt * sizeof(double), hipMemcpyHostToDevice, k.stream);
    int kr = (e1 == hipSuccess && e2 == hipSuccess) ? qgdk_tables_from_host(&k, tmp, tmp + cnt) : 1;
    (void)hipStreamSynchronize(k.stream);
    (void)hipFree(tmp);
    if (kr) return fail(h, QGD_ERR_NO_DEVICE, "uploading control tables failed");
    return QGD_OK;
}


// window r takes over the per-time-point buffers: its layout, its slice of the caller's control tables (no pcof) and, with
// with_start_state, the state the forward sweep of the window starts from (stored by the window before it)
int enter_window(qgd_handle h, const double *pcof, int r, bool with_start_state)
{
    qgdk_ctx &k = h->k;
    int rc = plan_windows(h, h->chunks_req, r);
    if (rc) return rc;
    if (!pcof && k.n_ops > 0 && (rc = window_tables(h))) return rc;
    if (with_start_state) {
        const size_t hstep = (size_t)k.Np * 2 * k.cp;
        const double *start = h->chunk_state + (size_t)r * hstep;
        for (double *dst : {k.psi0, k.hist, k.bnd, k.bnd2})
            HIP_TRY(h, hipMemcpyAsync(dst, start, hstep * sizeof(double), hipMemcpyDeviceToDevice, k.stream));
    }
    return QGD_OK;
}


int chunk_forward(qgd_handle h, const double *pcof, int n_pcof, int r, bool rerun)
{
    qgdk_ctx &k = h->k;
    int rc = enter_window(h, pcof, r, true);
    if (rc) return rc;
    const size_t hstep = (size_t)k.Np * 2 * k.cp;
    k.keep_scal = (r > 0 || rerun) ? 1 : 0;
    double *scal_real = k.scal;
    if (rerun) k.scal = h->scal_scratch;          // (the guard sum of this window was counted by the forward pass)
    rc = forward_begin(h, pcof, n_pcof);
    if (!rc) { PhaseTimer t(h, "sweep_forward2"); int e = qgdk_forward_finish(&k); if (e) rc = fail(h, QGD_ERR_NO_DEVICE, "forward history pass failed to launch"); }
    if (!rc && !qgdk_guard_is_fused(&k) && (k.have_guard || !h->forcing_zero)) {
        PhaseTimer t(h, "guard");
        if (qgdk_guard(&k)) rc = fail(h, QGD_ERR_NO_DEVICE, "guard kernel failed to launch");
        if (k.have_guard == 0) h->forcing_zero = true;
    }
    if (!rc && k.gpart_on && k.have_guard && qgdk_guard_fold(&k)) rc = fail(h, QGD_ERR_NO_DEVICE, "guard fold failed to launch");
    k.scal = scal_real; k.keep_scal = 0;
    if (rc) return rc;
    if (!rerun)
        HIP_TRY(h, hipMemcpyAsync(h->chunk_state + (size_t)(r + 1) * hstep, k.hist + (size_t)(k.nt - 1) * hstep, hstep * sizeof(double),
                                  hipMemcpyDeviceToDevice, k.stream));
    h->resident_window = r;
    return QGD_OK;
}


int chunked_forward(qgd_handle h, const double *pcof, int n_pcof, double *uv_history, int save, const Observe *obs)
{
    qgdk_ctx &k = h->k;
    if (!pcof && !h->have_tables && k.n_ops > 0) return fail(h, QGD_ERR_STATE, "no control tables: call qgd_set_control_tables or pass pcof");
    int rc;
    for (int r = 0; r < h->chunks_eff; r++) {
        if ((rc = chunk_forward(h, pcof, n_pcof, r, false))) return rc;
        if (uv_history) {      // the window's share of the state history with its stage derivatives
            { PhaseTimer t(h, "derivs"); K_TRY(h, qgdk_derivs(&k)); }
            if ((rc = history_out(h, uv_history, save))) return rc;
        }
        if (obs && (rc = observe_out(h, *obs, save))) return rc;      // states, populations or expectation values of the window, nothing else
    }
    { PhaseTimer t(h, "terminal"); K_TRY(h, qgdk_terminal(&k, k.have_target)); }      // overlaps (and y_N) from the final state
    sweep_done(h, SWEEP_GENERAL, pcof, n_pcof);
    return QGD_OK;
}


int chunked_adjoint(qgd_handle h, double *lambda_history, double *adjoint_forcing)
{
    qgdk_ctx &k = h->k;
    const size_t hstep = (size_t)k.Np * 2 * k.cp;
    const int W = h->chunks_eff;
    const StoredSweep kept = h->sweep;      // (the window re-runs below leave the window-boundary states of this sweep as they are)
    int rc;
    if (lambda_history)      // (the library writes the j = 0 columns; the others, and time index 0, are zero as in the resident call)
        memset(lambda_history, 0, sizeof(double) * 2 * (size_t)k.N * (k.m + 1) * (size_t)k.nt_glob * k.c);
    for (int r = W - 1; r >= 0; r--) {
        if (h->resident_window != r) {
            if ((rc = chunk_forward(h, kept.has_pcof ? kept.pcof.data() : nullptr, (int)kept.pcof.size(), r, true))) return rc;
        } else if ((rc = plan_windows(h, h->chunks_req, r))) return rc;
        if (adjoint_forcing && (rc = panels_out(h, k.forcing, &h->stage_f, adjoint_forcing, 1, 0))) return rc;
        if (r == W - 1) { PhaseTimer t(h, "terminal"); K_TRY(h, qgdk_terminal(&k, 1)); }
        else            // y at the end of this window = y at the start of the next one
            for (double *dst : {k.yhist + (size_t)(k.nt - 1) * hstep, k.bndY + (size_t)k.scan_blocks * hstep, k.bndY2 + (size_t)k.scan_blocks2 * hstep})
                HIP_TRY(h, hipMemcpyAsync(dst, h->carry_y, hstep * sizeof(double), hipMemcpyDeviceToDevice, k.stream));
        k.grad_accumulate = (r != W - 1) ? 1 : 0;
        h->sweep.derivs = false;
        rc = adjoint_begin(h);
        if (!rc) rc = adjoint_end(h);
        k.grad_accumulate = 0;
        if (rc) return rc;
        if (lambda_history && (rc = lambda_history_out(h, lambda_history))) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->carry_y, k.yhist, hstep * sizeof(double), hipMemcpyDeviceToDevice, k.stream));
    }
    h->sweep = kept;
    return QGD_OK;
}


// buffers of the forced forward sweep for (up to) nt time points and B scan blocks
int forcing_buffers(qgd_handle h, size_t nt, size_t B)
{
    qgdk_ctx &k = h->k;
    const size_t m = k.m, hstep = (size_t)k.Np * 2 * k.cp;
    const int rc = pool_ensure(h, h->pools[POOL_FORCING], {{nt, B}, {
        {&k.ff_F, nt * m * hstep}, {&k.ff_E, nt * m * hstep}, {&k.ff_XR, nt * hstep}, {&k.ff_XL, nt * hstep}, {&k.ff_Q, nt * hstep},
        {&k.ff_phi, (B + 1) * hstep}, {&k.ff_bnd, (B + 2) * hstep},
        // (N > 64 at high order: the m+2 work panels of k_forcing_terms do not fit in LDS)
        {&h->fsc_forcing, nt * (size_t)(k.cp / 8) * (m + 2) * k.Np * 16, (size_t)(m + 2) * k.Np * 16 * sizeof(double) > 150 * 1024}}});
    if (!rc) k.fs_scratch = h->fsc_forcing;
    return rc;
}


// forcing [2N, m, nt_glob, c] (Julia layout, forward_evolution.jl:42-44), time points n_off .. n_off + nt - 1 -> panels [nt][m][Np][2cp]
int upload_forcing(qgd_handle h, const double *forcing, size_t nt, size_t n_off)
{
    qgdk_ctx &k = h->k;
    const size_t m = k.m, n2 = 2 * (size_t)k.N, PWc = 2 * k.cp, hstep = (size_t)k.Np * PWc, ntg = (size_t)h->nsteps + 1;
    std::vector<double> f(nt * m * hstep, 0.0);
    for (size_t n = 0; n < nt; n++) for (size_t j = 0; j < m; j++)
        pack_panel(f.data() + (n * m + j) * hstep, (int)PWc, forcing + ((n_off + n) * m + j) * n2, k.N, k.c, ntg * m * n2);
    HIP_TRY(h, hipMemcpyAsync(k.ff_F, f.data(), f.size() * sizeof(double), hipMemcpyHostToDevice, k.stream));
    HIP_TRY(h, hipStreamSynchronize(k.stream));
    return QGD_OK;
}

}  // namespace qgdh
