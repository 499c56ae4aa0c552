// qgd_host_eval.cpp -- host side of the C ABI (include/qgd.h), one evaluation: the forward and adjoint phases (orchestration mirrors eval_forward!, src/forward_evolution.jl:33-70, and
// discrete_adjoint!, src/eval_grad_discrete_adjoint.jl:107-160), the transport of results, the evaluation entry points.
#include "qgd_host.h"

namespace qgdh {


int upload_pcof(qgd_handle h, const double *pcof, int n_pcof)
{
    const double *src = pcof;
    if (h->host_in && h->host_out_len >= (size_t)n_pcof) {   // every evaluation ends with a stream synchronisation: the buffer is free
        memcpy(h->host_in, pcof, sizeof(double) * n_pcof);
        src = h->host_in;
    }
    HIP_TRY(h, hipMemcpyAsync(h->pcof_dev, src, sizeof(double) * n_pcof, hipMemcpyHostToDevice, h->k.stream));
    return QGD_OK;
}


// Does this evaluation take the fused front (qgd_front.h)?  A full evaluation on one rank with the grid resident, the control
// basis on the device and pcof small enough for the kernel arguments, a diagonal guard projector or none -- and a grid on which
// it wins: 513 .. 704 time points, where k_front is one round of two to three workgroups per CU and the tail workgroups start
// from pre-built panels (qgdk_front_pre_plan).  Measured (scripts/front_crossover.py, cnot3, us per evaluation front / general):
// 100 steps 185 / 178, 256: 233 / 217, 400: 254 / 256, 512: 284 / 282, 550: 297 / 306, 700: 339 / 342, 800: 430 / 431,
// 1100: 530 / 522 -- without the tail to balance, two launches with eight waves per half time point build faster than four
// waves per time point do.  QGD_PATHS=front takes the front wherever it is supported (tests).
static bool front_applies(qgd_handle h, const double *pcof, int n_pcof)
{
    const qgdk_ctx &k = h->k;
    if (!(pcof && h->have_basis && n_pcof == k.n_pcof && n_pcof <= QGD_PCOF_KERNARG && h->graph_off && !qgd_path("pcof_copy") &&
          !qgd_path("no_front") && !qgd_path("inv_panels") && h->chunks_eff == 1 && h->part_world == 1 && k.part_world == 1 && !h->comm && k.g_nt == 0 &&
          !k.keep_scal && !k.grad_accumulate && k.nt >= 2 && (k.have_guard == 0 || k.have_guard == 2) &&
          (size_t)k.Np * 2 * k.cp < 32768 && k.phi0 && k.hforc && k.termU && k.n_ops > 0 && qgdk_front_supported(&k) != 0)) return false;
    int q2 = 0, q1 = 0;
    return qgd_path("front") != nullptr || qgdk_front_pre_plan(&k, &q2, &q1) > 0;
}


// forward, part 1: everything that needs no other rank (tables .. block propagators)
int forward_begin(qgd_handle h, const double *pcof, int n_pcof, bool allow_front)
{
    qgdk_ctx &k = h->k;
    if (pcof && !h->have_basis) return fail(h, QGD_ERR_STATE, "qgd_set_control_basis must be called before passing pcof");
    if (pcof && n_pcof != k.n_pcof) return fail(h, QGD_ERR_ARGUMENT, "length of pcof does not match the control basis");
    if (!pcof && !h->have_tables && k.n_ops > 0) return fail(h, QGD_ERR_STATE, "no control tables: call qgd_set_control_tables or pass pcof");
    k.front = (allow_front && front_applies(h, pcof, n_pcof)) ? 1 : 0;
    sweep_begin(h);
    // guard penalty: the guard stage stores its workgroups' partial sums and a later stage adds them in a fixed order (the
    // same bits on every run)
    k.gpart_on = k.gpart ? 1 : 0;
    k.gpart_n = qgdk_guard_parts(&k);
    // who adds the partials up: the terminal stage where this handle runs one right behind the guard stage (the grid
    // resident and the final time its own); a window of a long grid and the other ranks of a partition launch k_guard_fold
    k.gpart_terminal = (h->chunks_eff == 1 && k.part_rank == k.part_world - 1) ? 1 : 0;
    if (pcof) {
        PhaseTimer t(h, "tables");
        if (k.front) {
            K_TRY(h, qgdk_tables_front(&k, pcof, n_pcof));      // tables + the step matrices k_front's workgroups past two per CU start from + phi_0
        } else if (n_pcof <= QGD_PCOF_KERNARG && h->graph_off && !qgd_path("pcof_copy")) {   // (a captured graph would freeze the values)
            K_TRY(h, qgdk_tables_kernarg(&k, pcof, n_pcof));      // pcof rides in the kernel arguments: no copy packet
        } else {
            int rc = upload_pcof(h, pcof, n_pcof);
            if (rc) return rc;
            K_TRY(h, qgdk_tables(&k, h->pcof_dev));
        }
    }
    if (!pcof) {   // (with pcof, k_tables clears them)
        if (!k.keep_scal) HIP_TRY(h, hipMemsetAsync(k.scal, 0, 4 * sizeof(double), k.stream));      // (a later window of a long grid keeps the running guard sum)
        HIP_TRY(h, hipMemsetAsync(k.status, 0, 3 * sizeof(int), k.stream));      // (flag and the two counters; the fourth word is the inverse's memory of the last evaluation)
    }
    if (k.front) {
        { PhaseTimer t(h, "front"); K_TRY(h, qgdk_front(&k)); }      // L_n^-H and S_n = R_n L_n^-1 of every time point, one workgroup each
        { PhaseTimer t(h, "sweep_forward"); K_TRY(h, qgdk_forward_blocks(&k)); }
    } else {
        { PhaseTimer t(h, "build_LR"); K_TRY(h, qgdk_build_LR(&k)); }
        { PhaseTimer t(h, "inverse"); K_TRY(h, qgdk_inverse(&k)); }
        if (qgdk_propagator_is_fused(&k)) { K_TRY(h, qgdk_propagator(&k)); }   // k_inverse_mfma formed P_n already
        else { PhaseTimer t(h, "propagator"); K_TRY(h, qgdk_propagator(&k)); }
        { PhaseTimer t(h, "sweep_forward"); K_TRY(h, qgdk_forward_blocks(&k)); }
    }
    h->status_dirty = true;       // (a general-path evaluation can leave the status word set without its result passing through fail():
                                  //  qgd_cols_forward, qgd_dist_* without qgd_dist_finish -- the small-problem path clears it from the host)
    return QGD_OK;
}


// forward, part 2: after the block propagators of all ranks are in PiX
int forward_end(qgd_handle h)
{
    qgdk_ctx &k = h->k;
    { PhaseTimer t(h, "sweep_forward2"); K_TRY(h, qgdk_forward_finish(&k)); }
    if (k.front) {
        // the sweep ran in phi = L psi: state history, guard forcing and penalty, the adjoint sweep's forcing L^-H f
        if (k.have_guard == 0 && !h->forcing_zero) {
            HIP_TRY(h, hipMemsetAsync(k.forcing, 0, (size_t)k.nt * k.Np * 2 * k.cp * sizeof(double), k.stream));
            h->forcing_zero = true;
        }
        if (k.have_guard) h->forcing_zero = false;
        PhaseTimer t(h, "psi"); K_TRY(h, qgdk_psi(&k));
    } else if (k.have_guard == 0 && h->forcing_zero) {
        // nothing to do: without a guard projector the kernel only re-clears the forcing (6 us of the 100 us of a cnot2 evaluation)
    } else if (!qgdk_guard_is_fused(&k)) {
        PhaseTimer t(h, "guard"); K_TRY(h, qgdk_guard(&k));      // else: done by the history pass
        if (k.have_guard == 0) h->forcing_zero = true;
    }
    if (k.part_rank == k.part_world - 1 && !h->defer_terminal) {   // the rank that owns the final time
        PhaseTimer t(h, "terminal"); K_TRY(h, qgdk_terminal(&k, k.have_target));
    }
    if (k.gpart_on && !k.gpart_terminal && k.have_guard) { PhaseTimer t(h, "guard"); K_TRY(h, qgdk_guard_fold(&k)); }
    return QGD_OK;
}


int adjoint_begin(qgd_handle h)
{
    qgdk_ctx &k = h->k;
    k.fuse_terminal = h->defer_terminal ? 1 : 0;     // (the forward sweep left the terminal condition to this launch)
    h->defer_terminal = false;
    { PhaseTimer t(h, "sweep_adjoint"); K_TRY(h, qgdk_adjoint_blocks(&k)); }
    k.fuse_terminal = 0;
    return QGD_OK;
}


int adjoint_end(qgd_handle h)
{
    qgdk_ctx &k = h->k;
    { PhaseTimer t(h, "sweep_adjoint2"); K_TRY(h, qgdk_adjoint_finish(&k)); }
    if (!k.front) { PhaseTimer t(h, "lambda"); K_TRY(h, qgdk_lambda(&k)); }      // (fused front: the sweep ran in lambda itself)
    if (h->lambda_out) {      // its download runs beside the gradient kernels
        double *out = h->lambda_out; h->lambda_out = nullptr;
        int rc = lambda_history_out(h, out);
        if (rc) return rc;
    }
    if (!h->sweep.derivs && qgdk_gradient_needs_derivs(&k)) { PhaseTimer t(h, "derivs"); K_TRY(h, qgdk_derivs(&k)); h->sweep.derivs = true; }
    { PhaseTimer t(h, "gradient"); K_TRY(h, qgdk_gradient(&k)); }
    return QGD_OK;
}


int run_forward(qgd_handle h, const double *pcof, int n_pcof, bool allow_front)
{
    if (h->chunks_eff > 1) return chunked_forward(h, pcof, n_pcof);
    if (h->part_world != 1) return fail(h, QGD_ERR_STATE, "partitioned handle: use the qgd_dist_* entry points");
    int rc = forward_begin(h, pcof, n_pcof, allow_front);
    if (rc) return rc;
    if ((rc = forward_end(h))) return rc;
    sweep_done(h, h->k.front ? SWEEP_FRONT : SWEEP_GENERAL, pcof, n_pcof);
    return QGD_OK;
}



// the small-problem evaluation (qgd_k_tiny.hip); results through the mirror when there is one
bool tiny_applies(qgd_handle h, const double *pcof, int n_pcof)
{
    const qgdk_ctx &k = h->k;
    return h->small_path && pcof && h->have_basis && n_pcof == k.n_pcof && !h->timing && h->graph_off && !h->comm && h->part_world == 1 &&
           h->chunks_eff == 1 && k.redbuf && h->host_out && qgdk_tiny_supported(&k, n_pcof) != 0;
}


int tiny_evaluate(qgd_handle h, const double *pcof, int n_pcof, bool gradient, double *grad, double *out3)
{
    qgdk_ctx &k = h->k;
    const bool mirror = h->mirror_dev != nullptr && h->mirror_ticket != nullptr;
    if (mirror) { k.mirror_dev = h->mirror_dev; k.mirror_ticket = h->mirror_ticket; k.mirror_seq = ++h->mirror_seq; }
    // (the status word: the general path clears it in its first kernel and sets it in a later one; here the kernel that could
    //  clear it -- the per-time-point front -- is also the one that sets it, so it is cleared from the host, and only after an
    //  evaluation that left it set)
    if (h->status_dirty) { HIP_TRY(h, hipMemsetAsync(k.status, 0, 3 * sizeof(int), k.stream)); h->status_dirty = false; }
    int e = qgdk_tiny_eval(&k, pcof, n_pcof, gradient ? 1 : 0);
    if (!e && gradient) e = qgdk_contract_rows(&k, k.nt);
    k.mirror_dev = nullptr;
    if (e) return fail(h, QGD_ERR_NO_DEVICE, std::string("small-problem evaluation failed to launch: ") + hipGetErrorString((hipError_t)e));
    h->mirror_armed = mirror;
    h->forcing_zero = false;
    sweep_done(h, SWEEP_SMALL, pcof, n_pcof, gradient);
    return fetch_results(h, gradient ? grad : nullptr, out3, nullptr);
}


int check_status(qgd_handle h)
{
    int st = 0;
    HIP_TRY(h, hipMemcpyAsync(&st, h->k.status, sizeof(int), hipMemcpyDeviceToHost, h->k.stream));
    HIP_TRY(h, hipStreamSynchronize(h->k.stream));
    if (st) return fail(h, QGD_ERR_NUMERIC, "singular implicit step matrix L(t_n)");
    return QGD_OK;
}



// status + results of an evaluation in one device-to-host copy (the three separate copies cost
// ~25 us of the 0.5 ms evaluation on cnot3)
int fetch_results(qgd_handle h, double *grad, double *out3, const double *src)
{
    qgdk_ctx &k = h->k;
    if (!src) src = k.redbuf;
    if (!k.redbuf || !h->host_out) {
        int rc = check_status(h);
        if (rc) return rc;
        // (src != redbuf: the reduced [grad | scalars | flag] of a time-sharded collective evaluation -- never the rank's own sums)
        const double *g = (src && src != k.redbuf) ? src : k.grad, *sc = (src && src != k.redbuf) ? src + k.n_pcof : k.scal;
        if (src && src != k.redbuf) {
            double flag = 0.0;
            HIP_TRY(h, hipMemcpy(&flag, src + k.n_pcof + 3, sizeof(double), hipMemcpyDeviceToHost));
            if (flag != 0.0) return fail(h, QGD_ERR_NUMERIC, "singular implicit step matrix L(t_n)");
        }
        if (grad && g) HIP_TRY(h, hipMemcpy(grad, g, sizeof(double) * k.n_pcof, hipMemcpyDeviceToHost));
        if (out3) HIP_TRY(h, hipMemcpy(out3, sc, 3 * sizeof(double), hipMemcpyDeviceToHost));
        return QGD_OK;
    }
    const size_t np = (size_t)k.n_pcof;
    if (!h->mirror_armed && !grad && src == k.redbuf && h->mirror_dev && h->mirror_ticket && !h->comm && h->chunks_eff == 1 && h->part_world == 1) {
        // an evaluation without a gradient (qgd_eval_forward): a one-workgroup kernel publishes the scalars the same way
        k.mirror_dev = h->mirror_dev; k.mirror_ticket = h->mirror_ticket; k.mirror_seq = ++h->mirror_seq;
        const int e = qgdk_mirror_scalars(&k);
        k.mirror_dev = nullptr;
        if (e) return fail(h, QGD_ERR_NO_DEVICE, "result mirror kernel failed to launch");
        h->mirror_armed = true;
    }
    if (h->mirror_armed && src == k.redbuf) {
        // the last kernel wrote the results into host memory itself: poll its sequence number (no copy packet, no wait for
        // the stream's completion signal -- the next evaluation's first launch overlaps the tail of this one's last kernel)
        h->mirror_armed = false;
        const volatile unsigned long long *seq = reinterpret_cast<const volatile unsigned long long *>(h->mirror_host + np + 5);
        const auto t0 = std::chrono::steady_clock::now();
        bool ok = true;
        for (unsigned spin = 1; *seq != h->mirror_seq; spin++) {
            if ((spin & 0xfffu) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 5.0) {
                // (never in a healthy run: fall back to the stream's own completion, which also surfaces a device error)
                HIP_TRY(h, hipStreamSynchronize(k.stream));
                ok = (*seq == h->mirror_seq);
                break;
            }
        }
        if (!ok) return fail(h, QGD_ERR_NO_DEVICE, "the evaluation finished without publishing its results (result mirror)");
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        const double *mh = h->mirror_host;
        if (mh[np + 4] != 0.0 || mh[np + 3] != 0.0) return fail(h, QGD_ERR_NUMERIC, "singular implicit step matrix L(t_n)");
        if (grad) memcpy(grad, mh, np * sizeof(double));
        if (out3) memcpy(out3, mh + np, 3 * sizeof(double));
        return QGD_OK;
    }
    HIP_TRY(h, hipMemcpyAsync(h->host_out, src, (np + 5) * sizeof(double), hipMemcpyDeviceToHost, k.stream));
    if (h->comm) { int rcw = comm_wait(h); if (rcw) return rcw; }      // collective evaluation: the wait is bounded
    else HIP_TRY(h, hipStreamSynchronize(k.stream));      // (spinning on hipStreamQuery instead: no difference, 359 us either way)
    int st = 0;
    if (src == k.redbuf) memcpy(&st, h->host_out + np + 4, sizeof(int));      // (a reduced buffer carries the flag as the double in front of it)
    // (host_out[np + 3]: the same flag as a double, summed over the ranks of a time-partitioned evaluation)
    if (st || h->host_out[np + 3] != 0.0) return fail(h, QGD_ERR_NUMERIC, "singular implicit step matrix L(t_n)");
    if (grad) memcpy(grad, h->host_out, np * sizeof(double));
    if (out3) memcpy(out3, h->host_out + np, 3 * sizeof(double));
    return QGD_OK;
}


}  // namespace qgdh

using namespace qgdh;

extern "C" {


int qgd_eval_forward(qgd_handle h, const double *pcof, int32_t n_pcof, double *uv_history, double *out3)
{
    ENTER(h, ENTER_KEEPS_GRAPH);
    qgdk_ctx &k = h->k;
    if (h->comm) return comm_eval_forward(h, pcof, n_pcof, uv_history, out3);
    if (h->chunks_eff > 1 && uv_history) {      // the history of a chunked grid comes out window by window
        int rcw = chunked_forward(h, pcof, n_pcof, uv_history, h->save_every);
        return rcw ? rcw : fetch_results(h, nullptr, out3);
    }
    if (!uv_history && tiny_applies(h, pcof, n_pcof)) return tiny_evaluate(h, pcof, n_pcof, false, nullptr, out3);
    int rc = run_forward(h, pcof, n_pcof, true);
    if (rc) return rc;
    if (uv_history) {
        { PhaseTimer t(h, "derivs"); K_TRY(h, qgdk_derivs(&k)); }
        h->sweep.derivs = true;
    }
    if (uv_history && (rc = history_out(h, uv_history, h->save_every))) return rc;
    if ((rc = fetch_results(h, nullptr, out3))) { (void)finish_copies(h); return rc; }
    return finish_copies(h);
}


int qgd_discrete_adjoint(qgd_handle h, const double *pcof, int32_t n_pcof, int32_t history_precomputed,
                         double *grad, double *uv_history, double *lambda_history, double *adjoint_forcing,
                         double *out3)
{
    if (!grad) return fail(h, QGD_ERR_ARGUMENT, "null argument");
    ENTER(h, ENTER_KEEPS_GRAPH);
    qgdk_ctx &k = h->k;
    if (!k.have_target) return fail(h, QGD_ERR_STATE, "qgd_set_target must be called before qgd_discrete_adjoint");
    if (!h->have_basis) return fail(h, QGD_ERR_STATE, "qgd_set_control_basis must be called before qgd_discrete_adjoint");
    if (h->comm) return comm_discrete_adjoint(h, pcof, n_pcof, history_precomputed, grad, uv_history, lambda_history, adjoint_forcing, out3);
    if (h->part_world != 1) return fail(h, QGD_ERR_STATE, "partitioned handle: use the qgd_dist_* entry points, or give the handle a communicator (qgd_comm_init_rccl)");
    int rc;
    if (h->chunks_eff > 1) {      // bounded-memory time grid: forward pass over the windows, adjoint pass back over them
        if ((rc = refuse_reuse(h, history_precomputed))) return rc;
        // (uv_history is an output: a reused forward pass would have nothing to copy it from, so the pass is redone)
        if ((uv_history || !(history_precomputed && sweep_reusable(h, pcof, n_pcof))) && (rc = chunked_forward(h, pcof, n_pcof, uv_history))) return rc;
        if ((rc = chunked_adjoint(h, lambda_history, adjoint_forcing))) return rc;
        return fetch_results(h, grad, out3);
    }
    if (!uv_history && !lambda_history && !adjoint_forcing && tiny_applies(h, pcof, n_pcof)) {
        if ((rc = refuse_reuse(h, history_precomputed))) return rc;
        return tiny_evaluate(h, pcof, n_pcof, true, grad, out3);      // (four launches redo the sweep faster than the stored one could be reused)
    }
    // full evaluation, nothing but [grad | scalars] coming back, no event bracketing: replay the captured launch sequence
    const bool graph_ok = !h->graph_off && !history_precomputed && !uv_history && !lambda_history && !adjoint_forcing &&
                          !h->timing && k.redbuf && h->host_out && h->host_in && h->host_out_len >= (size_t)n_pcof && pcof;
    if (graph_ok) {
        if (n_pcof != k.n_pcof) return fail(h, QGD_ERR_ARGUMENT, "length of pcof does not match the control basis");
        if (!h->graph_exec && ++h->graph_calls >= 3) {      // the first calls set function attributes and fill caches
            hipGraph_t g = nullptr;
            bool ok = hipStreamBeginCapture(k.stream, hipStreamCaptureModeRelaxed) == hipSuccess;
            if (ok) {
                h->defer_terminal = qgdk_terminal_can_fuse(&k) != 0;
                rc = run_forward(h, pcof, n_pcof);
                if (!rc) rc = adjoint_begin(h);
                if (!rc) rc = adjoint_end(h);
                if (!rc && hipMemcpyAsync(h->host_out, k.redbuf, ((size_t)k.n_pcof + 5) * sizeof(double), hipMemcpyDeviceToHost, k.stream) != hipSuccess) rc = 1;
                ok = (hipStreamEndCapture(k.stream, &g) == hipSuccess) && !rc && g;
                if (ok) ok = hipGraphInstantiate(&h->graph_exec, g, nullptr, nullptr, 0) == hipSuccess;
                if (ok) h->graph = g; else { if (g) (void)hipGraphDestroy(g); h->graph_exec = nullptr; }
            }
            (void)hipGetLastError();
            if (!ok) {      // e.g. the legacy default stream cannot be captured: plain launches from now on
                h->graph_off = true;
                h->forcing_zero = false;      // (the capture only RECORDED the guard clear: the plain path must run it)
            }
        }
        if (h->graph_exec) {
            memcpy(h->host_in, pcof, sizeof(double) * n_pcof);
            HIP_TRY(h, hipGraphLaunch(h->graph_exec, k.stream));
            HIP_TRY(h, hipStreamSynchronize(k.stream));
            sweep_done(h, SWEEP_GENERAL, pcof, n_pcof);
            h->sweep.derivs = qgdk_gradient_needs_derivs(&k) != 0;
            const size_t np = (size_t)k.n_pcof;
            int st;
            memcpy(&st, h->host_out + np + 4, sizeof(int));
            if (st) return fail(h, QGD_ERR_NUMERIC, "singular implicit step matrix L(t_n)");
            memcpy(grad, h->host_out, np * sizeof(double));
            if (out3) memcpy(out3, h->host_out + np, 3 * sizeof(double));
            return QGD_OK;
        }
    }
    struct CopyGuard { qgd_handle h; ~CopyGuard() { (void)finish_copies(h); h->defer_terminal = false; } } guard{h};   // no copy (and no deferred terminal condition) outlives the call
    // history_precomputed: the reference differentiates the history it is GIVEN with the pcof it is given
    // (eval_grad_discrete_adjoint.jl:118-124).  The device keeps its own copy of the last forward sweep; it is
    // reused only when it was computed from this very pcof, otherwise the sweep is simply redone.
    if ((rc = refuse_reuse(h, history_precomputed))) return rc;
    const bool reuse = history_precomputed && sweep_reusable(h, pcof, n_pcof);
    if (reuse) {
        // the terminal right-hand side may not have been written if the target was set later
        { PhaseTimer t(h, "terminal"); K_TRY(h, qgdk_terminal(&k, 1)); }
    } else {
        h->defer_terminal = k.have_target && qgdk_terminal_can_fuse(&k) != 0;
        rc = run_forward(h, pcof, n_pcof, true);
        if (rc) { h->defer_terminal = false; return rc; }
    }
    // The downloads run on the copy stream beside the adjoint sweep and are what bounds this form of the call (PCIe):
    // the guard forcing goes first -- it is final once the forward sweep is (eval_grad_discrete_adjoint.jl:732-752) and
    // keeps the link busy while the stage derivatives of the state history are still being computed and laid out
    if (adjoint_forcing && (rc = panels_out(h, k.forcing, &h->stage_f, adjoint_forcing, 1, 0))) return rc;
    if (uv_history) {
        if (!h->sweep.derivs) { PhaseTimer t(h, "derivs"); K_TRY(h, qgdk_derivs(&k)); h->sweep.derivs = true; }
        if ((rc = history_out(h, uv_history))) return rc;
    }
    if ((rc = adjoint_begin(h))) return rc;
    h->lambda_out = lambda_history;
    // (result mirror: single GPU, resident grid; with event bracketing on too -- qgd_get_timings synchronises the stream itself)
    const bool mirror = h->mirror_dev && h->mirror_ticket && k.redbuf && k.n_ops > 0;
    if (mirror) { k.mirror_dev = h->mirror_dev; k.mirror_ticket = h->mirror_ticket; k.mirror_seq = ++h->mirror_seq; }
    rc = adjoint_end(h);
    k.mirror_dev = nullptr;
    h->lambda_out = nullptr;
    if (rc) return rc;
    h->mirror_armed = mirror;
    if ((rc = fetch_results(h, grad, out3))) return rc;
    rc = finish_copies(h);
    return rc;
}


// eval_forward(...; forcing) (forward_evolution.jl:118-129,167-206).  A windowed grid runs its windows in order, each from the
// forced state the previous one ended in, with its slice of the caller's forcing; the guard penalty accumulates over the
// windows, the overlaps come from the final state; uv_history (stage derivatives w_j = D_j w_0 + E_j included) window by
// window as in chunked_forward.
// (states: qgd_eval_states with a forcing -- the forced states alone, no stage derivatives)
// Both callers have entered and dropped a captured graph.
static int forward_forced(qgd_handle h, const double *pcof, int32_t n_pcof, const double *forcing,
                          double *uv_history, double *states, double *out3)
{
    qgdk_ctx &k = h->k;
    if (h->part_world != 1) return fail(h, QGD_ERR_STATE, "partitioned handle: the forced forward sweep is single-GPU");
    const int W = h->chunks_eff;
    const size_t hstep = (size_t)k.Np * 2 * k.cp;
    if (W > 1) {
        if (!pcof && !h->have_tables && k.n_ops > 0) return fail(h, QGD_ERR_STATE, "no control tables: call qgd_set_control_tables or pass pcof");
        sweep_void(h); h->resident_window = -1;       // (the window-boundary states are those of the FORCED sweep from here on)
    }
    size_t nt0 = 0, B0 = 0;
    int rc;
    for (int r = 0; r < W; r++) {
        if (W > 1 && (rc = enter_window(h, pcof, r, true))) return rc;
        if (r == 0) { nt0 = (size_t)k.nt; B0 = (size_t)k.scan_blocks; }      // (the first window is the longest)
        k.keep_scal = (r > 0) ? 1 : 0;      // (a later window adds to the guard sum of the ones before it)
        rc = forward_begin(h, pcof, n_pcof);
        k.keep_scal = 0;
        if (rc) return rc;
        if ((rc = forcing_buffers(h, std::max(nt0, (size_t)k.nt), std::max(B0, (size_t)k.scan_blocks)))) return rc;
        if ((rc = upload_forcing(h, forcing, (size_t)k.nt, (size_t)k.n_off))) return rc;
        { PhaseTimer t(h, "forcing_terms"); K_TRY(h, qgdk_forcing_terms(&k)); }
        { PhaseTimer t(h, "sweep_forced"); K_TRY(h, qgdk_forcing_sweep(&k)); }
        // (the stand-alone guard kernel stores ONE partial penalty per time point; forward_begin sized the fixed-order sum for
        //  the history pass that fuses the guard work -- fewer, per-block partials -- which this sweep does not run: round 3's
        //  sum added only the first of them and returned a guard penalty that was too small)
        k.gpart_n = k.nt;
        { PhaseTimer t(h, "guard"); K_TRY(h, qgdk_guard_kernel(&k)); }
        h->forcing_zero = k.have_guard == 0;
        if (k.gpart_on && !k.gpart_terminal && k.have_guard) { PhaseTimer t(h, "guard"); K_TRY(h, qgdk_guard_fold(&k)); }
        if (W > 1)
            HIP_TRY(h, hipMemcpyAsync(h->chunk_state + (size_t)(r + 1) * hstep, k.hist + (size_t)(k.nt - 1) * hstep, hstep * sizeof(double),
                                      hipMemcpyDeviceToDevice, k.stream));
        if (uv_history) {
            { PhaseTimer t(h, "derivs"); K_TRY(h, qgdk_derivs(&k)); }
            K_TRY(h, qgdk_forcing_add_derivs(&k));     // w_j = D_j w_0 + E_j
            if ((rc = history_out(h, uv_history, h->save_every))) return rc;
        }
        if (states && (rc = observe_out(h, Observe{{true}, states}, h->save_every))) return rc;
    }
    { PhaseTimer t(h, "terminal"); K_TRY(h, qgdk_terminal(&k, k.have_target)); }
    if ((rc = fetch_results(h, nullptr, out3))) { (void)finish_copies(h); return rc; }
    return finish_copies(h);
}


}  // extern "C"

// The device arrays of a batch chunk (POOL_BATCH) and its pinned staging buffer.  *members: in, the chunk the call would like;
// out, the chunk it gets -- what the memory budget and the free device memory hold, never below one member.  A pool made for a
// larger chunk of the same problem is kept as it is.  (qgd_eval_ensemble takes its per-member arrays from here too.)
int qgdh::batch_buffers(qgd_handle h, int n_pcof, int *members)
{
    const qgdk_ctx &k = h->k;
    Pool &pool = h->pools[POOL_BATCH];
    size_t st, sm, sc;
    qgdk_tiny_batch_layout(&k, n_pcof, &st, &sm, &sc);
    const size_t np = (size_t)n_pcof, per = st + 4 * sm + sc + QGD_TINY_BATCH_SMALL + np + (np + 5);      // doubles of one member
    const std::vector<size_t> shape{(size_t)k.nt, (size_t)k.m, (size_t)k.n_ops, np};
    size_t Kc = (size_t)*members;
    if (pool.key.size() == 5 && std::equal(shape.begin(), shape.end(), pool.key.begin() + 1) && pool.key[0] >= Kc) Kc = pool.key[0];
    else {
        pool_release(pool);      // (what it held counts as free memory)
        size_t limit = h->mem_budget, fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && (!limit || fr < limit)) limit = fr;
        if (limit) Kc = std::max<size_t>(1, std::min(Kc, limit / (per * sizeof(double) + 9 * 64)));      // (9 buffers, dev_alloc pads each)
    }
    qgd_handle_s::BatchBufs &b = h->bt;
    const int rc = pool_ensure(h, pool, {{Kc, shape[0], shape[1], shape[2], shape[3]}, {
        {&b.pcofs, Kc * np}, {&b.tab, Kc * st}, {&b.Rg, Kc * sm}, {&b.Linv, Kc * sm}, {&b.psi, Kc * sm}, {&b.lam, Kc * sm},
        {&b.cpart, Kc * sc}, {&b.small, Kc * QGD_TINY_BATCH_SMALL}, {&b.rows, Kc * (np + 5)}}},
        "one member of a batch does not fit the memory budget or the free device memory", 0, [&]() -> int {
            // (the status words: the front sets one, the batched k_contract_sum reads and clears it)
            HIP_TRY(h, hipMemsetAsync(b.small, 0, Kc * QGD_TINY_BATCH_SMALL * sizeof(double), k.stream));
            return QGD_OK;
        });
    if (rc) return rc;
    const size_t stage = Kc * (2 * np + 5);
    if (h->batch_host_len < stage) {
        if (h->batch_host) (void)hipHostFree(h->batch_host);
        h->batch_host = nullptr; h->batch_host_len = 0;
        HIP_TRY(h, hipHostMalloc((void **)&h->batch_host, stage * sizeof(double), hipHostMallocDefault));
        h->batch_host_len = stage;
    }
    *members = (int)std::min<size_t>(Kc, (size_t)*members);
    return QGD_OK;
}

extern "C" {


// Many coefficient vectors of one problem in one call.  On the small-problem path the members of a
// chunk run side by side: one upload, four launches, one download, whatever the chunk holds.  Everywhere else the single
// evaluations run one after another through the entry points above.
int qgd_eval_batch(qgd_handle h, const double *pcofs, int32_t n_members, int32_t n_pcof, double *grads, double *out3,
                   int32_t *member_status)
{
    if (!pcofs || !out3) return fail(h, QGD_ERR_ARGUMENT, "null argument");
    if (n_members < 1) return fail(h, QGD_ERR_ARGUMENT, "a batch needs at least one member");
    if (h && (h->comm || h->part_world != 1)) return fail(h, QGD_ERR_UNSUPPORTED, "qgd_eval_batch is single-GPU: this handle has a communicator or a partition");
    ENTER(h, ENTER_KEEPS_GRAPH);
    qgdk_ctx &k = h->k;
    if (!h->have_basis) return fail(h, QGD_ERR_STATE, "qgd_set_control_basis must be called before qgd_eval_batch");
    if (n_pcof != k.n_pcof) return fail(h, QGD_ERR_ARGUMENT, "length of a member's pcof does not match the control basis");
    if (grads && !k.have_target) return fail(h, QGD_ERR_STATE, "qgd_set_target must be called before a batch with gradients");
    const size_t np = (size_t)n_pcof;
    int first_singular = -1;
    if (member_status) memset(member_status, 0, sizeof(int32_t) * (size_t)n_members);
    if (!tiny_applies(h, pcofs, n_pcof)) {      // the loop route
        for (int m = 0; m < n_members; m++) {
            const double *p = pcofs + (size_t)m * np;
            const int rc = grads ? qgd_discrete_adjoint(h, p, n_pcof, 0, grads + (size_t)m * np, nullptr, nullptr, nullptr, out3 + 3 * (size_t)m)
                                 : qgd_eval_forward(h, p, n_pcof, nullptr, out3 + 3 * (size_t)m);
            if (rc == QGD_ERR_NUMERIC) {
                if (member_status) member_status[m] = 1;
                if (first_singular < 0) first_singular = m;
            } else if (rc) { sweep_void(h); h->batch_path = false; return rc; }
        }
        sweep_void(h);
        h->batch_path = false;
    } else {
        int chunk = std::min((int)n_members, h->batch_chunk_max);
        int rc = batch_buffers(h, n_pcof, &chunk);
        if (rc) return rc;
        sweep_void(h);
        h->batch_path = true;
        const qgd_handle_s::BatchBufs &b = h->bt;
        const qgdk_tiny_batch dev{b.pcofs, b.tab, b.Rg, b.Linv, b.psi, b.lam, b.cpart, b.small, b.rows};
        double *hin = h->batch_host, *hout = h->batch_host + (size_t)chunk * np;
        for (int m0 = 0; m0 < n_members; m0 += chunk) {
            const int Kc = std::min(chunk, (int)n_members - m0);
            memcpy(hin, pcofs + (size_t)m0 * np, sizeof(double) * Kc * np);
            HIP_TRY(h, hipMemcpyAsync(b.pcofs, hin, sizeof(double) * Kc * np, hipMemcpyHostToDevice, k.stream));
            int e = qgdk_tiny_eval_batch(&k, &dev, Kc, n_pcof, grads ? 1 : 0);
            if (!e) e = qgdk_contract_rows_batch(&k, &dev, Kc, n_pcof, grads ? k.nt : 0);
            if (e) return fail(h, QGD_ERR_NO_DEVICE, std::string("batched small-problem evaluation failed to launch: ") + hipGetErrorString((hipError_t)e));
            HIP_TRY(h, hipMemcpyAsync(hout, b.rows, sizeof(double) * Kc * (np + 5), hipMemcpyDeviceToHost, k.stream));
            HIP_TRY(h, hipStreamSynchronize(k.stream));
            for (int q = 0; q < Kc; q++) {
                const double *row = hout + (size_t)q * (np + 5);
                if (grads) memcpy(grads + (size_t)(m0 + q) * np, row, sizeof(double) * np);
                memcpy(out3 + 3 * (size_t)(m0 + q), row + np, 3 * sizeof(double));
                if (row[np + 3] != 0.0) {
                    if (member_status) member_status[m0 + q] = 1;
                    if (first_singular < 0) first_singular = m0 + q;
                }
            }
        }
    }
    if (first_singular >= 0) {
        const bool dirty = h->status_dirty;
        const int rc = fail(h, QGD_ERR_NUMERIC, "singular implicit step matrix L(t_n) in member " + std::to_string(first_singular) + " of the batch");
        if (h->batch_path) h->status_dirty = dirty;      // (the batched route has status words of its own, which it clears itself)
        return rc;
    }
    return QGD_OK;
}


int qgd_eval_forward_forced(qgd_handle h, const double *pcof, int32_t n_pcof, const double *forcing,
                            double *uv_history, double *out3)
{
    if (!forcing) return fail(h, QGD_ERR_ARGUMENT, "null argument");
    ENTER(h);
    return forward_forced(h, pcof, n_pcof, forcing, uv_history, nullptr, out3);
}


// The forward sweep (or, history_precomputed under the rule of qgd_discrete_adjoint, the stored one) and nothing of it but what
// `obs` names, behind the upload of its level map or observable planes into the staging pool.  The sweep record ends as
// qgd_eval_forward without an output array leaves it.  (refuse_reuse: every caller has asked already, before the uploads.)
static int observe_eval(qgd_handle h, const double *pcof, int n_pcof, int history_precomputed, const Observe &obs, double *out3)
{
    qgdk_ctx &k = h->k;
    int rc;
    const OutputSizes z = output_sizes(obs.sel, (size_t)k.N, 0);
    if (z.map && (rc = grow_stage(h, h->obs_map, z.map))) return rc;
    if (z.planes && (rc = grow_stage(h, h->obs_planes, z.planes))) return rc;
    if ((rc = upload_selection(h, obs.sel, z, h->obs_map.p, h->obs_planes.p))) return rc;
    const int save = obs.refine ? 1 : h->save_every;      // (the dense output returns every sub-point)
    if (h->chunks_eff > 1) {      // one window is resident at a time: the pass over the windows is redone, each hands out its share
        if ((rc = chunked_forward(h, pcof, n_pcof, nullptr, save, &obs))) return rc;
        return fetch_results(h, nullptr, out3);
    }
    struct CopyGuard { qgd_handle h; ~CopyGuard() { (void)finish_copies(h); } } guard{h};      // no copy outlives the call
    if (history_precomputed && sweep_reusable(h, pcof, n_pcof)) {
        // (the overlaps in out3 belong to the present target, which may have been set after the sweep)
        PhaseTimer t(h, "terminal"); K_TRY(h, qgdk_terminal(&k, k.have_target));
    } else if ((rc = run_forward(h, pcof, n_pcof, true))) return rc;
    if ((rc = observe_out(h, obs, save))) return rc;
    if ((rc = fetch_results(h, nullptr, out3))) return rc;
    return finish_copies(h);
}


int qgd_eval_states(qgd_handle h, const double *pcof, int32_t n_pcof, const double *forcing, double *states, double *out3)
{
    if (!states) return fail(h, QGD_ERR_ARGUMENT, "null output array");
    ENTER(h, ENTER_KEEPS_GRAPH);
    if (h->comm || h->part_world != 1) return fail(h, QGD_ERR_UNSUPPORTED, "qgd_eval_states is single-GPU: this handle has a communicator or a partition");
    if (forcing) { drop_graph(h); return forward_forced(h, pcof, n_pcof, forcing, nullptr, states, out3); }
    return observe_eval(h, pcof, n_pcof, 0, Observe{{true}, states}, out3);
}


int qgd_eval_populations(qgd_handle h, const double *pcof, int32_t n_pcof, int32_t history_precomputed,
                         const double *level_map, int32_t n_groups, double *populations, double *out3)
{
    const Observe obs{{false, true, false, level_map, n_groups}, populations};
    if (!populations) return fail(h, QGD_ERR_ARGUMENT, "null output array");
    int rc;
    if ((rc = selection_refusals(h, obs.sel, "qgd_eval_populations"))) return rc;
    ENTER(h, ENTER_KEEPS_GRAPH);
    if (h->comm || h->part_world != 1) return fail(h, QGD_ERR_UNSUPPORTED, "qgd_eval_populations is single-GPU: this handle has a communicator or a partition");
    if ((rc = refuse_reuse(h, history_precomputed))) return rc;
    return observe_eval(h, pcof, n_pcof, history_precomputed, obs, out3);
}


int qgd_eval_expectations(qgd_handle h, const double *pcof, int32_t n_pcof, int32_t history_precomputed,
                          const double *obs_re, const double *obs_im, int32_t n_obs, double *expect, double *out3)
{
    const Observe obs{{false, false, true, nullptr, 0, obs_re, obs_im, n_obs}, expect};
    if (!expect) return fail(h, QGD_ERR_ARGUMENT, "null output array");
    int rc;
    if ((rc = selection_refusals(h, obs.sel, "qgd_eval_expectations"))) return rc;
    ENTER(h, ENTER_KEEPS_GRAPH);
    if (h->comm || h->part_world != 1) return fail(h, QGD_ERR_UNSUPPORTED, "qgd_eval_expectations is single-GPU: this handle has a communicator or a partition");
    if ((rc = refuse_reuse(h, history_precomputed))) return rc;
    return observe_eval(h, pcof, n_pcof, history_precomputed, obs, out3);
}


// Hermite dense output: the sweep of the three calls above, then the states, populations or expectation
// values of the interpolant at refine points per step (observe_out: stage derivatives, qgd_k_interp.hip, the same output kernels
// and transport).  Everything that can refuse the call does so here, before the first launch or upload.  The selection holds
// the level map only for populations and the observables only for expectation values: what the kind does not use is not looked at.
int qgd_eval_dense(qgd_handle h, const double *pcof, int32_t n_pcof, int32_t history_precomputed, int32_t refine, int32_t kind,
                   const double *level_map, int32_t n_groups, const double *obs_re, const double *obs_im, int32_t n_obs,
                   double *out, double *out3)
{
    if (!out) return fail(h, QGD_ERR_ARGUMENT, "null output array");
    if (refine < 1 || (h && (long long)h->nsteps * refine + 1 > 0x7fffffffLL))
        return fail(h, QGD_ERR_ARGUMENT, "refine must be >= 1 and 1 + nsteps * refine fit a 32-bit integer");
    if (kind != QGD_DENSE_STATES && kind != QGD_DENSE_POPULATIONS && kind != QGD_DENSE_EXPECTATIONS)
        return fail(h, QGD_ERR_ARGUMENT, "unknown kind of dense output");
    Observe obs{{kind == QGD_DENSE_STATES, kind == QGD_DENSE_POPULATIONS, kind == QGD_DENSE_EXPECTATIONS}, out, refine};
    if (obs.sel.pops) { obs.sel.level_map = level_map; obs.sel.n_groups = n_groups; }
    if (obs.sel.expect) { obs.sel.obs_re = obs_re; obs.sel.obs_im = obs_im; obs.sel.n_obs = n_obs; }
    int rc;
    if ((rc = selection_refusals(h, obs.sel, "qgd_eval_dense", " for expectation values"))) return rc;
    ENTER(h, ENTER_KEEPS_GRAPH);
    const qgdk_ctx &k = h->k;
    if (h->comm || h->part_world != 1) return fail(h, QGD_ERR_UNSUPPORTED, "qgd_eval_dense is single-GPU: this handle has a communicator or a partition");
    if (pcof && !h->have_basis) return fail(h, QGD_ERR_STATE, "qgd_set_control_basis must be called before passing pcof");
    if (pcof && n_pcof != k.n_pcof) return fail(h, QGD_ERR_ARGUMENT, "length of pcof does not match the control basis");
    if (!pcof && !h->have_tables && k.n_ops > 0) return fail(h, QGD_ERR_STATE, "no control tables: call qgd_set_control_tables or pass pcof");
    if ((rc = refuse_reuse(h, history_precomputed))) return rc;
    if (refine > 1 && (rc = dense_buffers(h, refine))) return rc;      // (QGD_ERR_MEMORY before the sweep is touched)
    return observe_eval(h, pcof, n_pcof, history_precomputed, obs, out3);
}


// eval_adjoint (forward_evolution.jl:352-483): lambda from the given terminal condition lambda_N and forcing, no forward
// history (none is read).  A windowed grid runs its windows in reverse; each forms its matrices, takes its slice of the forcing
// and the y the next window ended in (the last one: y_N = L_N^H lambda_N), and writes its share of lambda_history (global time
// indices n_off+1 .. n_off+nt-1).
int qgd_eval_adjoint(qgd_handle h, const double *pcof, int32_t n_pcof, const double *terminal_condition,
                     const double *forcing, double *lambda_history)
{
    if (!terminal_condition || !lambda_history) return fail(h, QGD_ERR_ARGUMENT, "null argument");
    ENTER(h);
    qgdk_ctx &k = h->k;
    if (h->part_world != 1) return fail(h, QGD_ERR_STATE, "partitioned handle: eval_adjoint is single-GPU");
    const int W = h->chunks_eff;
    const size_t PWc = 2 * k.cp, hstep = (size_t)k.Np * PWc, n2 = 2 * (size_t)k.N, m = k.m, ntg = k.nt_glob;
    if (W > 1) {
        if (!pcof && !h->have_tables && k.n_ops > 0) return fail(h, QGD_ERR_STATE, "no control tables: call qgd_set_control_tables or pass pcof");
        memset(lambda_history, 0, sizeof(double) * n2 * (m + 1) * ntg * k.c);      // (a window writes only its j = 0 columns)
        sweep_void(h); h->resident_window = -1;      // (the buffers will hold no window's forward history)
    }
    // terminal condition [2N, c] and forcing [2N, nt_glob, c] into panel layout
    std::vector<double> lamN(hstep, 0.0), f;
    pack_panel(lamN.data(), (int)PWc, terminal_condition, k.N, k.c, n2);
    int rc;
    for (int r = W - 1; r >= 0; r--) {
        if (W > 1 && (rc = enter_window(h, pcof, r, false))) return rc;
        const size_t nt = k.nt;
        if ((rc = forward_begin(h, pcof, n_pcof))) return rc;      // tables, L/R, inverses, propagators, block propagators
        { PhaseTimer t(h, "sweep_forward2"); K_TRY(h, qgdk_forward_finish(&k)); }      // (the super-block propagators)
        f.assign(nt * hstep, 0.0);
        if (forcing)
            for (size_t n = 0; n < nt; n++) pack_panel(f.data() + n * hstep, (int)PWc, forcing + ((size_t)k.n_off + n) * n2, k.N, k.c, ntg * n2);
        // (on the library's stream: behind the history pass, which writes the guard forcing of the window into this buffer)
        HIP_TRY(h, hipMemcpyAsync(k.forcing, f.data(), f.size() * sizeof(double), hipMemcpyHostToDevice, k.stream));
        HIP_TRY(h, hipStreamSynchronize(k.stream));         // (f is filled again for the next window)
        h->forcing_zero = false;
        if (r == W - 1) {      // y_N = L(t_N)^H lambda_N  (the terminal condition is lambda itself here, forward_evolution.jl:411-414)
            HIP_TRY(h, hipMemcpyAsync(k.lam + (nt - 1) * hstep, lamN.data(), hstep * sizeof(double), hipMemcpyHostToDevice, k.stream));
            K_TRY(h, qgdk_apply_LH(&k));
        } else {               // y at the end of this window = y at the start of the next one
            for (double *dst : {k.yhist + (nt - 1) * hstep, k.bndY + (size_t)k.scan_blocks * hstep, k.bndY2 + (size_t)k.scan_blocks2 * hstep})
                HIP_TRY(h, hipMemcpyAsync(dst, h->carry_y, hstep * sizeof(double), hipMemcpyDeviceToDevice, k.stream));
        }
        if ((rc = adjoint_begin(h))) return rc;
        { PhaseTimer t(h, "sweep_adjoint2"); K_TRY(h, qgdk_adjoint_finish(&k)); }
        { PhaseTimer t(h, "lambda"); K_TRY(h, qgdk_lambda(&k)); }
        if ((rc = check_status(h))) return rc;
        if (r == W - 1)      // lambda_N is the given one (not L_N^-H L_N^H of it)
            HIP_TRY(h, hipMemcpyAsync(k.lam + (nt - 1) * hstep, lamN.data(), hstep * sizeof(double), hipMemcpyHostToDevice, k.stream));
        // (with qgd_set_lambda_derivatives the reference's derivative columns too, forward_evolution.jl:427-433, :471-480)
        // (a resident grid downloads its zero-filled staging buffer whole: time index 0 stays zero)
        rc = lambda_history_out(h, lambda_history);
        const int rc2 = finish_copies(h);      // (a resident grid's download is left running)
        if (rc || rc2) return rc ? rc : rc2;
        if (r > 0) HIP_TRY(h, hipMemcpyAsync(h->carry_y, k.yhist, hstep * sizeof(double), hipMemcpyDeviceToDevice, k.stream));
    }
    HIP_TRY(h, hipStreamSynchronize(k.stream));
    return QGD_OK;
}


int qgd_apply_hamiltonian(qgd_handle h, int32_t time_index, int32_t deriv_order, int32_t use_adjoint,
                          const double *in, double *out)
{
    if (!in || !out) return fail(h, QGD_ERR_ARGUMENT, "null argument");
    ENTER(h);
    qgdk_ctx &k = h->k;
    NEEDS_RESIDENT_GRID(h, "qgd_apply_hamiltonian");
    if (time_index < 0 || time_index >= k.nt || deriv_order < 0 || deriv_order > k.m)
        return fail(h, QGD_ERR_ARGUMENT, "time index or derivative order out of range");
    const size_t PWc = 2 * k.cp, cnt = (size_t)k.Np * PWc;
    std::vector<double> p(cnt, 0.0), q(cnt, 0.0);
    pack_panel(p.data(), (int)PWc, in, k.N, k.c, (size_t)2 * k.N);
    double *din = nullptr, *dout = nullptr;
    HIP_TRY(h, hipMalloc((void **)&din, cnt * sizeof(double)));
    HIP_TRY(h, hipMalloc((void **)&dout, cnt * sizeof(double)));
    HIP_TRY(h, hipMemcpy(din, p.data(), cnt * sizeof(double), hipMemcpyHostToDevice));
    int kr = qgdk_apply(&k, din, dout, time_index, deriv_order, use_adjoint ? -1.0 : 1.0);
    hipError_t e = hipStreamSynchronize(k.stream);
    if (!kr && e == hipSuccess) e = hipMemcpy(q.data(), dout, cnt * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(din); (void)hipFree(dout);
    if (kr || e != hipSuccess) return fail(h, QGD_ERR_NO_DEVICE, "apply kernel failed");
    unpack_panel(out, (size_t)2 * k.N, q.data(), (int)PWc, k.N, k.c);
    return QGD_OK;
}


int qgd_get_intermediate(qgd_handle h, const char *name, double *out, size_t capacity, size_t *needed)
{
    if (!name) return fail(h, QGD_ERR_ARGUMENT, "null argument");
    ENTER(h, ENTER_KEEPS_GRAPH);
    qgdk_ctx &k = h->k;
    const size_t Np = k.Np, N = k.N, nt = k.nt, PW = 2 * Np, panel = Np * PW, pl = Np * Np;
    std::string s(name);
    size_t need = 0;
    if (s == "L" || s == "R" || s == "Linv" || s == "P") need = nt * N * N * 2;
    else if (s == "sigma") need = nt * (size_t)k.n_ops * k.m * 2;
    else if (s == "tables") need = nt * (size_t)(k.m + 1) * k.n_ops * 2;
    else if (s == "repivoted") need = 1;
    else if (s == "selection") need = 4;
    else if (s == "small_path") need = 1;
    else if (s == "front_path") need = 1;
    else if (s == "batch_path") need = 1;
    else if (s == "column_overlaps") need = (size_t)k.c * 2;
    else return fail(h, QGD_ERR_ARGUMENT, "unknown intermediate '" + s + "'");
    if (needed) *needed = need;
    if (!out) return QGD_OK;
    if (capacity < need) return fail(h, QGD_ERR_ARGUMENT, "buffer too small");
    if (s == "small_path") { out[0] = h->sweep.kind == SWEEP_SMALL ? 1.0 : 0.0; return QGD_OK; }
    if (s == "front_path") { out[0] = h->sweep.front ? 1.0 : 0.0; return QGD_OK; }
    if (s == "batch_path") { out[0] = h->batch_path ? 1.0 : 0.0; return QGD_OK; }
    if (s == "selection") {      // which kernel families this problem runs on (tests assert that a shape selects what it is meant to)
        out[0] = k.use_sparse ? 2.0 : (k.dense_gemm ? 1.0 : 0.0);      // 2 sparse (ELL), 1 N > 64 GEMM-style kernels, 0 dense N <= 64
        out[1] = (k.dense_gemm && !k.use_sparse) ? (double)qgdk_dense_sigma_form(&k) : -1.0;
        out[2] = (k.dense_gemm && k.binv) ? 1.0 : 0.0;               // block Gauss-Jordan inverse over 64-column blocks
        out[3] = (double)h->chunks_eff;
        return QGD_OK;
    }
    if (s == "column_overlaps") {      // refused from the handle's state alone, before anything is launched
        if (h->chunks_eff > 1 || h->part_world != 1 || k.part_world != 1 || h->comm)
            return fail(h, QGD_ERR_UNSUPPORTED, "qgd_get_intermediate(\"column_overlaps\") needs the whole time grid resident on one handle");
        if (!k.have_target) return fail(h, QGD_ERR_STATE, "qgd_set_target must be called before qgd_get_intermediate(\"column_overlaps\")");
        if (h->sweep.kind == SWEEP_NONE) return fail(h, QGD_ERR_STATE, "no stored forward sweep for qgd_get_intermediate(\"column_overlaps\") (none yet, or a batch since)");
    }
    NEEDS_RESIDENT_GRID(h, "qgd_get_intermediate");
    const bool matrices = s == "L" || s == "R" || s == "Linv" || s == "P";
    if ((h->sweep.kind == SWEEP_SMALL && s != "repivoted") || (h->sweep.front && h->sweep.has_pcof && matrices)) {
        // the small-problem path keeps no intermediates, the front's step matrices are the same-point form's (L^H, R^H, L^-H,
        // S): the evaluation once more on the general path (diagnostics only; the copy: run_forward records its pcof)
        const std::vector<double> pc = h->sweep.pcof;
        const bool adjoint = h->sweep.kind == SWEEP_SMALL && h->sweep.gradient && k.have_target;
        int rcs = run_forward(h, pc.data(), (int)pc.size());
        if (!rcs && adjoint) { rcs = adjoint_begin(h); if (!rcs) rcs = adjoint_end(h); }
        if (rcs) return rcs;
    }
    HIP_TRY(h, hipStreamSynchronize(k.stream));
    if (s == "repivoted") {     // last inverse launch: matrices not done by the first attempt + 65536 * (N = 64: matrices that went on to the
                                // fully pivoted elimination); qgd_inverse_cb.h, qgd_k_dense.hip
        int v[3] = {0, 0, 0};
        HIP_TRY(h, hipMemcpy(v, k.status, 3 * sizeof(int), hipMemcpyDeviceToHost));
        out[0] = (double)v[1] + 65536.0 * (double)v[2];
        return QGD_OK;
    }
    if (s == "sigma") {      // (the column groups' planes of the N <= 64 gradient kernels are summed here)
        const bool planes = true;      // (every gradient kernel stores one plane per contributing workgroup)
        const int nplanes = k.dense_gemm ? qgdk_dense_sigma_planes(&k) : k.cp / 8;
        HIP_TRY(h, hipMemcpy(out, k.sigma, need * sizeof(double), hipMemcpyDeviceToHost));
        std::vector<double> pl_(need);
        for (int g = 1; planes && g < nplanes; g++) {
            HIP_TRY(h, hipMemcpy(pl_.data(), k.sigma + (size_t)g * need, need * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t e = 0; e < need; e++) out[e] += pl_[e];
        }
        return QGD_OK;
    }
    if (s == "column_overlaps") {      // (a_j, b_j) of the stored final state against the target, whatever the cost type
        K_TRY(h, qgdk_column_overlaps(&k));
        HIP_TRY(h, hipMemcpyAsync(out, k.colab, need * sizeof(double), hipMemcpyDeviceToHost, k.stream));
        HIP_TRY(h, hipStreamSynchronize(k.stream));
        return QGD_OK;
    }
    if (s == "tables") { HIP_TRY(h, hipMemcpy(out, k.tab, need * sizeof(double), hipMemcpyDeviceToHost)); return QGD_OK; }
    memset(out, 0, need * sizeof(double));
    if (s == "Linv") {
        std::vector<double> b(nt * 2 * pl);
        HIP_TRY(h, hipMemcpy(b.data(), k.LinvT, b.size() * sizeof(double), hipMemcpyDeviceToHost));   // row-major planes
        for (size_t n = 1; n < nt; n++) for (size_t r = 0; r < N; r++) for (size_t c = 0; c < N; c++) {
            out[((n * N + r) * N + c) * 2] = b[n * 2 * pl + r * Np + c];
            out[((n * N + r) * N + c) * 2 + 1] = b[n * 2 * pl + pl + r * Np + c];
        }
        return QGD_OK;
    }
    const double *src = (s == "L") ? k.L : (s == "R") ? k.R : k.Pr;
    const size_t cnt = (s == "P") ? nt - 1 : nt;
    std::vector<double> b(cnt * panel);
    HIP_TRY(h, hipMemcpy(b.data(), src, b.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t n = 0; n < cnt; n++) for (size_t r = 0; r < N; r++) for (size_t c = 0; c < N; c++) {
        size_t o = n * panel + panel_index((int)r, (int)c, (int)PW);
        out[((n * N + r) * N + c) * 2] = b[o];
        out[((n * N + r) * N + c) * 2 + 1] = b[o + 8];
    }
    return QGD_OK;
}


int qgd_exchange_buffer(qgd_handle h, int32_t which, void **dev_ptr, size_t *total_doubles, size_t *own_offset,
                        size_t *own_doubles)
{
    if (!dev_ptr || !total_doubles || !own_offset || !own_doubles) return QGD_ERR_ARGUMENT;
    ENTER(h, ENTER_KEEPS_GRAPH);
    const qgdk_ctx &k = h->k;
    const size_t pl = (size_t)k.Np * k.Np, hstep = (size_t)k.Np * 2 * k.cp, W = (size_t)k.part_world;
    if (which == 0) {          // block propagators, all-gather
        const size_t chunk = (size_t)4 * pl;               // [R planes | R panel] of one window
        *dev_ptr = k.RX; *total_doubles = W * chunk; *own_offset = (size_t)k.part_rank * chunk; *own_doubles = chunk;
    } else if (which == 1) {   // affine parts + y_N, all-gather
        const size_t chunk = (size_t)2 * hstep;            // [phi^rank | y_N]
        *dev_ptr = k.phiRX; *total_doubles = W * chunk; *own_offset = (size_t)k.part_rank * chunk; *own_doubles = chunk;
    } else if (which == 2) {   // gradient + scalars, all-reduce(sum)
        if (!k.redbuf) return fail(h, QGD_ERR_STATE, "no control basis set");
        *dev_ptr = k.redbuf; *total_doubles = (size_t)k.n_pcof + 4; *own_offset = 0; *own_doubles = (size_t)k.n_pcof + 4;
    } else if (which == 3) {   // column shards: the three objective scalars at the turnaround, all-reduce(sum)
        if (!k.redbuf) return fail(h, QGD_ERR_STATE, "no control basis set");
        *dev_ptr = k.scal; *total_doubles = 3; *own_offset = 0; *own_doubles = 3;
    } else return fail(h, QGD_ERR_ARGUMENT, "unknown exchange buffer");
    return QGD_OK;
}


int qgd_dist_forward_begin(qgd_handle h, const double *pcof, int32_t n_pcof)
{
    ENTER(h, ENTER_KEEPS_GRAPH);
    if (!h->have_basis) return fail(h, QGD_ERR_STATE, "qgd_set_control_basis must be called first");
    return forward_begin(h, pcof, n_pcof);
}


int qgd_dist_forward_end(qgd_handle h)
{
    ENTER(h, ENTER_KEEPS_GRAPH | ENTER_NO_GRID);
    const int rc = forward_end(h);
    if (!rc) sweep_done(h, SWEEP_GENERAL, nullptr, 0);      // (no pcof: a partitioned handle never reuses its sweep, qgd_discrete_adjoint refuses it)
    return rc;
}


int qgd_dist_adjoint_begin(qgd_handle h)
{
    ENTER(h, ENTER_KEEPS_GRAPH | ENTER_NO_GRID);
    if (!h->k.have_target) return fail(h, QGD_ERR_STATE, "qgd_set_target must be called first");
    if (!sweep_stored(h)) return fail(h, QGD_ERR_STATE, "no forward evaluation to differentiate (qgd_dist_forward_* first)");
    return adjoint_begin(h);
}


int qgd_dist_adjoint_end(qgd_handle h)
{
    ENTER(h, ENTER_KEEPS_GRAPH | ENTER_NO_GRID);
    return adjoint_end(h);
}


int qgd_dist_finish(qgd_handle h, double *grad, double *out3)
{
    ENTER(h, ENTER_KEEPS_GRAPH | ENTER_NO_GRID);
    return fetch_results(h, grad, out3);
}


// ---------------------------------------------------------------------------
// Column-sharded evaluation: the reference's own parallel axis (Threads.@threads over initial conditions,
// src/forward_evolution.jl:48,332) and the split BASELINE.json's north star sketches.  Every rank's handle is built
// from ITS columns of u0, v0 and the target, with the global N_ess.  Everything is independent per column except the
// overlaps <w_N,R>, <w_N,T> in the terminal condition (global sums, infidelity.jl:13-17): one all-reduce of three
// scalars at the turnaround, one of [grad | scalars] at the end.  The propagator build is replicated on every rank --
// that is why time windows are the default split.
// ---------------------------------------------------------------------------
int qgd_cols_forward(qgd_handle h, const double *pcof, int32_t n_pcof)
{
    if (!pcof) return fail(h, QGD_ERR_ARGUMENT, "null argument");
    ENTER(h, ENTER_KEEPS_GRAPH);
    if (!h->k.have_target) return fail(h, QGD_ERR_STATE, "qgd_set_target must be called first");
    if (!h->have_basis) return fail(h, QGD_ERR_STATE, "qgd_set_control_basis must be called first");
    if (h->k.cost_type == QGD_COST_STATE_TRANSFER) return fail(h, QGD_ERR_UNSUPPORTED, COLUMN_SHARD_STATE_TRANSFER);
    return run_forward(h, pcof, n_pcof);        // scal = this rank's <w,R>, <w,T>, guard: exchange buffer 3
}


int qgd_cols_adjoint(qgd_handle h, int32_t keep_scalars)
{
    ENTER(h, ENTER_KEEPS_GRAPH | ENTER_NO_GRID);
    qgdk_ctx &k = h->k;
    if (k.cost_type == QGD_COST_STATE_TRANSFER) return fail(h, QGD_ERR_UNSUPPORTED, COLUMN_SHARD_STATE_TRANSFER);
    if (!sweep_stored(h)) return fail(h, QGD_ERR_STATE, "no forward evaluation to differentiate (qgd_cols_forward first)");
    { PhaseTimer t(h, "terminal"); K_TRY(h, qgdk_terminal_given(&k)); }      // y_N from the all-reduced overlaps
    int rc;
    if ((rc = adjoint_begin(h))) return rc;
    if ((rc = adjoint_end(h))) return rc;
    // the final all-reduce sums [grad | scalars]; the scalars are global already: all ranks but one contribute zeros
    if (!keep_scalars) HIP_TRY(h, hipMemsetAsync(k.scal, 0, 3 * sizeof(double), k.stream));
    return QGD_OK;
}

}  // extern "C"
