// qgd_host_sens.cpp -- host side of the C ABI (include/qgd.h), sensitivities of the state to the parameters: the forced gradient
// (eval_grad_forced.jl:17-194), the exact Hessian, Hessian-vector products (section 4d) and the pullback of
// trajectory outputs (sections 4g, 4j).  The first three share the forced gradient's buffers, and the two second-order entry points
// their refusals and their setup; the pullback runs the second-order adjoint's sweep with a forcing of the caller's, and the
// pullback of the dense output (section 4j) the same sweep behind the transposed interpolation.  qgd_eval_pushforward
// (qgd_host_pushforward.cpp) takes the pullbacks' refusals behind the prologue and their forward sweep from here.
#include "qgd_host.h"

using namespace qgdh;

// the forced gradient's pool for (up to) nt time points and B scan blocks: its key and its plan
static KeyedPlan forced_plan(qgd_handle h, size_t nt, size_t B)
{
    qgdk_ctx &k = h->k;
    const size_t hstep = (size_t)k.Np * 2 * k.cp, NB = (size_t)k.n_ops * 2 * k.m;
    const size_t cpS = (size_t)k.n_pcof * k.cp, hstepS = (size_t)k.Np * 2 * cpS;
    return {{nt, (size_t)k.n_pcof, B}, {
        {&k.fs_BR, nt * NB * hstep}, {&k.fs_BL, nt * NB * hstep}, {&k.fs_phi, B * hstepS}, {&k.fs_bnd, (B + 1) * hstepS},
        {&k.fs_gacc, (size_t)k.n_pcof + 1},
        // (the 2m+2 work panels of k_forced_basis: LDS up to 150 KB, else an HBM slab per workgroup)
        {&h->fsc_forced, nt * (size_t)(k.cp / 8) * (size_t)(2 * k.m + 2) * k.Np * 16, qgdk_forced_lds(k.Np, k.m) > 150 * 1024}}};
}

namespace qgdh {

int forced_buffers(qgd_handle h, size_t nt, size_t B)
{
    const int rc = pool_ensure(h, h->pools[POOL_FORCED], forced_plan(h, nt, B));
    if (!rc) h->k.fs_scratch = h->fsc_forced;
    return rc;
}

// QGD_ERR_MEMORY of a second-order entry point (and of qgd_eval_pushforward) is decided from what ITS call allocates: its own plan
// and, when they are not there under the right key, the forced gradient's buffers -- these bytes
size_t forced_missing(qgd_handle h) { return pool_missing(h->pools[POOL_FORCED], forced_plan(h, (size_t)h->k.nt, (size_t)h->k.scan_blocks)); }

}  // namespace qgdh


// what both second-order entry points refuse once they have entered (`name`: the entry point, `what`: its result, for the messages)
static int second_order_refusals(qgd_handle h, const double *pcof, int n_pcof, const std::string &name, const char *what)
{
    const qgdk_ctx &k = h->k;
    if (h->part_world != 1 || h->comm) return fail(h, QGD_ERR_STATE, std::string("partitioned handle: ") + what + " is single-GPU");
    if (!k.have_target) return fail(h, QGD_ERR_STATE, "qgd_set_target must be called before " + name);
    if (!h->have_basis) return fail(h, QGD_ERR_STATE, "qgd_set_control_basis must be called before " + name);
    if (!pcof) return fail(h, QGD_ERR_UNSUPPORTED, name + " needs pcof: with control tables set directly the second derivative of the controls is unknown");
    if (n_pcof != k.n_pcof) return fail(h, QGD_ERR_ARGUMENT, "length of pcof does not match the control basis");
    if (h->chunks_eff > 1) return fail(h, QGD_ERR_UNSUPPORTED, name + " needs the whole time grid resident (this handle processes it in windows)");
    if (k.N > 64) return fail(h, QGD_ERR_UNSUPPORTED, name + " supports N <= 64");
    if (k.n_ops < 1 || k.n_ops * 2 * k.m > 64) return fail(h, QGD_ERR_UNSUPPORTED, name + " needs 1 <= 2 * n_ops * order/2 <= 64 basis directions");
    return QGD_OK;
}


// what both second-order entry points start from: the forward sweep on the general two-point path, lambda (and the adjoint
// gradient), the stage derivatives, the forced gradient's buffers and the forced basis responses in them (fs_BR, fs_BL)
static int second_order_setup(qgd_handle h, const double *pcof, int n_pcof)
{
    qgdk_ctx &k = h->k;
    int rc;
    if ((rc = run_forward(h, pcof, n_pcof))) return rc;
    if ((rc = adjoint_begin(h))) return rc;
    if ((rc = adjoint_end(h))) return rc;
    if (!h->sweep.derivs) { PhaseTimer t(h, "derivs"); K_TRY(h, qgdk_derivs(&k)); h->sweep.derivs = true; }
    if ((rc = forced_buffers(h, (size_t)k.nt, (size_t)k.scan_blocks))) return rc;
    { PhaseTimer t(h, "forced_basis"); K_TRY(h, qgdk_forced_basis(&k)); }
    h->sweep.forced_basis = true;
    return QGD_OK;
}


// <s,R> and <s,T>, T = [R_im; -R_re] (infidelity.jl:13-17), of a host array s [2N x c] with the target
static void target_overlaps(qgd_handle h, const double *s, double &sR, double &sT)
{
    const size_t N = h->k.N, c = h->k.c;
    const double *R = h->target_host.data();
    double aR = 0.0, aT = 0.0;      // (sums in registers: the references may alias the arrays)
    for (size_t col = 0; col < c; col++)
        for (size_t i = 0; i < N; i++) {
            const size_t e = i + 2 * N * col;
            const double sre = s[e], sim = s[N + e], rre = R[e], rim = R[N + e];
            aR += sre * rre + sim * rim;
            aT += sre * rim - sim * rre;
        }
    sR = aR; sT = aT;
}


// the same column by column (:StateTransfer): sR[col], sT[col] = <s_col,R_col>, <s_col,T_col>
static void column_target_overlaps(qgd_handle h, const double *s, double *sR, double *sT)
{
    const size_t N = h->k.N, c = h->k.c;
    const double *R = h->target_host.data();
    for (size_t col = 0; col < c; col++) {
        double aR = 0.0, aT = 0.0;
        for (size_t i = 0; i < N; i++) {
            const size_t e = i + 2 * N * col;
            const double sre = s[e], sim = s[N + e], rre = R[e], rim = R[N + e];
            aR += sre * rre + sim * rim;
            aT += sre * rim - sim * rre;
        }
        sR[col] = aR; sT[col] = aT;
    }
}


// The terminal part of the forced gradient from s_N, the sensitivities of the final state to every parameter (sN_dev: panels
// with parameter p in columns p * cp ..), plus the guard part the forced sweeps accumulated in fs_gacc (grad may be NULL):
//   :Infidelity  -(2/N_ess^2) (<w_N,R> <s_N,R> + <w_N,T> <s_N,T>)
//   :Tracking    d(0.5 |w_N - R|^2) = <s_N, w_N - R>;  :Norm  d(0.5 |w_N|^2) = <s_N, w_N>  (eval_grad_forced.jl:160-163)
//   :StateTransfer  -(2/c) sum_j (a_j <s_j,R_j> + b_j <s_j,T_j>) with the overlaps a_j, b_j of column j of w_N
// Also returns what the Hessian's terminal part is made of: the overlaps, and with keep_s s_N itself as [2N x c] per parameter.
struct ForcedTerminal {
    double f = 0.0;                 // -2 / N_ess^2
    std::vector<double> sR, sT;     // <s_N,R>, <s_N,T> of every parameter
    std::vector<double> cR, cT;     // (:StateTransfer; f is then -2 / c) the same column by column: parameter p, column j at p * c + j
    std::vector<double> s;          // (keep_s) s_N of parameter p at p * 2N * c
};

static int forced_terminal(qgd_handle h, const double *sN_dev, double *grad, ForcedTerminal &t, bool keep_s = false)
{
    qgdk_ctx &k = h->k;
    const size_t np = (size_t)k.n_pcof, N = k.N, L = 2 * N * k.c, hstep = (size_t)k.Np * 2 * k.cp, PWs = 2 * np * k.cp;
    std::vector<double> sN((size_t)k.Np * PWs), gacc(np), scal(4), d, s_one(L);
    HIP_TRY(h, hipMemcpy(sN.data(), sN_dev, sN.size() * sizeof(double), hipMemcpyDeviceToHost));
    const bool per_col = k.cost_type == QGD_COST_STATE_TRANSFER;
    const size_t nc = (size_t)k.c;
    std::vector<double> wa(per_col ? nc : 0), wb(per_col ? nc : 0);
    if (k.cost_type) {     // :Tracking / :Norm need the final state itself: d = w_N - R, or w_N; :StateTransfer its column overlaps
        std::vector<double> wN(hstep);
        HIP_TRY(h, hipMemcpy(wN.data(), k.hist + ((size_t)k.nt - 1) * hstep, hstep * sizeof(double), hipMemcpyDeviceToHost));
        d.resize(L);
        unpack_panel(d.data(), 2 * N, wN.data(), 2 * k.cp, k.N, k.c);
        if (k.cost_type == QGD_COST_TRACKING) for (size_t e = 0; e < L; e++) d[e] -= h->target_host[e];
        if (per_col) column_target_overlaps(h, d.data(), wa.data(), wb.data());
    }
    HIP_TRY(h, hipMemcpy(gacc.data(), k.fs_gacc, sizeof(double) * np, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(scal.data(), k.scal, 3 * sizeof(double), hipMemcpyDeviceToHost));
    const double a = scal[0], b = scal[1];
    t.f = per_col ? -2.0 / (double)k.c : -2.0 / ((double)k.n_ess * k.n_ess);
    t.sR.assign(np, 0.0); t.sT.assign(np, 0.0); t.s.assign(keep_s ? np * L : 0, 0.0);
    t.cR.assign(per_col ? np * nc : 0, 0.0); t.cT.assign(per_col ? np * nc : 0, 0.0);
    for (size_t p = 0; p < np; p++) {
        double *s = keep_s ? t.s.data() + p * L : s_one.data();
        unpack_panel(s, 2 * N, sN.data() + 2 * p * k.cp, (int)PWs, k.N, k.c);
        target_overlaps(h, s, t.sR[p], t.sT[p]);
        double sW = 0.0;
        if (per_col) {
            column_target_overlaps(h, s, t.cR.data() + p * nc, t.cT.data() + p * nc);
            for (size_t col = 0; col < nc; col++) sW += wa[col] * t.cR[p * nc + col] + wb[col] * t.cT[p * nc + col];
            if (grad) grad[p] = t.f * sW + gacc[p];
            continue;
        }
        for (size_t col = 0; k.cost_type && col < (size_t)k.c; col++)
            for (size_t i = 0; i < N; i++) {
                const size_t e = i + 2 * N * col;
                sW += s[e] * d[e] + s[N + e] * d[N + e];
            }
        if (grad) grad[p] = (k.cost_type ? sW : t.f * (a * t.sR[p] + b * t.sT[p])) + gacc[p];
    }
    return QGD_OK;
}


// buffers of qgd_eval_hessian for the present grid, basis and guard kind
static int hess_buffers(qgd_handle h)
{
    qgdk_ctx &k = h->k;
    const size_t nt = k.nt, np = (size_t)k.n_pcof, NB = (size_t)k.n_ops * 2 * k.m, gpc = (size_t)k.cp / 8;
    const size_t hstep = (size_t)k.Np * 2 * k.cp, n_shist = nt * (size_t)k.Np * 2 * np * k.cp, n_ws = k.have_guard == 1 ? n_shist : 0;
    auto &b = h->hs;
    return pool_ensure(h, h->pools[POOL_HESS], {{nt, np, NB, (size_t)(n_ws != 0)}, {
        {&b.shist, n_shist}, {&b.ws, n_ws, n_ws != 0}, {&b.Z, nt * NB * hstep}, {&b.half, nt * gpc * NB * NB},
        {&b.slab, nt * gpc * qgdk_hess_slab(k.Np, k.m, k.n_ops)}, {&b.zt, nt * NB * np},
        {&b.Y, 2 * np * np + (k.have_guard ? qgdk_hess_gram_part((int)np, (int)nt) : 0)}}},
        "the sensitivity history of qgd_eval_hessian does not fit", forced_missing(h));
}


// buffers of qgd_eval_hessian_vec for the present grid, basis and guard kind (nothing depends on the number of parameters but
// three vectors)
static int hvp_buffers(qgd_handle h)
{
    qgdk_ctx &k = h->k;
    const size_t nt = k.nt, np = (size_t)k.n_pcof, NB = (size_t)k.n_ops * 2 * k.m, gpc = (size_t)k.cp / 8, B = (size_t)k.scan_blocks;
    const size_t hstep = (size_t)k.Np * 2 * k.cp, hist = nt * hstep, n_ws = k.have_guard == 1 ? hist : 0, n_gv = qgdk_hvp_gv_len(&k);
    const std::vector<size_t> key = {nt, np, NB, (size_t)(n_ws != 0), B};
    if (h->pools[POOL_HVP].key != key) hvp_void(h);
    auto &b = h->hv;
    return pool_ensure(h, h->pools[POOL_HVP], {key, {
        {&b.Z, nt * NB * hstep}, {&b.half, nt * gpc * NB * NB}, {&b.slab, nt * gpc * qgdk_hess_slab(k.Np, k.m, k.n_ops)},
        {&b.sv, hist}, {&b.F, hist}, {&b.Y, hist}, {&b.mu, hist}, {&b.ws, n_ws, n_ws != 0}, {&b.phi, B * hstep},
        {&b.bnd, (B + 1) * hstep}, {&b.gvt, n_gv}, {&b.term, hstep}, {&b.part, nt * gpc * NB}, {&b.v, np}, {&b.gB, np},
        {&b.out, np}, {&b.scal, 4}, {&b.one3, 2}}},
        "the buffers of qgd_eval_hessian_vec do not fit", forced_missing(h), [&]() -> int {
        // s_v(0) = 0 and mu_0 = 0 are never written again; the unused (M+1)-th Taylor slot of the direction table stays zero
        const struct { int64_t goff; int32_t ncoef, poff; } one = {0, 1, 0};      // the one-operator, one-coefficient basis of the direction table
        HIP_TRY(h, hipMemcpyAsync(b.one3, &one, sizeof(one), hipMemcpyHostToDevice, k.stream));
        HIP_TRY(h, hipMemsetAsync(b.sv, 0, hist * sizeof(double), k.stream));
        HIP_TRY(h, hipMemsetAsync(b.mu, 0, hist * sizeof(double), k.stream));
        HIP_TRY(h, hipMemsetAsync(b.Y, 0, hist * sizeof(double), k.stream));
        HIP_TRY(h, hipMemsetAsync(b.bnd, 0, (B + 1) * hstep * sizeof(double), k.stream));
        HIP_TRY(h, hipMemsetAsync(b.gvt, 0, n_gv * sizeof(double), k.stream));
        HIP_TRY(h, hipMemsetAsync(b.scal, 0, 4 * sizeof(double), k.stream));
        HIP_TRY(h, hipStreamSynchronize(k.stream));      // (`one` leaves scope)
        return QGD_OK;
    });
}


// Phi'' s_v(N) as the terminal part of the second-order adjoint's right-hand side F = -f, in panel layout:
//   :Infidelity  +(2/N_ess^2) (<s_v,R> R + <s_v,T> T);   :Tracking / :Norm  -s_v(N);
//   :StateTransfer  +(2/c) (<s_j,R_j> R_j + <s_j,T_j> T_j) column by column
static int hvp_terminal(qgd_handle h, const double *svN_dev, double *term_dev)
{
    qgdk_ctx &k = h->k;
    const size_t N = k.N, PWc = 2 * (size_t)k.cp, hstep = (size_t)k.Np * PWc, L = 2 * N * k.c;
    std::vector<double> sN(hstep), s(L), t(L), out(hstep, 0.0);
    HIP_TRY(h, hipMemcpyAsync(sN.data(), svN_dev, hstep * sizeof(double), hipMemcpyDeviceToHost, k.stream));
    HIP_TRY(h, hipStreamSynchronize(k.stream));
    unpack_panel(s.data(), 2 * N, sN.data(), (int)PWc, k.N, k.c);
    if (k.cost_type && k.cost_type != QGD_COST_STATE_TRANSFER) {
        for (size_t e = 0; e < L; e++) t[e] = -s[e];
    } else {
        const bool per_col = k.cost_type == QGD_COST_STATE_TRANSFER;
        std::vector<double> cR(k.c), cT(k.c);
        double sR = 0.0, sT = 0.0;
        if (per_col) column_target_overlaps(h, s.data(), cR.data(), cT.data());
        else target_overlaps(h, s.data(), sR, sT);
        const double f = per_col ? 2.0 / (double)k.c : 2.0 / ((double)k.n_ess * k.n_ess);
        for (size_t col = 0; col < (size_t)k.c; col++)
            for (size_t i = 0; i < N; i++) {
                if (per_col) { sR = cR[col]; sT = cT[col]; }
                const size_t e = i + 2 * N * col;
                const double rre = h->target_host[e], rim = h->target_host[N + e];
                t[e] = f * (sR * rre + sT * rim);            // T = [R_im; -R_re]
                t[N + e] = f * (sR * rim - sT * rre);
            }
    }
    pack_panel(out.data(), (int)PWc, t.data(), k.N, k.c, 2 * N);
    HIP_TRY(h, hipMemcpyAsync(term_dev, out.data(), hstep * sizeof(double), hipMemcpyHostToDevice, k.stream));
    HIP_TRY(h, hipStreamSynchronize(k.stream));      // (`out` leaves scope)
    return QGD_OK;
}


// The pool of a pullback entry point for the present grid and basis and the sizes of this call's uploads (doubles; 0: not given).
// Its key: the entry point's `key`, then those five sizes.  Its plan: the entry point's `plan`, F, Y, mu, its `mid`, then the rest
// of PullbackBufs (qgd_eval_pullback has neither `plan` nor `mid`).
static int pullback_buffers(qgd_handle h, Pool &pool, qgd_handle_s::PullbackBufs &b, std::vector<size_t> key, const OutputSizes &z, const char *fit,
                            std::vector<Buf> plan = {}, const std::vector<Buf> &mid = {})
{
    qgdk_ctx &k = h->k;
    const size_t hist = (size_t)k.nt * k.Np * 2 * k.cp, np = (size_t)k.n_pcof;
    key.insert(key.end(), {z.states, z.pops, z.map, z.expect, z.planes});
    plan.insert(plan.end(), {{&b.F, hist}, {&b.Y, hist}, {&b.mu, hist}});
    plan.insert(plan.end(), mid.begin(), mid.end());
    plan.insert(plan.end(), {{&b.gB, np}, {&b.scal, 4}, {&b.sbar, z.states, z.states != 0}, {&b.pbar, z.pops, z.pops != 0},
                             {&b.map, z.map, z.map != 0}, {&b.ebar, z.expect, z.expect != 0}, {&b.planes, z.planes, z.planes != 0}});
    return pool_ensure(h, pool, {key, plan}, fit, 0, [&]() -> int {
        // mu_0 and y_0 are never written; the kernels write every panel and entry of the other work buffers on every call
        HIP_TRY(h, hipMemsetAsync(b.mu, 0, hist * sizeof(double), k.stream));
        HIP_TRY(h, hipMemsetAsync(b.Y, 0, hist * sizeof(double), k.stream));
        HIP_TRY(h, hipMemsetAsync(b.scal, 0, 4 * sizeof(double), k.stream));
        return QGD_OK;
    });
}


// The context of a second-order adjoint sweep: a copy of the handle's with the sweep's forcing, y, mu, gradient and scalars in
// buffers of its own, so that lambda, the guard forcing and the scalars of the kept evaluation stay as they are
static qgdk_ctx adjoint_context(const qgdk_ctx &k, double *F, double *Y, double *mu, double *gB, double *scal)
{
    qgdk_ctx a = k;
    a.forcing = F; a.yhist = Y; a.lam = mu; a.grad = gB; a.scal = scal;
    a.front = 0; a.fuse_terminal = 0; a.grad_accumulate = 0; a.mirror_dev = nullptr; a.mirror_ticket = nullptr;
    return a;
}


namespace qgdh {

// what the pullbacks and qgd_eval_pushforward refuse once they have entered (`name`: the entry point, `what`: "pullback" or
// "pushforward", for the messages; basis_bound: the forced scan's bound on the basis directions applies)
int trajectory_refusals(qgd_handle h, const std::string &name, const char *what, const double *pcof, int n_pcof, int history_precomputed, bool basis_bound)
{
    const qgdk_ctx &k = h->k;
    if (!h->have_basis) return fail(h, QGD_ERR_STATE, "qgd_set_control_basis must be called before " + name);
    if (h->part_world != 1 || h->comm) return fail(h, QGD_ERR_STATE, std::string("partitioned handle: the ") + what + " is single-GPU");
    if (pcof && n_pcof != k.n_pcof) return fail(h, QGD_ERR_ARGUMENT, "length of pcof does not match the control basis");
    if (h->chunks_eff > 1) return fail(h, QGD_ERR_UNSUPPORTED, name + " needs the whole time grid resident (this handle processes it in windows)");
    if (k.N > 64) return fail(h, QGD_ERR_UNSUPPORTED, name + " supports N <= 64");
    if (k.n_ops < 1) return fail(h, QGD_ERR_UNSUPPORTED, name + " needs control operators");
    if (basis_bound && k.n_ops * 2 * k.m > 64) return fail(h, QGD_ERR_UNSUPPORTED, name + " needs 2 * n_ops * order/2 <= 64 basis directions");
    if (!pcof && !h->have_tables) return fail(h, QGD_ERR_STATE, "no control tables: call qgd_set_control_tables or pass pcof");
    return refuse_reuse(h, history_precomputed);
}

// their forward sweep: the general two-point one unless history_precomputed finds one of the same pcof, and the stage derivatives
int pullback_sweep(qgd_handle h, const double *pcof, int n_pcof, int history_precomputed)
{
    int rc;
    if (!(history_precomputed && h->sweep.kind == SWEEP_GENERAL && sweep_reusable(h, pcof, n_pcof)) && (rc = run_forward(h, pcof, n_pcof))) return rc;
    if (!h->sweep.derivs) { PhaseTimer t(h, "derivs"); K_TRY(h, qgdk_derivs(&h->k)); h->sweep.derivs = true; }
    return QGD_OK;
}

}  // namespace qgdh


// The arguments of a pullback entry point (`name`: for the messages; sel: the outputs whose cotangent is given), what both entry
// points refuse from them alone, in front of ENTER, and the steps they share around their forcing kernels: the uploads and the
// forward sweep (the pool `b` is ensured), and the adjoint sweep with the forcing in b.F, the gradient kernels with mu in place
// of lambda -- the dense pullback then accumulates its explicit part -- the status and the download.
struct PullbackCall {
    const char *name;
    const double *pcof; int32_t n_pcof, history_precomputed;
    const double *states_bar, *pop_bar, *expect_bar;
    OutputSelection sel;
    double *grad;
};

static int pullback_arguments(qgd_handle h, const PullbackCall &p)
{
    if (!p.grad) return fail(h, QGD_ERR_ARGUMENT, "null argument");
    if (!p.states_bar && !p.pop_bar && !p.expect_bar) return fail(h, QGD_ERR_ARGUMENT, std::string(p.name) + " needs at least one of states_bar, pop_bar, expect_bar");
    return selection_refusals(h, p.sel, "expect_bar");
}

static int pullback_begin(qgd_handle h, const PullbackCall &p, const OutputSizes &z, const qgd_handle_s::PullbackBufs &b)
{
    const struct { double *dst; const double *src; size_t n; } up[] = {{b.sbar, p.states_bar, z.states}, {b.pbar, p.pop_bar, z.pops}, {b.ebar, p.expect_bar, z.expect}};
    for (const auto &u : up)
        if (u.n) HIP_TRY(h, hipMemcpyAsync(u.dst, u.src, u.n * sizeof(double), hipMemcpyHostToDevice, h->k.stream));
    const int rc = upload_selection(h, p.sel, z, b.map, b.planes);
    return rc ? rc : pullback_sweep(h, p.pcof, p.n_pcof, p.history_precomputed);
}

static int pullback_end(qgd_handle h, const qgd_handle_s::PullbackBufs &b, double *grad, const qgd_handle_s::DensePullbackBufs *dense = nullptr)
{
    qgdk_ctx &k = h->k;
    const qgdk_ctx a = adjoint_context(k, b.F, b.Y, b.mu, b.gB, b.scal);
    { PhaseTimer t(h, dense ? "dense_pullback_adjoint" : "pullback_adjoint"); K_TRY(h, qgdk_hvp_adjoint(&a)); }
    { PhaseTimer t(h, dense ? "dense_pullback_gradient" : "pullback_gradient"); K_TRY(h, qgdk_gradient(&a)); }      // gB = the implicit part
    if (dense) {   // gB += the explicit part: k_contract over the planes of the column groups of the call's own sigma
        qgdk_ctx e = a;
        e.sigma = dense->sigma; e.cpart = dense->cpart; e.dense_gemm = 0; e.grad_accumulate = 1;
        PhaseTimer t(h, "dense_pullback_explicit");
        K_TRY(h, qgdk_contract(&e));
    }
    int rc;
    if ((rc = check_status(h))) return rc;
    HIP_TRY(h, hipMemcpyAsync(grad, b.gB, (size_t)k.n_pcof * sizeof(double), hipMemcpyDeviceToHost, k.stream));
    HIP_TRY(h, hipStreamSynchronize(k.stream));
    return QGD_OK;
}

// the grid-point pullback, slot k at time point k * save
static int pullback_grid(qgd_handle h, const PullbackCall &p, int save)
{
    qgdk_ctx &k = h->k;
    const OutputSizes z = output_sizes(p.sel, (size_t)k.N, (size_t)(1 + (k.nt - 1) / save) * k.c);
    auto &b = h->pb;
    int rc;
    if ((rc = pullback_buffers(h, h->pools[POOL_PULLBACK], b, {(size_t)k.nt, (size_t)k.n_pcof}, z, "the buffers of qgd_eval_pullback do not fit"))) return rc;
    if ((rc = pullback_begin(h, p, z, b))) return rc;
    { PhaseTimer t(h, "pullback_forcing");
      K_TRY(h, qgdk_pullback_forcing(&k, b.F, save, b.sbar, b.pbar, b.map, p.sel.n_groups, b.ebar, b.planes, p.sel.with_im() ? b.planes + z.plane : nullptr, p.sel.n_obs)); }
    return pullback_end(h, b, p.grad);
}


extern "C" {

int qgd_eval_grad_forced(qgd_handle h, const double *pcof, int32_t n_pcof, double *grad)
{
    if (!grad) return fail(h, QGD_ERR_ARGUMENT, "null argument");     // (pcof may be NULL when the tables were set directly)
    ENTER(h);
    qgdk_ctx &k = h->k;
    if (!k.have_target) return fail(h, QGD_ERR_STATE, "qgd_set_target must be called before qgd_eval_grad_forced");
    if (!h->have_basis) return fail(h, QGD_ERR_STATE, "qgd_set_control_basis must be called before qgd_eval_grad_forced");
    if (h->part_world != 1) return fail(h, QGD_ERR_STATE, "partitioned handle: the forced gradient is single-GPU");
    int rc;
    if ((rc = run_forward(h, pcof, n_pcof))) return rc;      // (a windowed grid: every window, the state at each window start kept)
    const int W = h->chunks_eff;
    const size_t hstepS = (size_t)k.Np * 2 * k.n_pcof * k.cp;
    // A windowed grid: windows in order, each forms its matrices and forward history again from its stored start state (as the
    // adjoint pass does), the sensitivities of all parameters continue from where the previous window left them, the guard part
    // of the gradient accumulates.  (eval_grad_forced.jl:17-194 keeps no matrices either: one forced sweep per parameter.)
    // The sweep record differs between the grids: a resident one keeps run_forward's sweep (SWEEP_GENERAL, with its stage
    // derivatives), a windowed one ends at SWEEP_NONE because chunk_forward's reruns go through sweep_begin.
    for (int r = 0; r < W; r++) {
        if (W > 1 && (rc = chunk_forward(h, pcof, n_pcof, r, true))) return rc;
        if (r == 0) {      // (the first window is the longest)
            if ((rc = forced_buffers(h, (size_t)k.nt, (size_t)k.scan_blocks))) return rc;
            HIP_TRY(h, hipMemsetAsync(k.fs_bnd, 0, hstepS * sizeof(double), k.stream));
            HIP_TRY(h, hipMemsetAsync(k.fs_gacc, 0, ((size_t)k.n_pcof + 1) * sizeof(double), k.stream));
        }
        if (!h->sweep.derivs) { PhaseTimer t(h, "derivs"); K_TRY(h, qgdk_derivs(&k)); h->sweep.derivs = W == 1; }
        { PhaseTimer t(h, "forced_basis"); K_TRY(h, qgdk_forced_basis(&k)); }
        h->sweep.forced_basis = W == 1;
        { PhaseTimer t(h, "forced_sweeps"); K_TRY(h, qgdk_forced_chains(&k)); }
        if (r + 1 < W)      // s at the start of the next window
            HIP_TRY(h, hipMemcpyAsync(k.fs_bnd, k.fs_bnd + (size_t)k.scan_blocks * hstepS, hstepS * sizeof(double), hipMemcpyDeviceToDevice, k.stream));
    }
    if ((rc = check_status(h))) return rc;
    ForcedTerminal t;
    return forced_terminal(h, k.fs_bnd + (size_t)k.scan_blocks * hstepS, grad, t);
}


// exact Hessian of the objective: the adjoint evaluation (lambda), the forced sweep with its history
// of sensitivities kept, then the second-order contraction of qgd_k_hessian.hip.  The terminal part is host arithmetic on s_N.
int qgd_eval_hessian(qgd_handle h, const double *pcof, int32_t n_pcof, double *hess, double *grad)
{
    if (!hess) return fail(h, QGD_ERR_ARGUMENT, "null argument");
    ENTER(h);
    qgdk_ctx &k = h->k;
    int rc;
    if ((rc = second_order_refusals(h, pcof, n_pcof, "qgd_eval_hessian", "the Hessian"))) return rc;
    if ((rc = hess_buffers(h))) return rc;
    if ((rc = second_order_setup(h, pcof, n_pcof))) return rc;      // (lambda; the adjoint gradient is unused)
    const size_t nt = k.nt, np = (size_t)k.n_pcof, hstepS = (size_t)k.Np * 2 * np * k.cp;
    const auto &b = h->hs;
    double *Gm = b.Y + np * np, *gpartial = b.Y + 2 * np * np;
    HIP_TRY(h, hipMemsetAsync(k.fs_bnd, 0, hstepS * sizeof(double), k.stream));
    HIP_TRY(h, hipMemsetAsync(k.fs_gacc, 0, (np + 1) * sizeof(double), k.stream));
    HIP_TRY(h, hipMemsetAsync(b.shist, 0, hstepS * sizeof(double), k.stream));      // s_0 = 0
    HIP_TRY(h, hipMemsetAsync(Gm, 0, np * np * sizeof(double), k.stream));
    k.fs_shist = b.shist;
    { PhaseTimer t(h, "forced_sweeps"); rc = qgdk_forced_chains(&k); }
    k.fs_shist = nullptr;
    if (rc) return fail(h, QGD_ERR_NO_DEVICE, std::string("kernel launch failed: qgdk_forced_chains: ") + hipGetErrorString((hipError_t)rc));
    { PhaseTimer t(h, "hess_terms"); K_TRY(h, qgdk_hess_kernels(&k, b.shist, b.Z, b.half, b.slab, b.zt, b.Y)); }
    if (k.have_guard) { PhaseTimer t(h, "hess_guard"); K_TRY(h, qgdk_hess_gram(&k, b.shist, b.ws, gpartial, Gm)); }
    if ((rc = check_status(h))) return rc;
    // terminal part: the overlaps <s_N,R>, <s_N,T> of every parameter (:Infidelity; per column for :StateTransfer) or s_N itself (:Tracking / :Norm)
    ForcedTerminal t;
    const bool local_cost = k.cost_type == QGD_COST_TRACKING || k.cost_type == QGD_COST_NORM;
    if ((rc = forced_terminal(h, b.shist + (nt - 1) * hstepS, grad, t, local_cost))) return rc;
    std::vector<double> Yh(np * np), Gh(np * np);
    HIP_TRY(h, hipMemcpy(Yh.data(), b.Y, np * np * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(Gh.data(), Gm, np * np * sizeof(double), hipMemcpyDeviceToHost));
    const size_t L = 2 * (size_t)k.N * k.c;
    for (size_t p = 0; p < np; p++)
        for (size_t q = 0; q < np; q++) {
            double phi;
            if (local_cost) {
                phi = 0.0;
                for (size_t e = 0; e < L; e++) phi += t.s[p * L + e] * t.s[q * L + e];
            } else if (k.cost_type == QGD_COST_STATE_TRANSFER) {      // the :Infidelity expression per column, summed over the columns, with -2/c
                phi = 0.0;
                for (size_t j = 0; j < (size_t)k.c; j++) phi += t.cR[p * k.c + j] * t.cR[q * k.c + j] + t.cT[p * k.c + j] * t.cT[q * k.c + j];
                phi *= t.f;
            } else {
                phi = t.f * (t.sR[p] * t.sR[q] + t.sT[p] * t.sT[q]);
            }
            hess[p * np + q] = (Yh[p * np + q] + Yh[q * np + p]) + Gh[p * np + q] + phi;      // (Gh: both triangles from the same sums)
        }
    return QGD_OK;
}


// exact Hessian-vector products.  Setup, once per pcof and kept on the handle: forward sweep, lambda,
// stage derivatives, forced basis responses, k_hess_basis.  Per vector: the direction table, one forced sweep, k_hvp_forcing,
// the adjoint sweep with that forcing (mu), the gradient kernels with mu in place of lambda, k_hvp_contract.
int qgd_eval_hessian_vec(qgd_handle h, const double *pcof, int32_t n_pcof, const double *v, int32_t n_vec, double *hv, double *grad)
{
    if (!v || !hv) return fail(h, QGD_ERR_ARGUMENT, "null argument");
    if (n_vec < 1) return fail(h, QGD_ERR_ARGUMENT, "qgd_eval_hessian_vec needs at least one vector");
    ENTER(h);
    qgdk_ctx &k = h->k;
    int rc;
    if ((rc = second_order_refusals(h, pcof, n_pcof, "qgd_eval_hessian_vec", "the Hessian-vector product"))) return rc;
    const size_t nt = k.nt, np = (size_t)k.n_pcof, hstep = (size_t)k.Np * 2 * k.cp;
    if ((rc = hvp_buffers(h))) return rc;
    auto &b = h->hv;
    if (!(h->hvp_valid && h->sweep.kind == SWEEP_GENERAL && sweep_reusable(h, pcof, n_pcof))) {
        if ((rc = second_order_setup(h, pcof, n_pcof))) return rc;
        { PhaseTimer t(h, "hess_basis"); K_TRY(h, qgdk_hess_basis(&k, b.Z, b.half, b.slab)); }
        if ((rc = check_status(h))) return rc;
        h->hvp_grad.resize(np);
        HIP_TRY(h, hipMemcpyAsync(h->hvp_grad.data(), k.grad, np * sizeof(double), hipMemcpyDeviceToHost, k.stream));
        HIP_TRY(h, hipStreamSynchronize(k.stream));
        h->hvp_valid = true;
    }
    const qgdk_ctx a = adjoint_context(k, b.F, b.Y, b.mu, b.gB, b.scal);      // (the same for every vector)
    for (int32_t j = 0; j < n_vec; j++) {
        HIP_TRY(h, hipMemcpyAsync(b.v, v + (size_t)j * np, np * sizeof(double), hipMemcpyHostToDevice, k.stream));
        { PhaseTimer t(h, "hvp_direction"); K_TRY(h, qgdk_hvp_gv(&k, b.v, b.gvt)); }
        { PhaseTimer t(h, "hvp_sweep"); K_TRY(h, qgdk_hvp_forced_sweep(&k, b.gvt, b.one3, b.phi, b.bnd, b.sv)); }
        if (k.have_guard == 1) { PhaseTimer t(h, "hvp_guard"); K_TRY(h, qgdk_hess_wapply(&k, b.sv, b.ws, 1)); }
        if ((rc = hvp_terminal(h, b.sv + (nt - 1) * hstep, b.term))) return rc;
        { PhaseTimer t(h, "hvp_forcing"); K_TRY(h, qgdk_hvp_forcing(&k, b.Z, b.half, b.sv, b.ws, b.gvt, b.term, b.F, b.part)); }
        { PhaseTimer t(h, "hvp_adjoint"); K_TRY(h, qgdk_hvp_adjoint(&a)); }
        { PhaseTimer t(h, "hvp_gradient"); K_TRY(h, qgdk_gradient(&a)); K_TRY(h, qgdk_hvp_contract(&k, b.part, b.gB, b.out)); }
        HIP_TRY(h, hipMemcpyAsync(hv + (size_t)j * np, b.out, np * sizeof(double), hipMemcpyDeviceToHost, k.stream));
        HIP_TRY(h, hipStreamSynchronize(k.stream));
    }
    if (grad) memcpy(grad, h->hvp_grad.data(), np * sizeof(double));
    return QGD_OK;
}



// pullback of the trajectory outputs to pcof: the forward sweep on the general two-point path (or the
// stored one), the stage derivatives, k_pullback_forcing, then term (B) of the Hessian-vector product as it stands -- the adjoint
// sweep with that forcing (mu) and the gradient kernels with mu in place of lambda, on a context copy with buffers of its own.
int qgd_eval_pullback(qgd_handle h, const double *pcof, int32_t n_pcof, int32_t history_precomputed,
                      const double *states_bar,
                      const double *pop_bar, const double *level_map, int32_t n_groups,
                      const double *expect_bar, const double *obs_re, const double *obs_im, int32_t n_obs,
                      double *grad)
{
    const PullbackCall p{"qgd_eval_pullback", pcof, n_pcof, history_precomputed, states_bar, pop_bar, expect_bar,
                         {states_bar != nullptr, pop_bar != nullptr, expect_bar != nullptr, level_map, n_groups, obs_re, obs_im, n_obs}, grad};
    int rc;
    if ((rc = pullback_arguments(h, p))) return rc;
    ENTER(h);
    if ((rc = trajectory_refusals(h, p.name, "pullback", pcof, n_pcof, history_precomputed, false))) return rc;
    return pullback_grid(h, p, h->save_every);
}


// pullback of the DENSE trajectory outputs to pcof.  The sweep handling of qgd_eval_pullback; then
// qgdk_interp into the dense panels, k_pullback_forcing on them as a history of 1 + (nt-1) refine points (G), the transposed
// interpolation (gbar), the reverse sweep of the stage-derivative recursion (F = the states cotangent's forcing, and sigma: the
// part through the tables at the time points themselves), the adjoint sweep and the gradient kernels of qgd_eval_pullback with
// that F (the implicit part, stored into the call's gradient), and last k_contract on the call's own sigma, ACCUMULATING the
// explicit part into it: grad = implicit + explicit, in this order on every call.  refine = 1 is the grid-point call itself.
int qgd_eval_dense_pullback(qgd_handle h, const double *pcof, int32_t n_pcof, int32_t history_precomputed, int32_t refine,
                            const double *states_bar,
                            const double *pop_bar, const double *level_map, int32_t n_groups,
                            const double *expect_bar, const double *obs_re, const double *obs_im, int32_t n_obs,
                            double *grad)
{
    const PullbackCall p{"qgd_eval_dense_pullback", pcof, n_pcof, history_precomputed, states_bar, pop_bar, expect_bar,
                         {states_bar != nullptr, pop_bar != nullptr, expect_bar != nullptr, level_map, n_groups, obs_re, obs_im, n_obs}, grad};
    if (grad && (refine < 1 || (h && (long long)h->nsteps * refine + 1 > 0x7fffffffLL)))
        return fail(h, QGD_ERR_ARGUMENT, "refine must be >= 1 and 1 + nsteps * refine fit a 32-bit integer");
    int rc;
    if ((rc = pullback_arguments(h, p))) return rc;
    ENTER(h);
    if ((rc = trajectory_refusals(h, p.name, "pullback", pcof, n_pcof, history_precomputed, false))) return rc;
    if (refine == 1) return pullback_grid(h, p, 1);      // (whatever qgd_set_save_every says: the dense output returns every point)
    qgdk_ctx &k = h->k;
    if (k.m > 8) return fail(h, QGD_ERR_UNSUPPORTED, "qgd_eval_dense_pullback with refine > 1 supports order <= 16 (the interpolation kernels cover order/2 <= 8)");
    const size_t nt = k.nt, pts = 1 + (nt - 1) * (size_t)refine, np = (size_t)k.n_pcof, m = k.m, hstep = (size_t)k.Np * 2 * k.cp;
    const OutputSizes z = output_sizes(p.sel, (size_t)k.N, pts * k.c);
    // buffers: the dense panels and the weight table under POOL_DENSE's key, the rest in a pool of this call's own
    if ((rc = dense_buffers(h, refine))) return rc;
    size_t dt_bits = 0;
    memcpy(&dt_bits, &k.dt, sizeof(double) < sizeof(size_t) ? sizeof(double) : sizeof(size_t));
    auto &b = h->dpb;
    if ((rc = pullback_buffers(h, h->pools[POOL_DENSE_PULLBACK], b, {nt, (size_t)refine, np, m, dt_bits}, z, "the buffers of qgd_eval_dense_pullback do not fit",
                               {{&b.G, pts * hstep}, {&b.gbar, nt * (m + 1) * hstep}},
                               {{&b.sigma, (size_t)(k.cp / 8) * nt * k.n_ops * m * 2}, {&b.cpart, ((nt + 7) / 8) * np}}))) return rc;
    if ((rc = pullback_begin(h, p, z, b))) return rc;
    { PhaseTimer t(h, "dense_pullback_interp"); K_TRY(h, qgdk_interp(&k, k.hist, k.dpsi, h->dense_panels, refine, h->dense_w, k.stream)); }
    {   // the forcing kernel takes its history and its point count from the context: the dense panels, every slot addressed
        qgdk_ctx d = k;
        d.hist = h->dense_panels; d.nt = (int)pts;
        PhaseTimer t(h, "dense_pullback_forcing");
        K_TRY(h, qgdk_pullback_forcing(&d, b.G, 1, b.sbar, b.pbar, b.map, n_groups, b.ebar, b.planes, p.sel.with_im() ? b.planes + z.plane : nullptr, n_obs));
    }
    { PhaseTimer t(h, "dense_pullback_transpose"); K_TRY(h, qgdk_interp_transpose(&k, b.G, b.gbar, refine, h->dense_w)); }
    { PhaseTimer t(h, "dense_pullback_sweep"); K_TRY(h, qgdk_dense_pullback_sweep(&k, b.gbar, b.F, b.sigma)); }
    return pullback_end(h, b, grad, &b);
}

}  // extern "C"
