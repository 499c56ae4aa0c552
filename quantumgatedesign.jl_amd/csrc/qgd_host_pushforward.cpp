// qgd_host_pushforward.cpp -- host side of the C ABI (include/qgd_pushforward.h, include/qgd_dense_pushforward.h): directional
// derivatives of the trajectory outputs along directions in pcof, at the grid points and of the Hermite
// dense output (section 4n).  s_v = sum_l v_l dw/dpcof_l is the forced scan of qgd_eval_hessian_vec (section 4d) without the rest
// of that product: no adjoint sweep, no lambda, no k_hess_basis.  The directions of a chunk ride along as column groups of ONE
// scan, the way the parameters of qgd_eval_grad_forced do; the states tangent leaves through the re-layout kernel of the
// reference-layout outputs, the other two through qgd_k_pushforward.hip.  The dense call puts the tangent of the stage
// derivatives (qgd_k_dense_pushforward.hip) and the interpolation kernel of the dense output between the scan and those two.
#include "qgd_host.h"

using namespace qgdh;

namespace {

struct PushforwardCall {
    const double *pcof; int32_t n_pcof, history_precomputed;
    const double *v; int32_t n_vec;
    double *states_dot, *pop_dot, *expect_dot;
    OutputSelection sel;      // the outputs whose array is given
    int refine = 0;           // 0: the grid points, every qgd_set_save_every-th; r >= 1: the dense output, every slot (r = 1: every grid point)
};

// the pool for chunks of up to `cap` directions, z: the doubles of one direction of each output as the caller gets it and of the
// two uploads (the states are staged with their padding columns: cp of them per direction, `slots` slots)
KeyedPlan pushforward_plan(qgd_handle h, const OutputSizes &z, size_t slots, size_t cap)
{
    const qgdk_ctx &k = h->k;
    const size_t nt = k.nt, np = (size_t)k.n_pcof, NB = (size_t)k.n_ops * 2 * k.m, B = (size_t)k.scan_blocks;
    const size_t hstep = (size_t)k.Np * 2 * k.cp, st = z.states ? 2 * (size_t)k.N * slots * k.cp : 0;
    auto &b = h->pf;
    return {{nt, np, NB, B, cap, z.states, z.pops, z.expect, z.map, z.planes}, {
        {&b.sv, nt * hstep * cap}, {&b.phi, B * hstep * cap}, {&b.bnd, (B + 1) * hstep * cap}, {&b.gvt, qgdk_hvp_gv_len(&k) * cap},
        {&b.bases, 2 * cap}, {&b.v, np * cap}, {&b.st, st * cap, st != 0}, {&b.po, z.pops * cap, z.pops != 0}, {&b.ex, z.expect * cap, z.expect != 0},
        {&b.map, z.map, z.map != 0}, {&b.planes, z.planes, z.planes != 0}}};
}

// what the dense call holds beside that pool and POOL_DENSE, for chunks of up to `cap` directions: the tangents of the stage
// derivatives, the interpolated tangent panels and the staged outputs of `pts` slots (z: the doubles of one direction)
KeyedPlan dense_pushforward_plan(qgd_handle h, const OutputSizes &z, int refine, size_t cap)
{
    const qgdk_ctx &k = h->k;
    const size_t nt = k.nt, np = (size_t)k.n_pcof, NB = (size_t)k.n_ops * 2 * k.m, B = (size_t)k.scan_blocks, m = k.m;
    const size_t hstep = (size_t)k.Np * 2 * k.cp, pts = 1 + (nt - 1) * (size_t)refine, st = z.states ? 2 * (size_t)k.N * pts * k.cp : 0;
    size_t dt_bits = 0;
    memcpy(&dt_bits, &k.dt, sizeof(double) < sizeof(size_t) ? sizeof(double) : sizeof(size_t));
    auto &b = h->dpf;
    return {{nt, np, NB, B, cap, z.states, z.pops, z.expect, (size_t)refine, m, dt_bits}, {
        {&b.dsv, nt * m * hstep * cap}, {&b.dd, pts * hstep * cap}, {&b.st, st * cap, st != 0}, {&b.po, z.pops * cap, z.pops != 0},
        {&b.ex, z.expect * cap, z.expect != 0}}};
}

// The pool of this call: chunks of `want` directions when that fits, else of as many as the memory budget and the free device
// memory hold beside the forced gradient's buffers (halving, never below one: QGD_ERR_MEMORY is then the pool's own answer).
// A pool of the same problem and outputs that is wide enough already is kept.  Returns the chunk's width in `chunk`.
// refine > 1 (the dense call, z: the dense sizes): the staged outputs and the dense buffers of that width go into
// the dense pushforward's own pool, ensured here too, and count in the halving rule; POOL_PUSHFORWARD then stages no output.
int pushforward_buffers(qgd_handle h, const OutputSizes &z, size_t slots, size_t want, size_t &chunk, int refine = 0)
{
    qgdk_ctx &k = h->k;
    Pool &pool = h->pools[POOL_PUSHFORWARD], &dpool = h->dense_pushforward_pool;
    const bool dense = refine > 1;
    OutputSizes zp = z;
    if (dense) zp.states = zp.pops = zp.expect = 0;
    auto beside = [&](size_t cap) { return dense ? pool_missing(dpool, dense_pushforward_plan(h, z, refine, cap)) : (size_t)0; };
    size_t fr = 0, tot = 0;
    int have_free = -1;      // (asked once, and only by a call that sizes a new pool)
    auto fits = [&](size_t bytes) {
        if (have_free < 0) have_free = hipMemGetInfo(&fr, &tot) == hipSuccess;
        return !(h->mem_budget && bytes > h->mem_budget) && !(have_free && bytes > fr);
    };
    size_t cap = want;
    KeyedPlan p = pushforward_plan(h, zp, slots, cap);
    bool kept = pool.key.size() == p.key.size() && pool.key[4] >= want;
    for (size_t i = 0; kept && i < p.key.size(); i++) kept = i == 4 || pool.key[i] == p.key[i];
    if (kept && dense && beside(pool.key[4]) && !fits(beside(pool.key[4]) + forced_missing(h))) kept = false;      // (the dense buffers of that width do not fit: a narrower chunk may)
    if (kept) {
        cap = pool.key[4];
    } else {
        const size_t extra = forced_missing(h);
        while (cap > 1 && !fits(plan_bytes(pushforward_plan(h, zp, slots, cap).plan) + beside(cap) + extra)) cap = (cap + 1) / 2;
    }
    chunk = std::min(cap, want);
    auto &b = h->pf;
    const char *fit = dense ? "the buffers of qgd_eval_dense_pushforward do not fit" : "the buffers of qgd_eval_pushforward do not fit";
    int rc = pool_ensure(h, pool, pushforward_plan(h, zp, slots, cap), fit, forced_missing(h) + beside(cap), [&]() -> int {
        // s_v(0) = 0 and the scan's start are never written: zeroed here for the full width and again whenever a chunk of another
        // width moves the panels; the one-operator bases {goff = 0 | ncoef = w, poff = 0} of every width w
        const size_t hstep = (size_t)k.Np * 2 * k.cp;
        struct Basis { int64_t goff; int32_t ncoef, poff; };
        std::vector<Basis> bases(cap);
        for (size_t w = 1; w <= cap; w++) bases[w - 1] = {0, (int32_t)w, 0};
        HIP_TRY(h, hipMemcpyAsync(b.bases, bases.data(), cap * sizeof(Basis), hipMemcpyHostToDevice, k.stream));
        HIP_TRY(h, hipMemsetAsync(b.sv, 0, hstep * cap * sizeof(double), k.stream));
        HIP_TRY(h, hipMemsetAsync(b.bnd, 0, hstep * cap * sizeof(double), k.stream));
        HIP_TRY(h, hipStreamSynchronize(k.stream));      // (`bases` leaves scope)
        b.width = cap;
        return QGD_OK;
    });
    if (rc || !dense) return rc;
    return pool_ensure(h, dpool, dense_pushforward_plan(h, z, refine, cap), fit, forced_missing(h));      // (every buffer is written whole before it is read)
}

int pushforward(qgd_handle h, const PushforwardCall &p)
{
    qgdk_ctx &k = h->k;
    const bool dense = p.refine > 1;
    const int save = p.refine ? 1 : h->save_every, refine = dense ? p.refine : 1;
    const size_t slots = dense ? 1 + (size_t)(k.nt - 1) * refine : 1 + (size_t)(k.nt - 1) / save;
    const OutputSizes z = output_sizes(p.sel, (size_t)k.N, slots * k.c);
    const size_t np = (size_t)k.n_pcof, hstep = (size_t)k.Np * 2 * k.cp, n_vec = (size_t)p.n_vec, B8 = sizeof(double);
    size_t chunk = 0;
    int rc;
    if (dense && (rc = dense_buffers(h, refine))) return rc;      // (the dense panels and the weight table, under POOL_DENSE's key)
    if ((rc = pushforward_buffers(h, z, slots, std::min(n_vec, (size_t)h->pf_chunk_max), chunk, refine))) return rc;
    auto &b = h->pf;
    auto &db = h->dpf;
    double *const st = dense ? db.st : b.st, *const po = dense ? db.po : b.po, *const ex = dense ? db.ex : b.ex;
    if ((rc = upload_selection(h, p.sel, z, b.map, b.planes))) return rc;
    // the pullbacks' forward sweep and stage derivatives; the forced basis responses unless the stored sweep has them (an earlier
    // pushforward, the setup of qgd_eval_hessian_vec) and their pool still stands
    if ((rc = pullback_sweep(h, p.pcof, p.n_pcof, p.history_precomputed))) return rc;
    const bool formed = h->sweep.forced_basis && forced_missing(h) == 0;
    if ((rc = forced_buffers(h, (size_t)k.nt, (size_t)k.scan_blocks))) return rc;
    if (!formed) { PhaseTimer t(h, "forced_basis"); K_TRY(h, qgdk_forced_basis(&k)); h->sweep.forced_basis = true; }
    if (dense) {      // the dense state panels, as qgd_eval_dense forms them: the same for every chunk
        PhaseTimer t(h, "dense_pushforward_interp", nullptr, -1);
        K_TRY(h, qgdk_interp(&k, k.hist, k.dpsi, h->dense_panels, refine, h->dense_w, k.stream));
    }
    for (size_t j0 = 0; j0 < n_vec; j0 += chunk) {
        const size_t w = std::min(chunk, n_vec - j0);
        const int slot = (int)(j0 / chunk);      // (a chunk's launches are a piece of their phase: qgd_get_timings adds the chunks up)
        if (w != b.width) {      // (panels of another width: s_v(0) and the scan's start lie elsewhere)
            HIP_TRY(h, hipMemsetAsync(b.sv, 0, hstep * w * B8, k.stream));
            HIP_TRY(h, hipMemsetAsync(b.bnd, 0, hstep * w * B8, k.stream));
            b.width = w;
        }
        HIP_TRY(h, hipMemcpyAsync(b.v, p.v + j0 * np, w * np * B8, hipMemcpyHostToDevice, k.stream));
        { PhaseTimer t(h, "pushforward_direction", nullptr, slot); K_TRY(h, qgdk_hvp_gv_dirs(&k, b.v, b.gvt, (int)w)); }
        { PhaseTimer t(h, "pushforward_sweep", nullptr, slot); K_TRY(h, qgdk_hvp_forced_sweep_dirs(&k, b.gvt, b.bases + 2 * (w - 1), b.phi, b.bnd, b.sv, (int)w)); }
        if (j0 == 0 && (rc = check_status(h))) return rc;
        // a context whose columns are the w cp columns of the chunk (padding columns included): the reference-layout transport of
        // qgd_eval_states below and, in the dense call, the interpolation of the tangent panels
        qgdk_ctx d = k;
        d.cp = (int)w * k.cp; d.c = d.cp;
        const double *tangent = b.sv;      // the tangent panels the outputs are formed from, [slots * save][Np][2 w cp]
        qgdk_ctx o = k;                    // ... and the context whose history holds the state panels beside them
        if (dense) {
            { PhaseTimer t(h, "dense_pushforward_derivs", nullptr, slot); K_TRY(h, qgdk_tangent_derivs(&k, b.sv, b.gvt, db.dsv, (int)w)); }
            { PhaseTimer t(h, "dense_pushforward_interp", nullptr, slot); K_TRY(h, qgdk_interp(&d, b.sv, db.dsv, db.dd, refine, h->dense_w, k.stream)); }
            tangent = db.dd;
            o.hist = h->dense_panels; o.nt = (int)slots;      // (as section 4j presents the dense panels to k_pullback_forcing)
        }
        if (p.states_dot) {
            // the reference-layout transport of qgd_eval_states with the tangent panels in place of the state panels, then one
            // pitched copy per chunk that takes the c columns of every direction
            const size_t rows = 2 * (size_t)k.N, per_dir = rows * slots * k.cp;
            K_TRY(h, qgdk_layout(&d, tangent, (long long)(hstep * w * save), 0, st, (long long)(slots * rows), (long long)rows, 0, 0, (int)slots, 1, 0, k.stream, 0));
            HIP_TRY(h, hipMemcpy2DAsync(p.states_dot + j0 * z.states, z.states * B8, st, per_dir * B8, z.states * B8, w, hipMemcpyDeviceToHost, k.stream));
        }
        if (p.pop_dot || p.expect_dot) {
            PhaseTimer t(h, dense ? "dense_pushforward_outputs" : "pushforward_outputs", nullptr, slot);
            K_TRY(h, qgdk_pushforward_outputs(&o, tangent, (int)w, save, po, b.map, p.sel.n_groups, ex, b.planes, p.sel.with_im() ? b.planes + z.plane : nullptr, p.sel.n_obs));
        }
        if (p.pop_dot) HIP_TRY(h, hipMemcpyAsync(p.pop_dot + j0 * z.pops, po, w * z.pops * B8, hipMemcpyDeviceToHost, k.stream));
        if (p.expect_dot) HIP_TRY(h, hipMemcpyAsync(p.expect_dot + j0 * z.expect, ex, w * z.expect * B8, hipMemcpyDeviceToHost, k.stream));
    }
    HIP_TRY(h, hipStreamSynchronize(k.stream));
    return QGD_OK;
}

// what both entry points refuse from their arguments alone, in front of ENTER
int pushforward_arguments(qgd_handle h, const PushforwardCall &p, const std::string &name)
{
    if (!p.v) return fail(h, QGD_ERR_ARGUMENT, "null argument");
    if (p.n_vec < 1) return fail(h, QGD_ERR_ARGUMENT, name + " needs at least one direction");
    if (!p.states_dot && !p.pop_dot && !p.expect_dot) return fail(h, QGD_ERR_ARGUMENT, name + " needs at least one of states_dot, pop_dot, expect_dot");
    return selection_refusals(h, p.sel, "expect_dot");
}

}  // namespace

extern "C" {

int qgd_eval_pushforward(qgd_handle h, const double *pcof, int32_t n_pcof, int32_t history_precomputed,
                         const double *v, int32_t n_vec,
                         double *states_dot,
                         double *pop_dot, const double *level_map, int32_t n_groups,
                         double *expect_dot, const double *obs_re, const double *obs_im, int32_t n_obs)
{
    const PushforwardCall p{pcof, n_pcof, history_precomputed, v, n_vec, states_dot, pop_dot, expect_dot,
                            {states_dot != nullptr, pop_dot != nullptr, expect_dot != nullptr, level_map, n_groups, obs_re, obs_im, n_obs}};
    int rc;
    if ((rc = pushforward_arguments(h, p, "qgd_eval_pushforward"))) return rc;
    ENTER(h);
    if ((rc = trajectory_refusals(h, "qgd_eval_pushforward", "pushforward", pcof, n_pcof, history_precomputed, true))) return rc;
    return pushforward(h, p);
}


// pushforward of directions in pcof to the DENSE trajectory outputs: the sweep handling and the forced scan
// of qgd_eval_pushforward; then, per chunk, the tangent of the stage derivatives, qgdk_interp on the tangent panels with the
// weight table of the dense output, and the output kernels of the grid-point call on the dense state and tangent panels as a
// history of 1 + nsteps refine points.  refine = 1 is the grid-point call itself with every time point saved.
int qgd_eval_dense_pushforward(qgd_handle h, const double *pcof, int32_t n_pcof, int32_t history_precomputed, int32_t refine,
                               const double *v, int32_t n_vec,
                               double *states_dot,
                               double *pop_dot, const double *level_map, int32_t n_groups,
                               double *expect_dot, const double *obs_re, const double *obs_im, int32_t n_obs)
{
    const PushforwardCall p{pcof, n_pcof, history_precomputed, v, n_vec, states_dot, pop_dot, expect_dot,
                            {states_dot != nullptr, pop_dot != nullptr, expect_dot != nullptr, level_map, n_groups, obs_re, obs_im, n_obs}, refine};
    int rc;
    if ((rc = pushforward_arguments(h, p, "qgd_eval_dense_pushforward"))) return rc;
    if (refine < 1 || (h && (long long)h->nsteps * refine + 1 > 0x7fffffffLL))
        return fail(h, QGD_ERR_ARGUMENT, "refine must be >= 1 and 1 + nsteps * refine fit a 32-bit integer");
    ENTER(h);
    if ((rc = trajectory_refusals(h, "qgd_eval_dense_pushforward", "pushforward", pcof, n_pcof, history_precomputed, true))) return rc;
    if (refine > 1 && h->k.m > 8)
        return fail(h, QGD_ERR_UNSUPPORTED, "qgd_eval_dense_pushforward with refine > 1 supports order <= 16 (the interpolation kernels cover order/2 <= 8)");
    return pushforward(h, p);
}

}  // extern "C"
