// qgd_host_pushforward.cpp -- host side of the C ABI (include/qgd_pushforward.h): directional derivatives of the trajectory outputs
// along directions in pcof.  s_v = sum_l v_l dw/dpcof_l is the forced scan of qgd_eval_hessian_vec
// (section 4d) without the rest of that product: no adjoint sweep, no lambda, no k_hess_basis.  The directions of a chunk ride
// along as column groups of ONE scan, the way the parameters of qgd_eval_grad_forced do; the states tangent leaves through the
// re-layout kernel of the reference-layout outputs, the other two through qgd_k_pushforward.hip.
#include "qgd_host.h"

using namespace qgdh;

namespace {

struct PushforwardCall {
    const double *pcof; int32_t n_pcof, history_precomputed;
    const double *v; int32_t n_vec;
    double *states_dot, *pop_dot, *expect_dot;
    OutputSelection sel;      // the outputs whose array is given
};

size_t pushforward_slots(qgd_handle h) { return 1 + (size_t)(h->k.nt - 1) / h->save_every; }

// the pool for chunks of up to `cap` directions, z: the doubles of one direction of each output as the caller gets it and of the
// two uploads (the states are staged with their padding columns: cp of them per direction)
KeyedPlan pushforward_plan(qgd_handle h, const OutputSizes &z, size_t cap)
{
    const qgdk_ctx &k = h->k;
    const size_t nt = k.nt, np = (size_t)k.n_pcof, NB = (size_t)k.n_ops * 2 * k.m, B = (size_t)k.scan_blocks;
    const size_t hstep = (size_t)k.Np * 2 * k.cp, st = z.states ? 2 * (size_t)k.N * pushforward_slots(h) * k.cp : 0;
    auto &b = h->pf;
    return {{nt, np, NB, B, cap, z.states, z.pops, z.expect, z.map, z.planes}, {
        {&b.sv, nt * hstep * cap}, {&b.phi, B * hstep * cap}, {&b.bnd, (B + 1) * hstep * cap}, {&b.gvt, qgdk_hvp_gv_len(&k) * cap},
        {&b.bases, 2 * cap}, {&b.v, np * cap}, {&b.st, st * cap, st != 0}, {&b.po, z.pops * cap, z.pops != 0}, {&b.ex, z.expect * cap, z.expect != 0},
        {&b.map, z.map, z.map != 0}, {&b.planes, z.planes, z.planes != 0}}};
}

// The pool of this call: chunks of `want` directions when that fits, else of as many as the memory budget and the free device
// memory hold beside the forced gradient's buffers (halving, never below one: QGD_ERR_MEMORY is then the pool's own answer).
// A pool of the same problem and outputs that is wide enough already is kept.  Returns the chunk's width in `chunk`.
int pushforward_buffers(qgd_handle h, const OutputSizes &z, size_t want, size_t &chunk)
{
    qgdk_ctx &k = h->k;
    Pool &pool = h->pools[POOL_PUSHFORWARD];
    size_t cap = want;
    KeyedPlan p = pushforward_plan(h, z, cap);
    bool kept = pool.key.size() == p.key.size() && pool.key[4] >= want;
    for (size_t i = 0; kept && i < p.key.size(); i++) kept = i == 4 || pool.key[i] == p.key[i];
    if (kept) {
        cap = pool.key[4];
    } else {
        size_t fr = 0, tot = 0;
        const bool have_free = hipMemGetInfo(&fr, &tot) == hipSuccess;
        const size_t extra = forced_missing(h);
        auto fits = [&](size_t bytes) { return !(h->mem_budget && bytes > h->mem_budget) && !(have_free && bytes > fr); };
        while (cap > 1 && !fits(plan_bytes(pushforward_plan(h, z, cap).plan) + extra)) cap = (cap + 1) / 2;
    }
    chunk = std::min(cap, want);
    auto &b = h->pf;
    return pool_ensure(h, pool, pushforward_plan(h, z, cap), "the buffers of qgd_eval_pushforward do not fit", forced_missing(h), [&]() -> int {
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
}

int pushforward(qgd_handle h, const PushforwardCall &p)
{
    qgdk_ctx &k = h->k;
    const int save = h->save_every;
    const size_t slots = pushforward_slots(h);
    const OutputSizes z = output_sizes(p.sel, (size_t)k.N, slots * k.c);
    const size_t np = (size_t)k.n_pcof, hstep = (size_t)k.Np * 2 * k.cp, n_vec = (size_t)p.n_vec, B8 = sizeof(double);
    size_t chunk = 0;
    int rc;
    if ((rc = pushforward_buffers(h, z, std::min(n_vec, (size_t)h->pf_chunk_max), chunk))) return rc;
    auto &b = h->pf;
    if ((rc = upload_selection(h, p.sel, z, b.map, b.planes))) return rc;
    // the pullbacks' forward sweep and stage derivatives; the forced basis responses unless the stored sweep has them (an earlier
    // pushforward, the setup of qgd_eval_hessian_vec) and their pool still stands
    if ((rc = pullback_sweep(h, p.pcof, p.n_pcof, p.history_precomputed))) return rc;
    const bool formed = h->sweep.forced_basis && forced_missing(h) == 0;
    if ((rc = forced_buffers(h, (size_t)k.nt, (size_t)k.scan_blocks))) return rc;
    if (!formed) { PhaseTimer t(h, "forced_basis"); K_TRY(h, qgdk_forced_basis(&k)); h->sweep.forced_basis = true; }
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
        if (p.states_dot) {
            // the reference-layout transport of qgd_eval_states with the tangent panels in place of the state panels: a context
            // whose columns are the w cp columns of the chunk (padding columns included), then one pitched copy per chunk that
            // takes the c columns of every direction
            qgdk_ctx d = k;
            d.cp = (int)w * k.cp; d.c = d.cp;
            const size_t rows = 2 * (size_t)k.N, per_dir = rows * slots * k.cp;
            K_TRY(h, qgdk_layout(&d, b.sv, (long long)(hstep * w * save), 0, b.st, (long long)(slots * rows), (long long)rows, 0, 0, (int)slots, 1, 0, k.stream, 0));
            HIP_TRY(h, hipMemcpy2DAsync(p.states_dot + j0 * z.states, z.states * B8, b.st, per_dir * B8, z.states * B8, w, hipMemcpyDeviceToHost, k.stream));
        }
        if (p.pop_dot || p.expect_dot) {
            PhaseTimer t(h, "pushforward_outputs", nullptr, slot);
            K_TRY(h, qgdk_pushforward_outputs(&k, b.sv, (int)w, save, b.po, b.map, p.sel.n_groups, b.ex, b.planes, p.sel.with_im() ? b.planes + z.plane : nullptr, p.sel.n_obs));
        }
        if (p.pop_dot) HIP_TRY(h, hipMemcpyAsync(p.pop_dot + j0 * z.pops, b.po, w * z.pops * B8, hipMemcpyDeviceToHost, k.stream));
        if (p.expect_dot) HIP_TRY(h, hipMemcpyAsync(p.expect_dot + j0 * z.expect, b.ex, w * z.expect * B8, hipMemcpyDeviceToHost, k.stream));
    }
    HIP_TRY(h, hipStreamSynchronize(k.stream));
    return QGD_OK;
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
    if (!v) return fail(h, QGD_ERR_ARGUMENT, "null argument");
    if (n_vec < 1) return fail(h, QGD_ERR_ARGUMENT, "qgd_eval_pushforward needs at least one direction");
    if (!states_dot && !pop_dot && !expect_dot) return fail(h, QGD_ERR_ARGUMENT, "qgd_eval_pushforward needs at least one of states_dot, pop_dot, expect_dot");
    int rc;
    if ((rc = selection_refusals(h, p.sel, "expect_dot"))) return rc;
    ENTER(h);
    if ((rc = trajectory_refusals(h, "qgd_eval_pushforward", "pushforward", pcof, n_pcof, history_precomputed, true))) return rc;
    return pushforward(h, p);
}

}  // extern "C"
