// qgd_host_ensemble.cpp -- host side of the C ABI (include/qgd_ensemble.h): one coefficient vector over the members of an
// ensemble, side by side on the small-problem path.  A member is the handle's problem with other operator
// planes: qgd_set_ensemble packs and uploads the planes of all members once; qgd_eval_ensemble runs the launches of
// qgd_eval_batch with the member axis on the planes instead of on pcof (qgd_k_tiny.hip: TinyPcofShared), on that call's
// per-member arrays (POOL_BATCH, batch_buffers), and a fifth launch per chunk that adds the chunk's rows into an accumulator row
// on the device in the order and with the roundings of ensemble_reduce (qgd_k_grad.hip: k_ensemble_reduce).  There is no loop
// route here: a handle has one set of operators, and the loop over handles exists above the library.
#include "qgd_host.h"

using namespace qgdh;

extern "C" {

int qgd_set_ensemble(qgd_handle h, int32_t n_members, const double *system_sym, const double *system_asym,
                     const double *sym_ops, const double *asym_ops, const double *weights)
{
    if (n_members < 0) return fail(h, QGD_ERR_ARGUMENT, "an ensemble cannot have a negative number of members");
    if (n_members > 0 && (!system_sym || !system_asym || !weights || (h && h->k.n_ops && (!sym_ops || !asym_ops))))
        return fail(h, QGD_ERR_ARGUMENT, "null argument");
    ENTER(h, ENTER_KEEPS_GRAPH | ENTER_NO_GRID);
    const qgdk_ctx &k = h->k;
    Pool &pool = h->pools[POOL_ENSEMBLE];
    pool_release(pool);
    h->ens.members = 0;
    if (n_members == 0) return QGD_OK;
    const size_t K = (size_t)n_members, N = (size_t)k.N, Np = (size_t)k.Np, n_ops = (size_t)k.n_ops, per = qgdk_tiny_ensemble_planes(&k);
    qgd_handle_s::EnsembleBufs &b = h->ens;
    // (the planes are the caller's data, like the control basis: they count against the device memory itself -- QGD_ERR_MEMORY
    //  from the allocation --, not against the memory budget, which sizes the chunks of the evaluation)
    const int rc = pool_ensure(h, pool, {{K, N, n_ops}, {{&b.ops, K * per}, {&b.w, K}, {&b.acc, QGD_ENSEMBLE_ACC}, {&b.tails, 5 * K}}});
    if (rc) return rc;
    // every member's planes as qgd_create lays out the handle's own: K_sys, S_sys, Asym_1, Sym_1, ...
    std::vector<double> planes(K * per, 0.0);
    for (size_t m = 0; m < K; m++) {
        double *p = planes.data() + m * per;
        pack_plane(p, 0, Np, k.N, system_asym + m * N * N); pack_plane(p, 1, Np, k.N, system_sym + m * N * N);
        for (size_t o = 0; o < n_ops; o++) {
            pack_plane(p, 2 + 2 * o, Np, k.N, asym_ops + (m * n_ops + o) * N * N);
            pack_plane(p, 3 + 2 * o, Np, k.N, sym_ops + (m * n_ops + o) * N * N);
        }
    }
    hipError_t e = hipMemcpy(b.ops, planes.data(), planes.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b.w, weights, K * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) { pool_release(pool); return fail(h, QGD_ERR_NO_DEVICE, std::string("upload of the ensemble: ") + hipGetErrorString(e)); }
    b.members = n_members;
    return QGD_OK;
}


int qgd_eval_ensemble(qgd_handle h, const double *pcof, int32_t n_pcof, int32_t gradient, double *grad, double *out2,
                      double *member_grads, double *member_out3, int32_t *member_status)
{
    if (!pcof || !out2 || (gradient && !grad)) return fail(h, QGD_ERR_ARGUMENT, "null argument");
    if (h && (h->comm || h->part_world != 1)) return fail(h, QGD_ERR_UNSUPPORTED, "qgd_eval_ensemble is single-GPU: this handle has a communicator or a partition");
    ENTER(h, ENTER_KEEPS_GRAPH);
    qgdk_ctx &k = h->k;
    if (!h->ens.ops || h->ens.members < 1) return fail(h, QGD_ERR_STATE, "qgd_set_ensemble must be called before qgd_eval_ensemble (and after qgd_set_control_basis)");
    if (!h->have_basis) return fail(h, QGD_ERR_STATE, "qgd_set_control_basis must be called before qgd_eval_ensemble");
    if (n_pcof != k.n_pcof) return fail(h, QGD_ERR_ARGUMENT, "length of pcof does not match the control basis");
    if (gradient && !k.have_target) return fail(h, QGD_ERR_STATE, "qgd_set_target must be called before an ensemble evaluation with gradients");
    if (!tiny_applies(h, pcof, n_pcof))
        return fail(h, QGD_ERR_UNSUPPORTED, "qgd_eval_ensemble runs on the small-problem path only (N <= 4, <= 4 columns, <= 128 resident time points, "
                                            "n_pcof <= 64, small path on, no event bracketing, no caller's control tables): evaluate the members on handles of their own");
    const int K = h->ens.members;
    const size_t np = (size_t)n_pcof;
    int chunk = std::min(K, h->batch_chunk_max);
    int rc = batch_buffers(h, n_pcof, &chunk);
    if (rc) return rc;
    sweep_void(h);
    const qgd_handle_s::BatchBufs &b = h->bt;
    const qgd_handle_s::EnsembleBufs &en = h->ens;
    const qgdk_tiny_batch dev{b.pcofs, b.tab, b.Rg, b.Linv, b.psi, b.lam, b.cpart, b.small, b.rows};
    const size_t planes = qgdk_tiny_ensemble_planes(&k);
    const bool rows_out = gradient && member_grads;
    double *hout = h->batch_host + (size_t)chunk * np;      // (the staging buffer of a batch chunk: [pcofs | rows])
    int first_singular = -1;
    if (member_status) memset(member_status, 0, sizeof(int32_t) * (size_t)K);
    for (int m0 = 0; m0 < K; m0 += chunk) {
        const int Kc = std::min(chunk, K - m0);
        // the chunk's planes and weights are addressed in place, m0 members into the uploaded arrays
        int e = qgdk_tiny_eval_ensemble(&k, &dev, en.ops + (size_t)m0 * planes, pcof, Kc, n_pcof, gradient ? 1 : 0);
        if (!e) e = qgdk_contract_rows_batch(&k, &dev, Kc, n_pcof, gradient ? k.nt : 0);
        if (!e) e = qgdk_ensemble_reduce(&k, b.rows, en.w + m0, en.acc, en.tails + 5 * (size_t)m0, Kc, n_pcof, m0 == 0, gradient ? 1 : 0);
        if (e) return fail(h, QGD_ERR_NO_DEVICE, std::string("ensemble evaluation failed to launch: ") + hipGetErrorString((hipError_t)e));
        if (rows_out) HIP_TRY(h, hipMemcpyAsync(hout, b.rows, sizeof(double) * Kc * (np + 5), hipMemcpyDeviceToHost, k.stream));
        else HIP_TRY(h, hipMemcpyAsync(hout, en.tails + 5 * (size_t)m0, sizeof(double) * Kc * 5, hipMemcpyDeviceToHost, k.stream));
        if (m0 + Kc == K) HIP_TRY(h, hipMemcpyAsync(h->host_out, en.acc, sizeof(double) * (np + 2), hipMemcpyDeviceToHost, k.stream));
        HIP_TRY(h, hipStreamSynchronize(k.stream));
        for (int q = 0; q < Kc; q++) {
            const double *tail = rows_out ? hout + (size_t)q * (np + 5) + np : hout + (size_t)q * 5;
            if (rows_out) memcpy(member_grads + (size_t)(m0 + q) * np, hout + (size_t)q * (np + 5), sizeof(double) * np);
            if (member_out3) memcpy(member_out3 + 3 * (size_t)(m0 + q), tail, 3 * sizeof(double));
            if (tail[3] != 0.0) {
                if (member_status) member_status[m0 + q] = 1;
                if (first_singular < 0) first_singular = m0 + q;
            }
        }
    }
    if (gradient) memcpy(grad, h->host_out, sizeof(double) * np);
    memcpy(out2, h->host_out + np, 2 * sizeof(double));
    if (first_singular >= 0) {
        const bool dirty = h->status_dirty;      // (the members have status words of their own, cleared on the device: as in qgd_eval_batch)
        rc = fail(h, QGD_ERR_NUMERIC, "singular implicit step matrix L(t_n) in member " + std::to_string(first_singular) + " of the ensemble");
        h->status_dirty = dirty;
        return rc;
    }
    return QGD_OK;
}

}  // extern "C"
