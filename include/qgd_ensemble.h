/* qgd_ensemble.h -- part of the C ABI of libqgd_hip.so, included by qgd.h (include that): ONE coefficient vector over the
 * members of an ensemble -- variants of the handle's problem that differ in their operators -- side by side in one device
 * call, with the weighted sums formed on the device.  Additive: QGD_ABI_VERSION stays as it is.
 *
 * The entry points stand in a header and a host unit of their own (csrc/qgd_host_ensemble.cpp) for the reason given in
 * qgd_pushforward.h: the list of entry points of qgd.h is pinned, name by name, by the tests of the prologue and of the dead
 * stream; what those tests ask of every entry point is asked of these two by their own tests.
 */
#ifndef QGD_ENSEMBLE_H
#define QGD_ENSEMBLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The members of the handle's ensemble: n_members sets of operators of the handle's N and n_ops, each array as
 * qgd_problem_desc has it for one problem (column-major [N x N] matrices), and a weight per member.  The control operators
 * are taken as they are: a caller with a scale factor per member and operator multiplies before the call.  The planes are
 * packed exactly as qgd_create packs the handle's own -- member k's are the bytes a handle created for member k would hold --
 * and uploaded once, with the weights; nothing is launched.  sym_ops / asym_ops may be NULL when the handle has no control
 * operators.  n_members = 0 releases the ensemble (the arrays are then not read).  The ensemble is also released by whatever
 * releases the sensitivity buffers: qgd_set_control_basis, qgd_set_nsteps, qgd_set_memory_budget, qgd_set_partition -- set
 * it after those.  The symmetry of the operators is not tested.
 * QGD_ERR_ARGUMENT: n_members < 0, a NULL array with n_members > 0.  QGD_ERR_MEMORY when the planes do not fit the device
 * memory (like the control basis they do not count against the memory budget, which sizes the chunks of the evaluation). */
int qgd_set_ensemble(qgd_handle h, int32_t n_members,
                     const double *system_sym,  const double *system_asym,   /* [n_members][N*N], column-major, as qgd_problem_desc */
                     const double *sym_ops,     const double *asym_ops,      /* [n_members][n_ops][N*N], already scaled by the caller */
                     const double *weights);                                /* [n_members] */

/* One evaluation of every member at pcof, under the handle's control basis, target, cost type, guard, initial conditions and
 * time grid, and the weighted sums of the results:
 *   member_grads [n_members][n_pcof], member_out3 [n_members][3]   what qgd_discrete_adjoint (gradient == 0: qgd_eval_forward)
 *                                                                 returns on a handle created for member k, bit for bit
 *   grad [n_pcof], out2 [2]     acc = 0.0; for k = 0 .. n_members-1: acc = acc + w_k * x_k, every product and every sum rounded
 *                               on its own, for x = each gradient entry, cost_k and guard_k = member_out3[k][2], where
 *                               cost_k = 1.0 - (a_k*a_k + b_k*b_k) / double(n_ess*n_ess) under QGD_COST_INFIDELITY
 *                               ((a_k, b_k) = member_out3[k][0..1]) and a_k under every other cost type
 * The members run side by side on the small-problem path (the launches of qgd_eval_batch with a member axis on the operator
 * planes instead of on pcof, plus one workgroup that forms the sums, k ascending, without atomics): in chunks as in
 * qgd_eval_batch (QGD_BATCH_CHUNK, the memory budget, the free device memory; the per-member arrays are that call's and a pool
 * made for a larger chunk is kept), the accumulators staying on the device from chunk to chunk.  member_grads NULL: no
 * member's gradient is downloaded, only [n_members][5] doubles of scalars and status and one row [n_pcof + 2] per call.
 * member_out3 and member_status (1: a step matrix of that member was singular) may each be NULL.  The same bits on every run.
 * The call leaves the stored sweep as qgd_eval_batch does (no later history_precomputed call may refer to it).
 * Refusals, before anything is launched and with the handle as it was:
 *   QGD_ERR_ARGUMENT     pcof or out2 NULL, gradient != 0 with grad NULL, n_pcof different from the control basis's
 *   QGD_ERR_STATE        no ensemble set, no control basis, gradient != 0 without a target
 *   QGD_ERR_UNSUPPORTED  a handle with a communicator or a partition; a problem the small-problem path does not take (N > 4,
 *                        more than 4 columns, a windowed time grid or more than 128 time points, n_pcof > 64, a dense guard
 *                        projector, qgd_set_small_path(h, 0), event bracketing on, control tables set by the caller): there is
 *                        no loop route inside the library -- evaluate the members on handles of their own
 *   QGD_ERR_MEMORY       not even one member's arrays fit the memory budget or the free device memory
 * QGD_ERR_NUMERIC: a step matrix of some member was singular.  The members' rows are written all the same (member_status says
 * which are valid); grad and out2 are unspecified.  DESIGN.md section 4m. */
int qgd_eval_ensemble(qgd_handle h, const double *pcof, int32_t n_pcof, int32_t gradient,
                      double *grad,           /* [n_pcof] or NULL when gradient == 0: sum_k w_k grad_k */
                      double *out2,           /* [2]: sum_k w_k cost_k, sum_k w_k guard_k */
                      double *member_grads,   /* [n_members][n_pcof] or NULL: not downloaded when NULL */
                      double *member_out3,    /* [n_members][3] or NULL */
                      int32_t *member_status  /* [n_members] or NULL */);

#ifdef __cplusplus
}
#endif
#endif
