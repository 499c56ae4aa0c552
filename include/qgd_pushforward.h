/* qgd_pushforward.h -- part of the C ABI of libqgd_hip.so, included by qgd.h (include that): the forward-mode half of the
 * derivative of the trajectory outputs, beside the pullbacks of qgd.h.  Additive: QGD_ABI_VERSION stays as it is.
 *
 * The entry point stands in a header and a host unit of its own (csrc/qgd_host_pushforward.cpp) because the list of entry
 * points of qgd.h is pinned, name by name, by the tests of the prologue and of the dead stream; what those tests ask of every
 * entry point -- a NULL handle is QGD_ERR_ARGUMENT, a dead stream QGD_ERR_COMM -- is asked of this one by its own tests.
 */
#ifndef QGD_PUSHFORWARD_H
#define QGD_PUSHFORWARD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Pushforward of directions in pcof to the trajectory outputs: J v for every column of v [n_pcof x n_vec] (column-major),
 * J = d output / d pcof, for the outputs asked for (each nullable, at least one):
 *   states_dot [2N, n_slots, n_cols, n_vec]              dw = [du; dv] = sum_l v_l dw/dpcof_l, the layout of qgd_eval_states
 *   pop_dot    [N or n_groups, n_slots, n_cols, n_vec]   2 (u_k du_k + v_k dv_k); with level_map [n_groups x N] (column-major)
 *                                                        sum_k level_map[g, k] pop_dot[k], k ascending
 *   expect_dot [n_obs, n_slots, n_cols, n_vec]           2 Re(psi^H O_j dpsi) of the observables obs_re + i obs_im
 *                                                        ([N x N x n_obs] column-major; obs_im NULL: real); as in
 *                                                        qgd_eval_expectations only the Hermitian part of what was passed
 *                                                        counts, and Hermiticity is not tested
 * all column-major with a trailing direction axis.  n_slots = 1 + nsteps / s with s of qgd_set_save_every, slot k at time
 * point k s; slot 0 is exact zeros (the initial state does not depend on pcof).
 * The call runs the forward sweep on the general two-point path (a small problem too) or, with history_precomputed under the
 * rule of qgd_discrete_adjoint, reuses the stored one; forms the stage derivatives and the forced basis responses where the
 * stored sweep does not have them yet; then, per chunk of directions, the direction table, ONE forced scan with the chunk's
 * directions side by side as column groups, and one pass over the state and tangent panels.  No adjoint sweep, no target.  pcof may be NULL when tables and basis were set
 * directly: the basis is then the Jacobian of the tables at the current coefficients.  Every sum runs in a fixed order without
 * atomics: the same bits on every run, and n_vec directions in one call are the bits of n_vec calls.
 * It leaves the stored sweep as qgd_eval_forward without an output array does, with the stage derivatives formed; lambda, the
 * guard forcing and the scalars are not touched; the kept setup of qgd_eval_hessian_vec stays valid when the sweep was reused.
 * Refusals, before anything is launched: QGD_ERR_ARGUMENT for NULL v, n_vec < 1, all three outputs NULL, level_map with
 * n_groups < 1, expect_dot without obs_re or with n_obs < 1, a pcof of another length; QGD_ERR_STATE without a control basis,
 * on a partitioned handle or one with a communicator, for history_precomputed without a previous forward evaluation;
 * QGD_ERR_UNSUPPORTED for a windowed time grid, N > 64, no control operators, more than 64 basis directions 2 n_ops order/2;
 * QGD_ERR_MEMORY when the buffers of one direction (its tangent history, the scan buffers, the staged outputs) and the forced
 * gradient's, where those are not there yet, do not fit the memory budget or the free device memory.  Directions ride along
 * in chunks of at most QGD_PUSHFORWARD_CHUNK (environment, read by qgd_create; default 256), fewer when the budget asks for it.
 * DESIGN.md section 4l. */
int qgd_eval_pushforward(qgd_handle h, const double *pcof, int32_t n_pcof, int32_t history_precomputed,
                         const double *v, int32_t n_vec,
                         double *states_dot,
                         double *pop_dot, const double *level_map, int32_t n_groups,
                         double *expect_dot, const double *obs_re, const double *obs_im, int32_t n_obs);

#ifdef __cplusplus
}
#endif
#endif
