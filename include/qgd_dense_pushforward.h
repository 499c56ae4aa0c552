/* qgd_dense_pushforward.h -- part of the C ABI of libqgd_hip.so, included by qgd.h (include that): the forward-mode half of the
 * derivative of the DENSE trajectory outputs, beside the pullback of the dense output of qgd.h and the grid-point pushforward of
 * qgd_pushforward.h.  Additive: QGD_ABI_VERSION stays as it is.
 *
 * The entry point stands in a header of its own for the reason given in qgd_pushforward.h (the list of entry points of qgd.h is
 * pinned, name by name, by the tests of the prologue and of the dead stream); its body is in csrc/qgd_host_pushforward.cpp beside
 * the grid-point call, whose helpers it shares.
 */
#ifndef QGD_DENSE_PUSHFORWARD_H
#define QGD_DENSE_PUSHFORWARD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Pushforward of directions in pcof to the dense trajectory outputs: J v for every column of v [n_pcof x n_vec] (column-major),
 * J = d output / d pcof of the outputs of qgd_eval_dense at `refine` points per step, for the outputs asked for (each nullable,
 * at least one), in the layouts and conventions of qgd_eval_pushforward with the slot axis of qgd_eval_dense:
 *   states_dot [2N, n_slots, n_cols, n_vec]              the tangent dd of the interpolated state d
 *   pop_dot    [N or n_groups, n_slots, n_cols, n_vec]   2 (u du + v dv) of d and dd, contracted with level_map when given
 *   expect_dot [n_obs, n_slots, n_cols, n_vec]           2 Re(d^H H_j dd), H_j the Hermitian part of obs_re + i obs_im
 * n_slots = 1 + nsteps * refine, slot k at time k dt / refine, whatever qgd_set_save_every says; slot 0 is exact zeros.
 * What is computed: with the state tangent dw_0(n) = s_v(n) of the forced scan and the tangent dA_d(t_n) of the assembled
 * operators along v (the direction table of the scan: no system term),
 *   dw_j(n) = (1/j) sum_{i<j} [ A_{j-1-i}(t_n) dw_i(n) + dA_{j-1-i}(t_n) w_i(n) ],  j = 1 .. order/2,
 * the tangent of the stage derivatives at every grid point, and the Hermite interpolant of qgd_eval_dense applied to them with the
 * same weights.  The result is the exact derivative of what qgd_eval_dense returns, the part through the control tables at the
 * grid points' own stage derivatives included: <ybar, J v> = <g, v> with g the gradient qgd_eval_dense_pullback returns for ybar.
 * What is reused: the sweep handling, the forced basis responses, the direction table and the forced scan of
 * qgd_eval_pushforward -- directions ride along in chunks of at most QGD_PUSHFORWARD_CHUNK, fewer when the memory budget asks for
 * it, the dense buffers counted; the interpolation kernel and weight table of qgd_eval_dense; the output kernels of
 * qgd_eval_pushforward on the dense panels.  Every sum runs in a fixed order without atomics: the same bits on every run, and
 * n_vec directions in one call are the bits of n_vec calls, whatever the chunk width.  The grid slots of states_dot are the bits
 * of qgd_eval_pushforward; refine = 1 is that call with every time point saved, for all three outputs.
 * What is left behind: the stored sweep as qgd_eval_forward without an output array leaves it, with the stage derivatives formed;
 * lambda, the guard forcing and the scalars are not touched; the kept setup of qgd_eval_hessian_vec stays valid when the sweep
 * was reused.
 * Refusals, before anything is launched: every refusal of qgd_eval_pushforward, each with its code (QGD_ERR_ARGUMENT for NULL v,
 * n_vec < 1, all three outputs NULL, level_map with n_groups < 1, expect_dot without obs_re or with n_obs < 1, a pcof of another
 * length; QGD_ERR_STATE without a control basis, on a partitioned handle or one with a communicator, for history_precomputed
 * without a previous forward evaluation; QGD_ERR_UNSUPPORTED for a windowed time grid, N > 64, no control operators, more than 64
 * basis directions 2 n_ops order/2); QGD_ERR_ARGUMENT for refine < 1 or 1 + nsteps * refine beyond a 32-bit integer;
 * QGD_ERR_UNSUPPORTED for refine > 1 at order > 16 (the interpolation kernels cover order/2 <= 8); QGD_ERR_MEMORY when the buffers
 * of one direction (tangent history, scan buffers, tangents of the stage derivatives, interpolated tangent panels, staged outputs)
 * and the forced gradient's, where those are not there yet, do not fit the memory budget or the free device memory.
 * DESIGN.md section 4n. */
int qgd_eval_dense_pushforward(qgd_handle h, const double *pcof, int32_t n_pcof, int32_t history_precomputed, int32_t refine,
                               const double *v, int32_t n_vec,
                               double *states_dot,
                               double *pop_dot, const double *level_map, int32_t n_groups,
                               double *expect_dot, const double *obs_re, const double *obs_im, int32_t n_obs);

#ifdef __cplusplus
}
#endif
#endif
