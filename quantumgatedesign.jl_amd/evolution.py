"""Host-side mirror of the reference's stepper / gradient entry points, calling the
C ABI (include/qgd.h) through ctypes.  Same names, argument meaning and error
behaviour as the reference:

  eval_forward(prob, controls, pcof; order, saveEveryNsteps)      forward_evolution.jl:15-29
  eval_forward_(uv_history, prob, controls, pcof; order)          forward_evolution.jl:33-70   (Julia eval_forward!)
  discrete_adjoint(prob, controls, pcof, target; order)           eval_grad_discrete_adjoint.jl:83-102
  discrete_adjoint_(grad, history, lambda_history, adjoint_forcing, prob, controls, pcof, target;
                    order, history_precomputed)                   eval_grad_discrete_adjoint.jl:107-160
  infidelity(...), infidelity_real, guard_penalty_real            infidelity.jl:7-96
  get_populations(history)                                        state_vector_helpers.jl:10-52
  eval_populations(prob, controls, pcof; order, saveEveryNsteps, level_map)   the same populations, formed on the device
  eval_expectations(prob, controls, pcof, observables; order, saveEveryNsteps)   Re(psi^H O psi) along the sweep, on the device
  eval_pullback(prob, controls, pcof; order, saveEveryNsteps, states_bar, populations_bar, level_map, expectations_bar,
                observables)                                       gradient of a cost written in those three outputs
  eval_dense(prob, controls, pcof; order, refine, output, level_map, observables)   the same outputs between the grid points
                                                                   (Hermite dense output; hermite_interpolate is its statement)
  discrete_adjoint_batch / eval_objective_batch(prob, controls, pcofs, target; order, cost_type)   many coefficient vectors in one
                                                                   call (qgd_eval_batch); member k = the single call on pcofs[k]

Julia's trailing ``!`` is spelled as a trailing underscore.  Arrays use the
reference's column-major layouts (numpy ``order="F"``).
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _lib
from .controls import as_control_list, control_basis, get_number_of_control_parameters


def _f(a):
    return np.asfortranarray(np.array(a, dtype=np.float64))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _check_out(a, shape, name):
    """Output arrays go to the C ABI as bare pointers: the shape, dtype and memory order the library will
    write must be exactly what it is given (the reference raises a DimensionMismatch here)."""
    if a is None:
        return None
    if not isinstance(a, np.ndarray) or a.dtype != np.float64 or a.shape != tuple(shape) or not a.flags.f_contiguous \
            or not a.flags.writeable:
        raise ValueError(f"{name} must be a writable float64 Fortran-ordered array of shape {tuple(shape)}; got "
                         f"{getattr(a, 'dtype', type(a))} {getattr(a, 'shape', None)}")
    return a


def complex_to_real(x):
    """state_vector_helpers.jl:72-74."""
    x = np.asarray(x)
    return np.asfortranarray(np.vstack([np.real(x), np.imag(x)]).astype(np.float64))


def real_to_complex(x):
    """state_vector_helpers.jl:78-87."""
    N = x.shape[0] // 2
    return x[:N] + 1j * x[N:]


def batch_pcofs(pcofs, n_pcof):
    """The coefficient vectors of a batch as the C ABI takes them: a C-contiguous float64 array ``[K, n_pcof]``.  Integer and
    Fortran-ordered input is converted, a single vector is a batch of one; anything else raises ValueError."""
    a = np.asarray(pcofs)
    if np.iscomplexobj(a):
        raise ValueError("pcofs must be real; got a complex array")
    if a.ndim > 2:
        raise ValueError(f"pcofs must be one vector or an array [K, n_pcof]; got {a.ndim} dimensions")
    try:
        a = np.ascontiguousarray(a, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"pcofs must be an array of real numbers: {e}") from None
    if a.ndim < 2:
        a = a.reshape(1, -1)
    if a.shape[0] < 1:
        raise ValueError("pcofs holds no member: a batch needs at least one coefficient vector")
    if a.shape[1] != n_pcof:
        raise ValueError(f"pcofs must have {n_pcof} coefficients per member; got {a.shape[1]}")
    return a


def finite_difference_points(pcof, dpcof):
    """The ``2n`` points of the centred differences of eval_grad_finite_difference as one batch ``[2n, n]``: row ``i`` is
    ``pcof + dpcof e_i``, row ``n + i`` is ``pcof - dpcof e_i`` (formed as ``pcof +- e`` with ``e = dpcof e_i``, the
    expression of the loop this replaces: the same bits)."""
    pcof = np.asarray(pcof, dtype=np.float64)
    e = np.zeros((len(pcof), len(pcof)))
    e[np.arange(len(pcof)), np.arange(len(pcof))] = dpcof
    return np.ascontiguousarray(np.vstack([pcof + e, pcof - e]))


def finite_difference_quotient(costs, dpcof):
    """``(c_plus - c_minus) / (2 dpcof)`` of the costs at finite_difference_points, in that order."""
    costs = np.asarray(costs, dtype=np.float64)
    n = len(costs) // 2
    return (costs[:n] - costs[n:]) / (2 * dpcof)


def objective_from_scalars(scalars, N_ess, plain):
    """The objective of every row of ``scalars [K, 3]`` (the three scalars of eval_forward): infidelity (``plain``) or the
    tracking / norm / state-transfer cost, plus the guard penalty -- the expression of eval_grad_finite_difference's cost."""
    sc = np.asarray(scalars, dtype=np.float64).reshape(-1, 3)
    a, b, guard = sc[:, 0], sc[:, 1], sc[:, 2]      # (:Tracking / :Norm / :StateTransfer: a is the cost itself, b = 0)
    return (1.0 - (a * a + b * b) / N_ess ** 2 if plain else a) + guard


COST_TYPES = {"Infidelity": 0, ":Infidelity": 0, "Tracking": 1, ":Tracking": 1, "Norm": 2, ":Norm": 2,
              "StateTransfer": 3, ":StateTransfer": 3}


class DeviceProblem:
    """One qgd handle: a SchrodingerProb resident on one GPU for one Hermite order."""

    def __init__(self, prob, order: int, device: int = 0, csc: bool = False, defer_grid: bool = False):
        """``csc=True`` hands the operators to the library as SparseMatrixCSC triples (qgd_create_csc), the
        form DispersiveProblem(sparse_rep=true) produces in the reference.  ``defer_grid=True`` (QGD_CREATE_DEFER_GRID):
        the time grid is not allocated by the constructor -- for a handle that is about to become a rank of a time
        partition (``comm_init``) and must never hold the whole grid first."""
        self.lib = _lib.lib()
        self.N = prob.N_tot_levels
        self.c = prob.N_initial_conditions
        self.n_ops = prob.N_operators
        self.order = int(order)
        self.m = self.order // 2
        self.nsteps = prob.nsteps
        self.tf = prob.tf
        N = self.N
        bufs = dict(
            ssym=_f(prob.system_sym), sasym=_f(prob.system_asym),
            sym=np.ascontiguousarray(np.stack([_f(o).T for o in prob.sym_operators])) if self.n_ops else np.zeros(1),
            asym=np.ascontiguousarray(np.stack([_f(o).T for o in prob.asym_operators])) if self.n_ops else np.zeros(1),
            u0=_f(prob.u0), v0=_f(prob.v0), guard=_f(prob.guard_subspace_projector))
        d = _lib.ProblemDesc(N, self.c, self.n_ops, prob.N_ess_levels, self.order, prob.nsteps, prob.tf,
                             _vp(bufs["ssym"]), _vp(bufs["sasym"]), _vp(bufs["sym"]), _vp(bufs["asym"]),
                             _vp(bufs["u0"]), _vp(bufs["v0"]), _vp(bufs["guard"]), device,
                             _lib.QGD_CREATE_DEFER_GRID if defer_grid else 0)
        h = C.c_void_p()
        if csc:
            from scipy.sparse import csc_matrix
            keep = []

            def triple(a):
                sp = csc_matrix(np.asarray(a))
                arrs = (sp.indptr.astype(np.int64), sp.indices.astype(np.int64), sp.data.astype(np.float64))
                keep.append(arrs)
                return _lib.CSC(_vp(arrs[0]), _vp(arrs[1]), _vp(arrs[2]), 0, 0)

            ssym, sasym = triple(prob.system_sym), triple(prob.system_asym)
            syms = (_lib.CSC * max(self.n_ops, 1))(*[triple(o) for o in prob.sym_operators])
            asyms = (_lib.CSC * max(self.n_ops, 1))(*[triple(o) for o in prob.asym_operators])
            rc = self.lib.qgd_create_csc(C.byref(d), C.byref(ssym), C.byref(sasym), syms, asyms, C.byref(h))
        else:
            rc = self.lib.qgd_create(C.byref(d), C.byref(h))
        _lib.check(None, rc)
        self.h = h
        self._finalizer = weakref.finalize(self, self.lib.qgd_destroy, h)
        self._basis_key = None
        self._target_key = None
        self.n_pcof = 0
        self.n_ess = prob.N_ess_levels
        self._operators = (tuple(prob.sym_operators), tuple(prob.asym_operators))      # (set_ensemble scales them per member)
        self._ensemble = None

    def close(self):
        self._finalizer()

    # -- setup -------------------------------------------------------------
    def set_nsteps(self, nsteps, tf):
        _lib.check(self.h, self.lib.qgd_set_nsteps(self.h, int(nsteps), float(tf)))
        self.nsteps, self.tf = int(nsteps), float(tf)
        self._basis_key = None

    def set_target(self, target):
        target = np.asarray(target)
        if target.ndim != 2 or target.shape[1] != self.c or target.shape[0] not in (self.N, 2 * self.N) \
                or (np.iscomplexobj(target) and target.shape[0] != self.N):
            raise ValueError(f"target must be [{self.N}, {self.c}] (complex or real) or the stacked real form "
                             f"[{2 * self.N}, {self.c}]; got {target.shape}")
        t = complex_to_real(target) if target.shape[0] == self.N else _f(target)
        key = t.tobytes()
        if key != self._target_key:
            _lib.check(self.h, self.lib.qgd_set_target(self.h, _vp(t)))
            self._target_key = key

    def set_controls(self, controls):
        cl = as_control_list(controls)
        if len(cl) != self.n_ops:
            raise ValueError(f"{len(cl)} controls for {self.n_ops} control operators")
        key = (tuple(id(c) for c in cl), self.nsteps, self.tf)
        if key == self._basis_key:
            return
        if not all(getattr(c, "is_linear", False) for c in cl):
            # general path (any AbstractControl): tables and their Jacobian at the current pcof are formed on the host
            # from the pointwise protocol at every evaluation (_upload_general)
            self._general = cl
            self._general_pcof = None
            self._basis_key = key
            self._controls_keepalive = cl
            self.n_pcof = int(sum(c.N_coeff for c in cl))
            return
        self._general = None
        Gp, Gq, _ = control_basis(cl, self.nsteps, self.tf, self.m)
        win = getattr(self, "window", None)
        if win is not None:                               # time-partitioned handle: the basis of the rank's own time points
            Gp = [np.ascontiguousarray(g[win[0]:win[1] + 1]) for g in Gp]
            Gq = [np.ascontiguousarray(g[win[0]:win[1] + 1]) for g in Gq]
        nco = np.array([c.N_coeff for c in cl], dtype=np.int32)
        gp_ptrs = (C.c_void_p * max(self.n_ops, 1))(*[_vp(g) for g in Gp])
        gq_ptrs = (C.c_void_p * max(self.n_ops, 1))(*[_vp(g) for g in Gq])
        _lib.check(self.h, self.lib.qgd_set_control_basis(self.h, _vp(nco), gp_ptrs, gq_ptrs))
        self._basis_key = key
        self._controls_keepalive = cl
        self.n_pcof = int(nco.sum())

    def _upload_general(self, pcof):
        """Non-linear controls: values and Jacobian of the control tables at this pcof (qgd.h: "Pair with
        qgd_set_control_basis holding the Jacobian at the current pcof when a gradient is wanted")."""
        pc = np.ascontiguousarray(pcof, dtype=np.float64)
        if len(pc) != self.n_pcof:
            raise ValueError("length of pcof does not match the controls")
        if self._general_pcof is not None and np.array_equal(pc, self._general_pcof):
            return
        from .controls import control_tables_general
        cl = self._general
        p, q, Gp, Gq = control_tables_general(cl, pc, self.nsteps, self.tf, self.m)
        nco = np.array([c.N_coeff for c in cl], dtype=np.int32)
        gp_ptrs = (C.c_void_p * max(self.n_ops, 1))(*[_vp(g) for g in Gp])
        gq_ptrs = (C.c_void_p * max(self.n_ops, 1))(*[_vp(g) for g in Gq])
        _lib.check(self.h, self.lib.qgd_set_control_basis(self.h, _vp(nco), gp_ptrs, gq_ptrs))
        _lib.check(self.h, self.lib.qgd_set_control_tables(self.h, _vp(p), _vp(q)))
        self._general_pcof = pc.copy()

    def set_control_tables(self, p_tables, q_tables):
        p, q = _f(p_tables), _f(q_tables)
        shape = (self.m + 1, self.n_ops, self.nsteps + 1)
        if p.shape != shape or q.shape != shape:
            raise ValueError(f"control tables must have shape {shape}")
        _lib.check(self.h, self.lib.qgd_set_control_tables(self.h, _vp(p), _vp(q)))

    # -- long time grids in bounded memory -----------------------------------
    def set_memory_budget(self, nbytes=0):
        """qgd_set_memory_budget: device bytes the per-time-point buffers may take (0 = automatic).  A grid that does not
        fit is processed in windows (same results to rounding, build + inverse done twice).  Re-allocates the grid."""
        _lib.check(self.h, self.lib.qgd_set_memory_budget(self.h, int(nbytes)))
        self._basis_key = None

    def memory_plan(self):
        out = np.zeros(4, dtype=np.int64)
        _lib.check(self.h, self.lib.qgd_get_memory_plan(self.h, _vp(out)))
        return dict(windows=int(out[0]), steps_per_window=int(out[1]), window_bytes=int(out[2]), budget=int(out[3]))

    # -- several GPUs behind one call (qgd_comm_init_rccl) -------------------
    def comm_init(self, unique_id: bytes, rank: int, world: int, shard: str = "time"):
        """Give the handle its RCCL communicator: discrete_adjoint / eval_forward become collective calls whose
        exchanges the library issues itself.  ``shard="time"``: this rank's window of the time grid (set the controls
        afterwards); ``"columns"``: the handle must have been created from this rank's columns."""
        if len(unique_id) != _lib.QGD_UNIQUE_ID_BYTES:
            raise ValueError("unique_id must be the 128 bytes of comm_unique_id()")
        code = {"time": _lib.QGD_SHARD_TIME, "columns": _lib.QGD_SHARD_COLUMNS}[shard]
        buf = C.create_string_buffer(bytes(unique_id), _lib.QGD_UNIQUE_ID_BYTES)
        _lib.check(self.h, self.lib.qgd_comm_init_rccl(self.h, buf, int(rank), int(world), code))
        self._basis_key = None
        self.window = None
        if shard == "time":
            part = np.zeros(8, dtype=np.int32)
            _lib.check(self.h, self.lib.qgd_get_partition(self.h, _vp(part)))
            self.window = (int(part[0]), int(part[1]))
            self.partition = dict(n_lo=int(part[0]), n_hi=int(part[1]), blocks=int(part[2]), blocks_per_rank=int(part[3]),
                                  block_len=int(part[4]), rank=int(part[5]), world=int(part[6]), nt=int(part[7]))

    def comm_destroy(self):
        _lib.check(self.h, self.lib.qgd_comm_destroy(self.h))

    def set_comm_timeout(self, milliseconds):
        """qgd_set_comm_timeout: the bound on the host wait of a collective evaluation; past it the communicator is
        aborted and the call raises QGDError(QGD_ERR_COMM)."""
        _lib.check(self.h, self.lib.qgd_set_comm_timeout(self.h, float(milliseconds)))

    def comm_info(self):
        out = (C.c_int32 * 3)()
        _lib.check(self.h, self.lib.qgd_comm_info(self.h, out))
        return dict(rank=out[0], world=out[1], shard="columns" if out[2] == _lib.QGD_SHARD_COLUMNS else "time")

    # -- evaluation --------------------------------------------------------
    def _hist_shape(self, save=1):
        win = getattr(self, "window", None)               # (a time-partitioned handle returns its own window)
        nt = self.nsteps + 1 if win is None else win[1] - win[0] + 1
        return (2 * self.N, self.m + 1, 1 + (nt - 1) // save, self.c)

    def set_save_every(self, save_every_nsteps=1):
        """eval_forward's saveEveryNsteps (forward_evolution.jl:104,239-241): uv_history of eval_forward then holds
        the time points 0, s, 2s, ... (qgd_set_save_every)."""
        save = int(save_every_nsteps)
        if save != getattr(self, "_save_every", 1):
            _lib.check(self.h, self.lib.qgd_set_save_every(self.h, save))
            self._save_every = save

    def pin(self, array):
        """Register (pin) an output array that will be handed to discrete_adjoint / eval_forward repeatedly
        (qgd_register_host_buffer): its downloads then run at PCIe speed.  Unpinned when the array dies."""
        if not isinstance(array, np.ndarray) or array.dtype != np.float64 or not array.flags.f_contiguous:
            raise ValueError("only float64 Fortran-ordered arrays can be pinned")
        key = (array.ctypes.data, array.nbytes)
        pins = self.__dict__.setdefault("_pins", {})
        if key in pins:
            return array
        _lib.check(self.h, self.lib.qgd_register_host_buffer(self.h, C.c_void_p(key[0]), key[1]))
        lib, h, fin = self.lib, self.h, self._finalizer

        def unpin(ptr=key[0]):
            pins.pop(key, None)
            if fin.alive:
                lib.qgd_unregister_host_buffer(h, C.c_void_p(ptr))
        pins[key] = weakref.finalize(array, unpin)
        return array

    def eval_forward(self, pcof=None, uv_history=None):
        _check_out(uv_history, self._hist_shape(getattr(self, "_save_every", 1)), "uv_history")
        out3 = np.zeros(3)
        if pcof is not None and getattr(self, "_general", None):
            self._upload_general(pcof)
            pcof = None                                   # (the tables are on the device)
        pc = None if pcof is None else np.ascontiguousarray(pcof, dtype=np.float64)
        _lib.check(self.h, self.lib.qgd_eval_forward(
            self.h, None if pc is None else _vp(pc), 0 if pc is None else len(pc),
            None if uv_history is None else _vp(uv_history), _vp(out3)))
        return out3

    # -- states, populations and expectation values alone (qgd_eval_states / qgd_eval_populations / qgd_eval_expectations) ---
    def observables_supported(self):
        """eval_states / eval_populations / eval_expectations are single-GPU calls: not for a handle with a communicator or a partition."""
        part = np.zeros(8, dtype=np.int32)
        _lib.check(self.h, self.lib.qgd_get_partition(self.h, _vp(part)))
        return part[6] == 1 and self.comm_info()["rank"] < 0

    def _slots(self):
        return 1 + self.nsteps // getattr(self, "_save_every", 1)

    def _pcof_arg(self, pcof):
        if pcof is not None and getattr(self, "_general", None):
            self._upload_general(pcof)
            pcof = None                                   # (the tables are on the device)
        pc = None if pcof is None else np.ascontiguousarray(pcof, dtype=np.float64)
        return pc, (None if pc is None else _vp(pc)), (0 if pc is None else len(pc))

    def eval_states(self, pcof=None, forcing=None, out=None):
        """The state trajectory alone, ``[2N, 1 + nsteps // save_every, n_cols]`` (Fortran order): Taylor index 0 of the
        ``uv_history`` of eval_forward, bit for bit, without the stage derivatives being formed or moved.  ``forcing``: as
        eval_forward_forced.  ``out``: an array to fill (e.g. a pinned one).  The scalars of the call are left in
        ``self.last_scalars``."""
        shape = (2 * self.N, self._slots(), self.c)
        fo = None
        if forcing is not None:
            fo = np.asfortranarray(forcing, dtype=np.float64)
            want = (2 * self.N, self.m, self.nsteps + 1, self.c)
            if fo.shape != want:
                raise ValueError(f"forcing must have shape {want}")
        out = np.zeros(shape, order="F") if out is None else _check_out(out, shape, "out")
        out3 = np.zeros(3)
        pc, ptr, n = self._pcof_arg(pcof)
        _lib.check(self.h, self.lib.qgd_eval_states(self.h, ptr, n, None if fo is None else _vp(fo), _vp(out), _vp(out3)))
        self.last_scalars = out3
        return out

    def eval_populations(self, pcof=None, level_map=None, history_precomputed=False, out=None):
        """Level populations along the sweep, formed on the device: ``[N, 1 + nsteps // save_every, n_cols]`` (what the
        reference's get_populations makes of uv_history), or with ``level_map`` ``[n_groups, N]`` the contraction
        ``level_map @ populations`` of every (time point, column), ``[n_groups, ..]`` (subsystem_population_map: per-qudit
        level populations).  ``history_precomputed``: reuse the stored forward sweep when it belongs to this pcof."""
        rows, lm = self.N, None
        if level_map is not None:
            lm = np.asarray(level_map)
            if lm.ndim != 2 or lm.shape[1] != self.N or lm.shape[0] < 1 or not np.issubdtype(lm.dtype, np.number) \
                    or np.iscomplexobj(lm):
                raise ValueError(f"level_map must be a real [n_groups >= 1, {self.N}] array; got {lm.dtype} {lm.shape}")
            lm = np.asfortranarray(lm, dtype=np.float64)
            rows = lm.shape[0]
        shape = (rows, self._slots(), self.c)
        out = np.zeros(shape, order="F") if out is None else _check_out(out, shape, "out")
        out3 = np.zeros(3)
        pc, ptr, n = self._pcof_arg(pcof)
        _lib.check(self.h, self.lib.qgd_eval_populations(self.h, ptr, n, 1 if history_precomputed else 0,
                                                         None if lm is None else _vp(lm), rows if lm is not None else 0,
                                                         _vp(out), _vp(out3)))
        self.last_scalars = out3
        return out

    def eval_expectations(self, observables, pcof=None, history_precomputed=False, out=None):
        """Expectation values ``Re(psi^H O_j psi)`` of Hermitian observables along the sweep, formed on the device:
        ``[n_obs, 1 + nsteps // save_every, n_cols]`` (Fortran order).  ``observables``: one ``[N, N]`` matrix, a sequence of
        them or an ``[n_obs, N, N]`` stack, real or complex, dense or scipy sparse (observable_planes).
        ``history_precomputed``: reuse the stored forward sweep when it belongs to this pcof.  The scalars of the call are left
        in ``self.last_scalars``."""
        re, im = observable_planes(observables, self.N)
        shape = (re.shape[2], self._slots(), self.c)
        out = np.zeros(shape, order="F") if out is None else _check_out(out, shape, "out")
        out3 = np.zeros(3)
        pc, ptr, n = self._pcof_arg(pcof)
        _lib.check(self.h, self.lib.qgd_eval_expectations(self.h, ptr, n, 1 if history_precomputed else 0, _vp(re),
                                                          None if im is None else _vp(im), re.shape[2], _vp(out), _vp(out3)))
        self.last_scalars = out3
        return out

    # -- Hermite dense output (qgd_eval_dense) ----------------------------------------------------------
    def _eval_dense(self, kind, rows, refine, pcof, history_precomputed, out, lm=None, re=None, im=None):
        shape = (rows, 1 + self.nsteps * refine, self.c)
        out = np.zeros(shape, order="F") if out is None else _check_out(out, shape, "out")
        out3 = np.zeros(3)
        pc, ptr, n = self._pcof_arg(pcof)
        opt = lambda a: None if a is None else _vp(a)
        _lib.check(self.h, self.lib.qgd_eval_dense(self.h, ptr, n, 1 if history_precomputed else 0, refine, kind, opt(lm),
                                                   0 if lm is None else lm.shape[0], opt(re), opt(im),
                                                   0 if re is None else re.shape[2], _vp(out), _vp(out3)))
        self.last_scalars = out3
        return out

    def eval_dense_states(self, refine, pcof=None, history_precomputed=False, out=None):
        """The state trajectory at ``refine`` points per step, ``[2N, 1 + nsteps * refine, n_cols]`` (Fortran order), slot k at
        time ``k * dt / refine``: the two-point Hermite interpolant of the stage derivatives the sweep forms anyway
        (hermite_interpolate is the statement of what the device computes), as accurate as the run itself.  Slots ``::refine``
        are the grid points, the bits eval_states returns.  Independent of set_save_every.  ``history_precomputed``: reuse the
        stored forward sweep when it belongs to this pcof.  The scalars of the call are left in ``self.last_scalars``."""
        refine = check_refine(refine)
        return self._eval_dense(0, 2 * self.N, refine, pcof, history_precomputed, out)

    def eval_dense_populations(self, refine, pcof=None, level_map=None, history_precomputed=False, out=None):
        """Level populations of the interpolated state (eval_dense_states), ``[N, 1 + nsteps * refine, n_cols]``, or with
        ``level_map`` ``[n_groups, N]`` their contraction ``[n_groups, ..]``, as eval_populations.  Between the grid points they
        sum to 1 only to the accuracy of the interpolant."""
        refine = check_refine(refine)
        rows, lm = self.N, None
        if level_map is not None:
            lm = np.asarray(level_map)
            if lm.ndim != 2 or lm.shape[1] != self.N or lm.shape[0] < 1 or not np.issubdtype(lm.dtype, np.number) \
                    or np.iscomplexobj(lm):
                raise ValueError(f"level_map must be a real [n_groups >= 1, {self.N}] array; got {lm.dtype} {lm.shape}")
            lm = np.asfortranarray(lm, dtype=np.float64)
            rows = lm.shape[0]
        return self._eval_dense(1, rows, refine, pcof, history_precomputed, out, lm=lm)

    def eval_dense_expectations(self, refine, observables, pcof=None, history_precomputed=False, out=None):
        """Expectation values ``Re(psi^H O_j psi)`` of the interpolated state (eval_dense_states),
        ``[n_obs, 1 + nsteps * refine, n_cols]``; ``observables`` as for eval_expectations."""
        refine = check_refine(refine)
        re, im = observable_planes(observables, self.N)
        return self._eval_dense(2, re.shape[2], refine, pcof, history_precomputed, out, re=re, im=im)

    def eval_pullback(self, pcof=None, states_bar=None, populations_bar=None, level_map=None, expectations_bar=None,
                      observables=None, history_precomputed=False):
        """Pullback of the trajectory outputs to pcof: ``grad[n_pcof]``, the sum over the parts given of
        ``<bar, d output / d pcof>`` with the cotangents ``states_bar`` (the shape of eval_states' result, or complex
        ``[N, n_slots, n_cols]``, split as complex_to_real does), ``populations_bar`` (eval_populations', with the same
        ``level_map``) and ``expectations_bar`` (eval_expectations', with the same ``observables``).  With ``bar = dJ/d output``
        this is the gradient of any cost J written in those outputs.  Honours set_save_every; slot 0 is ignored.
        ``history_precomputed``: reuse the stored forward sweep when it belongs to this pcof.  No target is needed."""
        sb, pb, lm, eb, re, im = pullback_cotangents(self.N, self._slots(), self.c, states_bar, populations_bar, level_map,
                                                     expectations_bar, observables)
        pc, ptr, n = self._pcof_arg(pcof)
        grad = np.zeros(self.n_pcof)
        opt = lambda a: None if a is None else _vp(a)
        _lib.check(self.h, self.lib.qgd_eval_pullback(self.h, ptr, n, 1 if history_precomputed else 0, opt(sb), opt(pb), opt(lm),
                                                      0 if lm is None else lm.shape[0], opt(eb), opt(re), opt(im),
                                                      0 if re is None else re.shape[2], _vp(grad)))
        return grad

    def eval_pushforward(self, pcof, v, states=False, populations=False, level_map=None, observables=None,
                         history_precomputed=False):
        """Pushforward of directions in pcof to the trajectory outputs: ``J v`` with
        ``J = d output / d pcof``, for ``v`` ``(n_pcof,)`` or ``(n_pcof, n_vec)`` (pushforward_directions).  Returns a dict of
        the parts asked for: ``"states"`` (``states=True``, the shape of eval_states' result), ``"populations"``
        (``populations=True``, or a ``level_map`` given: eval_populations' shape) and ``"expectations"`` (``observables`` given:
        eval_expectations' shape), each Fortran-ordered with a trailing direction axis, which a 1-D ``v`` drops.  The forward
        half of what eval_pullback transposes: ``<ybar, J v> = <eval_pullback(ybar), v>``.  All directions of a call share one
        forced scan.  Honours set_save_every; slot 0 is exact zeros.  ``history_precomputed``: reuse the stored forward sweep
        when it belongs to this pcof.  ``pcof=None``: tables and basis as they were set.  No target is needed."""
        cols, single = pushforward_directions(v, self.n_pcof)
        lm = None if level_map is None else level_map_array(level_map, self.N)
        re, im = (None, None) if observables is None else observable_planes(observables, self.N)
        if not (states or populations or lm is not None or re is not None):
            raise ValueError("eval_pushforward needs at least one of states, populations (or level_map), observables")
        tail = (self._slots(), self.c, cols.shape[1])
        out = {}
        if states:
            out["states"] = np.zeros((2 * self.N,) + tail, order="F")
        if populations or lm is not None:
            out["populations"] = np.zeros((self.N if lm is None else lm.shape[0],) + tail, order="F")
        if re is not None:
            out["expectations"] = np.zeros((re.shape[2],) + tail, order="F")
        pc, ptr, n = self._pcof_arg(pcof)
        opt = lambda a: None if a is None else _vp(a)
        _lib.check(self.h, self.lib.qgd_eval_pushforward(self.h, ptr, n, 1 if history_precomputed else 0, _vp(cols), cols.shape[1],
                                                         opt(out.get("states")), opt(out.get("populations")), opt(lm),
                                                         0 if lm is None else lm.shape[0], opt(out.get("expectations")), opt(re),
                                                         opt(im), 0 if re is None else re.shape[2]))
        return {key: (a[..., 0] if single else a) for key, a in out.items()}

    def eval_dense_pushforward(self, refine, pcof, v, states=False, populations=False, level_map=None, observables=None,
                               history_precomputed=False):
        """Pushforward of directions in pcof to the DENSE outputs: eval_pushforward for eval_dense_states,
        eval_dense_populations (same ``level_map``) and eval_dense_expectations (same ``observables``) at ``refine`` points per
        step.  Returns the dict of eval_pushforward, each part with ``1 + nsteps * refine`` slots and a trailing direction axis,
        which a 1-D ``v`` drops.  Exact for the interpolant: the part that reaches the stage derivatives through the control
        tables at their own grid point is included, so ``<ybar, J v> = <eval_dense_pullback(ybar), v>``.  Independent of
        set_save_every; slot 0 is exact zeros; the grid slots of ``"states"`` are eval_pushforward's bits and ``refine = 1`` is
        eval_pushforward of every grid point.  ``history_precomputed``: reuse the stored forward sweep when it belongs to this
        pcof.  ``pcof=None``: tables and basis as they were set.  No target is needed."""
        refine = check_refine(refine)
        cols, single = pushforward_directions(v, self.n_pcof)
        lm = None if level_map is None else level_map_array(level_map, self.N)
        re, im = (None, None) if observables is None else observable_planes(observables, self.N)
        if not (states or populations or lm is not None or re is not None):
            raise ValueError("eval_dense_pushforward needs at least one of states, populations (or level_map), observables")
        tail = (1 + self.nsteps * refine, self.c, cols.shape[1])
        out = {}
        if states:
            out["states"] = np.zeros((2 * self.N,) + tail, order="F")
        if populations or lm is not None:
            out["populations"] = np.zeros((self.N if lm is None else lm.shape[0],) + tail, order="F")
        if re is not None:
            out["expectations"] = np.zeros((re.shape[2],) + tail, order="F")
        pc, ptr, n = self._pcof_arg(pcof)
        opt = lambda a: None if a is None else _vp(a)
        _lib.check(self.h, self.lib.qgd_eval_dense_pushforward(self.h, ptr, n, 1 if history_precomputed else 0, refine, _vp(cols),
                                                               cols.shape[1], opt(out.get("states")), opt(out.get("populations")),
                                                               opt(lm), 0 if lm is None else lm.shape[0],
                                                               opt(out.get("expectations")), opt(re), opt(im),
                                                               0 if re is None else re.shape[2]))
        return {key: (a[..., 0] if single else a) for key, a in out.items()}

    def eval_dense_pullback(self, refine, pcof=None, states_bar=None, populations_bar=None, level_map=None,
                            expectations_bar=None, observables=None, history_precomputed=False):
        """Pullback of the DENSE outputs to pcof: eval_pullback for a cost written on eval_dense_states,
        eval_dense_populations (same ``level_map``) and eval_dense_expectations (same ``observables``) at ``refine`` points per
        step -- the cotangents have those results' shapes, ``[.., 1 + nsteps * refine, n_cols]``.  ``grad[n_pcof]``, exact for
        the interpolant: the part that reaches pcof through the control tables at the grid points' own stage derivatives is
        included.  Independent of set_save_every; slot 0 is ignored; ``refine = 1`` is eval_pullback of every grid point.
        ``history_precomputed``: reuse the stored forward sweep when it belongs to this pcof.  No target is needed."""
        refine = check_refine(refine)
        sb, pb, lm, eb, re, im = pullback_cotangents(self.N, 1 + self.nsteps * refine, self.c, states_bar, populations_bar,
                                                     level_map, expectations_bar, observables)
        pc, ptr, n = self._pcof_arg(pcof)
        grad = np.zeros(self.n_pcof)
        opt = lambda a: None if a is None else _vp(a)
        _lib.check(self.h, self.lib.qgd_eval_dense_pullback(self.h, ptr, n, 1 if history_precomputed else 0, refine, opt(sb),
                                                            opt(pb), opt(lm), 0 if lm is None else lm.shape[0], opt(eb), opt(re),
                                                            opt(im), 0 if re is None else re.shape[2], _vp(grad)))
        return grad

    def discrete_adjoint(self, pcof, history_precomputed=False, uv_history=None, lambda_history=None,
                         adjoint_forcing=None):
        if getattr(self, "_general", None):
            self._upload_general(pcof)
            _check_out(uv_history, self._hist_shape(), "history")
            _check_out(lambda_history, self._hist_shape(), "lambda_history")
            _check_out(adjoint_forcing, (2 * self.N, self.nsteps + 1, self.c), "adjoint_forcing")
            grad = np.zeros(self.n_pcof)
            out3 = np.zeros(3)
            _lib.check(self.h, self.lib.qgd_discrete_adjoint(
                self.h, None, 0, 1 if history_precomputed else 0, _vp(grad),
                None if uv_history is None else _vp(uv_history),
                None if lambda_history is None else _vp(lambda_history),
                None if adjoint_forcing is None else _vp(adjoint_forcing), _vp(out3)))
            return grad, out3
        if uv_history is None and lambda_history is None and adjoint_forcing is None and len(pcof) == self.n_pcof:
            # the optimiser's call: persistent host buffers with cached pointers (three ndarray.ctypes look-ups
            # cost 6 us, 1.5 % of a cnot3 evaluation)
            io = self.__dict__.get("_io")
            if io is None or len(io[0]) != self.n_pcof:
                bufs = (np.zeros(self.n_pcof), np.zeros(self.n_pcof), np.zeros(3))
                io = self._io = bufs + tuple(_vp(b) for b in bufs)
            io[0][:] = pcof
            rc = self.lib.qgd_discrete_adjoint(self.h, io[3], self.n_pcof, 1 if history_precomputed else 0, io[4],
                                               None, None, None, io[5])
            if rc:
                _lib.check(self.h, rc)
            return io[1].copy(), io[2].copy()
        _check_out(uv_history, self._hist_shape(), "history")
        _check_out(lambda_history, self._hist_shape(), "lambda_history")
        _check_out(adjoint_forcing, (2 * self.N, self._hist_shape()[2], self.c), "adjoint_forcing")
        pc = np.ascontiguousarray(pcof, dtype=np.float64)
        grad = np.zeros(len(pc))
        out3 = np.zeros(3)
        _lib.check(self.h, self.lib.qgd_discrete_adjoint(
            self.h, _vp(pc), len(pc), 1 if history_precomputed else 0, _vp(grad),
            None if uv_history is None else _vp(uv_history),
            None if lambda_history is None else _vp(lambda_history),
            None if adjoint_forcing is None else _vp(adjoint_forcing), _vp(out3)))
        return grad, out3

    def eval_batch(self, pcofs, gradient=True, out_grads=None, out_scalars=None):
        """qgd_eval_batch: ``K`` coefficient vectors ``pcofs [K, n_pcof]`` in one call.  Member ``k`` gets bit for bit what
        ``discrete_adjoint(pcofs[k])`` (``gradient=False``: ``eval_forward(pcofs[k])``) returns on this handle.  Returns
        ``(grads [K, n_pcof] or None, scalars [K, 3], status [K] int32)``; ``status[k] = 1`` where a step matrix of member
        ``k`` was singular -- that alone raises nothing here, the other members are valid.  Small problems (set_small_path) run
        their members side by side, everything else one after another inside the library (batch_path_taken)."""
        P = batch_pcofs(pcofs, self.n_pcof)
        K = P.shape[0]
        for a, shape, name in ((out_grads, (K, self.n_pcof), "out_grads"), (out_scalars, (K, 3), "out_scalars")):
            if a is not None and (not isinstance(a, np.ndarray) or a.dtype != np.float64 or a.shape != shape
                                  or not a.flags.c_contiguous or not a.flags.writeable):
                raise ValueError(f"{name} must be a writable C-contiguous float64 array of shape {shape}")
        grads = (np.zeros((K, self.n_pcof)) if out_grads is None else out_grads) if gradient else None
        scalars = np.zeros((K, 3)) if out_scalars is None else out_scalars
        status = np.zeros(K, dtype=np.int32)
        if getattr(self, "_general", None):               # non-linear controls: tables from the host at every member
            for k in range(K):
                if gradient:
                    grads[k], scalars[k] = self.discrete_adjoint(P[k])
                else:
                    scalars[k] = self.eval_forward(P[k])
            return grads, scalars, status
        rc = self.lib.qgd_eval_batch(self.h, _vp(P), K, self.n_pcof, None if grads is None else _vp(grads), _vp(scalars),
                                     _vp(status))
        if rc != _lib.QGD_ERR_NUMERIC:
            _lib.check(self.h, rc)
        return grads, scalars, status

    def set_ensemble(self, ensemble):
        """qgd_set_ensemble: the members of ``ensemble`` (an ``Ensemble`` of this problem's size) become the handle's -- their
        system Hamiltonians and the control operators ``op_scale[k, o] * operator_o`` (``Ensemble.operator_arrays``: the
        arithmetic of ``member_problem``), and ``effective_weights()``.  ``None`` releases them.  Skipped when this very object
        is already set; the library forgets an ensemble whenever the control basis or the time grid is set, so call this after
        ``set_controls``."""
        if ensemble is None:
            self._ensemble = None
            _lib.check(self.h, self.lib.qgd_set_ensemble(self.h, 0, None, None, None, None, None))
            return
        ent = self._ensemble
        if ent is not None and ent[0]() is ensemble and ent[1] is self._basis_key and ent[1] is not None:
            return
        if ensemble.N != self.N:
            raise ValueError(f"ensemble: the members have {ensemble.N} levels, the problem {self.N}")
        ss, sa, so, ao, w = ensemble.operator_arrays(*self._operators)
        self._ensemble = None
        _lib.check(self.h, self.lib.qgd_set_ensemble(self.h, ensemble.K, _vp(ss), _vp(sa), _vp(so) if self.n_ops else None,
                                                     _vp(ao) if self.n_ops else None, _vp(w)))
        self._ensemble = (weakref.ref(ensemble), self._basis_key, ensemble.K)

    def eval_ensemble(self, pcof, gradient=True, rows=True):
        """qgd_eval_ensemble: ``pcof`` over the members set by ``set_ensemble``, side by side on the device, under the handle's
        controls, target and cost type.  Returns ``(grad or None, cost, guard, member_grads, member_out3, status)``: the weighted
        sums (``ensemble_reduce`` is their statement, bit for bit) and, with ``rows``, the members' rows ``[K, n_pcof]`` (None
        without a gradient) and ``[K, 3]``, each what a handle made for that member returns; ``rows=False`` downloads neither
        (both None).  ``status [K]`` int32 is 1 where a step matrix of that member was singular: that raises QGD_ERR_NUMERIC."""
        if self._ensemble is None or self._ensemble[1] is not self._basis_key or self._basis_key is None:
            raise _lib.QGDError(_lib.QGD_ERR_STATE, "set_ensemble must be called before eval_ensemble (and after set_controls)")
        K = self._ensemble[2]
        pc = np.ascontiguousarray(pcof, dtype=np.float64)
        if pc.shape != (self.n_pcof,):
            raise ValueError(f"pcof must have shape ({self.n_pcof},); got {pc.shape}")
        grad = np.zeros(self.n_pcof) if gradient else None
        out2 = np.zeros(2)
        mg = np.zeros((K, self.n_pcof)) if rows and gradient else None
        mo = np.zeros((K, 3)) if rows else None
        status = np.zeros(K, dtype=np.int32)
        rc = self.lib.qgd_eval_ensemble(self.h, _vp(pc), self.n_pcof, 1 if gradient else 0, None if grad is None else _vp(grad),
                                        _vp(out2), None if mg is None else _vp(mg), None if mo is None else _vp(mo), _vp(status))
        _lib.check(self.h, rc)
        return grad, float(out2[0]), float(out2[1]), mg, mo, status

    def batch_path_taken(self):
        """Which route the last eval_batch call took: True the members side by side, False one after another."""
        return bool(self.intermediate("batch_path")[0])

    def eval_adjoint(self, pcof, terminal_condition, forcing=None):
        if getattr(self, "_general", None):
            self._upload_general(pcof)
            pcof = np.zeros(0)                            # (NULL pcof: the tables are on the device)
        pc = np.ascontiguousarray(pcof, dtype=np.float64)
        term = _f(terminal_condition).reshape(2 * self.N, self.c, order="F")
        fo = None if forcing is None else _f(forcing)
        if fo is not None and fo.shape != (2 * self.N, self.nsteps + 1, self.c):
            raise ValueError(f"forcing must have shape {(2 * self.N, self.nsteps + 1, self.c)}")
        lam = np.zeros((2 * self.N, self.m + 1, self.nsteps + 1, self.c), order="F")
        _lib.check(self.h, self.lib.qgd_eval_adjoint(self.h, _vp(pc) if len(pc) else None, len(pc), _vp(term),
                                                     None if fo is None else _vp(fo), _vp(lam)))
        return lam

    def set_cost_type(self, cost_type="Infidelity"):
        """cost_type of discrete_adjoint / eval_grad_forced (eval_grad_discrete_adjoint.jl:26-35): ``Infidelity``,
        ``Tracking`` (0.5 |w_N - target|^2), ``Norm`` (0.5 |w_N|^2) or ``StateTransfer`` (the per-column infidelity
        1 - mean_j |t_j^H psi_j|^2, ``state_transfer_infidelity``: every column may arrive with a phase of its own); a
        leading ':' as in Julia is accepted.  Anything else raises like the reference ("Invalid cost type")."""
        code = COST_TYPES.get(str(cost_type))
        if code is None:
            raise ValueError(f"Invalid cost type: {cost_type}")
        if code != getattr(self, "_cost_type", 0):
            _lib.check(self.h, self.lib.qgd_set_cost_type(self.h, code))
            self._cost_type = code

    def column_overlaps(self):
        """The overlaps ``o_j = t_j^H psi_j`` (complex, one per column) of the final state of the stored sweep with the
        target, whatever the cost type (qgd_get_intermediate "column_overlaps")."""
        ab = self.intermediate("column_overlaps")
        return ab[:, 0] - 1j * ab[:, 1]

    def column_fidelities(self):
        """``|o_j|^2`` of every column: ``1 - mean(column_fidelities())`` is the ``StateTransfer`` cost."""
        return np.abs(self.column_overlaps()) ** 2

    def set_small_path(self, on=True):
        """qgd_set_small_path: the four-launch evaluation of small problems (N <= 4: Rabi, cnot2) on / off for this handle."""
        _lib.check(self.h, self.lib.qgd_set_small_path(self.h, 1 if on else 0))

    def small_path_taken(self):
        """Whether the last evaluation of this handle ran on the small-problem path."""
        return bool(self.intermediate("small_path")[0])

    def front_path_taken(self):
        """Did the last forward evaluation take the fused front (csrc/qgd_front.h: same-point step propagators)?"""
        return bool(self.intermediate("front_path")[0])

    def set_lambda_derivatives(self, on=True):
        """Fill ``lambda_history[:, 1:, :, :]`` as the reference leaves it (forward_evolution.jl:427-433, :471-480):
        the adjoint derivatives of lambda_n with the controls at t_{n-1} (t_1 for n = 1).  Off by default -- nothing
        reads these columns, and they make the lambda download 1+m times as large."""
        _lib.check(self.h, self.lib.qgd_set_lambda_derivatives(self.h, 1 if on else 0))

    def apply_hamiltonian(self, w, time_index=0, derivative_order=0, use_adjoint=False):
        w = _f(w).reshape(2 * self.N, self.c, order="F")
        out = np.zeros_like(w, order="F")
        _lib.check(self.h, self.lib.qgd_apply_hamiltonian(self.h, time_index, derivative_order,
                                                          1 if use_adjoint else 0, _vp(w), _vp(out)))
        return out

    def intermediate(self, name):
        need = C.c_size_t()
        _lib.check(self.h, self.lib.qgd_get_intermediate(self.h, name.encode(), None, 0, C.byref(need)))
        out = np.zeros(need.value)
        _lib.check(self.h, self.lib.qgd_get_intermediate(self.h, name.encode(), _vp(out), need.value, C.byref(need)))
        nt = self.nsteps + 1
        if name in ("L", "R", "Linv", "P"):
            z = out.reshape(nt, self.N, self.N, 2)
            return z[..., 0] + 1j * z[..., 1]
        if name == "repivoted":
            return int(out[0])
        if name == "column_overlaps":
            return out.reshape(self.c, 2)
        if name in ("selection", "small_path", "front_path", "batch_path"):
            return out
        if name == "sigma":
            return out.reshape(nt, self.n_ops, self.m, 2)
        return out.reshape(nt, self.m + 1, self.n_ops, 2)

    def set_timing(self, mode, phase=None):
        """0: no events, 1: every phase (default), 2: only ``phase``."""
        _lib.check(self.h, self.lib.qgd_set_timing(self.h, int(mode), None if phase is None else phase.encode()))

    def eval_forward_forced(self, pcof, forcing, uv_history=None):
        """eval_forward with a forcing array ``[2N, order/2, 1+nsteps, n_cols]`` (Fortran order): the scaled
        Taylor coefficients of the forcing at every time point (forward_evolution.jl:118-129)."""
        if getattr(self, "_general", None):
            self._upload_general(pcof)
            pcof = np.zeros(0)
        pcof = np.ascontiguousarray(pcof, dtype=np.float64)
        forcing = np.asfortranarray(forcing, dtype=np.float64)
        want = (2 * self.N, self.m, self.nsteps + 1, self.c)
        if forcing.shape != want:
            raise ValueError(f"forcing must have shape {want}")
        _check_out(uv_history, self._hist_shape(getattr(self, "_save_every", 1)), "uv_history")
        out3 = np.zeros(3)
        _lib.check(self.h, self.lib.qgd_eval_forward_forced(self.h, _vp(pcof) if len(pcof) else None, len(pcof), _vp(forcing),
                                                             None if uv_history is None else _vp(uv_history), _vp(out3)))
        return out3

    def eval_grad_forced(self, pcof):
        """Gradient by forward sensitivities (eval_grad_forced.jl:17-194); needs controls and target."""
        if getattr(self, "_general", None):               # tables and Jacobian at this pcof are uploaded; NULL pcof
            self._upload_general(pcof)
            grad = np.zeros(self.n_pcof)
            _lib.check(self.h, self.lib.qgd_eval_grad_forced(self.h, None, 0, _vp(grad)))
            return grad
        pcof = np.ascontiguousarray(pcof, dtype=np.float64)
        grad = np.zeros(len(pcof))
        _lib.check(self.h, self.lib.qgd_eval_grad_forced(self.h, _vp(pcof), len(pcof), _vp(grad)))
        return grad

    def eval_hessian(self, pcof, grad=None):
        """Exact Hessian of the objective at pcof, [n_pcof, n_pcof] symmetric; ``grad``: an optional
        float64 array of n_pcof that receives the forced gradient.  Needs controls linear in pcof and the target."""
        if getattr(self, "_general", None):
            raise NotImplementedError("eval_hessian(method='exact') needs controls that are linear in pcof (is_linear = True)")
        pcof = np.ascontiguousarray(pcof, dtype=np.float64)
        hess = np.zeros((len(pcof), len(pcof)))
        if grad is not None:
            _check_out(grad, (len(pcof),), "grad")
        _lib.check(self.h, self.lib.qgd_eval_hessian(self.h, _vp(pcof), len(pcof), _vp(hess), None if grad is None else _vp(grad)))
        return hess

    def eval_hessian_vec(self, pcof, v, grad=None):
        """Exact Hessian-vector product(s) H v at pcof by a second-order adjoint sweep, without forming
        H.  ``v``: (n_pcof,) or (n_pcof, k); the result has the same shape.  ``grad``: an optional float64 array of n_pcof that
        receives the adjoint gradient.  What does not depend on v stays on the handle: further calls with the same pcof cost
        one forced sweep with a single direction and one adjoint sweep each.  Needs controls linear in pcof and the target."""
        if getattr(self, "_general", None):
            raise NotImplementedError("eval_hessian_vec needs controls that are linear in pcof (is_linear = True)")
        pcof = np.ascontiguousarray(pcof, dtype=np.float64)
        v = np.asarray(v, dtype=np.float64)
        if v.ndim not in (1, 2) or v.shape[0] != len(pcof):
            raise ValueError(f"v must have shape ({len(pcof)},) or ({len(pcof)}, k)")
        cols = np.asfortranarray(v.reshape(len(pcof), -1))
        hv = np.zeros(cols.shape, order="F")
        if grad is not None:
            _check_out(grad, (len(pcof),), "grad")
        _lib.check(self.h, self.lib.qgd_eval_hessian_vec(self.h, _vp(pcof), len(pcof), _vp(cols) if cols.size else None, cols.shape[1],
                                                          _vp(hv) if hv.size else None, None if grad is None else _vp(grad)))
        return hv.reshape(v.shape) if v.ndim == 1 else np.ascontiguousarray(hv)

    def set_operator_path(self, mode):
        """"auto" | "dense" (fp64 MFMA kernels) | "sparse" (ELL kernels; raises if the operators do not qualify)."""
        code = {"auto": 0, "dense": 1, "sparse": 2}[mode]
        _lib.check(self.h, self.lib.qgd_set_operator_path(self.h, code))

    def operator_path(self):
        """(path in use, entries per row of the union pattern, entries per row of the widest control)."""
        out = (C.c_int32 * 3)()
        _lib.check(self.h, self.lib.qgd_get_operator_path(self.h, out))
        return ("sparse" if out[0] == 2 else "dense", out[1], out[2])

    def timings(self):
        cap = 32
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = C.c_int32()
        _lib.check(self.h, self.lib.qgd_get_timings(self.h, names, ms, cap, C.byref(n)))
        return {names[i].decode(): ms[i] for i in range(min(n.value, cap))}


# ---------------------------------------------------------------------------
# handle cache: one DeviceProblem per (prob object, order)
# ---------------------------------------------------------------------------
_cache: dict = {}


try:
    from xxhash import xxh3_64_intdigest as _digest          # ~10 GB/s
except ImportError:                                           # pragma: no cover
    from zlib import crc32 as _digest


def _fingerprint(prob):
    """Digest of the fields a handle copies to the device at creation (operators, initial conditions,
    guard): a prob mutated in place gets a fresh handle instead of a stale device copy.  Arrays up to 1 MB are
    hashed whole, larger ones through 65536 evenly spaced elements (the digest runs on every reference-shaped
    call: ~40 us for a cnot3 problem)."""
    h = 0
    for a in (prob.system_sym, prob.system_asym, prob.u0, prob.v0, prob.guard_subspace_projector,
              *prob.sym_operators, *prob.asym_operators):
        a = np.asarray(a)
        flat = a.reshape(-1, order="A") if (a.flags.f_contiguous or a.flags.c_contiguous) else np.ascontiguousarray(a).reshape(-1)
        if flat.nbytes > (1 << 20):
            flat = np.ascontiguousarray(flat[:: max(1, flat.size // 65536)])
        h = (h * 1000003) ^ _digest(flat.view(np.uint8).data) ^ hash(a.shape)
    return (h, prob.N_tot_levels, prob.N_initial_conditions, prob.N_ess_levels, prob.N_operators)


def _evict(key):
    ent = _cache.pop(key, None)
    if ent is not None:
        ent[1].close()


def device_problem(prob, order: int, device: int = 0) -> DeviceProblem:
    """The handle of (prob, order) -- created on first use, released when ``prob`` is garbage-collected
    (or by release(prob) / clear_cache()), re-created when prob's operators or initial conditions changed."""
    key = (id(prob), int(order), device)
    ent = _cache.get(key)
    fp = _fingerprint(prob)
    if ent is not None and ent[0]() is prob and ent[2] == fp:
        dp = ent[1]
        if dp.nsteps != prob.nsteps or dp.tf != prob.tf:
            dp.set_nsteps(prob.nsteps, prob.tf)
        return dp
    if ent is not None:
        _evict(key)
    dp = DeviceProblem(prob, order, device)
    _cache[key] = (weakref.ref(prob), dp, fp)
    weakref.finalize(prob, _evict, key)
    return dp


def release(prob):
    """Close every cached handle of ``prob`` (all orders, all devices)."""
    for key in [k for k, ent in _cache.items() if k[0] == id(prob) and ent[0]() is prob]:
        _evict(key)


def clear_cache():
    for key in list(_cache):
        _evict(key)


# ---------------------------------------------------------------------------
# reference-shaped API
# ---------------------------------------------------------------------------
def _history_shape(prob, order, saveEveryNsteps=1):
    return (prob.real_system_size, 1 + order // 2, 1 + prob.nsteps // saveEveryNsteps, prob.N_initial_conditions)


def eval_forward_(uv_history, prob, controls, pcof, order=2, saveEveryNsteps=1, forcing=None):
    """eval_forward! (forward_evolution.jl:33-70): fills ``uv_history``
    ``[2N, 1+order/2, 1+nsteps, N_initial_conditions]`` (Fortran order) in place."""
    save = int(saveEveryNsteps)
    if save < 1:
        raise ValueError("saveEveryNsteps must be a positive integer")
    shape = _history_shape(prob, order, save)
    if uv_history.shape != shape or not uv_history.flags.f_contiguous:
        raise ValueError(f"uv_history must be Fortran-ordered with shape {shape}")
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    run = dp.eval_forward if forcing is None else (lambda p, hist: dp.eval_forward_forced(p, forcing, hist))
    # the device keeps every time point; the stored ones are n = 0, save, 2 save, ... <= nsteps
    # (forward_evolution.jl:104,178,239-241: slot 1 + div(n, saveEveryNsteps) when n % saveEveryNsteps == 0): the
    # library's re-layout kernel reads them with that stride (qgd_set_save_every)
    dp.set_save_every(save)
    try:
        run(pcof, uv_history)
    finally:
        dp.set_save_every(1)
    return None


def eval_forward(prob, controls, pcof, order=2, saveEveryNsteps=1, forcing=None):
    """forward_evolution.jl:15-29: complex state history ``[N, 1+nsteps, N_initial_conditions]``."""
    dp = device_problem(prob, order) if int(saveEveryNsteps) >= 1 else None
    if dp is None or not dp.observables_supported():
        hist = np.zeros(_history_shape(prob, order, int(saveEveryNsteps)), order="F")
        eval_forward_(hist, prob, controls, pcof, order=order, saveEveryNsteps=saveEveryNsteps, forcing=forcing)
        return real_to_complex(hist[:, 0, :, :])
    # the states are all that is returned: they alone are laid out and downloaded (qgd_eval_states), the same bits
    dp.set_controls(controls)
    dp.set_save_every(int(saveEveryNsteps))
    try:
        return real_to_complex(dp.eval_states(pcof, forcing=forcing))
    finally:
        dp.set_save_every(1)


def get_populations(history):
    """get_populations (state_vector_helpers.jl:10-52): level populations ``u^2 + v^2`` of a real history array
    ``[2N, 1+m, nt]`` or ``[2N, 1+m, nt, n_cols]`` -> ``[N, nt]`` / ``[N, nt, n_cols]``; the derivative axis is dropped.
    Host arithmetic on an array that is already there; eval_populations forms the same on the device."""
    h = np.asarray(history)
    if h.ndim not in (3, 4) or not np.issubdtype(h.dtype, np.floating) or h.shape[0] % 2:
        raise ValueError("history must be a real array [2N, 1+m, nt] or [2N, 1+m, nt, n_cols]")
    N = h.shape[0] // 2
    return np.asfortranarray(h[:N, 0] ** 2 + h[N:, 0] ** 2)


def subsystem_population_map(subsystem_sizes):
    """The 0/1 map ``[sum(sizes), prod(sizes)]`` of per-subsystem level populations for eval_populations: row
    ``sum(sizes[:q]) + l`` adds up the levels of the full system whose subsystem q is in level l.  Digit order of
    lowering_operators_system / basis_state: the first subsystem is the slowest digit of the level index."""
    sizes = [int(s) for s in subsystem_sizes]
    if not sizes or any(s < 1 for s in sizes):
        raise ValueError("subsystem_sizes must be positive integers")
    N = int(np.prod(sizes))
    M = np.zeros((sum(sizes), N), order="F")
    idx, row, stride = np.arange(N), 0, N
    for s in sizes:
        stride //= s
        M[row + (idx // stride) % s, idx] = 1.0
        row += s
    return M


def eval_populations(prob, controls, pcof, order=2, saveEveryNsteps=1, level_map=None):
    """Level populations along the forward sweep, ``[N, 1 + nsteps // saveEveryNsteps, N_initial_conditions]`` -- what
    ``get_populations`` makes of the history of eval_forward_ -- or, with ``level_map`` ``[n_groups, N]``, their contraction
    ``[n_groups, ..]``, formed on the device: neither the stage derivatives nor the states leave it."""
    save = int(saveEveryNsteps)
    if save < 1:
        raise ValueError("saveEveryNsteps must be a positive integer")
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    dp.set_save_every(save)
    try:
        return dp.eval_populations(pcof, level_map=level_map)
    finally:
        dp.set_save_every(1)


def observable_planes(observables, N):
    """Observables for eval_expectations as the planes the library takes: ``(obs_re, obs_im)``, Fortran-ordered float64
    ``[N, N, n_obs]`` with ``O_j = obs_re[:, :, j] + 1j * obs_im[:, :, j]``; ``obs_im`` is None when every imaginary part is
    exactly zero.  ``observables``: one ``[N, N]`` matrix, a sequence of them or an ``[n_obs, N, N]`` stack, real or complex;
    scipy sparse matrices are densified.  ValueError for a wrong shape, a non-numeric dtype or a matrix that is not
    Hermitian: ``max|O - O^H| > 1e-12 max(1, max|O|)`` (the library itself returns the expectation of the Hermitian part)."""
    def dense(o):
        return o.toarray() if hasattr(o, "toarray") else o

    obs = dense(observables)
    if isinstance(obs, (list, tuple)):
        obs = [np.asarray(dense(o)) for o in obs]
        if not obs or any(o.shape != obs[0].shape for o in obs):
            raise ValueError(f"observables must be [{N}, {N}] matrices")
    try:
        stack = np.asarray(obs)
    except ValueError as e:
        raise ValueError(f"observables must be [{N}, {N}] matrices") from e
    if stack.dtype == bool or not np.issubdtype(stack.dtype, np.number):
        raise ValueError(f"observables must be numeric; got dtype {stack.dtype}")
    if stack.ndim == 2:
        stack = stack[None]
    if stack.ndim != 3 or stack.shape[0] < 1 or stack.shape[1:] != (N, N):
        raise ValueError(f"observables must be one [{N}, {N}] matrix, a sequence of them or an [n_obs, {N}, {N}] stack; "
                         f"got shape {np.shape(obs)}")
    stack = stack.astype(np.complex128 if np.iscomplexobj(stack) else np.float64)
    for j, o in enumerate(stack):
        dev, size = np.abs(o - o.conj().T).max(), np.abs(o).max()
        if not dev <= 1e-12 * max(1.0, size):      # (also refuses NaN)
            raise ValueError(f"observable {j} is not Hermitian: max|O - O^H| = {dev:.3e}")
    planes = np.moveaxis(stack, 0, 2)
    re = np.asfortranarray(planes.real, dtype=np.float64)
    im = np.asfortranarray(planes.imag, dtype=np.float64) if np.iscomplexobj(planes) and np.any(planes.imag != 0.0) else None
    return re, im


def eval_expectations(prob, controls, pcof, observables, order=2, saveEveryNsteps=1):
    """Expectation values ``Re(psi^H O_j psi)`` of Hermitian observables along the forward sweep,
    ``[n_obs, 1 + nsteps // saveEveryNsteps, N_initial_conditions]``, formed on the device from the state panels: what
    ``get_populations`` cannot give because it is not diagonal in the level basis (Bloch components, quadratures, coherences,
    the energy).  ``observables`` as for observable_planes.  Not in the reference."""
    save = int(saveEveryNsteps)
    if save < 1:
        raise ValueError("saveEveryNsteps must be a positive integer")
    observable_planes(observables, prob.N_tot_levels)      # (refusals before a handle is made or anything is uploaded)
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    dp.set_save_every(save)
    try:
        return dp.eval_expectations(observables, pcof)
    finally:
        dp.set_save_every(1)


def check_refine(refine):
    """``refine`` of the dense output as an int; ValueError unless it is an integer >= 1 (a bool or a float with a fraction is not)."""
    if isinstance(refine, (bool, np.bool_)) or not isinstance(refine, (int, np.integer)):
        if not (isinstance(refine, (float, np.floating)) and float(refine).is_integer()):
            raise ValueError(f"refine must be an integer >= 1; got {refine!r}")
    if int(refine) < 1:
        raise ValueError(f"refine must be an integer >= 1; got {refine!r}")
    return int(refine)


def hermite_dense_weights(m, refine, dt):
    """Weights of the two-point Hermite interpolant of degree ``2m+1`` at ``theta = s / refine``, ``s = 1 .. refine-1``: the
    tables ``(a, b)``, each ``[refine-1, m+1]``, with ``a[s-1, j] = dt^j A_j(theta)`` (left end of the step) and
    ``b[s-1, j] = (-dt)^j A_j(1-theta)`` (right end), ``A_j(x) = x^j (1-x)^(m+1) sum_{k=0..m-j} C(m+k, k) x^k``.  Every term of
    ``A_j`` is non-negative on [0, 1].  ``m = 1``: the cubic Hermite basis."""
    from math import comb
    m, refine = int(m), check_refine(refine)
    if m < 1:
        raise ValueError("m must be >= 1")
    a, b = np.zeros((refine - 1, m + 1)), np.zeros((refine - 1, m + 1))

    def A(j, x, y):                                       # y = 1 - x, formed without rounding the difference
        return x ** j * y ** (m + 1) * sum(comb(m + k, k) * x ** k for k in range(m - j + 1))

    for s in range(1, refine):
        x, y = s / refine, (refine - s) / refine
        for j in range(m + 1):
            a[s - 1, j] = dt ** j * A(j, x, y)
            b[s - 1, j] = (-dt) ** j * A(j, y, x)
    return a, b


def hermite_interpolate(uv_history, dt, refine):
    """Hermite dense output of a history ``[2N, 1+m, nt, n_cols]`` of scaled Taylor coefficients ``w_j = w^(j)/j!`` (what
    eval_forward_ fills, from the device or from any other Hermite integrator): ``[2N, 1 + (nt-1) * refine, n_cols]`` (Fortran order), slot ``n * refine + s`` at
    time ``(n + s / refine) dt``,
        ``w = sum_{j=0..m} a[s-1, j] w_j(t_n) + b[s-1, j] w_j(t_{n+1})``       (hermite_dense_weights),
    summed over ascending j, left end before right end; slots ``n * refine`` are copies of ``uv_history[:, 0, n]``.  Local error
    ``O(dt^(2m+2))``, the order of the method.  Host arithmetic: the written statement of what eval_dense computes on the device."""
    h = np.asarray(uv_history)
    if h.ndim != 4 or h.shape[1] < 2 or h.shape[2] < 1 or not np.issubdtype(h.dtype, np.floating):
        raise ValueError("uv_history must be a real array [2N, 1+m, nt, n_cols] with m >= 1")
    refine = check_refine(refine)
    m, nt = h.shape[1] - 1, h.shape[2]
    out = np.zeros((h.shape[0], 1 + (nt - 1) * refine, h.shape[3]), order="F")
    out[:, ::refine] = h[:, 0]
    a, b = hermite_dense_weights(m, refine, float(dt))
    for s in range(1, refine):
        acc = np.zeros((h.shape[0], nt - 1, h.shape[3]))
        for j in range(m + 1):
            acc = acc + a[s - 1, j] * h[:, j, :-1]
            acc = acc + b[s - 1, j] * h[:, j, 1:]
        out[:, s::refine] = acc
    return out


def dense_times(prob, refine):
    """The ``1 + nsteps * refine`` time stamps of the dense output of ``prob``: slot k at ``k * tf / (nsteps * refine)``."""
    refine = check_refine(refine)
    n = prob.nsteps * refine
    return np.arange(n + 1) * (prob.tf / n)


def eval_dense(prob, controls, pcof, order=2, refine=2, output="states", level_map=None, observables=None):
    """The trajectory between the grid points: ``output="states"`` ``[2N, 1 + nsteps * refine, N_initial_conditions]``,
    ``"populations"`` (``[N, ..]``, or ``[n_groups, ..]`` with ``level_map``) or ``"expectations"`` (``[n_obs, ..]`` of
    ``observables``, as eval_expectations) of the Hermite interpolant of the order-``order`` sweep at ``refine`` points per step
    (DeviceProblem.eval_dense_states); dense_times gives the time stamps.  As accurate as the grid values
    themselves, for one memory-bound kernel instead of a sweep on a ``refine`` times finer grid.  Not in the reference."""
    refine = check_refine(refine)
    if output not in ("states", "populations", "expectations"):
        raise ValueError("output must be 'states', 'populations' or 'expectations'")
    if (output == "expectations") != (observables is not None):
        raise ValueError("observables go with output='expectations'")
    if level_map is not None and output != "populations":
        raise ValueError("level_map goes with output='populations'")
    N = prob.N_tot_levels
    if observables is not None:
        observable_planes(observables, N)                 # (refusals before a handle is made or anything is uploaded)
    if level_map is not None:
        lm = np.asarray(level_map)
        if lm.ndim != 2 or lm.shape[1] != N or lm.shape[0] < 1 or not np.issubdtype(lm.dtype, np.number) or np.iscomplexobj(lm):
            raise ValueError(f"level_map must be a real [n_groups >= 1, {N}] array; got {lm.dtype} {lm.shape}")
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    if output == "states":
        return dp.eval_dense_states(refine, pcof)
    if output == "populations":
        return dp.eval_dense_populations(refine, pcof, level_map=level_map)
    return dp.eval_dense_expectations(refine, observables, pcof)


def level_map_array(level_map, N):
    """A level map as the library takes it: Fortran-ordered float64 ``[n_groups >= 1, N]``; ValueError for anything else."""
    lm = np.asarray(level_map)
    if lm.ndim != 2 or lm.shape[1] != N or lm.shape[0] < 1 or lm.dtype == bool or not np.issubdtype(lm.dtype, np.number) \
            or np.iscomplexobj(lm):
        raise ValueError(f"level_map must be a real [n_groups >= 1, {N}] array; got {lm.dtype} {lm.shape}")
    return np.asfortranarray(lm, dtype=np.float64)


def pullback_cotangents(N, n_slots, n_cols, states_bar=None, populations_bar=None, level_map=None, expectations_bar=None,
                        observables=None):
    """The arguments of eval_pullback as the arrays the library takes, ``(states_bar, populations_bar, level_map,
    expectations_bar, obs_re, obs_im)``: Fortran-ordered float64, None for what was not given.  ``states_bar``: real
    ``[2N, n_slots, n_cols]`` or complex ``[N, n_slots, n_cols]`` (split as complex_to_real does: real parts on top);
    ``populations_bar``: real ``[N, ..]``, or ``[n_groups, ..]`` with ``level_map`` ``[n_groups, N]``; ``expectations_bar``: real
    ``[n_obs, ..]`` with ``observables`` as for observable_planes.  ValueError for a wrong shape or dtype, a cotangent that is
    complex where its output is real, a level map or observables without their cotangent (or the reverse), an observable that
    is not Hermitian, or no cotangent at all."""
    tail = (int(n_slots), int(n_cols))

    def real(a, rows, name):
        a = np.asarray(a)
        if a.dtype == bool or not np.issubdtype(a.dtype, np.number) or np.iscomplexobj(a):
            raise ValueError(f"{name} must be a real numeric array; got dtype {a.dtype}")
        if a.shape != (rows,) + tail:
            raise ValueError(f"{name} must have shape {(rows,) + tail}; got {a.shape}")
        return np.asfortranarray(a, dtype=np.float64)

    if states_bar is None and populations_bar is None and expectations_bar is None:
        raise ValueError("eval_pullback needs at least one of states_bar, populations_bar, expectations_bar")
    sb = pb = lm = eb = re = im = None
    if states_bar is not None:
        sb = np.asarray(states_bar)
        if sb.dtype == bool or not np.issubdtype(sb.dtype, np.number):
            raise ValueError(f"states_bar must be numeric; got dtype {sb.dtype}")
        rows = N if np.iscomplexobj(sb) else 2 * N
        if sb.shape != (rows,) + tail:
            raise ValueError(f"states_bar must be real {(2 * N,) + tail} or complex {(N,) + tail}; got {sb.dtype} {sb.shape}")
        sb = complex_to_real(sb) if np.iscomplexobj(sb) else np.asfortranarray(sb, dtype=np.float64)
    if level_map is not None:
        if populations_bar is None:
            raise ValueError("level_map given without populations_bar")
        lm = level_map_array(level_map, N)
    if populations_bar is not None:
        pb = real(populations_bar, N if lm is None else lm.shape[0], "populations_bar")
    if (expectations_bar is None) != (observables is None):
        raise ValueError("expectations_bar and observables go together")
    if expectations_bar is not None:
        re, im = observable_planes(observables, N)
        eb = real(expectations_bar, re.shape[2], "expectations_bar")
    return sb, pb, lm, eb, re, im


def eval_pullback(prob, controls, pcof, order=2, saveEveryNsteps=1, states_bar=None, populations_bar=None, level_map=None,
                  expectations_bar=None, observables=None):
    """Gradient with respect to pcof of a cost written in the outputs of eval_forward (its states as eval_states returns them),
    eval_populations and eval_expectations: ``sum <bar, d output / d pcof>`` over the cotangents given, ``bar = d cost / d output``
    in the shape of that output for the same ``saveEveryNsteps``, ``level_map`` and ``observables`` (DeviceProblem.eval_pullback,
    DESIGN.md section 4g).  One forward and one adjoint sweep on the device, whatever the number of parameters.  Not in the
    reference."""
    save = int(saveEveryNsteps)
    if save < 1:
        raise ValueError("saveEveryNsteps must be a positive integer")
    pullback_cotangents(prob.N_tot_levels, 1 + prob.nsteps // save, prob.N_initial_conditions, states_bar, populations_bar,
                        level_map, expectations_bar, observables)      # (refusals before a handle is made or anything is uploaded)
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    dp.set_save_every(save)
    try:
        return dp.eval_pullback(pcof, states_bar, populations_bar, level_map, expectations_bar, observables)
    finally:
        dp.set_save_every(1)


def eval_dense_pullback(prob, controls, pcof, order=2, refine=2, states_bar=None, populations_bar=None, level_map=None,
                        expectations_bar=None, observables=None):
    """Gradient with respect to pcof of a cost written on the outputs of eval_dense (states, populations with ``level_map``,
    expectations of ``observables``) at ``refine`` points per step: ``sum <bar, d output / d pcof>`` over the cotangents given,
    each in the shape of its output, ``[.., 1 + nsteps * refine, N_initial_conditions]`` (DeviceProblem.eval_dense_pullback,
    DESIGN.md section 4j).  One forward and one adjoint sweep on the device, whatever the number of parameters or ``refine``.
    Not in the reference."""
    refine = check_refine(refine)
    pullback_cotangents(prob.N_tot_levels, 1 + prob.nsteps * refine, prob.N_initial_conditions, states_bar, populations_bar,
                        level_map, expectations_bar, observables)      # (refusals before a handle is made or anything is uploaded)
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    return dp.eval_dense_pullback(refine, pcof, states_bar, populations_bar, level_map, expectations_bar, observables)


def pushforward_directions(v, n_pcof):
    """The directions of eval_pushforward as the library takes them: ``(cols, single)`` with ``cols`` a Fortran-ordered float64
    ``[n_pcof, n_vec]`` and ``single`` whether ``v`` was one vector ``(n_pcof,)`` (the results then lose their direction axis).
    ValueError for a wrong length or rank, complex or non-numeric input, an empty set of directions or non-finite values."""
    a = np.asarray(v)
    if a.dtype == bool or not np.issubdtype(a.dtype, np.number) or np.iscomplexobj(a):
        raise ValueError(f"v must be a real numeric array; got dtype {a.dtype}")
    if a.ndim not in (1, 2) or a.shape[0] != int(n_pcof):
        raise ValueError(f"v must have shape ({int(n_pcof)},) or ({int(n_pcof)}, n_vec); got {a.shape}")
    cols = np.asfortranarray(a.reshape(int(n_pcof), -1), dtype=np.float64)
    if cols.shape[1] < 1 or cols.shape[0] < 1:
        raise ValueError("v holds no direction")
    if not np.all(np.isfinite(cols)):
        raise ValueError("v must be finite")
    return cols, a.ndim == 1


def pushforward_outputs(N, output, level_map=None, observables=None):
    """What ``output=`` of the functional eval_pushforward asks of DeviceProblem.eval_pushforward, as keyword arguments; the
    refusals of eval_dense's ``output=`` argument, of level_map_array and of observable_planes."""
    if output not in ("states", "populations", "expectations"):
        raise ValueError("output must be 'states', 'populations' or 'expectations'")
    if (output == "expectations") != (observables is not None):
        raise ValueError("observables go with output='expectations'")
    if level_map is not None and output != "populations":
        raise ValueError("level_map goes with output='populations'")
    if observables is not None:
        observable_planes(observables, N)
    if level_map is not None:
        level_map_array(level_map, N)
    return dict(states=output == "states", populations=output == "populations", level_map=level_map, observables=observables)


def eval_pushforward(prob, controls, pcof, v, order=2, saveEveryNsteps=1, output="states", level_map=None, observables=None):
    """Directional derivative ``J v`` of a trajectory output along ``v`` in pcof, ``J = d output / d pcof``: of the states
    (``output="states"``, complex ``[N, slots, N_initial_conditions]`` as real_to_complex makes of the stacked tangent), of the
    populations (``"populations"``, real ``[N, ..]`` or ``[n_groups, ..]`` with ``level_map``) or of the expectation values of
    ``observables`` (``"expectations"``, real ``[n_obs, ..]``), ``slots = 1 + nsteps // saveEveryNsteps``.  ``v``: ``(n_pcof,)``, or
    ``(n_pcof, n_vec)`` for a result with a trailing direction axis (DeviceProblem.eval_pushforward).  One
    forward sweep and one forced scan on the device for all directions; exact for the discrete scheme, unlike differences of
    the output calls.  Not in the reference."""
    save = int(saveEveryNsteps)
    if save < 1:
        raise ValueError("saveEveryNsteps must be a positive integer")
    # (refusals before a handle is made or anything is uploaded)
    asked = pushforward_outputs(prob.N_tot_levels, output, level_map, observables)
    pushforward_directions(v, len(np.asarray(pcof).reshape(-1)))
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    dp.set_save_every(save)
    try:
        out = dp.eval_pushforward(pcof, v, **asked)
    finally:
        dp.set_save_every(1)
    return real_to_complex(out["states"]) if output == "states" else out[output]


def eval_dense_pushforward(prob, controls, pcof, v, order=2, refine=2, output="states", level_map=None, observables=None):
    """Directional derivative ``J v`` of an output of eval_dense at ``refine`` points per step along ``v`` in pcof: eval_pushforward
    with ``slots = 1 + nsteps * refine`` (``output="states"``: complex ``[N, slots, N_initial_conditions]``; ``"populations"``,
    ``"expectations"``: real), ``v`` ``(n_pcof,)`` or ``(n_pcof, n_vec)`` (DeviceProblem.eval_dense_pushforward, DESIGN.md section
    4n).  Exact for the interpolant, unlike differences of eval_dense.  Not in the reference."""
    refine = check_refine(refine)
    # (refusals before a handle is made or anything is uploaded)
    asked = pushforward_outputs(prob.N_tot_levels, output, level_map, observables)
    pushforward_directions(v, len(np.asarray(pcof).reshape(-1)))
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    out = dp.eval_dense_pushforward(refine, pcof, v, **asked)
    return real_to_complex(out["states"]) if output == "states" else out[output]


def eval_grad_forced(prob, controls, pcof, target, order=2, cost_type="Infidelity"):
    """eval_grad_forced(prob, controls, pcof, target; order, cost_type) (src/eval_grad_forced.jl:17-60):
    the gradient of infidelity + guard penalty by differentiating the forward sweep (one forced sweep
    per control parameter).  On the device all parameters run at once as extra columns of the scan."""
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    dp.set_target(target)
    dp.set_cost_type(cost_type)
    try:
        return dp.eval_grad_forced(pcof)
    finally:
        dp.set_cost_type("Infidelity")


def eval_hessian_vec(prob, controls, pcof, v, target, order=2, cost_type="Infidelity"):
    """Exact Hessian-vector product(s) of the discrete objective: ``eval_hessian(...) @ v`` without the Hessian (DESIGN.md
    section 4d).  ``v``: (n_pcof,) or (n_pcof, k).  Calls with the same pcof (and problem, controls, target, cost type) reuse
    the part that does not depend on v.  Controls linear in pcof."""
    cl = controls if isinstance(controls, (list, tuple)) else [controls]
    if not all(getattr(c, "is_linear", False) for c in cl):
        raise NotImplementedError("eval_hessian_vec needs controls that are linear in pcof (is_linear = True)")
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    dp.set_target(target)
    dp.set_cost_type(cost_type)
    try:
        return dp.eval_hessian_vec(np.asarray(pcof, dtype=np.float64), v)
    finally:
        dp.set_cost_type("Infidelity")


def eval_hessian(prob, controls, pcof, target, dpcof=1e-5, order=2, cost_type="Infidelity", method="exact"):
    """eval_hessian(prob, controls, pcof, target; dpcof, order) (src/eval_hessian.jl).  method="exact": the exact Hessian of
    the discrete objective on the device (controls linear in pcof).  method="finite_difference": the
    reference's own formula -- 4-point differences of the device objective with step dpcof, n(n-1)*4 + 3n forward solves."""
    if method not in ("exact", "finite_difference"):
        raise ValueError("method must be 'exact' or 'finite_difference'")
    cl = controls if isinstance(controls, (list, tuple)) else [controls]
    if method == "exact" and not all(getattr(c, "is_linear", False) for c in cl):
        raise NotImplementedError("eval_hessian(method='exact') needs controls that are linear in pcof (is_linear = True); "
                                  "use method='finite_difference' for non-linear controls")
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    dp.set_target(target)
    dp.set_cost_type(cost_type)
    pcof = np.asarray(pcof, dtype=np.float64)
    try:
        if method == "exact":
            return dp.eval_hessian(pcof)
        plain = COST_TYPES[str(cost_type)] == 0

        def cost(p):
            a, b, guard = dp.eval_forward(p)
            return (1.0 - (a * a + b * b) / prob.N_ess_levels ** 2 if plain else a) + guard

        n = len(pcof)
        hess = np.zeros((n, n))
        f0 = cost(pcof)
        for i in range(n):
            for j in range(n):
                if i != j:
                    def at(si, sj):
                        p = pcof.copy(); p[i] += si * dpcof; p[j] += sj * dpcof
                        return cost(p)
                    hess[i, j] = (at(1, 1) + at(-1, -1) - at(1, -1) - at(-1, 1)) / (4 * dpcof ** 2)
                else:
                    e = np.zeros(n); e[i] = dpcof
                    hess[i, i] = (cost(pcof + e) - 2 * f0 + cost(pcof - e)) / dpcof ** 2
        return hess
    finally:
        dp.set_cost_type("Infidelity")


def eval_grad_finite_difference(prob, controls, pcof, target, dpcof=1e-5, order=2, cost_type="Infidelity"):
    """eval_grad_finite_difference (src/eval_grad_finite_difference.jl:1-72): centred differences of
    infidelity + guard penalty, two device forward evaluations per control parameter (the third leg of
    the reference's adjoint / forced / finite-difference contract, compare_gradients.jl:47-65)."""
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    dp.set_target(target)
    dp.set_cost_type(cost_type)
    pcof = np.asarray(pcof, dtype=np.float64)
    plain = COST_TYPES[str(cost_type)] == 0
    try:
        # the 2 n_pcof points as one forward-only batch: one call instead of 2 n_pcof round trips
        _, scalars, status = dp.eval_batch(finite_difference_points(pcof, dpcof), gradient=False)
        _raise_singular(dp, status)
        return finite_difference_quotient(objective_from_scalars(scalars, prob.N_ess_levels, plain), dpcof)
    finally:
        dp.set_cost_type("Infidelity")


def _batch_problem(prob, controls, target, order, cost_type):
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    dp.set_target(target)
    dp.set_cost_type(cost_type)
    return dp


def _raise_singular(dp, status):
    if status.any():
        raise _lib.QGDError(_lib.QGD_ERR_NUMERIC, f"singular implicit step matrix L(t_n) in members {np.flatnonzero(status).tolist()} of the batch")


def discrete_adjoint_batch(prob, controls, pcofs, target, order=2, cost_type="Infidelity"):
    """discrete_adjoint for ``K`` coefficient vectors ``pcofs [K, n_pcof]`` in one device call: the gradients ``[K, n_pcof]``,
    row ``k`` bit for bit what ``discrete_adjoint(prob, controls, pcofs[k], target)`` returns (multi-start optimisation,
    populations of an evolutionary optimiser, the points of a line search)."""
    dp = _batch_problem(prob, controls, target, order, cost_type)
    try:
        grads, _, status = dp.eval_batch(pcofs, gradient=True)
    finally:
        dp.set_cost_type("Infidelity")
    _raise_singular(dp, status)
    return grads


def eval_objective_batch(prob, controls, pcofs, target, order=2, cost_type="Infidelity"):
    """The objective -- infidelity, or the tracking / norm cost, plus the guard penalty -- of ``K`` coefficient vectors
    ``pcofs [K, n_pcof]`` in one device call: ``K`` values, formed from the scalars as eval_grad_finite_difference forms its costs."""
    dp = _batch_problem(prob, controls, target, order, cost_type)
    try:
        _, scalars, status = dp.eval_batch(pcofs, gradient=False)
    finally:
        dp.set_cost_type("Infidelity")
    _raise_singular(dp, status)
    return objective_from_scalars(scalars, prob.N_ess_levels, COST_TYPES[str(cost_type)] == 0)


def eval_adjoint(prob, controls, pcof, terminal_condition, order=2, forcing=None, lambda_derivatives=False):
    """QuantumGateDesign.eval_adjoint (forward_evolution.jl:300-315), used by the reference's scripts
    (examples/cnot2_optimization.jl:56, regression.jl:49): lambda history ``[2N, 1+order/2, 1+nsteps, c]``
    from a given terminal condition; column j=0 holds lambda_n (the only column the package consumes);
    ``lambda_derivatives=True`` also fills the derivative columns the reference leaves there."""
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    dp.set_lambda_derivatives(lambda_derivatives)
    try:
        return dp.eval_adjoint(pcof, terminal_condition, forcing)
    finally:
        if lambda_derivatives:
            dp.set_lambda_derivatives(False)


def infidelity_real(psi, target, N_ess):
    """infidelity.jl:7-18 (host arithmetic on two small matrices)."""
    R = np.asarray(target, float)
    N = R.shape[0] // 2
    T = np.vstack([R[N:], -R[:N]])
    psi = np.asarray(psi, float)
    return 1 - (np.sum(psi * R) ** 2 + np.sum(psi * T) ** 2) / N_ess ** 2


def state_transfer_infidelity(psi, target):
    """The ``StateTransfer`` cost ``1 - (1/c) sum_j |t_j^H psi_j|^2`` (host arithmetic).  ``psi``: complex ``[N, c]``,
    real ``[2N, c]``, or a real history whose last slot is taken (``[2N, slots, c]`` of eval_states, ``[2N, 1 + m, nt, c]``
    of eval_forward).  ``target``: complex ``[N, c]`` or real ``[2N, c]``; its columns are expected to have unit norm."""
    psi, target = np.asarray(psi), np.asarray(target)
    if psi.ndim == 4:
        psi = psi[:, 0, -1, :]
    elif psi.ndim == 3:
        psi = psi[:, -1, :]
    R = target.astype(np.float64) if not np.iscomplexobj(target) else complex_to_real(target)
    w = psi.astype(np.float64) if not np.iscomplexobj(psi) else complex_to_real(psi)
    N = R.shape[0] // 2
    T = np.vstack([R[N:], -R[:N]])
    a, b = np.sum(w * R, axis=0), np.sum(w * T, axis=0)
    return 1.0 - np.sum(a * a + b * b) / R.shape[1]


def infidelity(*args, order=2):
    """infidelity(psi, target, N_ess)  or  infidelity(prob, controls, pcof, target; order)
    (infidelity.jl:20-47).  The second form runs the forward sweep on the device."""
    if len(args) == 3:
        psi, target, N_ess = args
        return infidelity_real(complex_to_real(psi), complex_to_real(target), N_ess)
    prob, controls, pcof, target = args
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    dp.set_target(target)
    a, b, _ = dp.eval_forward(pcof)
    return 1 - (a * a + b * b) / prob.N_ess_levels ** 2


def guard_penalty_real(history, dt, T, W):
    """infidelity.jl:56-96 (host; the device computes the same sum inside eval_forward)."""
    h = np.asarray(history)
    if h.ndim == 3:
        h = h[..., None]
    w = h[:, 0, :, :]
    Ww = np.einsum("ij,jnc->inc", np.asarray(W), w)
    trap = np.ones(w.shape[1]); trap[0] = trap[-1] = 0.5
    return float(np.einsum("n,inc,inc->", trap, w, Ww) * dt / T)


def discrete_adjoint_(grad, history, lambda_history, adjoint_forcing, prob, controls, pcof, target,
                      order=2, cost_type="Infidelity", history_precomputed=False, lambda_derivatives=False):
    """discrete_adjoint! (eval_grad_discrete_adjoint.jl:107-160).  ``lambda_derivatives=True``: columns 1..m of
    ``lambda_history`` as the reference leaves them (default: zeros; only column 0 is ever consumed)."""
    dp = device_problem(prob, order)
    dp.set_controls(controls)
    dp.set_target(target)
    dp.set_cost_type(cost_type)
    if lambda_derivatives:
        dp.set_lambda_derivatives(True)
    try:
        g, _ = dp.discrete_adjoint(pcof, history_precomputed, history, lambda_history, adjoint_forcing)
    finally:
        dp.set_cost_type("Infidelity")
        if lambda_derivatives:
            dp.set_lambda_derivatives(False)
    grad[:] = g
    return grad


def discrete_adjoint(prob, controls, pcof, target, order=2, cost_type="Infidelity"):
    """eval_grad_discrete_adjoint.jl:83-102: returns the gradient."""
    grad = np.zeros(get_number_of_control_parameters(controls))
    return discrete_adjoint_(grad, None, None, None, prob, controls, pcof, target, order=order, cost_type=cost_type)
