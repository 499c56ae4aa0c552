// qgd_host.h -- what the eight host-side translation units of the C ABI share (include/qgd.h): the handle, the error and
// launch macros, the phase timer and the internal entry points of each unit.
//   qgd_host_alloc.cpp    handles: creation, validation (SchrodingerProb.jl:73-154), the time grid and its windows, setters
//   qgd_host_eval.cpp     one evaluation: forward / adjoint phases, result transport, the evaluation entry points
//   qgd_host_sens.cpp     sensitivities of the state to the parameters: the forced gradient, the exact Hessian, Hessian-vector products, pullbacks (grid points and dense output); the refusals and the sweep they share with the pushforward
//   qgd_host_pushforward.cpp  directional derivatives of the trajectory outputs, at the grid points (include/qgd_pushforward.h) and of the dense output (include/qgd_dense_pushforward.h)
//   qgd_host_ensemble.cpp  one pcof over the members of an ensemble side by side, reduced on the device (include/qgd_ensemble.h)
//   qgd_host_output.cpp   reference-layout output arrays of a resident or windowed grid: the copy stream, staging, the one transport; the rules of an OutputSelection
//   qgd_host_windows.cpp  time grids in bounded memory: window entry, the windowed forward and adjoint passes
//   qgd_host_comm.cpp     several GPUs: the RCCL binding, the collective evaluation and its failure mode
// There is no CPU fallback: without a GPU every compute entry point fails.
// Every entry point that touches the device begins with ENTER (below), which also refuses a handle whose stream is dead; the
// entry points that only read or write fields of the handle do not, and keep working on such a handle.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>      // types only: the library is bound at run time (dlopen), see RcclApi
#include <dlfcn.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <sched.h>

#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <chrono>
#include <string>
#include <vector>
#include <algorithm>

#include "qgd.h"
#include "qgd_device.h"

namespace qgdh {

extern thread_local std::string g_create_error;

struct Phase { const char *name; int slot; hipEvent_t e0, e1; bool used; };

}  // namespace qgdh
using qgdh::Phase;

// What the per-time-point buffers hold of the last forward sweep, and what a later call may make of it:
//   SWEEP_NONE     nothing a history_precomputed call may refer to (none yet, a sweep in progress or one that failed, a
//                  sweep of another kind: eval_adjoint, the forced sweep, or a setter voided it)
//   SWEEP_GENERAL  the two-point form's sweep
//   SWEEP_FRONT    the fused front's sweep (qgd_device.h: qgdk_ctx::front): state history, lambda and forcing are the same
//                  quantities as ever, but L / R / Linv / P are the same-point form's -- qgd_get_intermediate redoes the
//                  forward evaluation on the general path from pcof before it returns them
//   SWEEP_SMALL    a small-problem evaluation (qgd_k_tiny.hip), which leaves none of its intermediates behind: only its pcof
//                  and whether it was a gradient are kept, so that a call that needs them (history_precomputed with output
//                  arrays, qgd_get_intermediate) redoes it on the general path
// has_pcof, pcof: the coefficients of the sweep (has_pcof false: it ran from the control tables the caller set, pcof NULL).
//   A setter that voids the sweep keeps them, for qgd_get_intermediate's redo of a front sweep -- except qgd_set_control_basis,
//   whose new basis they do not fit.
// reusable: a history_precomputed call with the same pcof may skip the sweep.  A new target or cost type clears it for
//   SWEEP_FRONT only, whose k_psi formed L_N^-H times the terminal value of the old ones (the general path re-forms the
//   terminal condition on reuse); kind and pcof stay, so the sweep can still be redone.
// derivs: the stage derivatives of the stored history are in place.  Every transition that replaces the history clears it.
// forced_basis: the forced basis responses of the stored history (k.fs_BR, k.fs_BL in POOL_FORCED) are in place, as long as that
//   pool still stands under its key (forced_missing(h) == 0); cleared with derivs.  qgd_eval_pushforward skips qgdk_forced_basis
//   on it; the other entry points that form the responses record it and form them on every call, as before.
// front: what qgd_get_intermediate("front_path") reports -- whether the last forward evaluation took the fused front.  A setter
//   that voids the sweep leaves it (and the same-point matrices in the buffers).
// New control tables void the sweep on a windowed grid only: there a reused sweep re-runs its windows from the caller's tables;
//   on a resident grid nothing is re-run, and a NULL-pcof history_precomputed call after new tables reuses the sweep -- the
//   caller's promise that the history belongs to them, as in the reference.
// A call that is refused before its first launch leaves the record as it was.
// A batch (qgd_eval_batch) ends at SWEEP_NONE on both of its routes: no later history_precomputed call may refer to a batch.
enum SweepKind { SWEEP_NONE, SWEEP_GENERAL, SWEEP_FRONT, SWEEP_SMALL };
struct StoredSweep {
    SweepKind kind = SWEEP_NONE;
    bool has_pcof = false;
    std::vector<double> pcof;
    bool gradient = false;
    bool reusable = false;
    bool derivs = false;
    bool forced_basis = false;
    bool front = false;
};

// A buffer plan: the device buffers of a keyed pool, each listed once -- where its pointer goes (its slot), its length in doubles,
// whether this problem has it (else the slot is set to NULL).  plan_bytes: what the plan asks for (without dev_alloc's pad).
// A pool of on-demand device buffers: the allocations, the slots their pointers were handed to (with the length that goes with
// a grow-to-largest buffer's pointer, Grown) and the exact tuple they were made for (empty: nothing allocated under a key).
// pool_release frees them, writes NULL (and length 0) into every slot and clears the key; pool_missing: the bytes pool_ensure
// would allocate for a (key, plan) pair.  The other functions are in qgd_host_alloc.cpp.
#define QGD_BATCH_CHUNK_MAX 1024      // members of a batch that share one set of launches (qgd_eval_batch)
#define QGD_ENSEMBLE_ACC 72           // doubles of the accumulator row of qgd_eval_ensemble: the small path's 64 coefficients at most, cost, guard
#define QGD_PUSHFORWARD_CHUNK_MAX 4096    // directions of a pushforward that ride along in one forced scan (qgd_eval_pushforward) ...
#define QGD_PUSHFORWARD_CHUNK_DEFAULT 256  // ... and without QGD_PUSHFORWARD_CHUNK (cnot3's 180 in one scan: 812 MB of tangent history; 13.2 ms against 16.8 in chunks of 32)
struct Buf { double **slot; size_t count; bool on = true; };
inline size_t plan_bytes(const std::vector<Buf> &plan) { size_t n = 0; for (const Buf &b : plan) n += b.on ? b.count : 0; return n * sizeof(double); }
struct Grown { double *p = nullptr; size_t len = 0; };
struct Pool {
    struct Held { void *mem; double **slot; size_t *len; };
    std::vector<Held> held;
    std::vector<size_t> key;
};
struct KeyedPlan { std::vector<size_t> key; std::vector<Buf> plan; };
inline size_t pool_missing(const Pool &pool, const KeyedPlan &p) { return pool.key == p.key ? 0 : plan_bytes(p.plan); }
enum { POOL_FORCED, POOL_HESS, POOL_HVP, POOL_PULLBACK, POOL_DENSE, POOL_BATCH, POOL_DENSE_PULLBACK, POOL_PUSHFORWARD, POOL_ENSEMBLE, N_SENS_POOLS, POOL_FORCING = N_SENS_POOLS, POOL_STAGE, N_POOLS };

struct qgd_handle_s {
    qgdk_ctx k{};
    int order = 0, nsteps = 0, device = 0;      // nsteps: GLOBAL number of timesteps
    int part_rank = 0, part_world = 1;
    bool own_stream = true;
    bool timing = false;                // per-phase HIP events are opt-in (qgd_set_timing): 26 event records cost ~0.17 ms
    std::string timing_only;            // when non-empty: only this phase is bracketed by events
    std::string err;
    std::vector<void *> static_bufs, grid_bufs, basis_bufs;
    // The device buffers that entry points make on demand, one pool per row.  An entry point ensures its pool under the exact
    // tuple of what sizes or fills it; the pointers below are the pools' slots, NULL whenever their pool is released.  alloc_grid
    // releases every pool, qgd_set_control_basis the sensitivity pools (free_sensitivity_buffers).
    //   POOL_FORCED    forced gradient (k.fs_*, fsc_forced), also under the two second-order entry points; key (nt, n_pcof, scan blocks)
    //   POOL_HESS      qgd_eval_hessian: sensitivity history, work buffers of qgd_k_hessian.hip (hs); key (nt, n_pcof, basis directions, general guard)
    //   POOL_HVP       qgd_eval_hessian_vec (hv); that key and the scan blocks
    //   POOL_PULLBACK  qgd_eval_pullback (pb); key (nt, n_pcof, the lengths of the five uploads)
    //   POOL_DENSE     qgd_eval_dense (dense_panels, dense_w); key (time points, refine, panel size, m, bits of dt)
    //   POOL_BATCH     qgd_eval_batch on the small-problem path (bt): the arrays of a chunk's members; key (chunk members, nt, m, n_ops, n_pcof)
    //   POOL_DENSE_PULLBACK  qgd_eval_dense_pullback (dpb); key (time points, refine, n_pcof, m, bits of dt, the lengths of the five uploads)
    //   POOL_PUSHFORWARD  qgd_eval_pushforward (pf); key (nt, n_pcof, basis directions, scan blocks, directions of a chunk, the lengths of the three staged outputs and the two uploads)
    //   POOL_ENSEMBLE  qgd_set_ensemble (ens): the members' operator planes and weights, the accumulator row and the rows' tails of qgd_eval_ensemble; key (members, N, n_ops)
    //   POOL_FORCING   qgd_eval_forward with a user forcing (k.ff_*, fsc_forcing); key (nt, scan blocks)
    //   POOL_STAGE     the staging buffers of the reference-layout outputs: no key, each made or grown on first need
    Pool pools[N_POOLS];
    std::vector<double> target_host;   // stacked real target [2N x c] (forced gradient: the overlaps are host arithmetic)
    double *fsc_forced = nullptr, *fsc_forcing = nullptr;      // HBM work-panel slabs of k_forced_basis / k_forcing_terms when their panels exceed the LDS (N > 64)
    struct HessBufs { double *shist = nullptr, *ws = nullptr, *Z = nullptr, *half = nullptr, *slab = nullptr, *zt = nullptr, *Y = nullptr; } hs;
    // qgd_eval_hessian_vec: the direction-independent setup of a product -- forward sweep, lambda, stage
    // derivatives, the forced basis responses (in POOL_FORCED), Z and the halves of e_n -- stays on the handle.  hvp_valid: it
    // belongs to the stored sweep (StoredSweep::pcof) and the present target, cost type, basis and grid; every transition of
    // the sweep record clears it (hvp_void), as do the setters that free these buffers.
    struct HvpBufs {
        double *Z = nullptr, *half = nullptr, *slab = nullptr, *sv = nullptr, *ws = nullptr, *F = nullptr, *Y = nullptr, *mu = nullptr;
        double *phi = nullptr, *bnd = nullptr, *gvt = nullptr, *term = nullptr, *part = nullptr, *v = nullptr, *gB = nullptr, *out = nullptr, *scal = nullptr;
        double *one3 = nullptr;        // (16 bytes: the one-operator, one-coefficient basis of the direction table)
    } hv;
    bool hvp_valid = false;
    std::vector<double> hvp_grad;      // the adjoint gradient of the setup
    // qgd_eval_pullback: the forcing, y and mu of its adjoint sweep -- three panel histories of its own,
    // none shared with the setup above, which a pullback therefore leaves valid -- its gradient and scalars, and the caller's
    // cotangents, level map and observable planes on the device
    struct PullbackBufs {
        double *F = nullptr, *Y = nullptr, *mu = nullptr, *gB = nullptr, *scal = nullptr;
        double *sbar = nullptr, *pbar = nullptr, *map = nullptr, *ebar = nullptr, *planes = nullptr;
    } pb;
    // qgd_eval_dense: the interpolated panels [1 + (points-1) refine][Np][2cp] of a resident grid or of the
    // longest window, and the weight table of qgd_k_interp.hip with its host copy (the upload reads it)
    double *dense_panels = nullptr, *dense_w = nullptr;
    // qgd_eval_dense_pullback: a set of the pullback's buffers of its own -- nothing shared with the
    // pullback or the Hessian-vector setup above -- and in front of them the cotangents of the dense panels (G) and of the state
    // and stage derivatives of every time point (gbar), sigma and cpart; the dense panels and the weight table are POOL_DENSE's,
    // under that pool's key
    struct DensePullbackBufs : PullbackBufs { double *G = nullptr, *gbar = nullptr, *sigma = nullptr, *cpart = nullptr; } dpb;
    // qgd_eval_pushforward: the tangent history sv of the directions of one chunk side by side, the scan
    // buffers and the direction table of that width, the one-operator bases {0 | w, 0} of every width w up to the chunk's, the
    // chunk's directions, the staged outputs and the caller's level map and observable planes on the device -- nothing shared
    // with the Hessian-vector setup, which a pushforward of the same sweep leaves valid.  width: the directions sv[0] and bnd[0]
    // were last zeroed for.  The largest chunk: QGD_PUSHFORWARD_CHUNK, read when the handle is created (the tests force small
    // chunks with it), and what fits the memory budget
    struct PushforwardBufs {
        double *sv = nullptr, *phi = nullptr, *bnd = nullptr, *gvt = nullptr, *bases = nullptr, *v = nullptr;
        double *st = nullptr, *po = nullptr, *ex = nullptr, *map = nullptr, *planes = nullptr;
        size_t width = 0;
    } pf;
    int pf_chunk_max = (getenv("QGD_PUSHFORWARD_CHUNK") && atoi(getenv("QGD_PUSHFORWARD_CHUNK")) >= 1) ? std::min(atoi(getenv("QGD_PUSHFORWARD_CHUNK")), QGD_PUSHFORWARD_CHUNK_MAX) : QGD_PUSHFORWARD_CHUNK_DEFAULT;
    // qgd_eval_batch: per member of a chunk the small-problem path's compact arrays, its scalars and
    // status word, its coefficients and its result row; the pinned staging buffer [pcofs | rows] of one chunk; the largest chunk
    // (QGD_BATCH_CHUNK, read when the handle is created: the tests force small chunks with it); the route of the last batch
    struct BatchBufs { double *pcofs = nullptr, *tab = nullptr, *Rg = nullptr, *Linv = nullptr, *psi = nullptr, *lam = nullptr, *cpart = nullptr, *small = nullptr, *rows = nullptr; } bt;
    double *batch_host = nullptr;
    size_t batch_host_len = 0;
    int batch_chunk_max = (getenv("QGD_BATCH_CHUNK") && atoi(getenv("QGD_BATCH_CHUNK")) >= 1) ? std::min(atoi(getenv("QGD_BATCH_CHUNK")), QGD_BATCH_CHUNK_MAX) : QGD_BATCH_CHUNK_MAX;
    bool batch_path = false;
    // qgd_set_ensemble / qgd_eval_ensemble: the members' operator planes [members][(2 + 2 n_ops) Np Np] in
    // the layout of k.ops, their weights, the accumulator row [QGD_ENSEMBLE_ACC] = (grad | cost | guard) that stays on the device
    // between the chunks of one call, and the tails [members][5] of the members' result rows.  ops == NULL: no ensemble is set
    // (the pool is released with the sensitivity pools).  The per-member arrays of a chunk are POOL_BATCH's.
    struct EnsembleBufs { double *ops = nullptr, *w = nullptr, *acc = nullptr, *tails = nullptr; int members = 0; } ens;
    std::vector<double> dense_w_host;
    bool have_basis = false, have_tables = false;
    StoredSweep sweep;
    std::vector<int32_t> ncoef, poff;
    std::vector<int64_t> goff;
    double *pcof_dev = nullptr;
    double *scal_static = nullptr;
    std::vector<Phase> phases;
    std::vector<double> u0v0_panel;   // host copy of the initial panel
    bool sparse_available = false;    // the ELL lists were built and fit the sparse kernels
    int *status_static = nullptr;     // singularity flag when no control basis is set (else it lives in redbuf)
    double *host_out = nullptr;       // pinned staging buffer for [grad | scal | status]: one copy per evaluation
    double *host_in = nullptr;        // pinned staging buffer for pcof (a pageable source makes the upload synchronous)
    size_t host_out_len = 0;
    // result mirror (qgd_device.h): [grad | scal(4) | status | sequence number] in coherent pinned host memory that the last
    // kernel of a gradient evaluation writes itself; the host polls the sequence number instead of waiting for a copy packet
    // and the stream's completion signal.  QGD_RESULT_MIRROR=0 keeps the copy + hipStreamSynchronize.
    double *mirror_host = nullptr, *mirror_dev = nullptr;
    unsigned int *mirror_ticket = nullptr;
    bool status_dirty = false;          // an evaluation ended with the singular-matrix flag set on the device (reset before the small-problem path runs)
    unsigned long long mirror_seq = 0;
    bool mirror_armed = false;          // the evaluation in flight ends with a mirrored k_contract_sum
    // Small problems (N <= 4, <= 4 columns, <= 128 time points: Rabi, the two-qubit CNOT) take the four-launch path of
    // qgd_k_tiny.hip for calls that return only [grad | scalars] (StoredSweep: SWEEP_SMALL).  QGD_TINY=0 /
    // qgd_set_small_path(h, 0): off.  The fused front (qgd_device.h: qgdk_ctx::front) takes full evaluations of
    // qgd_eval_forward / qgd_discrete_adjoint on problems qgdk_front_supported admits (SWEEP_FRONT).
    bool small_path = !(getenv("QGD_TINY") && atoi(getenv("QGD_TINY")) == 0);
    bool mirror_off = (getenv("QGD_RESULT_MIRROR") && atoi(getenv("QGD_RESULT_MIRROR")) == 0);
    // the launch sequence of one full gradient evaluation as a hipGraph, opt-in (QGD_GRAPH=1).  Measured: no gain
    // on cnot3 (420 us either way) and 5 % on cnot2 (98 vs 104 us) -- an evaluation is a chain of ~15 DEPENDENT
    // kernels and the ~6 us per dependent dispatch is spent on the device side, not in hipLaunchKernel; the
    // instantiation costs several ms once.  Captured on the third eligible call, dropped by every entry point
    // that changes buffers, sizes or options.
    // reference-layout outputs (uv_history, lambda_history, adjoint_forcing): re-laid out on the device
    // (qgd_k_layout.hip) into staging buffers and copied out on a second stream, so that the download of the
    // state history overlaps the adjoint sweep.  Host buffers the caller registered (qgd_register_host_buffer)
    // are pinned: the copies then run at PCIe speed.
    struct HostReg { void *host; void *dev; size_t bytes; bool zeroed; };
    std::vector<HostReg> regs;
    double *stage_hist = nullptr, *stage_lam = nullptr, *stage_f = nullptr;
    // qgd_eval_states / qgd_eval_populations / qgd_eval_expectations: compact staging buffer [rows, slots, c], the caller's level
    // map and the planes of the caller's observables ([N, N, n_obs] real parts, then as many imaginary parts when there are
    // any) on the device (all in POOL_STAGE, grown to the largest request so far)
    Grown stage_obs, obs_map, obs_planes;
    // qgd_set_lambda_derivatives: the m derivative columns of lambda_history as the reference leaves them
    bool lambda_derivs = false;
    double *dlam = nullptr, *dlam_scratch = nullptr, *stage_lam_full = nullptr;
    hipStream_t copy_stream = nullptr;
    hipStream_t copy_stream2 = nullptr;   // the second half of a large pinned download goes to a second DMA engine 
    hipEvent_t ev_ready = nullptr;
    std::vector<double> scatter_tmp;    // unregistered lambda_history: compact copy, scattered on the host
    bool copies_pending = false;
    bool forcing_zero = false;          // no guard projector: the adjoint forcing is all zeros and nothing has written it since
                                        // (alloc_grid clears it, qgd_eval_adjoint uploads a caller's forcing into it)
    bool defer_terminal = false;        // a full gradient evaluation: the overlaps and y_N ride in the first adjoint launch
    double *lambda_out = nullptr;       // lambda_history of the evaluation in flight (copied out right after the lambda phase)
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    int graph_calls = 0;
    bool graph_off = (getenv("QGD_GRAPH") == nullptr);
    // multi-GPU INSIDE the library (qgd_comm_init_rccl): the ranks that share one evaluation talk over an RCCL
    // communicator; qgd_discrete_adjoint / qgd_eval_forward then run the partitioned protocol themselves, the
    // collectives issued on the handle's stream between the phases (no host synchronisation in between).
    ncclComm_t comm = nullptr;
    int comm_shard = QGD_SHARD_TIME, comm_rank = 0, comm_world = 1;
    // failure mode of the collective calls (qgd_set_comm_timeout): the one host wait of a collective evaluation is bounded;
    // when it expires, when RCCL reports an asynchronous error, or when this rank fails locally between two collectives,
    // the communicator is ABORTED (ncclCommAbort: its kernels leave the stream) and the call returns QGD_ERR_COMM --
    // the other ranks then run into their own bound instead of waiting for this one forever.
    double comm_timeout_ms = 30000.0;
    bool stream_dead = false;           // a communicator had to be leaked with a collective stuck on the stream (no ncclCommAbort in this librccl):
                                        // every later entry point that touches the device is refused with QGD_ERR_COMM by enter(), before any HIP call that
                                        // could wait for the stream (setters and getters of host fields keep working); qgd_destroy does not wait for it either
    int comm_fail_at = 0;               // != 0: pretend a local failure in front of collective #n (set only by the tests' fault injector, tests/hooks/qgd_test_hooks.cpp -- no entry point of the library writes it)
    bool grid_ready = false;            // QGD_CREATE_DEFER_GRID: the time grid is allocated by the first entry point that needs it
    bool comm_pending = false;          // qgd_comm_init_rccl is re-allocating the grid for the communicator it is about to
                                        // create: the grid stays resident (comm_discrete_adjoint does not walk windows)
    // bounded-memory time grid (qgd_set_memory_budget): chunks_eff windows of the grid share the per-time-point buffers
    size_t mem_budget = 0;              // bytes; 0 = 70 % of the free device memory when the grid is allocated
    int chunks_eff = 1;                 // windows the grid is processed in (1: everything resident)
    int chunks_req = 1;                 // the count plan_windows derived that layout from
    size_t window_bytes = 0;            // device bytes of the per-window buffers
    int resident_window = 0;            // whose step matrices are in the buffers right now
    double *chunk_state = nullptr;      // [chunks_eff + 1][Np][2cp]: the state at the start of every window (+ the final state)
    double *carry_y = nullptr;          // y at the end of the window the adjoint pass does next
    std::vector<double> tab_p_host, tab_q_host;      // qgd_set_control_tables on a windowed grid: the caller's tables for the WHOLE grid
    double *scal_scratch = nullptr;     // where a re-run of a window's forward sweep puts its guard sum (already counted)
    int save_every = 1;                 // qgd_set_save_every: uv_history of qgd_eval_forward holds every save_every-th time point
    double *redglob = nullptr;          // [n_pcof + 8] time shards: the reductions are out of place (send = the rank's own
                                        // [grad | scalars], receive = this), so a later history_precomputed call still finds
                                        // the rank's OWN guard sum and overlaps on the device, not the sums over the ranks
    // qgd_eval_dense_pushforward, beside pf (scan buffers, direction table, uploads) and the dense panels and
    // weight table of POOL_DENSE: the tangents of the stage derivatives of one chunk (dsv [nt][m] panels of the chunk's width), the
    // interpolated tangent panels (dd [1 + (nt-1) refine]) and the staged outputs at their dense sizes, in a pool of their own
    // that is one of the sensitivity pools (free_sensitivity_buffers releases it with pools[0 .. N_SENS_POOLS)); key (nt, n_pcof,
    // basis directions, scan blocks, directions of a chunk, the lengths of the three staged outputs, refine, m, bits of dt).
    // Pool and slots stand behind every other member: the members above keep their places, and the units that do not know the
    // dense pushforward are compiled as before.
    struct DensePushforwardBufs { double *dsv = nullptr, *dd = nullptr, *st = nullptr, *po = nullptr, *ex = nullptr; } dpf;
    Pool dense_pushforward_pool;
};

namespace qgdh {

int fail(qgd_handle h, int code, const std::string &msg);


#define HIP_TRY(h, expr)                                                                    \
    do {                                                                                    \
        hipError_t e__ = (expr);                                                            \
        if (e__ != hipSuccess)                                                              \
            return fail((h), QGD_ERR_NO_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)


template <typename T>
int dev_alloc(qgd_handle h, T **p, size_t count)
{
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, count * sizeof(T) + 64);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        // an allocation that does not fit is the caller's problem size, not a missing device (qgd.h: QGD_ERR_MEMORY)
        return fail(h, e == hipErrorOutOfMemory ? QGD_ERR_MEMORY : QGD_ERR_NO_DEVICE,
                    std::string("hipMalloc of ") + std::to_string(count * sizeof(T)) + " bytes: " + hipGetErrorString(e));
    }
    *p = static_cast<T *>(q);
    return QGD_OK;
}

template <typename T>
int dev_alloc(qgd_handle h, std::vector<void *> &pool, T **p, size_t count)
{
    const int rc = dev_alloc(h, p, count);
    if (!rc) pool.push_back(*p);
    return rc;
}


inline double factorial(int n) { double f = 1; for (int i = 2; i <= n; i++) f *= i; return f; }

// hermite.jl:389-391
inline double hermite_coefficient(int j, int p, int q) { return factorial(p) * factorial(p + q - j) / (factorial(p + q) * factorial(p - j)); }


inline size_t panel_index(int row, int col, int PWc) { return (size_t)row * PWc + (col >> 3) * 16 + (col & 7); }

// A host array [2N x c] (real parts in rows 0 .. N-1, imaginary parts in rows N .. 2N-1, column stride ld) into the panel
// layout [Np][PW] and back.
inline void pack_panel(double *panel, int PW, const double *a, int N, int c, size_t ld)
{
    for (int col = 0; col < c; col++) for (int i = 0; i < N; i++) {
        const size_t o = panel_index(i, col, PW);
        panel[o] = a[i + ld * col]; panel[o + 8] = a[N + i + ld * col];
    }
}

// An operator [N x N] (column-major) into plane `slot` of the padded column-major planes [Np x Np] of qgdk_ctx::ops (zeroed by
// the caller): qgd_create's own planes and those of every member of qgd_set_ensemble.
inline void pack_plane(double *planes, size_t slot, size_t Np, int N, const double *A)
{
    for (int j = 0; j < N; j++) for (int i = 0; i < N; i++) planes[slot * Np * Np + i + Np * j] = A[i + (size_t)N * j];
}

inline void unpack_panel(double *a, size_t ld, const double *panel, int PW, int N, int c)
{
    for (int col = 0; col < c; col++) for (int i = 0; i < N; i++) {
        const size_t o = panel_index(i, col, PW);
        a[i + ld * col] = panel[o]; a[N + i + ld * col] = panel[o + 8];
    }
}


// One event pair per (phase, slot): the pieces of a phase that the time-chunk pipeline launches on its side streams
// are bracketed separately (slot = chunk) and qgd_get_timings adds them up.
struct PhaseTimer {
    qgd_handle h; size_t idx; bool on; hipStream_t stream;
    PhaseTimer(qgd_handle h_, const char *name, hipStream_t s = nullptr, int slot = 0) : h(h_), idx(0), on(h_->timing), stream(s ? s : h_->k.stream)
    {
        if (on && !h->timing_only.empty() && h->timing_only != name) on = false;
        if (!on) return;
        for (idx = 0; idx < h->phases.size(); idx++) if (!strcmp(h->phases[idx].name, name) && h->phases[idx].slot == slot) break;
        if (idx == h->phases.size()) {
            Phase p{name, slot, nullptr, nullptr, false};
            (void)hipEventCreate(&p.e0); (void)hipEventCreate(&p.e1);
            h->phases.push_back(p);
        }
        h->phases[idx].used = true;
        (void)hipEventRecord(h->phases[idx].e0, stream);
    }
    ~PhaseTimer() { if (on) (void)hipEventRecord(h->phases[idx].e1, stream); }
};


// The transitions of the StoredSweep record (described at its declaration).
inline void hvp_void(qgd_handle h) { h->hvp_valid = false; }
inline void sweep_void(qgd_handle h) { h->sweep.kind = SWEEP_NONE; h->sweep.derivs = false; h->sweep.forced_basis = false; hvp_void(h); }

// a forward sweep is about to overwrite the buffers (after the checks that can refuse the call, before the first launch)
inline void sweep_begin(qgd_handle h) { sweep_void(h); h->sweep.front = false; }

inline void sweep_done(qgd_handle h, SweepKind kind, const double *pcof, int n_pcof, bool gradient = false)
{
    StoredSweep &s = h->sweep;
    hvp_void(h);
    s.kind = kind;
    s.has_pcof = pcof != nullptr;
    if (pcof) s.pcof.assign(pcof, pcof + n_pcof); else s.pcof.clear();
    s.gradient = gradient;
    s.reusable = true;
    s.derivs = false;
    s.forced_basis = false;
    s.front = kind == SWEEP_FRONT;
}

// a new target or cost type
inline void sweep_terminal_changed(qgd_handle h) { if (h->sweep.kind == SWEEP_FRONT) h->sweep.reusable = false; hvp_void(h); }

// the buffers hold a forward sweep that an adjoint sweep can differentiate
inline bool sweep_stored(qgd_handle h) { return h->sweep.kind == SWEEP_GENERAL || h->sweep.kind == SWEEP_FRONT; }

// may a history_precomputed call with this pcof skip the forward sweep?
inline bool sweep_reusable(qgd_handle h, const double *pcof, int n_pcof)
{
    const StoredSweep &s = h->sweep;
    if (!sweep_stored(h) || !s.reusable || s.has_pcof != (pcof != nullptr)) return false;
    return !pcof || (n_pcof > 0 && (size_t)n_pcof == s.pcof.size() && !memcmp(pcof, s.pcof.data(), sizeof(double) * n_pcof));
}


// How every entry point of the C ABI that touches the device begins, behind the refusals it makes from its arguments alone:
// a null handle is QGD_ERR_ARGUMENT; the handle's device becomes the thread's (QGD_ERR_NO_DEVICE); a handle whose stream is dead
// (qgd_handle_s::stream_dead) is refused with QGD_ERR_COMM before any HIP call that could wait for that stream; a captured
// graph is dropped unless ENTER_KEEPS_GRAPH; the time grid of a QGD_CREATE_DEFER_GRID handle is allocated unless ENTER_NO_GRID
// (entry points that neither read nor size anything by the grid, or that allocate it anew themselves).
enum { ENTER_KEEPS_GRAPH = 1, ENTER_NO_GRID = 2 };
int enter(qgd_handle h, unsigned flags = 0);
#define ENTER(h, ...) do { int re__ = qgdh::enter((h), ##__VA_ARGS__); if (re__) return re__; } while (0)

// history_precomputed with nothing stored that it could refer to: the refusal (else QGD_OK)
inline int refuse_reuse(qgd_handle h, int history_precomputed)
{
    return history_precomputed && h->sweep.kind == SWEEP_NONE ? fail(h, QGD_ERR_STATE, "history_precomputed without a previous forward evaluation") : QGD_OK;
}


#define K_TRY(h, expr)                                                                         \
    do {                                                                                       \
        int e__ = (expr);                                                                      \
        if (e__ != 0)                                                                          \
            return fail((h), QGD_ERR_NO_DEVICE, std::string(#expr) + ": " + hipGetErrorString((hipError_t)e__)); \
    } while (0)


// :StateTransfer divides by the GLOBAL column count, which a column shard does not know
#define COLUMN_SHARD_STATE_TRANSFER "cost type :StateTransfer is not supported on column shards (the cost is normalised by the global column count)"

#define NEEDS_RESIDENT_GRID(h, what)                                                                                   \
    do { if ((h)->chunks_eff > 1) return fail((h), QGD_ERR_UNSUPPORTED, std::string(what) + " needs the whole time grid resident: this handle " \
                                               "processes it in " + std::to_string((h)->chunks_eff) + " windows (raise qgd_set_memory_budget)"); } while (0)



// ---------------------------------------------------------------------------
// RCCL, bound at run time.  libqgd_hip.so has no link-time dependency on librccl: a single-GPU host never loads
// it.  dlopen("librccl.so.1") returns the copy already in the process when there is one (torch ships its own under
// the same SONAME), else the loader's search path, else /opt/rocm/lib.  QGD_RCCL_LIB names another file.
// ---------------------------------------------------------------------------
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;                          // (optional: older builds fall back to CommDestroy)
    ncclResult_t (*CommGetAsyncError)(ncclComm_t, ncclResult_t *) = nullptr;  // (optional)
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
    bool ok = false;
};


#define NCCL_TRY(h, expr)                                                                      \
    do {                                                                                       \
        ncclResult_t r__ = (expr);                                                             \
        if (r__ != ncclSuccess)                                                                \
            return fail((h), QGD_ERR_COMM, std::string(#expr) + ": " + rccl().GetErrorString(r__)); \
    } while (0)

RcclApi &rccl();

// Which trajectory outputs a call has, with which level map and which observables: what qgd_eval_populations,
// qgd_eval_expectations and qgd_eval_dense (one output selected), the two pullbacks and qgd_eval_pushforward (the outputs whose
// array is non-NULL) take from the caller.  The rules that follow from it alone are stated once, in qgd_host_output.cpp:
// selection_refusals (in front of ENTER), output_sizes (with `sc` slots x columns), upload_selection (on k.stream).
struct OutputSelection {
    bool states = false, pops = false, expect = false;
    const double *level_map = nullptr; int32_t n_groups = 0;
    const double *obs_re = nullptr, *obs_im = nullptr; int32_t n_obs = 0;
    bool with_map() const { return pops && level_map; }      // the populations are contracted with the map
    bool with_im() const { return expect && obs_im; }        // imaginary planes behind the real ones
};
// doubles of each output (0: not selected), of the level map, of one set of observable planes and of all of them
struct OutputSizes { size_t states, pops, expect, map, plane, planes; };

// What qgd_eval_states / qgd_eval_populations / qgd_eval_expectations take out of the state panels of a sweep: the states
// themselves [2N, slots, c], the level populations [N, slots, c] (n_groups = 0) or their contraction with the level map on the
// device [n_groups, slots, c], or the expectation values [n_obs, slots, c] of the observables whose planes lie in obs_planes
// (obs_im: imaginary planes behind the real ones)
// refine = 0: of the grid points, every qgd_set_save_every-th (the three calls above).  refine = r >= 1 (qgd_eval_dense): of the
// Hermite dense output, slot k at time k dt / r, every slot whatever qgd_set_save_every says; r = 1 is the grid points themselves
struct Observe { OutputSelection sel; double *out; int refine = 0; };      // (sel: one output selected)

// qgd_host_alloc.cpp
void free_pool(std::vector<void *> &pool);
void pool_release(Pool &pool);
int pool_ensure(qgd_handle h, Pool &pool, const KeyedPlan &p, const char *fit = nullptr, size_t extra = 0, const std::function<int()> &fill = {});
int pool_add(qgd_handle h, Pool &pool, double **slot, size_t count, size_t *len = nullptr);
void free_sensitivity_buffers(qgd_handle h);
void drop_graph(qgd_handle h);
int plan_windows(qgd_handle h, int chunks, int win);
int alloc_grid(qgd_handle h);

// qgd_host_sens.cpp
int forced_buffers(qgd_handle h, size_t nt, size_t B);
size_t forced_missing(qgd_handle h);
int trajectory_refusals(qgd_handle h, const std::string &name, const char *what, const double *pcof, int n_pcof, int history_precomputed, bool basis_bound);
int pullback_sweep(qgd_handle h, const double *pcof, int n_pcof, int history_precomputed);

// qgd_host_output.cpp
int selection_refusals(qgd_handle h, const OutputSelection &s, const char *subject, const char *tail = "");
OutputSizes output_sizes(const OutputSelection &s, size_t N, size_t sc);
int upload_selection(qgd_handle h, const OutputSelection &s, const OutputSizes &z, double *map, double *planes);
qgd_handle_s::HostReg *find_reg(qgd_handle h, const void *p, size_t bytes);
int finish_copies(qgd_handle h);
int grow_stage(qgd_handle h, Grown &g, size_t need);
int history_out(qgd_handle h, double *uv_history, int save = 1);
int panels_out(qgd_handle h, const double *panels, double **stage, double *out, size_t J, int n_first);
int lambda_history_out(qgd_handle h, double *out);
int observe_out(qgd_handle h, const Observe &obs, int save);
int dense_buffers(qgd_handle h, int refine);

// qgd_host_eval.cpp
int upload_pcof(qgd_handle h, const double *pcof, int n_pcof);
int forward_begin(qgd_handle h, const double *pcof, int n_pcof, bool allow_front = false);
int forward_end(qgd_handle h);
int adjoint_begin(qgd_handle h);
int adjoint_end(qgd_handle h);
int run_forward(qgd_handle h, const double *pcof, int n_pcof, bool allow_front = false);
bool tiny_applies(qgd_handle h, const double *pcof, int n_pcof);
int tiny_evaluate(qgd_handle h, const double *pcof, int n_pcof, bool gradient, double *grad, double *out3);
int check_status(qgd_handle h);
int fetch_results(qgd_handle h, double *grad, double *out3, const double *src = nullptr);
int batch_buffers(qgd_handle h, int n_pcof, int *members);

// qgd_host_windows.cpp
int enter_window(qgd_handle h, const double *pcof, int r, bool with_start_state);
int chunk_forward(qgd_handle h, const double *pcof, int n_pcof, int r, bool rerun);
int chunked_forward(qgd_handle h, const double *pcof, int n_pcof, double *uv_history = nullptr, int save = 1, const Observe *obs = nullptr);
int chunked_adjoint(qgd_handle h, double *lambda_history = nullptr, double *adjoint_forcing = nullptr);
int forcing_buffers(qgd_handle h, size_t nt, size_t B);
int upload_forcing(qgd_handle h, const double *forcing, size_t nt, size_t n_off);

// qgd_host_comm.cpp
RcclApi load_rccl();
bool comm_abort(qgd_handle h);
int comm_failed(qgd_handle h, const std::string &why);
int comm_local_error(qgd_handle h, int rc);
int comm_wait(qgd_handle h);
int comm_collective(qgd_handle h, int which);
const double *comm_result(qgd_handle h);

int comm_forward(qgd_handle h, const double *pcof, int n_pcof);
int comm_discrete_adjoint(qgd_handle h, const double *pcof, int n_pcof, int history_precomputed, double *grad, double *uv_history, double *lambda_history, double *adjoint_forcing, double *out3);
int comm_discrete_adjoint_body(qgd_handle h, const double *pcof, int n_pcof, int history_precomputed, double *grad, double *uv_history, double *lambda_history, double *adjoint_forcing, double *out3);
int comm_eval_forward(qgd_handle h, const double *pcof, int n_pcof, double *uv_history, double *out3);
int comm_eval_forward_body(qgd_handle h, const double *pcof, int n_pcof, double *uv_history, double *out3);

}  // namespace qgdh
