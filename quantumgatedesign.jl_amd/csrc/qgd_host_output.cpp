// qgd_host_output.cpp -- host side of the C ABI (include/qgd.h), the reference-layout outputs (uv_history, lambda_history, adjoint_forcing,
// states, populations, expectation values) of a resident or a windowed grid: the copy stream, where the buffers' time points land in the caller's array, the
// one transport of staged bytes, the output functions.
#include "qgd_host.h"

namespace qgdh {


qgd_handle_s::HostReg *find_reg(qgd_handle h, const void *p, size_t bytes)
{
    for (auto &r : h->regs)
        if ((const char *)p >= (const char *)r.host && (const char *)p + bytes <= (const char *)r.host + r.bytes) return &r;
    return nullptr;
}


static int copy_side(qgd_handle h)
{
    if (!h->copy_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    // (two DMA engines for a large pinned download: 1.24 -> 0.87 ms for the reference-shaped cnot3 call on a box whose single
    //  engine path was slow)
    if (!h->copy_stream2) HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream2, hipStreamNonBlocking));
    if (!h->ev_ready) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_ready, hipEventDisableTiming));
    return QGD_OK;
}


// the copy stream takes over from the compute stream at this point of the launch sequence
static int hand_over(qgd_handle h)
{
    HIP_TRY(h, hipEventRecord(h->ev_ready, h->k.stream));
    HIP_TRY(h, hipStreamWaitEvent(h->copy_stream, h->ev_ready, 0));
    if (h->copy_stream2) HIP_TRY(h, hipStreamWaitEvent(h->copy_stream2, h->ev_ready, 0));
    h->copies_pending = true;
    return QGD_OK;
}


int finish_copies(qgd_handle h)
{
    if (h->copies_pending) {
        // (spinning on hipStreamQuery, or on an event recorded behind the copies: no difference, 0.94 ms either way)
        HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
        if (h->copy_stream2) HIP_TRY(h, hipStreamSynchronize(h->copy_stream2));
        h->copies_pending = false;
    }
    return QGD_OK;
}


// Device-to-host download on the copy stream.  A plain hipMemcpyAsync into REGISTERED host memory runs as a blit kernel
// (__amd_rocclr_copyBuffer): its waves fill the CUs and starve the adjoint chain kernels beside it (15 -> 410 us for the
// first of them on cnot3), which delays lambda and leaves the PCIe link idle at the end of the evaluation.  The same
// bytes as a pitched (rows x row_bytes, pitch = row_bytes) copy go through the DMA engine and leave the CUs alone.
static int download(qgd_handle h, void *dst, const void *src, size_t row_bytes, size_t rows)
{
    if (rows <= 1 || !find_reg(h, dst, row_bytes * rows))
        HIP_TRY(h, hipMemcpyAsync(dst, src, row_bytes * rows, hipMemcpyDeviceToHost, h->copy_stream));
    else if (h->copy_stream2 && rows >= 2 && row_bytes * rows > ((size_t)8 << 20)) {      // (experiment: two DMA engines side by side)
        const size_t r1 = rows / 2;
        HIP_TRY(h, hipMemcpy2DAsync(dst, row_bytes, src, row_bytes, row_bytes, r1, hipMemcpyDeviceToHost, h->copy_stream));
        HIP_TRY(h, hipMemcpy2DAsync((char *)dst + r1 * row_bytes, row_bytes, (const char *)src + r1 * row_bytes, row_bytes, row_bytes, rows - r1,
                                    hipMemcpyDeviceToHost, h->copy_stream2));
    } else
        HIP_TRY(h, hipMemcpy2DAsync(dst, row_bytes, src, row_bytes, row_bytes, rows, hipMemcpyDeviceToHost, h->copy_stream));
    return QGD_OK;
}


// Where the time points in the buffers land in the caller's array.  The buffers hold the local points 0 .. k.nt-1; of those from
// n_first on, every one whose GLOBAL index is a multiple of `save` is sent (saveEveryNsteps, forward_evolution.jl:104,178,239-241:
// slot s of the array holds global point s * save).  A windowed grid's array covers the whole grid and the buffers hold its
// points n_off .. n_off + nt - 1 (windows share their end points: same values, same slot); a resident grid is the one-window
// case of that.  The rank of a time partition has an n_off too, but its arrays hold its OWN points only (qgd_get_partition):
// it counts from its first point, like a resident grid.
struct Span {
    size_t first, count, stride;      // local points sent: first, first + stride, ... (count of them; 0: none falls into the buffers)
    size_t slot0;                     // the slot of the caller's array that `first` goes to
    size_t slots;                     // slots of the caller's array along time
};

// (refine = r > 1: the points are those of the Hermite dense output, r per step -- the buffers' nt points stand for the
//  1 + (nt-1) r of qgd_k_interp.hip's panels, a window's first one at n_off r)
static Span span_of(qgd_handle h, int save, int n_first, int refine = 1)
{
    const qgdk_ctx &k = h->k;
    const bool windowed = h->chunks_eff > 1;
    const size_t sv = (size_t)save, rf = (size_t)refine, base = windowed ? (size_t)k.n_off * rf : 0;
    const size_t total = ((windowed ? (size_t)k.nt_glob : (size_t)k.nt) - 1) * rf + 1, held = ((size_t)k.nt - 1) * rf + 1;
    const size_t g_lo = base + (size_t)n_first, g_hi = base + held - 1;      // global points on offer
    const size_t s_lo = (g_lo + sv - 1) / sv, s_hi = g_hi / sv;                      // the slots they fill
    const size_t slots = 1 + (total - 1) / sv;
    if (s_hi < s_lo) return Span{0, 0, sv, s_lo, slots};
    return Span{s_lo * sv - base, s_hi - s_lo + 1, sv, s_lo, slots};
}


// time points a staging buffer must hold: all of a resident grid (or of a partition rank's share), the longest window of a windowed one
static size_t stage_points(qgd_handle h)
{
    const qgdk_ctx &k = h->k;
    return h->chunks_eff > 1 ? std::min<size_t>((size_t)k.bpr * k.scan_blen + 1, (size_t)k.nt_glob) : (size_t)k.nt;
}


// staging buffers are allocated on first use, zero-filled (time points below n_first of a resident grid stay zero), and
// freed by alloc_grid
static int stage_alloc(qgd_handle h, double **stage, size_t doubles)
{
    if (*stage) return QGD_OK;
    int rc = pool_add(h, h->pools[POOL_STAGE], stage, doubles);
    if (rc) return rc;
    HIP_TRY(h, hipMemsetAsync(*stage, 0, doubles * sizeof(double), h->k.stream));
    return QGD_OK;
}


// a staging buffer that grows to the largest request (the copies that read the old one were awaited by the call that issued them)
int grow_stage(qgd_handle h, Grown &g, size_t need)
{
    return g.p && g.len >= need ? QGD_OK : pool_add(h, h->pools[POOL_STAGE], &g.p, need, &g.len);
}


// The one way out of a staging buffer [sd, lead + sp.count, c] -- `lead` slots in front of the span's first -- into the caller's
// [dd, sp.slots, c], behind everything on the compute stream so far.  dd > sd (lambda_history without derivative columns:
// sd = 2N of every dd = (1+m) 2N doubles, the rest zero): rows of sd doubles, dd apart.
// Resident grid: the staging buffer is the whole array, the slots in front (zeros) included; asynchronous -- the caller ends
// with finish_copies().  Windowed grid: a pitched copy into the span's slots (the zeros of the others are the pass's memset),
// awaited here, before the next window overwrites the panels.
static int send_staged(qgd_handle h, const double *stage, size_t sd, size_t lead, const Span &sp, double *out, size_t dd)
{
    const size_t c = h->k.c, held = lead + sp.count, B = sizeof(double);
    int rc = copy_side(h);
    if (rc || (rc = hand_over(h))) return rc;
    if (h->chunks_eff == 1) {
        const size_t rows = held * c;
        if (dd == sd) return download(h, out, stage, sd * B, rows);
        if (qgd_handle_s::HostReg *reg = find_reg(h, out, rows * dd * B)) {      // pinned: one strided copy; the rest is zero-filled once
            if (!reg->zeroed) { memset(out, 0, rows * dd * B); reg->zeroed = true; }
            HIP_TRY(h, hipMemcpy2DAsync(out, dd * B, stage, sd * B, sd * B, rows, hipMemcpyDeviceToHost, h->copy_stream));
            return QGD_OK;
        }
        h->scatter_tmp.resize(rows * sd);      // pageable: a compact copy, scattered on the host
        HIP_TRY(h, hipMemcpyAsync(h->scatter_tmp.data(), stage, rows * sd * B, hipMemcpyDeviceToHost, h->copy_stream));
        HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
        memset(out, 0, rows * dd * B);
        for (size_t r = 0; r < rows; r++) memcpy(out + r * dd, h->scatter_tmp.data() + r * sd, sd * B);
        return QGD_OK;
    }
    const double *src = stage + lead * sd;
    double *dst = out + sp.slot0 * dd;
    if (dd == sd) {      // one row per column
        HIP_TRY(h, hipMemcpy2DAsync(dst, sp.slots * dd * B, src, held * sd * B, sp.count * sd * B, c, hipMemcpyDeviceToHost, h->copy_stream));
    } else {
        for (size_t col = 0; col < c; col++)
            HIP_TRY(h, hipMemcpy2DAsync(dst + col * sp.slots * dd, dd * B, src + col * held * sd, sd * B, sd * B, sp.count, hipMemcpyDeviceToHost, h->copy_stream));
    }
    return finish_copies(h);
}


// state history: panels hist [nt][Np][2cp] (j = 0) and dpsi [nt][m][Np][2cp] (j = 1..m) -> the reference's
// uv_history[2N, 1+m, slots, c] (forward_evolution.jl:42-44); the re-layout kernel reads the panels with a stride of `save` points.
// (Writing registered host arrays in place with a few persistent workgroups instead of staging + copying was measured slower
// in round 2 -- 0.96 ms at best against 0.91 for the 31.6 MB of the cnot3 call -- and is gone.)
int history_out(qgd_handle h, double *uv_history, int save)
{
    qgdk_ctx &k = h->k;
    const size_t hstep = (size_t)k.Np * 2 * k.cp, m = k.m, n2 = 2 * (size_t)k.N, sd = (m + 1) * n2;
    const Span sp = span_of(h, save, 0);
    if (!sp.count) return QGD_OK;
    int rc = stage_alloc(h, &h->stage_hist, sd * stage_points(h) * k.c);      // (a strided call uses its front)
    if (rc) return rc;
    const long long dcol = (long long)(sp.count * sd), dn = (long long)sd, dj = (long long)n2;
    K_TRY(h, qgdk_layout(&k, k.hist + sp.first * hstep, (long long)(hstep * sp.stride), 0, h->stage_hist, dcol, dn, dj, 0, (int)sp.count, 1, 0, k.stream, 0));
    K_TRY(h, qgdk_layout(&k, k.dpsi + sp.first * m * hstep, (long long)(m * hstep * sp.stride), (long long)hstep, h->stage_hist + n2, dcol, dn, dj, 0, (int)sp.count, (int)m, 0, k.stream, 0));
    return send_staged(h, h->stage_hist, sd, 0, sp, uv_history, sd);
}


// one panel per time point (lambda, adjoint forcing), local points n_first .. nt-1 -> [2N, J, slots, c] with only Taylor index 0
// written (J = 1: adjoint_forcing; J = 1+m: lambda_history, whose other columns are zero)
int panels_out(qgd_handle h, const double *panels, double **stage, double *out, size_t J, int n_first)
{
    qgdk_ctx &k = h->k;
    const size_t hstep = (size_t)k.Np * 2 * k.cp, nt = k.nt, n2 = 2 * (size_t)k.N;
    const Span sp = span_of(h, 1, n_first);
    if (!sp.count) return QGD_OK;
    int rc = stage_alloc(h, stage, n2 * stage_points(h) * k.c);
    if (rc) return rc;
    K_TRY(h, qgdk_layout(&k, panels, (long long)hstep, 0, *stage, (long long)(nt * n2), (long long)n2, 0, n_first, (int)sp.count, 1, 0, k.stream, 0));
    return send_staged(h, *stage, n2, sp.first, sp, out, J * n2);
}


// lambda_history: local time indices 1 .. nt-1 (a window's first point is the previous window's last; global index 0 is never
// written and stays zero, as in the reference, forward_evolution.jl:414-480).  With qgd_set_lambda_derivatives its derivative
// columns too: lam [nt][Np][2cp] (j = 0) and dlam [nt][m][Np][2cp] (k_adjoint_derivs, j = 1..m) -> [2N, 1+m, slots, c].
int lambda_history_out(qgd_handle h, double *out)
{
    qgdk_ctx &k = h->k;
    const size_t hstep = (size_t)k.Np * 2 * k.cp, nt = k.nt, m = k.m, n2 = 2 * (size_t)k.N, sd = (m + 1) * n2;
    if (!h->lambda_derivs) return panels_out(h, k.lam, &h->stage_lam, out, m + 1, 1);
    const Span sp = span_of(h, 1, 1);
    if (!sp.count) return QGD_OK;
    const size_t P = stage_points(h);
    int rc;
    if (!h->dlam) {
        if ((rc = pool_add(h, h->pools[POOL_STAGE], &h->dlam, P * std::max<size_t>(m, 1) * hstep))) return rc;
        // (the 1+m work panels of k_adjoint_derivs: LDS up to 150 KB, else an HBM slab per workgroup)
        if ((m + 1) * (size_t)k.Np * 16 * sizeof(double) > 150 * 1024 &&
            (rc = pool_add(h, h->pools[POOL_STAGE], &h->dlam_scratch, (P - 1) * (size_t)(k.cp / 8) * (m + 1) * k.Np * 16))) return rc;
    }
    if ((rc = stage_alloc(h, &h->stage_lam_full, sd * P * k.c))) return rc;
    { PhaseTimer t(h, "lambda_derivs"); K_TRY(h, qgdk_adjoint_derivs(&k, h->dlam, h->dlam_scratch)); }
    const long long dcol = (long long)(nt * sd), dn = (long long)sd, dj = (long long)n2;
    K_TRY(h, qgdk_layout(&k, k.lam, (long long)hstep, 0, h->stage_lam_full, dcol, dn, dj, 1, (int)sp.count, 1, 0, k.stream, 0));
    K_TRY(h, qgdk_layout(&k, h->dlam, (long long)(m * hstep), (long long)hstep, h->stage_lam_full + n2, dcol, dn, dj, 1, (int)sp.count, (int)m, 0, k.stream, 0));
    return send_staged(h, h->stage_lam_full, sd, sp.first, sp, out, sd);
}


// Weights of the two-point Hermite interpolant of degree 2m+1 (qgd_k_interp.hip) at theta = s / r, s = 1 .. r-1, as the kernel
// reads them: w[s-1][j][0] = dt^j A_j(theta), w[s-1][j][1] = (-dt)^j A_j(1 - theta),
// A_j(x) = x^j (1-x)^(m+1) sum_{k=0..m-j} C(m+k, k) x^k.  Every term is non-negative on [0, 1]: no cancellation.
static void dense_weights(std::vector<double> &w, int m, int r, double dt)
{
    w.assign((size_t)2 * (m + 1) * (r - 1), 0.0);
    auto A = [m](int j, double x, double y) {      // y = 1 - x, formed without rounding the difference
        double sum = 0.0, binom = 1.0, xk = 1.0;
        for (int k = 0; k <= m - j; k++) { sum += binom * xk; binom = binom * (m + k + 1) / (k + 1); xk *= x; }
        return std::pow(x, j) * std::pow(y, m + 1) * sum;
    };
    for (int s = 1; s < r; s++) {
        const double x = (double)s / r, y = (double)(r - s) / r;
        for (int j = 0; j <= m; j++) {
            w[((size_t)(s - 1) * (m + 1) + j) * 2] = std::pow(dt, j) * A(j, x, y);
            w[((size_t)(s - 1) * (m + 1) + j) * 2 + 1] = std::pow(-dt, j) * A(j, y, x);
        }
    }
}


// buffers of qgd_eval_dense (refine > 1): the interpolated panels of a resident grid, or of the longest window of a windowed
// one, and the weight table, in a sensitivity pool with a fit check.  (One buffer, no slabs: 8 KB per sub-point at cnot3.)  The
// key holds all that sizes or fills them: the points, refine, the panel size, m and dt.
int dense_buffers(qgd_handle h, int refine)
{
    const qgdk_ctx &k = h->k;
    const size_t hstep = (size_t)k.Np * 2 * k.cp, P = stage_points(h), pts = 1 + (P - 1) * (size_t)refine;
    size_t dt_bits = 0;
    memcpy(&dt_bits, &k.dt, sizeof(double) < sizeof(size_t) ? sizeof(double) : sizeof(size_t));
    return pool_ensure(h, h->pools[POOL_DENSE], {{P, (size_t)refine, hstep, (size_t)k.m, dt_bits},
                       {{&h->dense_panels, pts * hstep}, {&h->dense_w, (size_t)2 * (k.m + 1) * (refine - 1)}}},
                       "the interpolated panels of qgd_eval_dense do not fit", 0, [&]() -> int {
        dense_weights(h->dense_w_host, k.m, refine, k.dt);
        HIP_TRY(h, hipMemcpyAsync(h->dense_w, h->dense_w_host.data(), h->dense_w_host.size() * sizeof(double), hipMemcpyHostToDevice, k.stream));
        return QGD_OK;
    });
}


// qgd_eval_states / qgd_eval_populations / qgd_eval_expectations: the state panels hist [nt][Np][2cp] in the buffers -> the
// caller's [rows, slots, c], rows = 2N (the states: Taylor index 0 of uv_history, through the same re-layout kernel), N (level
// populations), n_groups (populations contracted with the level map in obs_map) or n_obs (expectation values of the observables
// in obs_planes).  No stage derivatives, a staging buffer of exactly the bytes that leave.
// qgd_eval_dense with refine > 1: the stage derivatives are formed where the sweep has none, qgd_k_interp.hip turns the buffers'
// nt points into 1 + (nt-1) refine panels of the same layout, and those take the place of hist (save = 1).
int observe_out(qgd_handle h, const Observe &obs, int save)
{
    qgdk_ctx &k = h->k;
    const size_t hstep = (size_t)k.Np * 2 * k.cp;
    const OutputSelection &s = obs.sel;
    const OutputSizes z = output_sizes(s, (size_t)k.N, 1);
    const size_t rows = z.states + z.pops + z.expect;      // (one of them is selected)
    const bool dense = obs.refine > 1;
    const Span sp = span_of(h, save, 0, dense ? obs.refine : 1);
    if (!sp.count) return QGD_OK;
    int rc;
    const double *panels = k.hist;
    if (dense) {
        // (qgd_eval_dense made the buffers for the longest window before the sweep: this finds them under their key and
        //  allocates nothing, so QGD_ERR_MEMORY is decided there, before anything ran)
        if ((rc = dense_buffers(h, obs.refine))) return rc;
        if (!h->sweep.derivs) { PhaseTimer t(h, "derivs"); K_TRY(h, qgdk_derivs(&k)); h->sweep.derivs = true; }
        PhaseTimer t(h, "dense_output");
        K_TRY(h, qgdk_interp(&k, k.hist, k.dpsi, h->dense_panels, obs.refine, h->dense_w, k.stream));
        panels = h->dense_panels;
    }
    if ((rc = grow_stage(h, h->stage_obs, rows * sp.count * k.c))) return rc;
    const double *src = panels + sp.first * hstep;
    if (s.states) {
        K_TRY(h, qgdk_layout(&k, src, (long long)(hstep * sp.stride), 0, h->stage_obs.p, (long long)(sp.count * rows), (long long)rows, 0, 0, (int)sp.count, 1, 0, k.stream, 0));
    } else if (s.expect) {
        PhaseTimer t(h, "expectations");
        K_TRY(h, qgdk_expectations(&k, src, (long long)(hstep * sp.stride), h->stage_obs.p, (long long)(sp.count * rows), (long long)rows, (int)sp.count,
                                   h->obs_planes.p, s.with_im() ? h->obs_planes.p + z.plane : nullptr, s.n_obs, k.stream));
    } else {
        PhaseTimer t(h, "populations");
        K_TRY(h, qgdk_populations(&k, src, (long long)(hstep * sp.stride), h->stage_obs.p, (long long)(sp.count * rows), (long long)rows, (int)sp.count,
                                  s.with_map() ? h->obs_map.p : nullptr, s.with_map() ? s.n_groups : 0, k.stream));
    }
    return send_staged(h, h->stage_obs.p, rows, 0, sp, obs.out, rows);
}


// The rules of an OutputSelection (qgd_host.h).  What a call refuses from its selection alone, in front of ENTER (`subject`,
// `tail`: the caller's wording of the observable message):
int selection_refusals(qgd_handle h, const OutputSelection &s, const char *subject, const char *tail)
{
    if (s.level_map && s.n_groups < 1) return fail(h, QGD_ERR_ARGUMENT, "a level map needs n_groups >= 1");
    if (s.expect && (!s.obs_re || s.n_obs < 1)) return fail(h, QGD_ERR_ARGUMENT, std::string(subject) + " needs obs_re and n_obs >= 1" + tail);
    return QGD_OK;
}

// the doubles of its outputs [2N | n_groups or N | n_obs, sc] and of its uploads [n_groups, N], [N, N, n_obs] once or twice
OutputSizes output_sizes(const OutputSelection &s, size_t N, size_t sc)
{
    OutputSizes z;
    z.states = s.states ? 2 * N * sc : 0;
    z.pops = s.pops ? (s.with_map() ? (size_t)s.n_groups : N) * sc : 0;
    z.expect = s.expect ? (size_t)s.n_obs * sc : 0;
    z.map = s.with_map() ? (size_t)s.n_groups * N : 0;
    z.plane = s.expect ? (size_t)s.n_obs * N * N : 0;
    z.planes = (s.with_im() ? 2 : 1) * z.plane;
    return z;
}

// and the uploads themselves: the map, the real planes and the imaginary ones behind them
int upload_selection(qgd_handle h, const OutputSelection &s, const OutputSizes &z, double *map, double *planes)
{
    const struct { double *dst; const double *src; size_t n; } up[] = {
        {map, s.level_map, z.map}, {planes, s.obs_re, z.plane}, {planes + z.plane, s.obs_im, s.with_im() ? z.plane : 0}};
    for (const auto &u : up)
        if (u.n) HIP_TRY(h, hipMemcpyAsync(u.dst, u.src, u.n * sizeof(double), hipMemcpyHostToDevice, h->k.stream));
    return QGD_OK;
}

}  // namespace qgdh
