// qgd_k_hvp.hip -- exact Hessian-vector products by a second-order adjoint sweep.
// (conventions: qgd_kernels_common.h; notation: qgd_k_hessian.hip)
//
// With s_v = sum_l v_l s_l (ONE forced sweep with the direction gv[n][b] = sum_l G[n][b][l] v_l), z_b(n) and the
// half-matrices of e_n as k_hess_basis leaves them (they do not depend on v):
//   (H v)_k = - sum_{n,b} G[n][b][k] ( Re<s_v(n), z_b(n)> + sum_b' e_n[b][b'] gv[n][b'] )          (A)
//             + sum_n Re<s_k(n), f_n>                                                              (B)
//   f_n = - sum_b gv[n][b] z_b(n) + (2 dt/tf) trap_n W s_v(n),   f_N += Phi'' s_v(N)
// (B) has the shape of the first-order gradient: the adjoint sweep with terminal condition and forcing F = -f gives mu, and
// the gradient kernels run with mu in place of lambda.  No sensitivity of a single parameter is formed.
//
// The direction table is laid out as a control basis with ONE operator of NB/2 Taylor orders and ONE coefficient,
//   gvt[(tau' nt + n)(M + 1) + d'],  M = NB / 2,  b = tau' M + d',
// so that qgdk_forced_chains assembles the forcing of s_v from the basis responses through a context copy (n_ops = 1,
// m = M, n_pcof = 1): its index (k 2 + tau) fs_m + d of a basis response is b itself.
// Every sum runs in a fixed order: the product is the same bits on every run.
#include "qgd_kernels_common.h"

__host__ __device__ __forceinline__ size_t hv_gvi(int n, int b, int M, int nt) { return ((size_t)(b / M) * nt + n) * (M + 1) + b % M; }

// One workgroup = time point, one thread = basis direction b.
__global__ __launch_bounds__(64) void k_hvp_gv(const double *__restrict__ G, const int64_t *__restrict__ goff, const int32_t *__restrict__ ncoef,
                                               const int32_t *__restrict__ poff, const double *__restrict__ v, double *__restrict__ gvt,
                                               int m, int NB, int nt, int gnt, int gn0)
{
    const int n = blockIdx.x, b = threadIdx.x;
    if (b >= NB) return;
    const int o = b / (2 * m), tau = (b / m) % 2, d = b % m, nc = ncoef[o];
    const double *g = G + goff[o] + (((size_t)tau * gnt + n + gn0) * (m + 1) + d) * nc, *vo = v + poff[o];
    double acc = 0.0;
    for (int l = 0; l < nc; l++) acc += g[l] * vo[l];
    gvt[hv_gvi(n, b, NB / 2, nt)] = acc;
}

// The same for n_dir directions at once (qgd_eval_pushforward): one workgroup = (time point, direction j), v [n_pcof x n_dir]
// column-major.  The table gets n_dir coefficient columns, gvt[((tau' nt + n)(M + 1) + d') n_dir + j]: a one-operator basis with
// n_dir coefficients, whose "parameters" are the directions.  Each entry is the sum k_hvp_gv forms, in its order.
__global__ __launch_bounds__(64) void k_hvp_gv_dirs(const double *__restrict__ G, const int64_t *__restrict__ goff, const int32_t *__restrict__ ncoef,
                                                    const int32_t *__restrict__ poff, const double *__restrict__ v, double *__restrict__ gvt,
                                                    int m, int NB, int nt, int gnt, int gn0, int n_pcof, int n_dir)
{
    const int n = blockIdx.x, j = blockIdx.y, b = threadIdx.x;
    if (b >= NB) return;
    const int o = b / (2 * m), tau = (b / m) % 2, d = b % m, nc = ncoef[o];
    const double *g = G + goff[o] + (((size_t)tau * gnt + n + gn0) * (m + 1) + d) * nc, *vo = v + (size_t)j * n_pcof + poff[o];
    double acc = 0.0;
    for (int l = 0; l < nc; l++) acc += g[l] * vo[l];
    gvt[hv_gvi(n, b, NB / 2, nt) * n_dir + j] = acc;
}

// One workgroup = (column group, time point); Np <= 64, NB <= 64.  One pass over the NB panels z_b(n) of the column group
// (16-byte loads, a panel row of the group is 128 contiguous bytes) gives
//   part[n][grp][b] = sum_{rows, columns of grp} s_v(n) . z_b(n) + sum_b' (half[b][b'] + half[b'][b]) gv[n][b']
//   F[n] = sum_b gv[n][b] z_b(n) - gsc trap_n (W s_v)(n)  (+ term at the final time): the adjoint scan's forcing, its y_N
// W s_v from `ws` (general W) or the diagonal `gd` [2N] on the fly (both null: no guard).
__global__ __launch_bounds__(256) void k_hvp_forcing(const double *__restrict__ Z, const double *__restrict__ half,
                                                     const double *__restrict__ sv, const double *__restrict__ ws,
                                                     const double *__restrict__ gd, const double *__restrict__ gvt,
                                                     const double *__restrict__ term, double *__restrict__ F,
                                                     double *__restrict__ part, int Np, int N, int cp, int NB, int nt, double gsc)
{
    __shared__ double gvs[64];
    __shared__ double wsum[64][4];
    const int grp = blockIdx.x, n = blockIdx.y, gpc = gridDim.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int PWc = 2 * cp;
    const size_t hstep = (size_t)Np * PWc;
    if (tid < NB) gvs[tid] = gvt[hv_gvi(n, tid, NB / 2, nt)];
    __syncthreads();
    // the (at most two) pairs of panel entries of this thread
    bool on[2];
    size_t off[2];
    double2 s[2], f[2];
    const double tw = gsc * ((n == 0 || n == nt - 1) ? 0.5 : 1.0);
    #pragma unroll
    for (int it = 0; it < 2; it++) {
        const int e2 = tid + it * 256, row = e2 >> 3, q = (e2 & 7) * 2;
        on[it] = e2 < Np * 8;
        off[it] = on[it] ? (size_t)row * PWc + (size_t)grp * 16 + q : 0;      // (an idle thread reads entry 0 against s = 0 and stores nothing)
        s[it] = make_double2(0.0, 0.0);
        f[it] = make_double2(0.0, 0.0);
        if (!on[it]) continue;
        s[it] = *reinterpret_cast<const double2 *>(sv + (size_t)n * hstep + off[it]);
        if (ws) {
            const double2 w = *reinterpret_cast<const double2 *>(ws + (size_t)n * hstep + off[it]);
            f[it].x = -tw * w.x; f[it].y = -tw * w.y;
        } else if (gd && row < N) {
            const double g = gd[(q < 8 ? 0 : N) + row];
            f[it].x = -tw * g * s[it].x; f[it].y = -tw * g * s[it].y;
        }
        if (term && n == nt - 1) {
            const double2 t = *reinterpret_cast<const double2 *>(term + off[it]);
            f[it].x += t.x; f[it].y += t.y;
        }
    }
    const double *zn = Z + (size_t)n * NB * hstep;
    // four directions per trip, their loads issued together (a trip past NB re-reads the last panel with weight 0)
    for (int b0 = 0; b0 < NB; b0 += 4) {
        double2 z[4][2];
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            const int b = min(b0 + j, NB - 1);
            #pragma unroll
            for (int it = 0; it < 2; it++) z[j][it] = *reinterpret_cast<const double2 *>(zn + (size_t)b * hstep + off[it]);
        }
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool live = b0 + j < NB;
            const double gb = live ? gvs[min(b0 + j, NB - 1)] : 0.0;
            double p = 0.0;
            #pragma unroll
            for (int it = 0; it < 2; it++) {
                p += s[it].x * z[j][it].x + s[it].y * z[j][it].y;
                f[it].x += gb * z[j][it].x; f[it].y += gb * z[j][it].y;
            }
            #pragma unroll
            for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o);      // (a fixed butterfly: the same bits every run)
            if (lane == 0 && live) wsum[b0 + j][wave] = p;
        }
    }
    #pragma unroll
    for (int it = 0; it < 2; it++)
        if (on[it]) *reinterpret_cast<double2 *>(F + (size_t)n * hstep + off[it]) = f[it];
    __syncthreads();
    if (tid < NB) {
        const double *h = half + ((size_t)n * gpc + grp) * NB * NB;
        double acc = 0.0;
        for (int b2 = 0; b2 < NB; b2++) acc += (h[(size_t)tid * NB + b2] + h[(size_t)b2 * NB + tid]) * gvs[b2];
        part[((size_t)n * gpc + grp) * NB + tid] = (((wsum[tid][0] + wsum[tid][1]) + wsum[tid][2]) + wsum[tid][3]) + acc;
    }
}

// One workgroup = parameter k: out[k] = gB[k] - sum_{n, b of k's operator} G[n][b][k] sum_grp part[n][grp][b]
// (thread-strided ascending sums over n, then a fixed tree)
__global__ __launch_bounds__(256) void k_hvp_contract(const double *__restrict__ part, const double *__restrict__ G,
                                                      const int64_t *__restrict__ goff, const int32_t *__restrict__ ncoef,
                                                      const int32_t *__restrict__ poff, const double *__restrict__ gB,
                                                      double *__restrict__ out, int n_ops, int m, int nt, int gpc, int gnt, int gn0)
{
    __shared__ double red[256];
    const int k = blockIdx.x, NB = n_ops * 2 * m;
    int o = 0;
    while (o + 1 < n_ops && k >= poff[o + 1]) o++;
    const int nc = ncoef[o], lo = k - poff[o];
    double acc = 0.0;
    for (int n = threadIdx.x; n < nt; n += blockDim.x)
        for (int bb = 0; bb < 2 * m; bb++) {
            const int b = o * 2 * m + bb, tau = bb / m, d = bb % m;
            double a = 0.0;
            for (int grp = 0; grp < gpc; grp++) a += part[((size_t)n * gpc + grp) * NB + b];
            acc += G[goff[o] + (((size_t)tau * gnt + n + gn0) * (m + 1) + d) * nc + lo] * a;
        }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = gB[k] - red[0];
}

extern "C" {

size_t qgdk_hvp_gv_len(const qgdk_ctx *c) { const size_t M = (size_t)c->n_ops * c->m; return 2 * (size_t)c->nt * (M + 1); }

int qgdk_hvp_gv(const qgdk_ctx *c, const double *v, double *gvt)
{
    const int NB = c->n_ops * 2 * c->m;
    if (NB < 1 || NB > 64) return -1;
    hipLaunchKernelGGL(k_hvp_gv, dim3(c->nt), dim3(64), 0, c->stream, c->G, c->goff, c->ncoef, c->poff, v, gvt, c->m, NB, c->nt,
                       c->g_nt ? c->g_nt : c->nt, c->g_n0);
    return (int)hipGetLastError();
}

// the direction table of n_dir directions at once (v [n_pcof x n_dir] column-major on the device; gvt: n_dir * qgdk_hvp_gv_len doubles)
int qgdk_hvp_gv_dirs(const qgdk_ctx *c, const double *v, double *gvt, int n_dir)
{
    const int NB = c->n_ops * 2 * c->m;
    if (NB < 1 || NB > 64 || n_dir < 1 || n_dir > 65535) return -1;
    hipLaunchKernelGGL(k_hvp_gv_dirs, dim3(c->nt, n_dir), dim3(64), 0, c->stream, c->G, c->goff, c->ncoef, c->poff, v, gvt, c->m, NB, c->nt,
                       c->g_nt ? c->g_nt : c->nt, c->g_n0, c->n_pcof, n_dir);
    return (int)hipGetLastError();
}

// s_v at every time point: the forced scan with the single direction gvt (sv [nt][Np][2cp], sv[0] zeroed by the caller;
// phi [B][Np][2cp] and bnd [B+1][Np][2cp] scan buffers, bnd[0] zeroed by the caller; one3: device {goff = 0 | ncoef = 1, poff = 0})
int qgdk_hvp_forced_sweep(const qgdk_ctx *c, const double *gvt, const void *one3, double *phi, double *bnd, double *sv)
{
    return qgdk_hvp_forced_sweep_dirs(c, gvt, one3, phi, bnd, sv, 1);
}

// the same with n_dir directions side by side, as column groups of one scan: the table of qgdk_hvp_gv_dirs, sv [nt][Np][2 n_dir cp]
// with direction j in the columns j cp .. (the layout of qgd_eval_hessian's sensitivity history), phi and bnd n_dir times as wide,
// basis: device {goff = 0 | ncoef = n_dir, poff = 0}
int qgdk_hvp_forced_sweep_dirs(const qgdk_ctx *c, const double *gvt, const void *one3, double *phi, double *bnd, double *sv, int n_dir)
{
    qgdk_ctx d = *c;
    d.n_ops = 1; d.m = c->n_ops * c->m; d.n_pcof = n_dir;
    d.G = const_cast<double *>(gvt);
    d.goff = (int64_t *)one3; d.ncoef = (int32_t *)((char *)one3 + 8); d.poff = (int32_t *)((char *)one3 + 12);
    d.g_nt = 0; d.g_n0 = 0;
    d.have_guard = 0;        // (the guard part of the product comes from s_v's history, not from a sum accumulated by the scan)
    d.fs_phi = phi; d.fs_bnd = bnd; d.fs_gacc = nullptr; d.fs_shist = sv;
    return qgdk_forced_chains(&d);
}

int qgdk_hvp_forcing(const qgdk_ctx *c, const double *Z, const double *half, const double *sv, const double *ws,
                     const double *gvt, const double *term, double *F, double *part)
{
    const int NB = c->n_ops * 2 * c->m;
    if (NB < 1 || NB > 64 || c->Np > 64) return -1;      // (two pairs of panel entries per thread, 64 LDS slots)
    hipLaunchKernelGGL(k_hvp_forcing, dim3(c->cp / 8, c->nt), dim3(256), 0, c->stream, Z, half, sv,
                       c->have_guard == 1 ? ws : (const double *)nullptr, c->have_guard == 2 ? c->guard_diag : (const double *)nullptr,
                       gvt, term, F, part, c->Np, c->N, c->cp, NB, c->nt, 2.0 * c->dt / c->tf);
    return (int)hipGetLastError();
}

// mu: the adjoint sweep of `a` (a context copy whose forcing / yhist / lam are the product's own buffers) from the terminal
// value y_N = forcing[nt-1], copied to every place the adjoint scan starts from
int qgdk_hvp_adjoint(const qgdk_ctx *a)
{
    int rc;
    if ((rc = qgdk_copy_yN_to_starts(a, a->forcing + (size_t)(a->nt - 1) * a->Np * 2 * a->cp))) return rc;
    if ((rc = qgdk_adjoint_blocks(a)) || (rc = qgdk_adjoint_finish(a))) return rc;
    return qgdk_lambda(a);
}

int qgdk_hvp_contract(const qgdk_ctx *c, const double *part, const double *gB, double *out)
{
    hipLaunchKernelGGL(k_hvp_contract, dim3(c->n_pcof), dim3(256), 0, c->stream, part, c->G, c->goff, c->ncoef, c->poff, gB, out,
                       c->n_ops, c->m, c->nt, c->cp / 8, c->g_nt ? c->g_nt : c->nt, c->g_n0);
    return (int)hipGetLastError();
}

} // extern "C"
