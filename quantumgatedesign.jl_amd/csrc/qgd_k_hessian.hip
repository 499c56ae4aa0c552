// qgd_k_hessian.hip -- exact Hessian of the discrete objective.  (conventions: qgd_kernels_common.h)
//
//   H_kl = Phi''[s_k(N), s_l(N)] + Gamma''[s_k, s_l] + G^_k(s_l) + G^_l(s_k) + E_kl
//
// with s_l the forced-sweep sensitivities (their history is written by the third pass of qgdk_forced_chains), lambda and
// the reverse-swept gradient seeds g_j of the adjoint evaluation, and b = (operator, p|q, d) the 2 n_ops m basis
// directions of dA_d, Omega_b = -i Sym_k (p) or Asym_k (q).  Per time point, with h_{b,i} = Omega_b^H g_{i+d_b+1}/(i+d_b+1),
// the adjoint of the homogeneous Taylor recursion (y_i = h_{b,i}, then y_i += A_{J-1-i}^H y_J / J for J = m-1 .. 1) gives
//   z_b = y_0:                 sigma^s[n][b][l] = Re<s_l(n), z_b(n)>  (the gradient formula with psi replaced by s_l)
//   half[b][b'] = sum_{J > d'} Re<Omega_b' w_{J-1-d'}, y_J>/J,  e_n[b][b'] = half[b][b'] + half[b'][b]
// (the basis responses U^b' of k_forced_basis contracted with the seeds, without forming U), and
//   H = Y + Y^T + Gamma'' + Phi'',   Y[k][l] = -sum_{n,b} G[n][b][k] (sigma^s[n][b][l] + 1/2 sum_b' e_n[b][b'] G[n][b'][l]).
// Phi'' is host arithmetic on s_N (as the forced gradient's terminal part).  Every sum runs in a fixed order: the Hessian is
// the same bits on every run.  Plain fp64 FMA loops over panel slices; the working panels live in a global slab per workgroup.
#include "qgd_kernels_common.h"

#define HS_SYNC() do { __threadfence_block(); __syncthreads(); } while (0)

// deterministic sum over the 256 threads of a workgroup (red: 256 doubles of LDS)
__device__ __forceinline__ double hs_block_sum(double v, double *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// out (+)= f * Op x on a panel slice [Np][16] (x row stride ldx, out row stride 16).  Op: the real plane M (column-major
// Np x Np) or its transpose.  Rows >= N are zero.
__device__ __forceinline__ void hs_plane(const double *__restrict__ M, int trans, double fr, double fi, double sc,
                                         const double *x, int ldx, double *out, int Np, int N, bool acc)
{
    for (int e = threadIdx.x; e < Np * 8; e += blockDim.x) {
        const int i = e >> 3, j = e & 7;
        double sr = 0.0, si = 0.0;
        if (i < N)
            for (int k = 0; k < N; k++) {
                const double v = trans ? M[(size_t)k + (size_t)Np * i] : M[(size_t)i + (size_t)Np * k];
                sr += v * x[(size_t)k * ldx + j];
                si += v * x[(size_t)k * ldx + 8 + j];
            }
        const double orr = sc * (fr * sr - fi * si), oi = sc * (fr * si + fi * sr);
        if (acc) { out[i * 16 + j] += orr; out[i * 16 + 8 + j] += oi; }
        else { out[i * 16 + j] = orr; out[i * 16 + 8 + j] = oi; }
    }
}

// out += sc * A_d(t_n)^H x (panel slices, row stride 16)
template <int NOPS>
__device__ __forceinline__ void hs_aH(const double *__restrict__ ops, const OpCoef &cf, double sc, const double *x, double *out,
                                      int Np, int N, int n_ops)
{
    for (int e = threadIdx.x; e < Np * 8; e += blockDim.x) {
        const int i = e >> 3, j = e & 7;
        if (i >= N) continue;
        double sr = 0.0, si = 0.0;
        for (int k = 0; k < N; k++) {      // A^H(i,k) = conj(A(k,i))
            double are, aim;
            assembled_a<NOPS>(ops, Np, n_ops, cf, k, i, are, aim);
            const double xr = x[k * 16 + j], xi = x[k * 16 + 8 + j];
            sr += are * xr + aim * xi;
            si += are * xi - aim * xr;
        }
        out[i * 16 + j] += sc * sr;
        out[i * 16 + 8 + j] += sc * si;
    }
}

__host__ __device__ __forceinline__ size_t hess_slab(int Np, int m, int n_ops) { return (size_t)(2 * m + 2 * n_ops * (m > 1 ? m - 1 : 0) + 1) * Np * 16; }

// One workgroup = (column group, time point).  Outputs Z [nt][NB][Np][2cp] and half [nt][gpc][NB][NB].
template <int NOPS>
__global__ __launch_bounds__(256) void k_hess_basis(const double *__restrict__ ops, const double *__restrict__ tab,
                                                    const double *__restrict__ hist, const double *__restrict__ dpsi,
                                                    const double *__restrict__ lam, const double *__restrict__ cw,
                                                    double *__restrict__ Z, double *__restrict__ half, double *__restrict__ slab,
                                                    int Np, int N, int cp, int n_ops, int m, int nt)
{
    __shared__ double red[256];
    const int grp = blockIdx.x, n = blockIdx.y, gpc = gridDim.x;
    const int PWc = 2 * cp, ps = Np * 16, NB = n_ops * 2 * m, mv = m > 1 ? m - 1 : 0;
    const size_t hstep = (size_t)Np * PWc, pl = (size_t)Np * Np;
    double *Gs = slab + ((size_t)n * gpc + grp) * hess_slab(Np, m, n_ops);
    double *Ys = Gs + (size_t)m * ps, *Vs = Ys + (size_t)m * ps;
    // seeds g_j = c_j dt^j lambda_{n+1} - c_j (-dt)^j lambda_n  (lambda_0 and lambda_nt taken as zero)
    for (int e = threadIdx.x; e < ps; e += blockDim.x) {
        const size_t o = (size_t)(e >> 4) * PWc + grp * 16 + (e & 15);
        const double ln = (n + 1 < nt) ? lam[(size_t)(n + 1) * hstep + o] : 0.0;
        const double lh = (n >= 1) ? lam[(size_t)n * hstep + o] : 0.0;
        for (int j = 1; j <= m; j++) Gs[(size_t)(j - 1) * ps + e] = cw[2 * j] * ln - cw[2 * j + 1] * lh;
    }
    HS_SYNC();
    // the gradient's reverse sweep: g_i += (1/j) A_{j-1-i}^H g_j, j = m .. 2
    for (int j = m; j >= 2; j--) {
        for (int i = 1; i < j; i++) {
            OpCoef cf;
            load_coef(cf, tab, n, j - 1 - i, m, n_ops);
            hs_aH<NOPS>(ops, cf, 1.0 / j, Gs + (size_t)(j - 1) * ps, Gs + (size_t)(i - 1) * ps, Np, N, n_ops);
        }
        HS_SYNC();
    }
    // V_{o,tau,i} = Omega w_i, i < m-1
    for (int o = 0; o < n_ops; o++)
        for (int tau = 0; tau < 2; tau++)
            for (int i = 0; i < mv; i++) {
                const double *w = (i == 0 ? hist + (size_t)n * hstep : dpsi + ((size_t)n * m + (i - 1)) * hstep) + grp * 16;
                const double *M = ops + (size_t)(tau == 0 ? 3 + 2 * o : 2 + 2 * o) * pl;
                hs_plane(M, 0, tau ? 1.0 : 0.0, tau ? 0.0 : -1.0, 1.0, w, PWc, Vs + ((size_t)(o * 2 + tau) * mv + i) * ps, Np, N, false);
            }
    HS_SYNC();
    for (int b = 0; b < NB; b++) {
        const int o = b / (2 * m), tau = (b / m) % 2, d = b % m;
        const double *M = ops + (size_t)(tau == 0 ? 3 + 2 * o : 2 + 2 * o) * pl;
        // y_i = Omega_b^H g_{i+d+1} / (i+d+1); Omega^H = i Sym (p), Asym^T (q)
        for (int i = 0; i < m; i++) {
            if (i + d + 1 <= m) hs_plane(M, 1, tau ? 1.0 : 0.0, tau ? 0.0 : 1.0, 1.0 / (i + d + 1), Gs + (size_t)(i + d) * ps, 16,
                                         Ys + (size_t)i * ps, Np, N, false);
            else for (int e = threadIdx.x; e < ps; e += blockDim.x) Ys[(size_t)i * ps + e] = 0.0;
        }
        HS_SYNC();
        for (int J = m - 1; J >= 1; J--) {
            for (int i = 0; i < J; i++) {
                OpCoef cf;
                load_coef(cf, tab, n, J - 1 - i, m, n_ops);
                hs_aH<NOPS>(ops, cf, 1.0 / J, Ys + (size_t)J * ps, Ys + (size_t)i * ps, Np, N, n_ops);
            }
            HS_SYNC();
        }
        double *zo = Z + ((size_t)n * NB + b) * hstep + grp * 16;
        for (int e = threadIdx.x; e < ps; e += blockDim.x) zo[(size_t)(e >> 4) * PWc + (e & 15)] = Ys[e];
        double *ho = half + (((size_t)n * gpc + grp) * NB + b) * NB;
        for (int b2 = 0; b2 < NB; b2++) {
            const int o2 = b2 / (2 * m), tau2 = (b2 / m) % 2, d2 = b2 % m;
            double part = 0.0;
            for (int J = d2 + 1; J <= m - 1; J++) {
                const double *v = Vs + ((size_t)(o2 * 2 + tau2) * mv + (J - 1 - d2)) * ps, *y = Ys + (size_t)J * ps;
                double p = 0.0;
                for (int e = threadIdx.x; e < ps; e += blockDim.x) p += v[e] * y[e];
                part += p / J;
            }
            const double tot = hs_block_sum(part, red);
            if (threadIdx.x == 0) ho[b2] = tot;
        }
        HS_SYNC();
    }
}

// G[n][b][l] of the control basis (0 when l is not a coefficient of b's operator)
__device__ __forceinline__ double hs_gtab(const double *__restrict__ G, const int64_t *__restrict__ goff, const int32_t *__restrict__ ncoef,
                                          const int32_t *__restrict__ poff, int n, int b, int l, int m, int gnt)
{
    const int o = b / (2 * m), tau = (b / m) % 2, d = b % m;
    const int lo = l - poff[o], nc = ncoef[o];
    if (lo < 0 || lo >= nc) return 0.0;
    return G[goff[o] + (((size_t)tau * gnt + n) * (m + 1) + d) * nc + lo];
}

// One workgroup = (parameter l, time point n), four waves: zt[n][b][l] = Re<s_l(n), z_b(n)> + 1/2 sum_b' e_n[b][b'] G[n][b'][l]
__global__ __launch_bounds__(256) void k_hess_sigma(const double *__restrict__ shist, const double *__restrict__ Z,
                                                    const double *__restrict__ half, const double *__restrict__ G,
                                                    const int64_t *__restrict__ goff, const int32_t *__restrict__ ncoef,
                                                    const int32_t *__restrict__ poff, double *__restrict__ zt,
                                                    int Np, int cp, int n_pcof, int NB, int m, int gnt)
{
    __shared__ double wsum[64][4];
    __shared__ double sig[64];
    const int l = blockIdx.x, n = blockIdx.y, gpc = cp / 8, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int PWc = 2 * cp, PWs = 2 * n_pcof * cp, W = gpc * 16;
    const size_t hstep = (size_t)Np * PWc, hstepS = (size_t)Np * PWs;
    const int cnt = Np * W;
    const double *sl = shist + (size_t)n * hstepS + (size_t)l * W;
    for (int b = 0; b < NB; b++) {
        const double *zb = Z + ((size_t)n * NB + b) * hstep;
        double p = 0.0;
        for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
            const int row = e / W, x = e - row * W;
            p += sl[(size_t)row * PWs + x] * zb[(size_t)row * PWc + x];
        }
        #pragma unroll
        for (int off = 32; off > 0; off >>= 1) p += __shfl_xor(p, off);      // (a fixed butterfly: the same bits every run)
        if (lane == 0) wsum[b][wave] = p;
    }
    __syncthreads();
    if ((int)threadIdx.x < NB) sig[threadIdx.x] = ((wsum[threadIdx.x][0] + wsum[threadIdx.x][1]) + wsum[threadIdx.x][2]) + wsum[threadIdx.x][3];
    __syncthreads();
    if ((int)threadIdx.x < NB) {
        const int b = threadIdx.x;
        double acc = 0.0;
        for (int b2 = 0; b2 < NB; b2++) {
            const double g = hs_gtab(G, goff, ncoef, poff, n, b2, l, m, gnt);
            if (g == 0.0) continue;
            double e = 0.0;
            for (int grp = 0; grp < gpc; grp++) {
                const double *h = half + ((size_t)n * gpc + grp) * NB * NB;
                e += h[(size_t)b * NB + b2] + h[(size_t)b2 * NB + b];
            }
            acc += e * g;
        }
        zt[((size_t)n * NB + b) * n_pcof + l] = sig[b] + 0.5 * acc;
    }
}

// One workgroup = parameter k: Y[k][l] = -sum_{n, b of k's operator} G[n][b][k] zt[n][b][l]
__global__ __launch_bounds__(256) void k_hess_contract(const double *__restrict__ zt, const double *__restrict__ G,
                                                       const int64_t *__restrict__ goff, const int32_t *__restrict__ ncoef,
                                                       const int32_t *__restrict__ poff, double *__restrict__ Y,
                                                       int n_pcof, int n_ops, int m, int nt, int gnt)
{
    const int k = blockIdx.x, NB = n_ops * 2 * m;
    int o = 0;
    while (o + 1 < n_ops && k >= poff[o + 1]) o++;
    for (int l = threadIdx.x; l < n_pcof; l += blockDim.x) {
        double acc = 0.0;
        for (int n = 0; n < nt; n++)
            for (int bb = 0; bb < 2 * m; bb++) {
                const int b = o * 2 * m + bb;
                acc += hs_gtab(G, goff, ncoef, poff, n, b, k, m, gnt) * zt[((size_t)n * NB + b) * n_pcof + l];
            }
        Y[(size_t)k * n_pcof + l] = -acc;
    }
}

// ws = W s for a general (non-diagonal) guard matrix W [2N][2N] column-major, real stacked form.
// One workgroup = (sensitivity column group, time point).
__global__ __launch_bounds__(256) void k_hess_wapply(const double *__restrict__ W, const double *__restrict__ shist,
                                                     double *__restrict__ ws, int Np, int N, int PWs)
{
    const int gs = blockIdx.x, n = blockIdx.y, N2 = 2 * N;
    const size_t base = (size_t)n * Np * PWs + (size_t)gs * 16;
    for (int e = threadIdx.x; e < Np * 16; e += blockDim.x) {
        const int row = e >> 4, q = e & 15, j = q & 7;
        double acc = 0.0;
        if (row < N) {
            const int r = (q < 8) ? row : N + row;
            for (int r2 = 0; r2 < N2; r2++) {
                const int srow = r2 < N ? r2 : r2 - N, sq = r2 < N ? j : 8 + j;
                acc += W[(size_t)r + (size_t)N2 * r2] * shist[base + (size_t)srow * PWs + sq];
            }
        }
        ws[base + (size_t)row * PWs + q] = acc;
    }
}

// Guard Gram  out[k][l] = sc * sum_n trap_n sum_{row < N, columns < c} s_k(n) . (W s_l)(n),  W s from `ws` (general W)
// or the diagonal `gd` [2N] applied on the fly.  fp64 MFMA 16x16x4: A = trap_n s_k (16 parameters x 4 history entries),
// B = (W s_l) (4 x 16 parameters).  For one (n, row) the history entries of a parameter are gpc*16 consecutive doubles, so no
// index arithmetic beyond shifts.  One workgroup = (upper-triangle tile, slice of the time points); its four waves take the
// (n, row) pairs of the slice in turn and add their accumulators in wave order; k_hess_gram_sum adds the slices in order.
__host__ __device__ __forceinline__ int hs_gram_splits(int n_pcof, int nt)
{
    const int T = (n_pcof + 15) / 16, ntu = T * (T + 1) / 2;
    int s = (2048 + ntu - 1) / ntu;
    return s < 1 ? 1 : (s > nt ? nt : s);
}

__global__ __launch_bounds__(256) void k_hess_gram(const double *__restrict__ shist, const double *__restrict__ ws,
                                                   const double *__restrict__ gd, double *__restrict__ part,
                                                   int Np, int N, int c, int cp, int n_pcof, int nt)
{
    __shared__ double red[4][4][64];
    const int T = (n_pcof + 15) / 16, ntu = gridDim.x, t0 = blockIdx.x, sp = blockIdx.y, nsp = gridDim.y;
    int ti = 0, t = t0;
    while (t >= T - ti) { t -= T - ti; ti++; }
    const int tj = ti + t, k0 = ti * 16, l0 = tj * 16;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c16 = lane & 15, kk = lane >> 4;
    const int W = (cp / 8) * 16, PWs = 2 * n_pcof * cp;
    const size_t hstepS = (size_t)Np * PWs;
    const int chunk = (nt + nsp - 1) / nsp, n_lo = sp * chunk, n_hi = min(nt, n_lo + chunk);
    const bool ka = k0 + c16 < n_pcof, lb = l0 + c16 < n_pcof;
    d4 acc = (d4){0, 0, 0, 0};
    const int items = (n_hi > n_lo ? n_hi - n_lo : 0) * N;
    for (int it = wave; it < items; it += 4) {
        const int n = n_lo + it / N, row = it % N;
        const double wn = (n == 0 || n == nt - 1) ? 0.5 : 1.0;
        const size_t base = (size_t)n * hstepS + (size_t)row * PWs;
        const double *pa = shist + base + (size_t)(k0 + c16) * W;
        const size_t ob = base + (size_t)(l0 + c16) * W;
        for (int x0 = 0; x0 < W; x0 += 4) {
            const int x = x0 + kk, q = x & 15;
            const bool valid = (x >> 4) * 8 + (q & 7) < c;
            const double a = (ka && valid) ? wn * pa[x] : 0.0;
            double b = 0.0;
            if (lb && valid) b = ws ? ws[ob + x] : gd[(q < 8 ? 0 : N) + row] * shist[ob + x];
            acc = MFMA(a, b, acc);
        }
    }
    #pragma unroll
    for (int r = 0; r < 4; r++) red[wave][r][lane] = acc[r];
    __syncthreads();
    if (wave == 0) {
        double *o = part + ((size_t)sp * ntu + t0) * 256;
        #pragma unroll
        for (int r = 0; r < 4; r++)
            o[(kk + 4 * r) * 16 + c16] = ((red[0][r][lane] + red[1][r][lane]) + red[2][r][lane]) + red[3][r][lane];
    }
}

// the slices of every upper tile added in order, scaled and written to both triangles (diagonal tiles: the upper half)
__global__ __launch_bounds__(256) void k_hess_gram_sum(const double *__restrict__ part, double *__restrict__ out, int n_pcof, int nsp, double sc)
{
    const int T = (n_pcof + 15) / 16, ntu = gridDim.x, t0 = blockIdx.x;
    int ti = 0, t = t0;
    while (t >= T - ti) { t -= T - ti; ti++; }
    const int tj = ti + t, i = threadIdx.x >> 4, j = threadIdx.x & 15, k = ti * 16 + i, l = tj * 16 + j;
    if (k >= n_pcof || l >= n_pcof || (ti == tj && i > j)) return;
    double v = 0.0;
    for (int s = 0; s < nsp; s++) v += part[((size_t)s * ntu + t0) * 256 + threadIdx.x];
    out[(size_t)k * n_pcof + l] = sc * v;
    out[(size_t)l * n_pcof + k] = sc * v;
}

extern "C" {

size_t qgdk_hess_slab(int Np, int m, int n_ops) { return hess_slab(Np, m, n_ops); }

// k_hess_basis alone: Z and the half-matrices of e_n depend on pcof only, not on the direction a Hessian is applied to
// (qgd_eval_hessian_vec keeps them on the handle)
int qgdk_hess_basis(const qgdk_ctx *c, double *Z, double *half, double *slab)
{
    if (c->n_ops * 2 * c->m > 64) return -1;      // (k_hess_sigma / k_hvp_forcing keep one value per direction in 64 LDS slots)
#define CALL_HB(NO) hipLaunchKernelGGL((k_hess_basis<NO>), dim3(c->cp / 8, c->nt), dim3(256), 0, c->stream, c->ops, c->tab, c->hist, \
                                       c->dpsi, c->lam, c->cw, Z, half, slab, c->Np, c->N, c->cp, c->n_ops, c->m, c->nt)
    DISPATCH_NOPS(c->n_ops, CALL_HB)
#undef CALL_HB
    return (int)hipGetLastError();
}

int qgdk_hess_kernels(const qgdk_ctx *c, const double *shist, double *Z, double *half, double *slab, double *zt, double *Y)
{
    const int NB = c->n_ops * 2 * c->m, gnt = c->g_nt ? c->g_nt : c->nt;
    HIPCHK((hipError_t)qgdk_hess_basis(c, Z, half, slab));
    hipLaunchKernelGGL(k_hess_sigma, dim3(c->n_pcof, c->nt), dim3(256), 0, c->stream, shist, Z, half, c->G, c->goff, c->ncoef, c->poff,
                       zt, c->Np, c->cp, c->n_pcof, NB, c->m, gnt);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_hess_contract, dim3(c->n_pcof), dim3(256), 0, c->stream, zt, c->G, c->goff, c->ncoef, c->poff, Y,
                       c->n_pcof, c->n_ops, c->m, c->nt, gnt);
    return (int)hipGetLastError();
}

// ws = W s for n_dir sensitivity directions side by side (general guard matrix)
int qgdk_hess_wapply(const qgdk_ctx *c, const double *shist, double *ws, int n_dir)
{
    hipLaunchKernelGGL(k_hess_wapply, dim3(n_dir * (c->cp / 8), c->nt), dim3(256), 0, c->stream, c->guard, shist, ws, c->Np, c->N, 2 * n_dir * c->cp);
    return (int)hipGetLastError();
}

size_t qgdk_hess_gram_part(int n_pcof, int nt)
{
    const int T = (n_pcof + 15) / 16;
    return (size_t)hs_gram_splits(n_pcof, nt) * (T * (T + 1) / 2) * 256;
}

int qgdk_hess_gram(const qgdk_ctx *c, const double *shist, double *ws, double *part, double *out)
{
    const int PWs = 2 * c->n_pcof * c->cp;
    if (c->have_guard == 1) {
        hipLaunchKernelGGL(k_hess_wapply, dim3(c->n_pcof * (c->cp / 8), c->nt), dim3(256), 0, c->stream, c->guard, shist, ws, c->Np, c->N, PWs);
        HIPCHK(hipGetLastError());
    }
    const int T = (c->n_pcof + 15) / 16, ntu = T * (T + 1) / 2, nsp = hs_gram_splits(c->n_pcof, c->nt);
    hipLaunchKernelGGL(k_hess_gram, dim3(ntu, nsp), dim3(256), 0, c->stream, shist, c->have_guard == 1 ? (const double *)ws : nullptr,
                       c->guard_diag, part, c->Np, c->N, c->c, c->cp, c->n_pcof, c->nt);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_hess_gram_sum, dim3(ntu), dim3(256), 0, c->stream, part, out, c->n_pcof, nsp, 2.0 * c->dt / c->tf);
    return (int)hipGetLastError();
}

} // extern "C"
