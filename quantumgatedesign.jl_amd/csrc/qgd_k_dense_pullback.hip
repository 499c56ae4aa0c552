// qgd_k_dense_pullback.hip -- the two kernels qgd_eval_dense_pullback adds to what the grid-point pullback runs (DESIGN.md
// section 4j): the transpose of the Hermite interpolation and the reverse sweep of the stage-derivative recursion seeded by
// cotangents of the stage derivatives.  (conventions: qgd_kernels_common.h)
//
// The dense output is, per step n and s = 1 .. r-1 (qgd_k_interp.hip),
//   d[n r + s] = sum_{j=0..m} a[s-1][j] w_j(n) + b[s-1][j] w_j(n+1),    d[n r] = w_0(n),
// with the stage derivatives w_j(n) = (1/j) sum_{i<j} A_{j-1-i}(t_n) w_i(n) of k_derivs.  k_pullback_forcing, pointed at the
// dense panels, leaves G[slot] = -dJ/dd[slot] (its sign: the adjoint sweep's forcing); everything below is linear in G and
// carries that sign through, which is the one qgdk_hvp_adjoint (forcing F = -dJ/dw_0) and qgdk_contract (grad -= G sigma) expect.
//
// k_interp_transpose<M>: gbar[n][j] = sum over the slots that read w_j(n): the interior slots of the step to the LEFT of n in
//   ascending s (weights b), then G[n r] into j = 0, then the interior slots of the step to the RIGHT in ascending s (weights a).
//   One workgroup per (time point, column group of 8) tile, grid-stride; a thread owns 16-byte pairs of the tile as in k_interp
//   and keeps its pair of the M+1 outputs in registers; every G panel is read once per end.  Padding rows and columns are
//   written as zeros on every call: no memset, no atomics, ordinary 16-byte vector stores.  Nothing depends on N <= 64.
//
// k_dense_pullback_sweep<NOPS>: per (time point, column group), in the manner of k_gradsweep (qgd_k_grad.hip) on the assembled
//   dense operator planes: w_0 .. w_{m-1} and g_0 .. g_m in LDS,
//     sweep   j = m..1, i = 0..j-1:  g_i += (1/j) A_{j-1-i}^H g_j     (A^H = -A; the state row i = 0 included)
//     sigma   sigP[k][d] += (1/j) <(dA/dp_k) w_i, g_j>,  sigQ likewise, d = j-1-i   (g_j after the sweep)
//     F[n]    = g_0 (zeros at n = 0 and in padding rows and columns): the forcing of the adjoint sweep, terminal panel included
//   The tables are those of the time point's own index n, as in k_derivs.  sigma: one plane [nt][n_ops][m][2] per column group,
//   the layout k_contract reads.  Per-wave sig slots, one writer each, added in wave order: no atomics, the same bits on every run.
#include "qgd_kernels_common.h"

typedef double d2 __attribute__((ext_vector_type(2)));

struct InterpTArgs {
    const double *G;            // [1 + (nt-1) r][Np][2cp]
    double *gbar;               // [nt][m+1][Np][2cp]
    const double *w;            // [r-1][m+1][2]: a (left end), b (right end) -- the table of k_interp
    int N, Np, c, cp, nt, r;
    int total;                  // (time point, column group) tiles
};

template <int M>
__global__ __launch_bounds__(256) void k_interp_transpose(InterpTArgs a)
{
    const int t = threadIdx.x;
    const int ngrp = a.cp >> 3, PWc = 2 * a.cp;
    const size_t hstep = (size_t)a.Np * PWc;
    const double *__restrict__ w = a.w;
    for (int tl = blockIdx.x; tl < a.total; tl += gridDim.x) {
        const int g = tl % ngrp, n = tl / ngrp;
        const double *Gn = a.G + (size_t)n * a.r * hstep;      // slot n r
        double *op = a.gbar + (size_t)n * (M + 1) * hstep;
        for (int idx = t; idx < 8 * a.Np; idx += 256) {
            const int row = idx >> 3, q = idx & 7, col = 8 * g + 2 * (q & 3);
            const size_t off = (size_t)row * PWc + 16 * g + 2 * q;
            d2 acc[M + 1];
            #pragma unroll
            for (int j = 0; j <= M; j++) acc[j] = (d2){0.0, 0.0};
            if (row < a.N && col < a.c) {      // (a padding row or column pair: zeros by selection, nothing is read)
                if (n > 0)
                    for (int s = 1; s < a.r; s++) {
                        const d2 x = *reinterpret_cast<const d2 *>(Gn - (size_t)(a.r - s) * hstep + off);
                        const double *ws = w + (size_t)(s - 1) * 2 * (M + 1);
                        #pragma unroll
                        for (int j = 0; j <= M; j++) { const double wb = ws[2 * j + 1]; acc[j].x = fma(wb, x.x, acc[j].x); acc[j].y = fma(wb, x.y, acc[j].y); }
                    }
                const d2 x0 = *reinterpret_cast<const d2 *>(Gn + off);
                acc[0].x += x0.x; acc[0].y += x0.y;
                if (n < a.nt - 1)
                    for (int s = 1; s < a.r; s++) {
                        const d2 x = *reinterpret_cast<const d2 *>(Gn + (size_t)s * hstep + off);
                        const double *ws = w + (size_t)(s - 1) * 2 * (M + 1);
                        #pragma unroll
                        for (int j = 0; j <= M; j++) { const double wa = ws[2 * j]; acc[j].x = fma(wa, x.x, acc[j].x); acc[j].y = fma(wa, x.y, acc[j].y); }
                    }
                if (col + 1 >= a.c) {
                    #pragma unroll
                    for (int j = 0; j <= M; j++) acc[j].y = 0.0;
                }
            }
            #pragma unroll
            for (int j = 0; j <= M; j++) *reinterpret_cast<d2 *>(op + (size_t)j * hstep + off) = acc[j];
        }
    }
}

#define SWEEP_MAX_M 8      // m = order/2 <= 8: one accumulator per target panel of a sweep pass
template <int NOPS>
__global__ __launch_bounds__(256) void k_dense_pullback_sweep(const double *__restrict__ ops,
                                                              const double *__restrict__ tab,
                                                              const double *__restrict__ hist,
                                                              const double *__restrict__ dpsi,
                                                              const double *__restrict__ gbar,
                                                              double *__restrict__ F,
                                                              double *__restrict__ sigma, int N, int Np, int c, int cp,
                                                              int n_ops, int m, int nt)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];     // w_0..w_{m-1} (m panels), g_0..g_m (m+1 panels), sig[waves][n_ops*m*2], cfl[m][CF_STRIDE]
    const int n = blockIdx.y, grp = blockIdx.x;
    const int PWc = 2 * cp;
    const size_t hstep = (size_t)Np * PWc;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int c16 = lane & 15, kk = lane >> 4;
    const size_t ps = (size_t)Np * 16;
    double *psi = smem, *gs = smem + (size_t)m * ps;      // gs[j * ps]: g_j
    double *sig = gs + (size_t)(m + 1) * ps;
    const int nsig = n_ops * m * 2;        // per-wave slots sig[wave][nsig]: one writer each, added in wave order below
    double *cfl = sig + (size_t)nw * nsig;                // [m][CF_STRIDE]: the coefficients of A_0 .. A_{m-1} at t_n (combine_opvals)
    const size_t pl = (size_t)Np * Np;
    const int nks = Np >> 2;      // k-steps of 4 (Np is a multiple of 16)

    for (int e = threadIdx.x; e < Np * 16; e += blockDim.x) {
        const size_t src = (size_t)(e >> 4) * PWc + grp * 16 + (e & 15);
        psi[e] = hist[(size_t)n * hstep + src];
        for (int i = 1; i < m; i++) psi[(size_t)i * ps + e] = dpsi[(((size_t)n * m + (i - 1)) * Np) * PWc + src];
        for (int j = 0; j <= m; j++) gs[(size_t)j * ps + e] = gbar[((size_t)n * (m + 1) + j) * hstep + src];
    }
    for (int e = threadIdx.x; e < nw * nsig; e += blockDim.x) sig[e] = 0.0;
    for (int e = threadIdx.x; e < m * CF_STRIDE; e += blockDim.x) {
        const int d = e / CF_STRIDE, q = e % CF_STRIDE, o = (q - 1) >> 1;      // q = 0: the system flag, 1 + 2o: p_o, 2 + 2o: q_o
        cfl[e] = q == 0 ? (d == 0 ? 1.0 : 0.0) : (o < n_ops ? tab[(((size_t)n * (m + 1) + d) * n_ops + o) * 2 + ((q - 1) & 1)] : 0.0);
    }
    __threadfence_block();
    __syncthreads();

    // reverse sweep, the state row included.  One pass over the operator elements per j: an element is loaded once and combined
    // with the coefficients of every order it is needed at, one accumulator per target panel i < j.
    for (int j = m; j >= 1; j--) {
        const double *src = gs + (size_t)j * ps;
        for (int rb = wave; rb * 16 < Np; rb += nw) {      // a wave owns its rows of every target panel
            const int arow = rb * 16 + c16;
            d4 t[SWEEP_MAX_M];
            #pragma unroll
            for (int i = 0; i < SWEEP_MAX_M; i++) t[i] = (d4){0, 0, 0, 0};
            // the operator elements of a k-step are loaded three k-steps ahead into a register ring (the branches on j below keep
            // the compiler from moving loads across k-steps itself); nks is a multiple of 4, the ring wraps around at its end
            OpVals ring[4];
            #pragma unroll
            for (int q = 0; q < 3; q++) load_opvals<NOPS>(ring[q], ops, Np, n_ops, (size_t)arow + (size_t)Np * (4 * q + kk));
            for (int ks4 = 0; ks4 < nks; ks4 += 4) {
                #pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int ks = ks4 + q, kn = ks + 3 < nks ? ks + 3 : ks + 3 - nks;
                    load_opvals<NOPS>(ring[(q + 3) & 3], ops, Np, n_ops, (size_t)arow + (size_t)Np * (4 * kn + kk));
                    double b1, b2;
                    panel_b(src + (size_t)(4 * ks + kk) * 16, c16, b1, b2);
                    #pragma unroll
                    for (int i = 0; i < SWEEP_MAX_M; i++)
                        if (i < j) {
                            double are, aim;
                            combine_opvals<NOPS>(ring[q], cfl + (size_t)(j - 1 - i) * CF_STRIDE, n_ops, are, aim);
                            t[i] = MFMA(are, b1, t[i]);
                            t[i] = MFMA(aim, b2, t[i]);
                        }
                }
            }
            const double sc = -1.0 / (double)j;     // A^H = -A
            #pragma unroll
            for (int i = 0; i < SWEEP_MAX_M; i++)
                if (i < j) {
                    #pragma unroll
                    for (int r = 0; r < 4; r++) gs[(size_t)i * ps + (size_t)(rb * 16 + kk + 4 * r) * 16 + c16] += sc * t[i][r];
                }
        }
        __threadfence_block();
        __syncthreads();
    }

    // F[n] = g_0: whole panel tile, zeros at n = 0 and in padding rows and columns (16-byte stores, a row of the group is 128 bytes)
    for (int idx = threadIdx.x; idx < 8 * Np; idx += blockDim.x) {
        const int row = idx >> 3, q = idx & 7, col = 8 * grp + 2 * (q & 3);
        d2 x = (d2){0.0, 0.0};
        if (n > 0 && row < N && col < c) {
            x = *reinterpret_cast<const d2 *>(gs + (size_t)row * 16 + 2 * q);
            if (col + 1 >= c) x.y = 0.0;
        }
        *reinterpret_cast<d2 *>(F + (size_t)n * hstep + (size_t)row * PWc + 16 * grp + 2 * q) = x;
    }

    // inner products: per operator and row block the operator elements are loaded once for four panels w_i at a time
    for (int o = 0; o < n_ops; o++) {
        const double *Asym = ops + (size_t)(2 + 2 * o) * pl, *Sym = ops + (size_t)(3 + 2 * o) * pl;
        for (int rb = wave; rb * 16 < Np; rb += nw) {
            const int arow = rb * 16 + c16;
            double sp[SWEEP_MAX_M], sq[SWEEP_MAX_M];
            #pragma unroll
            for (int d = 0; d < SWEEP_MAX_M; d++) { sp[d] = 0.0; sq[d] = 0.0; }
            for (int i0 = 0; i0 < m; i0 += 4) {
                d4 U[4], V[4];
                #pragma unroll
                for (int ii = 0; ii < 4; ii++) { U[ii] = (d4){0, 0, 0, 0}; V[ii] = (d4){0, 0, 0, 0}; }
                double rs[4], ra[4];      // (the same ring for the two operator planes)
                #pragma unroll
                for (int q = 0; q < 3; q++) { const size_t e = (size_t)arow + (size_t)Np * (4 * q + kk); rs[q] = Sym[e]; ra[q] = Asym[e]; }
                for (int ks4 = 0; ks4 < nks; ks4 += 4) {
                    #pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int ks = ks4 + q, kn = ks + 3 < nks ? ks + 3 : ks + 3 - nks;
                        { const size_t e = (size_t)arow + (size_t)Np * (4 * kn + kk); rs[(q + 3) & 3] = Sym[e]; ra[(q + 3) & 3] = Asym[e]; }
                        #pragma unroll
                        for (int ii = 0; ii < 4; ii++)
                            if (i0 + ii < m) {
                                const double b1 = psi[(size_t)(i0 + ii) * ps + (size_t)(4 * ks + kk) * 16 + c16];
                                U[ii] = MFMA(rs[q], b1, U[ii]);
                                V[ii] = MFMA(ra[q], b1, V[ii]);
                            }
                    }
                }
                // this lane's share of every <(dA/dp) w_i, g_j>/j, kept by d = j-1-i; the lanes are added once per (o, rb) below
                #pragma unroll
                for (int ii = 0; ii < 4; ii++) {
                    const int i = i0 + ii;
                    #pragma unroll
                    for (int d = 0; d < SWEEP_MAX_M; d++) {
                        const int j = i + 1 + d;
                        if (j > m) continue;
                        const double *gj = gs + (size_t)j * ps;
                        double ap = 0.0, aq = 0.0;
                        #pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int row = rb * 16 + kk + 4 * r;
                            double g1, g2;
                            panel_b(gj + (size_t)row * 16, c16, g1, g2);
                            aq += V[ii][r] * g1;              // Re<V, g>
                            ap += U[ii][r] * g2;              // Re<-iU, g> = Uim*gre - Ure*gim
                        }
                        sp[d] += ap / (double)j;
                        sq[d] += aq / (double)j;
                    }
                }
            }
            #pragma unroll
            for (int d = 0; d < SWEEP_MAX_M; d++) {
                if (d >= m) continue;
                double vp = sp[d], vq = sq[d];
                for (int off = 32; off > 0; off >>= 1) { vp += __shfl_down(vp, off); vq += __shfl_down(vq, off); }
                if (lane == 0) {      // (the wave's own slot, in program order)
                    sig[wave * nsig + (o * m + d) * 2] += vp;
                    sig[wave * nsig + (o * m + d) * 2 + 1] += vq;
                }
            }
        }
    }
    __syncthreads();
    // the workgroup's own plane of sigma (plane = column group): stored, k_contract adds the planes in order
    for (int e = threadIdx.x; e < nsig; e += blockDim.x) {
        double v = 0.0;
        for (int q = 0; q < nw; q++) v += sig[q * nsig + e];
        sigma[((size_t)grp * nt + n) * nsig + e] = v;
    }
}

// dynamic LDS of k_dense_pullback_sweep (256 threads: four waves)
static size_t dense_pullback_lds(int Np, int m, int n_ops)
{
    return ((size_t)(2 * m + 1) * Np * 16 + (size_t)4 * n_ops * m * 2 + (size_t)m * CF_STRIDE) * sizeof(double);
}

extern "C" {

// G [1 + (nt-1) refine] panels -> gbar [nt][m+1] panels; w_dev: the weight table of qgdk_interp
int qgdk_interp_transpose(const qgdk_ctx *c, const double *G, double *gbar, int refine, const double *w_dev)
{
    if (c->nt < 2 || refine < 1 || c->m < 1 || c->m > 8) return (int)hipErrorInvalidValue;
    const long long total = (long long)c->nt * (c->cp / 8);
    if (total > 0x7fffffffLL || (long long)(c->nt - 1) * refine + 1 > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    InterpTArgs a;
    a.G = G; a.gbar = gbar; a.w = w_dev;
    a.N = c->N; a.Np = c->Np; a.c = c->c; a.cp = c->cp; a.nt = c->nt; a.r = refine; a.total = (int)total;
    const int grid = a.total < 2048 ? a.total : 2048;
#define LAUNCH_IT(M) hipLaunchKernelGGL(k_interp_transpose<M>, dim3(grid), dim3(256), 0, c->stream, a)
    switch (c->m) {
    case 1: LAUNCH_IT(1); break; case 2: LAUNCH_IT(2); break; case 3: LAUNCH_IT(3); break; case 4: LAUNCH_IT(4); break;
    case 5: LAUNCH_IT(5); break; case 6: LAUNCH_IT(6); break; case 7: LAUNCH_IT(7); break; default: LAUNCH_IT(8); break;
    }
#undef LAUNCH_IT
    return (int)hipGetLastError();
}

// gbar [nt][m+1] panels and the stage derivatives of c (hist, dpsi) -> F [nt] panels and sigma [cp/8][nt][n_ops][m][2]
int qgdk_dense_pullback_sweep(const qgdk_ctx *c, const double *gbar, double *F, double *sigma)
{
    if (c->m < 1 || c->m > SWEEP_MAX_M || c->n_ops < 1 || c->n_ops > QGD_MAX_OPS_DEV || c->nt > 65535) return (int)hipErrorInvalidValue;
    const size_t shm = dense_pullback_lds(c->Np, c->m, c->n_ops);
    if (shm > 160 * 1024) return (int)hipErrorInvalidValue;      // LDS of a gfx950 CU, all of which one workgroup may take
#define CALL_DPS(NO) do { if (shm > 64 * 1024) SET_LDS_ONCE(k_dense_pullback_sweep<NO>, shm); \
        hipLaunchKernelGGL((k_dense_pullback_sweep<NO>), dim3(c->cp / 8, c->nt), dim3(256), shm, c->stream, c->ops, c->tab, c->hist, \
                           c->dpsi, gbar, F, sigma, c->N, c->Np, c->c, c->cp, c->n_ops, c->m, c->nt); } while (0)
    DISPATCH_NOPS(c->n_ops, CALL_DPS)
#undef CALL_DPS
    return (int)hipGetLastError();
}

} // extern "C"
