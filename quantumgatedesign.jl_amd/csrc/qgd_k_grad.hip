// qgd_k_grad.hip -- state derivatives, gradient scalars, contraction, Hamiltonian apply
// (conventions and layouts: qgd_kernels_common.h; algorithm: DESIGN.md)
#include "qgd_kernels_common.h"

// ---------------------------------------------------------------------------
// K9: state derivatives at every time point (the stored history of
// forward_evolution.jl:172-179,:236-242):  psi_{j+1} = 1/(j+1) sum_{i<=j} A_{j-i} psi_i
// One workgroup per (time point, column group).  dpsi: [nt][m][Np][2cp].
// ---------------------------------------------------------------------------
template <int NOPS>
__global__ __launch_bounds__(256) void k_derivs(const double *__restrict__ ops,
                                                const double *__restrict__ tab,
                                                const double *__restrict__ hist,
                                                double *__restrict__ dpsi, int Np, int cp,
                                                int n_ops, int m, double *__restrict__ gpanels)
{
    extern __shared__ double lds_panels[];              // (m+1) panels [Np][16] ...
    const int n = blockIdx.y, grp = blockIdx.x;
    // ... or, when they do not fit in LDS (large N), a slab of global scratch per workgroup
    double *smem = gpanels ? gpanels + ((size_t)n * gridDim.x + grp) * (size_t)(m + 1) * Np * 16 : lds_panels;
    const int PWc = 2 * cp;
    const size_t hstep = (size_t)Np * PWc;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int c16 = lane & 15, kk = lane >> 4;
    const size_t ps = (size_t)Np * 16;
    for (int e = threadIdx.x; e < Np * 16; e += blockDim.x)
        smem[e] = hist[(size_t)n * hstep + (size_t)(e >> 4) * PWc + grp * 16 + (e & 15)];
    __threadfence_block();
    __syncthreads();
    for (int j = 0; j < m; j++) {
        for (int rb = wave; rb * 16 < Np; rb += nw) {
            d4 acc = (d4){0, 0, 0, 0};
            const int arow = rb * 16 + c16;
            for (int i = 0; i <= j; i++) {
                OpCoef cf;
                load_coef(cf, tab, n, j - i, m, n_ops);
                const double *src = smem + (size_t)i * ps;
                for (int k0 = 0; k0 < Np; k0 += 4) {
                    double are, aim, b1, b2;
                    assembled_a<NOPS>(ops, Np, n_ops, cf, arow, k0 + kk, are, aim);
                    panel_b(src + (size_t)(k0 + kk) * 16, c16, b1, b2);
                    acc = MFMA(are, b1, acc);
                    acc = MFMA(aim, b2, acc);
                }
            }
            const double inv = 1.0 / (double)(j + 1);
            #pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = rb * 16 + kk + 4 * r;
                const double v = acc[r] * inv;
                smem[(size_t)(j + 1) * ps + (size_t)row * 16 + c16] = v;
                dpsi[(((size_t)n * m + j) * Np + row) * PWc + grp * 16 + c16] = v;
            }
        }
        __threadfence_block();
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// K10: gradient scalars.  Per (time point, column group):
//   seeds   g_j = c_j dt^j lambda_{n+1} [n<=nt-2]  -  c_j (-dt)^j lambda_n [n>=1]
//   sweep   j = m..2, i = 1..j-1:  g_i += (1/j) A_{j-1-i}^H g_j     (A^H = -A)
//   sigma   sigP[k][d] += (1/j) <(dA/dp_k) psi_i, g_j>,  sigQ likewise, d = j-1-i
// This is the O(m^2) reverse form of accumulate_gradient_arbitrary_fast! /
// recursive_magic! (eval_grad_discrete_adjoint.jl:582-726); inner products as
// compute_inner_prod_S!/K! (:764-800).  sigma: one plane [nt][n_ops][m][2] per column
// group, added in order by k_contract.
// ---------------------------------------------------------------------------
template <int NOPS>
__global__ __launch_bounds__(256) void k_gradsweep(const double *__restrict__ ops,
                                                   const double *__restrict__ tab,
                                                   const double *__restrict__ hist,
                                                   const double *__restrict__ dpsi,
                                                   const double *__restrict__ lam,
                                                   double *__restrict__ sigma,
                                                   const double *__restrict__ cw, int Np, int cp,
                                                   int n_ops, int m, int nt, double *__restrict__ gpanels)
{
    extern __shared__ double smem[];     // psi_0..psi_{m-1} (m panels), g_1..g_m (m panels), sig[n_ops*m*2]
    const int n = blockIdx.y, grp = blockIdx.x;
    const int PWc = 2 * cp;
    const size_t hstep = (size_t)Np * PWc;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int c16 = lane & 15, kk = lane >> 4;
    const size_t ps = (size_t)Np * 16;
    // panels in LDS, or (large N) in a slab of global scratch per workgroup; sig always in LDS
    double *pbase = gpanels ? gpanels + ((size_t)n * gridDim.x + grp) * (size_t)(2 * m) * Np * 16 : smem;
    double *psi = pbase, *gs = pbase + (size_t)m * ps;   // gs[(j-1)*ps]
    double *sig = gpanels ? smem : gs + (size_t)m * ps;
    const size_t pl = (size_t)Np * Np;

    for (int e = threadIdx.x; e < Np * 16; e += blockDim.x) {
        const size_t src = (size_t)(e >> 4) * PWc + grp * 16 + (e & 15);
        psi[e] = hist[(size_t)n * hstep + src];
        for (int i = 1; i < m; i++) psi[(size_t)i * ps + e] = dpsi[(((size_t)n * m + (i - 1)) * Np) * PWc + src];
        const double ln = (n >= 1) ? lam[(size_t)n * hstep + src] : 0.0;
        const double lx = (n <= nt - 2) ? lam[(size_t)(n + 1) * hstep + src] : 0.0;
        for (int j = 1; j <= m; j++) gs[(size_t)(j - 1) * ps + e] = cw[2 * j] * lx - cw[2 * j + 1] * ln;
    }
    const int nsig = n_ops * m * 2;        // per-wave slots sig[wave][nsig]: one writer each, added in wave order below (no atomics across waves)
    for (int e = threadIdx.x; e < nw * nsig; e += blockDim.x) sig[e] = 0.0;
    __threadfence_block();
    __syncthreads();

    // reverse sweep
    for (int j = m; j >= 2; j--) {
        const double *src = gs + (size_t)(j - 1) * ps;
        for (int rb = wave; rb * 16 < Np; rb += nw) {
            const int arow = rb * 16 + c16;
            for (int i = 1; i <= j - 1; i++) {
                OpCoef cf;
                load_coef(cf, tab, n, j - 1 - i, m, n_ops);
                d4 acc = (d4){0, 0, 0, 0};
                for (int k0 = 0; k0 < Np; k0 += 4) {
                    double are, aim, b1, b2;
                    assembled_a<NOPS>(ops, Np, n_ops, cf, arow, k0 + kk, are, aim);
                    panel_b(src + (size_t)(k0 + kk) * 16, c16, b1, b2);
                    acc = MFMA(are, b1, acc);
                    acc = MFMA(aim, b2, acc);
                }
                const double sc = -1.0 / (double)j;     // A^H = -A
                #pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = rb * 16 + kk + 4 * r;
                    gs[(size_t)(i - 1) * ps + (size_t)row * 16 + c16] += sc * acc[r];
                }
            }
        }
        __threadfence_block();
        __syncthreads();
    }

    // inner products
    for (int o = 0; o < n_ops; o++) {
        const double *Asym = ops + (size_t)(2 + 2 * o) * pl, *Sym = ops + (size_t)(3 + 2 * o) * pl;
        for (int i = 0; i < m; i++) {
            const double *src = psi + (size_t)i * ps;
            for (int rb = wave; rb * 16 < Np; rb += nw) {
                const int arow = rb * 16 + c16;
                d4 U = (d4){0, 0, 0, 0}, V = (d4){0, 0, 0, 0};
                for (int k0 = 0; k0 < Np; k0 += 4) {
                    const size_t e = (size_t)arow + (size_t)Np * (k0 + kk);
                    const double b1 = src[(size_t)(k0 + kk) * 16 + c16];
                    U = MFMA(Sym[e], b1, U);
                    V = MFMA(Asym[e], b1, V);
                }
                for (int j = i + 1; j <= m; j++) {
                    const double *gj = gs + (size_t)(j - 1) * ps;
                    double sp = 0.0, sq = 0.0;
                    #pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int row = rb * 16 + kk + 4 * r;
                        double g1, g2;
                        panel_b(gj + (size_t)row * 16, c16, g1, g2);
                        sq += V[r] * g1;              // Re<V, g>
                        sp += U[r] * g2;              // Re<-iU, g> = Uim*gre - Ure*gim
                    }
                    for (int off = 32; off > 0; off >>= 1) { sp += __shfl_down(sp, off); sq += __shfl_down(sq, off); }
                    if (lane == 0) {
                        const int d = j - 1 - i;
                        atomicAdd(&sig[wave * nsig + (o * m + d) * 2], sp / (double)j);          // (own slot: LDS executes a wave's adds in order)
                        atomicAdd(&sig[wave * nsig + (o * m + d) * 2 + 1], sq / (double)j);
                    }
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

// ---------------------------------------------------------------------------
// K9+K10 fused (fast path, Np = 64): everything the gradient needs at one time point, one
// launch, no derivative history in HBM.  Workgroup = (time point, group of 8 columns), 4 waves =
// 4 row blocks.  psi_0..psi_{m-1} live in LDS; g_1..g_m live in REGISTERS in accumulator layout
// (each wave owns its 16 rows) and only the g_j currently acting as right operand is staged in
// LDS.  All passes share one register ring of operator elements that wraps around across passes
// (the (row,k) elements are the same in every pass), so the ring never drains.
//   D passes  psi_{j+1} = 1/(j+1) sum_{i<=j} A_{j-i} psi_i          j = 0..m-2
//   G passes  g_i += (1/j) A_{j-1-i}^H g_j (A^H = -A), i = 1..j-1   j = m..2
//   S passes  per operator o: U_i = Sym_o psi_i, V_i = Asym_o psi_i, then the inner products
// ---------------------------------------------------------------------------
template <int M, int NOPS>
__global__ __launch_bounds__(256) void k_gradpoint64(const double *__restrict__ ops,
                                                     const double *__restrict__ tab,
                                                     const double *__restrict__ hist,
                                                     const double *__restrict__ lam,
                                                     double *__restrict__ sigma,
                                                     const double *__restrict__ cw, int cp, int nt,
                                                     int n_ops)
{
    constexpr int NP = 64, NKS = NP / 4, PS = NP * 16, RD = 4;
    extern __shared__ double smem[];
    double *psi = smem;                         // [M][PS]
    double *gsrc = smem + (size_t)M * PS;       // [PS]
    double *sig = gsrc + PS;                    // [n_ops*M*2][4 waves]
    const int n = blockIdx.y, grp = blockIdx.x;
    const int PWc = 2 * cp;
    const size_t hstep = (size_t)NP * PWc, pl = (size_t)NP * NP;
    const int tid = threadIdx.x, rb = tid >> 6, lane = tid & 63;
    const int c16 = lane & 15, kk = lane >> 4;
    const int arow = rb * 16 + c16;

    for (int e = tid; e < PS; e += 256)
        psi[e] = hist[(size_t)n * hstep + (size_t)(e >> 4) * PWc + grp * 16 + (e & 15)];
    // seeds in accumulator layout
    d4 g[M];
    {
        double ln[4], lx[4];
        #pragma unroll
        for (int r = 0; r < 4; r++) {
            const size_t o = (size_t)(rb * 16 + kk + 4 * r) * PWc + grp * 16 + c16;
            ln[r] = (n >= 1) ? lam[(size_t)n * hstep + o] : 0.0;
            lx[r] = (n <= nt - 2) ? lam[(size_t)(n + 1) * hstep + o] : 0.0;
        }
        #pragma unroll
        for (int j = 1; j <= M; j++)
            #pragma unroll
            for (int r = 0; r < 4; r++) g[j - 1][r] = cw[2 * j] * lx[r] - cw[2 * j + 1] * ln[r];
    }
    // coefficients of derivative orders 0..M-2 (uniform -> scalar registers)
    constexpr int ND = (M > 1) ? M - 1 : 1;
    double cfr[ND][CF_STRIDE];
    #pragma unroll
    for (int d = 0; d < ND; d++) {
        cfr[d][0] = (d == 0) ? 1.0 : 0.0;
        #pragma unroll
        for (int o = 0; o < NOPS_LIM(NOPS); o++) {
            const bool on = NOPS_ON(NOPS, o, n_ops);
            cfr[d][1 + 2 * o] = on ? tab[(((size_t)n * (M + 1) + d) * n_ops + o) * 2] : 0.0;
            cfr[d][2 + 2 * o] = on ? tab[(((size_t)n * (M + 1) + d) * n_ops + o) * 2 + 1] : 0.0;
        }
    }
    // operator ring, wraps around over k-steps and passes
    OpVals ring[RD];
    auto ring_load = [&](int slot, int ks) {
        load_opvals<NOPS>(ring[slot], ops, NP, n_ops, (size_t)arow + (size_t)NP * ((ks & (NKS - 1)) * 4 + kk));
    };
    if (M > 1) {
        #pragma unroll
        for (int q = 0; q < RD - 1; q++) ring_load(q, q);
    }
    __syncthreads();

    // ---- D passes
    #pragma unroll
    for (int j = 0; j + 1 < M; j++) {
        d4 acc = (d4){0, 0, 0, 0};
        for (int ks4 = 0; ks4 < NKS; ks4 += RD) {
            #pragma unroll
            for (int q = 0; q < RD; q++) {
                const int ks = ks4 + q, k = ks * 4 + kk;
                ring_load((q + RD - 1) % RD, ks + RD - 1);
                #pragma unroll
                for (int i = 0; i <= j; i++) {
                    double are, aim, b1, b2;
                    combine_opvals<NOPS>(ring[q], cfr[j - i], n_ops, are, aim);
                    panel_b(psi + (size_t)i * PS + (size_t)k * 16, c16, b1, b2);
                    acc = MFMA(are, b1, acc);
                    acc = MFMA(aim, b2, acc);
                }
            }
        }
        const double inv = 1.0 / (double)(j + 1);
        #pragma unroll
        for (int r = 0; r < 4; r++) psi[(size_t)(j + 1) * PS + (size_t)(rb * 16 + kk + 4 * r) * 16 + c16] = acc[r] * inv;
        __syncthreads();
    }

    // ---- G passes
    #pragma unroll
    for (int j = M; j >= 2; j--) {
        #pragma unroll
        for (int r = 0; r < 4; r++) gsrc[(size_t)(rb * 16 + kk + 4 * r) * 16 + c16] = g[j - 1][r];
        __syncthreads();
        d4 t[M];
        #pragma unroll
        for (int i = 0; i < M; i++) t[i] = (d4){0, 0, 0, 0};
        for (int ks4 = 0; ks4 < NKS; ks4 += RD) {
            #pragma unroll
            for (int q = 0; q < RD; q++) {
                const int ks = ks4 + q, k = ks * 4 + kk;
                ring_load((q + RD - 1) % RD, ks + RD - 1);
                double b1, b2;
                panel_b(gsrc + (size_t)k * 16, c16, b1, b2);
                #pragma unroll
                for (int i = 1; i <= j - 1; i++) {
                    double are, aim;
                    combine_opvals<NOPS>(ring[q], cfr[j - 1 - i], n_ops, are, aim);
                    t[i] = MFMA(are, b1, t[i]);
                    t[i] = MFMA(aim, b2, t[i]);
                }
            }
        }
        const double sc = -1.0 / (double)j;              // A^H = -A
        #pragma unroll
        for (int i = 1; i <= j - 1; i++)
            #pragma unroll
            for (int r = 0; r < 4; r++) g[i - 1][r] += sc * t[i][r];
        __syncthreads();                                 // gsrc is rewritten by the next pass
    }

    // [-g_im | g_re] partner of every g_j, for the <(dA/dp) psi, g> products
    d4 gs[M];
    #pragma unroll
    for (int j = 0; j < M; j++)
        #pragma unroll
        for (int r = 0; r < 4; r++) {
            const double o = __shfl_xor(g[j][r], 8);
            gs[j][r] = (c16 < 8) ? -o : o;
        }

    // ---- S passes
    #pragma unroll
    for (int o = 0; o < NOPS_LIM(NOPS); o++) {
        if (!NOPS_ON(NOPS, o, n_ops)) continue;
        const double *Asym = ops + (size_t)(2 + 2 * o) * pl, *Sym = ops + (size_t)(3 + 2 * o) * pl;
        d4 U[M], V[M];
        #pragma unroll
        for (int i = 0; i < M; i++) { U[i] = (d4){0, 0, 0, 0}; V[i] = (d4){0, 0, 0, 0}; }
        double rs[RD], ra[RD];
        #pragma unroll
        for (int q = 0; q < RD - 1; q++) {
            const size_t e = (size_t)arow + (size_t)NP * (q * 4 + kk);
            rs[q] = Sym[e]; ra[q] = Asym[e];
        }
        for (int ks4 = 0; ks4 < NKS; ks4 += RD) {
            #pragma unroll
            for (int q = 0; q < RD; q++) {
                const int ks = ks4 + q, k = ks * 4 + kk;
                {
                    const size_t e = (size_t)arow + (size_t)NP * ((((ks + RD - 1) & (NKS - 1)) * 4) + kk);
                    rs[(q + RD - 1) % RD] = Sym[e]; ra[(q + RD - 1) % RD] = Asym[e];
                }
                #pragma unroll
                for (int i = 0; i < M; i++) {
                    const double b1 = psi[(size_t)i * PS + (size_t)k * 16 + c16];
                    U[i] = MFMA(rs[q], b1, U[i]);
                    V[i] = MFMA(ra[q], b1, V[i]);
                }
            }
        }
        double sp[M], sq[M];
        #pragma unroll
        for (int d = 0; d < M; d++) { sp[d] = 0.0; sq[d] = 0.0; }
        #pragma unroll
        for (int i = 0; i < M; i++)
            #pragma unroll
            for (int j = i + 1; j <= M; j++) {
                double ap = 0.0, aq = 0.0;
                #pragma unroll
                for (int r = 0; r < 4; r++) { ap += U[i][r] * gs[j - 1][r]; aq += V[i][r] * g[j - 1][r]; }
                sp[j - 1 - i] += ap / (double)j;
                sq[j - 1 - i] += aq / (double)j;
            }
        #pragma unroll
        for (int d = 0; d < M; d++) {
            #pragma unroll
            for (int off = 32; off > 0; off >>= 1) { sp[d] += __shfl_down(sp[d], off); sq[d] += __shfl_down(sq[d], off); }
            if (lane == 0) { sig[((o * M + d) * 2) * 4 + rb] = sp[d]; sig[((o * M + d) * 2 + 1) * 4 + rb] = sq[d]; }   // one slot per wave
        }
    }
    __syncthreads();
    for (int e = tid; e < n_ops * M * 2; e += 256)      // the four waves in order, into this column group's plane (no atomics)
        sigma[((size_t)grp * nt + n) * n_ops * M * 2 + e] = ((sig[e * 4] + sig[e * 4 + 1]) + sig[e * 4 + 2]) + sig[e * 4 + 3];
}

template <int M, int NOPS>
static int launch_gradpoint64(const qgdk_ctx *c)
{
    const size_t shm = ((size_t)(M + 1) * 64 * 16 + (size_t)c->n_ops * M * 2 * 4) * sizeof(double);
    SET_LDS_ONCE((k_gradpoint64<M, NOPS>), shm);
    hipLaunchKernelGGL((k_gradpoint64<M, NOPS>), dim3(c->cp / 8, c->nt), dim3(256), shm, c->stream, c->ops, c->tab,
                       c->hist, c->lam, c->sigma, c->cw, c->cp, c->nt, c->n_ops);
    return (int)hipGetLastError();
}

template <int M>
static int launch_gradpoint64_m(const qgdk_ctx *c)
{
#define CALL_GP(N) return launch_gradpoint64<M, N>(c)
    DISPATCH_NOPS(c->n_ops, CALL_GP)
#undef CALL_GP
    return 0;
}

// ---------------------------------------------------------------------------
// K11: gradient contraction  grad[off_k + l] = - sum_{n,d} Gp[k][n][d][l] sigP[n][k][d] + Gq.. sigQ..
// (the "grad_slice .-= contrib" of eval_grad_discrete_adjoint.jl:642-643)
// grid: (time chunks of 8 points, n_ops, coefficient tiles of 64); every chunk stores its row of cpart, k_contract_sum adds the rows.
// ---------------------------------------------------------------------------
#define CT_CHUNK 8
__global__ __launch_bounds__(256) void k_contract(const double *__restrict__ G, const int64_t *__restrict__ goff,
                                                  const int32_t *__restrict__ ncoef,
                                                  const int32_t *__restrict__ poff,
                                                  const double *__restrict__ sigma,
                                                  int nt, int m, int n_ops,
                                                  const int *__restrict__ status, double *__restrict__ scal,
                                                  int planes, double *__restrict__ cpart, int n_pcof, int g_nt, int g_n0)
{
    // grid (time chunks, n_ops, coefficient tiles of 64); thread = (coefficient, time sub-slot).
    // No atomics: every time chunk STORES its partial sums, and k_contract_sum adds the chunks in chunk order -- the
    // gradient is bitwise reproducible from run to run (the reference accumulates serially,
    // eval_grad_discrete_adjoint.jl:603-643).  (One kernel with a "last workgroup adds" ticket was measured: the
    // device-scope release/acquire around the ticket cost 10 us against 4 us for this second launch.)
    __shared__ double red[4][64];
    // the singularity flag also travels as a double in the spare scalar slot, INSIDE the range the ranks all-reduce:
    // every rank of a time-partitioned evaluation then fails together (qgd_dist_finish)
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0 && *status) scal[3] = 1.0;
    const int k = blockIdx.y;
    const int nc = ncoef[k];
    const int l = blockIdx.z * 64 + (threadIdx.x & 63), sub = threadIdx.x >> 6;
    const double *gp = G + goff[k];
    const double *gq = gp + (size_t)g_nt * (m + 1) * nc;      // (the basis holds g_nt time points; this window starts at g_n0)
    const size_t plane = (size_t)nt * n_ops * m * 2;
    double s = 0.0;
    if (l < nc) {
        const int n1 = min(nt, (int)(blockIdx.x + 1) * CT_CHUNK);
        for (int n = blockIdx.x * CT_CHUNK + sub; n < n1; n += 4)
            for (int d = 0; d < m; d++) {
                const size_t e = (((size_t)n * n_ops + k) * m + d) * 2;
                double sp = sigma[e], sq = sigma[e + 1];
                for (int g = 1; g < planes; g++) { sp += sigma[g * plane + e]; sq += sigma[g * plane + e + 1]; }   // column groups, in order
                s += gp[((size_t)(n + g_n0) * (m + 1) + d) * nc + l] * sp + gq[((size_t)(n + g_n0) * (m + 1) + d) * nc + l] * sq;
            }
    }
    red[sub][threadIdx.x & 63] = s;
    __syncthreads();
    if (sub == 0 && l < nc)
        cpart[(size_t)blockIdx.x * n_pcof + poff[k] + l] = -(((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x]);
}

// grad[p] (=, or += for a later window of a chunked time grid) the time chunks of k_contract in chunk order:
// thread = (coefficient, quarter of the chunks), the four quarters added in order
// grad[p] (=, or += for a later window of a chunked time grid) the rows of cpart in a FIXED order: workgroup = 16
// coefficients x 64 row slots; a slot adds its rows (slot, slot + 64, ...) in order with the loads issued four at a time
// (a rolled loop waited one memory round trip per row: 11 us for the 551 rows of the benchmark grid), then a fixed binary
// tree over the 64 slots.  Same shape on every run => same bits.
struct ResultMirror { double *host; unsigned long long seq; unsigned int *ticket; const double *scal; const int *status; };
// BATCH (qgd_eval_batch, grid (coefficient tiles, members)): member b = blockIdx.y adds ITS rows, cpart + b * cpart_stride, into
// row b of out[members][n_pcof + 5] = (grad | the member's three scalars | singular flag | status word) and clears the member's
// status word for the next batch (it is the last kernel to read it).  The sums are those of the single launch: same bits.
struct ContractBatch { long long cpart_stride; double *out; const double *scal; int *status; int scal_stride, status_stride; };

template <bool BATCH>
__global__ __launch_bounds__(1024) void k_contract_sum(const double *__restrict__ cpart, double *__restrict__ grad, int n_pcof, int rows,
                                                       int accumulate, const int *__restrict__ status, double *__restrict__ scal,
                                                       const ResultMirror mir, const ContractBatch bt)
{
    __shared__ double red[64][17];
    if (BATCH) {
        cpart += (size_t)blockIdx.y * bt.cpart_stride;
        grad = bt.out + (size_t)blockIdx.y * (n_pcof + 5);
    }
    // the singularity flag also travels as a double in the spare scalar slot, INSIDE the range the ranks all-reduce
    if (!BATCH && status && blockIdx.x == 0 && threadIdx.x == 0 && *status) scal[3] = 1.0;
    const int pl = threadIdx.x & 15, slot = threadIdx.x >> 4, p = blockIdx.x * 16 + pl;
    double tot = 0.0;
    if (p < n_pcof) {
        int c = slot;
        for (; c + 192 < rows; c += 256) {
            const double v0 = cpart[(size_t)c * n_pcof + p], v1 = cpart[(size_t)(c + 64) * n_pcof + p];
            const double v2 = cpart[(size_t)(c + 128) * n_pcof + p], v3 = cpart[(size_t)(c + 192) * n_pcof + p];
            tot = (((tot + v0) + v1) + v2) + v3;
        }
        for (; c < rows; c += 64) tot += cpart[(size_t)c * n_pcof + p];
    }
    red[slot][pl] = tot;
    __syncthreads();
    #pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        if (slot < w) red[slot][pl] += red[slot + w][pl];
        __syncthreads();
    }
    if (slot == 0 && p < n_pcof) {
        const double v = accumulate ? grad[p] + red[0][pl] : red[0][pl];
        grad[p] = v;
        if (mir.host) { mir.host[p] = v; __threadfence_system(); }      // (this thread's own posted write, ordered before the ticket below)
    }
    if (BATCH) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const double *sc = bt.scal + (size_t)blockIdx.y * bt.scal_stride;
            int *st = bt.status + (size_t)blockIdx.y * bt.status_stride;
            const int flag = *st;
            grad[n_pcof] = sc[0]; grad[n_pcof + 1] = sc[1]; grad[n_pcof + 2] = sc[2];
            grad[n_pcof + 3] = flag ? 1.0 : 0.0; grad[n_pcof + 4] = (double)flag;
            *st = 0;
        }
        return;
    }
    // Result mirror: the workgroup that draws the last ticket adds the scalars and the status word and then publishes the
    // sequence number the host polls (system-scope release: every workgroup's values are in host memory before it).
    if (mir.host) {
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence();
            const unsigned int t = atomicAdd(mir.ticket, 1u);
            if (t == gridDim.x - 1) {
                __threadfence();
                #pragma unroll
                for (int q = 0; q < 4; q++) mir.host[n_pcof + q] = __hip_atomic_load(mir.scal + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                mir.host[n_pcof + 4] = (double)__hip_atomic_load(mir.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                *mir.ticket = 0u;
                __threadfence_system();
                __hip_atomic_store(reinterpret_cast<unsigned long long *>(mir.host + n_pcof + 5), mir.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// The weighted sums of an ensemble (qgd_eval_ensemble) over the result rows of one chunk,
// rows[members][n_pcof + 5] as the batched k_contract_sum leaves them: ONE workgroup, lane e < n_pcof owns gradient entry e,
// lanes n_pcof and n_pcof + 1 own cost and guard (a forward-only call runs those two alone).  The statement is ensemble_reduce
// of ensemble.py, operation for operation, every operation rounded on its own:
//   cost_k = 1.0 - (a_k a_k + b_k b_k) / double(n_ess n_ess) for :Infidelity, a_k for every other cost type; guard_k = row[n_pcof + 2]
//   acc = acc + w_k x_k, k ascending, from the double 0.0 (first chunk of a call) or from acc[] (the chunks before this one)
// The compiler's default contraction would fuse the product into the sum (the _rn intrinsics do not keep it from that
// here): it is switched off for these two bodies, and the division is the IEEE one.  The loads of four members are issued
// ahead of the add chain, which stays in order.  No atomics, nothing waits for another workgroup.  Behind the sums the
// workgroup packs the rows' tails (three scalars, singular flag, status word) into tails[members][5]: what a call that wants no
// member gradients downloads.
struct EnsembleReduce { const double *rows, *w; double *acc, *tails; int members, n_pcof, first, gradient, infidelity, n_ess; };
__device__ __forceinline__ double ensemble_entry(const double *__restrict__ row, const int e, const int n_pcof, const int infidelity, const double d)
{
    #pragma clang fp contract(off)
    if (e < n_pcof) return row[e];
    if (e > n_pcof) return row[n_pcof + 2];
    const double a = row[n_pcof], b = row[n_pcof + 1];
    return infidelity ? 1.0 - (a * a + b * b) / d : a;
}
__global__ __launch_bounds__(128) void k_ensemble_reduce(const EnsembleReduce r)
{
    #pragma clang fp contract(off)
    const int e = threadIdx.x, np = r.n_pcof, ld = np + 5, K = r.members;
    if ((e < np && r.gradient) || e == np || e == np + 1) {
        const double d = (double)(r.n_ess * r.n_ess);
        double acc = r.first ? 0.0 : r.acc[e];
        int k = 0;
        for (; k + 4 <= K; k += 4) {
            const double x0 = ensemble_entry(r.rows + (size_t)k * ld, e, np, r.infidelity, d), w0 = r.w[k];
            const double x1 = ensemble_entry(r.rows + (size_t)(k + 1) * ld, e, np, r.infidelity, d), w1 = r.w[k + 1];
            const double x2 = ensemble_entry(r.rows + (size_t)(k + 2) * ld, e, np, r.infidelity, d), w2 = r.w[k + 2];
            const double x3 = ensemble_entry(r.rows + (size_t)(k + 3) * ld, e, np, r.infidelity, d), w3 = r.w[k + 3];
            acc = acc + w0 * x0;
            acc = acc + w1 * x1;
            acc = acc + w2 * x2;
            acc = acc + w3 * x3;
        }
        for (; k < K; k++) acc = acc + r.w[k] * ensemble_entry(r.rows + (size_t)k * ld, e, np, r.infidelity, d);
        r.acc[e] = acc;
    }
    for (int t = threadIdx.x; t < 5 * K; t += blockDim.x) r.tails[t] = r.rows[(size_t)(t / 5) * ld + np + t % 5];
}

// ---------------------------------------------------------------------------
// Derivative columns of lambda_history (optional output, qgd_set_lambda_derivatives).  The reference's eval_adjoint!
// stores, beside lambda_n, the m "adjoint derivatives" it built the explicit side of step n from
// (forward_evolution.jl:427-433; compute_adjoint_derivatives!, hermite.jl:284-305, a tree recursion of
// 2^j - 1 Hamiltonian applications per order).  They are w_j = D_j(t)^T lambda_n with the D_j of K9, so the
// reverse sweep of that recursion gives them in j(j+1)/2 applications:
//   g_j = lambda_n;  k = j..1, i = 0..k-1:  g_i -= (1/k) A_{k-1-i}(t) g_k   (A^T = -A);   w_j = g_0
// The reference evaluates the controls at t_{n-1} for time index n >= 2 and at t_1 for n = 1 (:423, :472); index 0
// is never written.  One workgroup per (time point, column group); dlam: [nt][m][Np][2cp].
// ---------------------------------------------------------------------------
template <int NOPS>
__global__ __launch_bounds__(256) void k_adjoint_derivs(const double *__restrict__ ops,
                                                        const double *__restrict__ tab,
                                                        const double *__restrict__ lam,
                                                        double *__restrict__ dlam, int Np, int cp,
                                                        int n_ops, int m, double *__restrict__ gpanels, int n_off)
{
    extern __shared__ double lds_panels[];              // g_0 .. g_m
    const int n = blockIdx.y + 1, grp = blockIdx.x;
    // (n_off: global index of this grid's first time point -- a window of a long grid, a rank's window: only GLOBAL
    //  time index 1 takes the controls of its own time point, forward_evolution.jl:423,472)
    const int tn = (n + n_off >= 2) ? n - 1 : 1;
    double *smem = gpanels ? gpanels + ((size_t)blockIdx.y * gridDim.x + grp) * (size_t)(m + 1) * Np * 16 : lds_panels;
    const int PWc = 2 * cp;
    const size_t hstep = (size_t)Np * PWc;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int c16 = lane & 15, kk = lane >> 4;
    const size_t ps = (size_t)Np * 16;
    for (int j = 1; j <= m; j++) {
        for (int e = threadIdx.x; e < Np * 16; e += blockDim.x) {
            smem[(size_t)j * ps + e] = lam[(size_t)n * hstep + (size_t)(e >> 4) * PWc + grp * 16 + (e & 15)];
            for (int i = 0; i < j; i++) smem[(size_t)i * ps + e] = 0.0;
        }
        __threadfence_block();
        __syncthreads();
        for (int k = j; k >= 1; k--) {
            const double *src = smem + (size_t)k * ps;
            const double inv = 1.0 / (double)k;
            for (int rb = wave; rb * 16 < Np; rb += nw) {         // a wave owns its rows of every target panel
                const int arow = rb * 16 + c16;
                for (int i = 0; i < k; i++) {
                    OpCoef cf;
                    load_coef(cf, tab, tn, k - 1 - i, m, n_ops);
                    d4 acc = (d4){0, 0, 0, 0};
                    for (int k0 = 0; k0 < Np; k0 += 4) {
                        double are, aim, b1, b2;
                        assembled_a<NOPS>(ops, Np, n_ops, cf, arow, k0 + kk, are, aim);
                        panel_b(src + (size_t)(k0 + kk) * 16, c16, b1, b2);
                        acc = MFMA(are, b1, acc);
                        acc = MFMA(aim, b2, acc);
                    }
                    #pragma unroll
                    for (int r = 0; r < 4; r++) smem[(size_t)i * ps + (size_t)(rb * 16 + kk + 4 * r) * 16 + c16] -= acc[r] * inv;
                }
            }
            __threadfence_block();
            __syncthreads();
        }
        for (int e = threadIdx.x; e < Np * 16; e += blockDim.x)
            dlam[(((size_t)n * m + (j - 1)) * Np + (e >> 4)) * PWc + grp * 16 + (e & 15)] = smem[e];
        __threadfence_block();
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Test hook: out = (+/-) A_d(t_n) * in for a panel of columns (apply_hamiltonian!,
// hermite.jl:556-588, batched over all initial-condition columns).
// ---------------------------------------------------------------------------
template <int NOPS>
__global__ __launch_bounds__(256) void k_apply(const double *__restrict__ ops,
                                               const double *__restrict__ tab,
                                               const double *__restrict__ in,
                                               double *__restrict__ out, int Np, int cp, int n_ops,
                                               int m, int n, int d, double sign)
{
    extern __shared__ double smem[];
    const int grp = blockIdx.x;
    const int PWc = 2 * cp;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int c16 = lane & 15, kk = lane >> 4;
    for (int e = threadIdx.x; e < Np * 16; e += blockDim.x)
        smem[e] = in[(size_t)(e >> 4) * PWc + grp * 16 + (e & 15)];
    __syncthreads();
    OpCoef cf;
    load_coef(cf, tab, n, d, m, n_ops);
    for (int rb = wave; rb * 16 < Np; rb += nw) {
        d4 acc = (d4){0, 0, 0, 0};
        const int arow = rb * 16 + c16;
        for (int k0 = 0; k0 < Np; k0 += 4) {
            double are, aim, b1, b2;
            assembled_a<NOPS>(ops, Np, n_ops, cf, arow, k0 + kk, are, aim);
            panel_b(smem + (size_t)(k0 + kk) * 16, c16, b1, b2);
            acc = MFMA(are, b1, acc);
            acc = MFMA(aim, b2, acc);
        }
        #pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = rb * 16 + kk + 4 * r;
            out[(size_t)row * PWc + grp * 16 + c16] = sign * acc[r];
        }
    }
}

extern "C" {

int qgdk_derivs(const qgdk_ctx *c)
{
    if (c->dense_gemm && !c->use_sparse) return qgdk_dense_derivs(c);
    if (c->use_sparse) return qgdk_derivs_sparse(c);
    size_t shm = (size_t)(c->m + 1) * c->Np * 16 * sizeof(double);
    double *gp = nullptr;
    if (c->panel_scratch) { gp = c->panel_scratch; shm = 0; }
#define CALL_DV(N) do { if (shm > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)k_derivs<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm)); \
        hipLaunchKernelGGL((k_derivs<N>), dim3(c->cp / 8, c->nt), dim3(256), shm, c->stream, c->ops, c->tab, c->hist, c->dpsi, \
                           c->Np, c->cp, c->n_ops, c->m, gp); } while (0)
    DISPATCH_NOPS(c->n_ops, CALL_DV)
#undef CALL_DV
    return (int)hipGetLastError();
}

// the result mirror of an evaluation WITHOUT a gradient (qgd_eval_forward): one small workgroup behind the last kernel
// publishes [scal(4) | status] and the sequence number
__global__ void k_mirror_scalars(const ResultMirror mir, int n_pcof)
{
    if (threadIdx.x == 0) {
        #pragma unroll
        for (int q = 0; q < 4; q++) mir.host[n_pcof + q] = mir.scal[q];
        mir.host[n_pcof + 4] = (double)*mir.status;
        __threadfence_system();
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(mir.host + n_pcof + 5), mir.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

static inline ResultMirror mirror_of(const qgdk_ctx *c)
{
    ResultMirror m;
    m.host = c->mirror_dev; m.seq = c->mirror_seq; m.ticket = c->mirror_ticket; m.scal = c->scal; m.status = c->status;
    return m;
}

int qgdk_mirror_scalars(const qgdk_ctx *c)
{
    hipLaunchKernelGGL(k_mirror_scalars, dim3(1), dim3(64), 0, c->stream, mirror_of(c), c->n_pcof);
    return (int)hipGetLastError();
}

// rows of cpart added in a fixed order -> grad (and the host mirror): the tail of the small-problem path (qgd_k_tiny.hip)
int qgdk_contract_rows(const qgdk_ctx *c, int rows)
{
    hipLaunchKernelGGL(k_contract_sum<false>, dim3((c->n_pcof + 15) / 16), dim3(1024), 0, c->stream, c->cpart, c->grad, c->n_pcof, rows,
                       0, c->status, c->scal, mirror_of(c), ContractBatch{});
    return (int)hipGetLastError();
}

// the same for every member of a batch in one launch (rows = 0: a forward-only batch, only the scalars and the status travel)
int qgdk_contract_rows_batch(const qgdk_ctx *c, const qgdk_tiny_batch *b, int members, int n_pcof, int rows)
{
    size_t st, sm, sc;
    qgdk_tiny_batch_layout(c, n_pcof, &st, &sm, &sc);
    ContractBatch bt{(long long)sc, b->rows, b->small, reinterpret_cast<int *>(b->small + 4), QGD_TINY_BATCH_SMALL, 2 * QGD_TINY_BATCH_SMALL};
    ResultMirror none{};
    hipLaunchKernelGGL(k_contract_sum<true>, dim3((n_pcof + 15) / 16, members), dim3(1024), 0, c->stream, b->cpart, (double *)nullptr, n_pcof, rows,
                       0, (const int *)nullptr, (double *)nullptr, none, bt);
    return (int)hipGetLastError();
}

// the weighted sums of an ensemble chunk behind it (k_ensemble_reduce), under the context's cost type
int qgdk_ensemble_reduce(const qgdk_ctx *c, const double *rows, const double *weights, double *acc, double *tails, int members, int n_pcof, int first, int gradient)
{
    if (members < 1 || n_pcof < 1 || n_pcof + 2 > 128) return (int)hipErrorInvalidValue;
    const EnsembleReduce r{rows, weights, acc, tails, members, n_pcof, first, gradient, c->cost_type == 0, c->n_ess};
    hipLaunchKernelGGL(k_ensemble_reduce, dim3(1), dim3(128), 0, c->stream, r);
    return (int)hipGetLastError();
}

int qgdk_gradient(const qgdk_ctx *c)
{
    if (c->n_ops == 0) return 0;                       // no control parameters: nothing to differentiate
    if (c->use_sparse) {      // k_gradpoint_ell contracts with the basis itself: one row of cpart per (column group, time point)
        const int rc = qgdk_gradient_sparse(c);
        if (rc) return rc;
        hipLaunchKernelGGL(k_contract_sum<false>, dim3((c->n_pcof + 15) / 16), dim3(1024), 0, c->stream, c->cpart, c->grad, c->n_pcof,
                           (c->cp / 8) * c->nt, c->grad_accumulate, c->status, c->scal, mirror_of(c), ContractBatch{});
        return (int)hipGetLastError();
    }
    if (c->dense_gemm) {
        const int rc = qgdk_dense_gradient(c);
        return rc ? rc : qgdk_contract(c);
    }
    size_t shm = ((size_t)2 * c->m * c->Np * 16 + (size_t)4 * c->n_ops * c->m * 2) * sizeof(double);
    double *gp = nullptr;
    if (c->panel_scratch) { gp = c->panel_scratch; shm = (size_t)4 * c->n_ops * c->m * 2 * sizeof(double); }
    if (c->Np == 64 && c->m <= 5 && c->n_ops >= 1) {
        int rc = 0;
        switch (c->m) {
        case 1: rc = launch_gradpoint64_m<1>(c); break;
        case 2: rc = launch_gradpoint64_m<2>(c); break;
        case 3: rc = launch_gradpoint64_m<3>(c); break;
        case 4: rc = launch_gradpoint64_m<4>(c); break;
        default: rc = launch_gradpoint64_m<5>(c); break;
        }
        if (rc) return rc;
        return qgdk_contract(c);
    }
#define CALL_GS(N) do { if (shm > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)k_gradsweep<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm)); \
        hipLaunchKernelGGL((k_gradsweep<N>), dim3(c->cp / 8, c->nt), dim3(256), shm, c->stream, c->ops, c->tab, c->hist, \
                           c->dpsi, c->lam, c->sigma, c->cw, c->Np, c->cp, c->n_ops, c->m, c->nt, gp); } while (0)
    DISPATCH_NOPS(c->n_ops, CALL_GS)
#undef CALL_GS
    return qgdk_contract(c);
}

int qgdk_contract(const qgdk_ctx *c)
{
    const int chunks = (c->nt + CT_CHUNK - 1) / CT_CHUNK;
    hipLaunchKernelGGL(k_contract, dim3(chunks, c->n_ops, (c->nc_max + 63) / 64), dim3(256), 0,
                       c->stream, c->G, c->goff, c->ncoef, c->poff, c->sigma, c->nt, c->m, c->n_ops, c->status, c->scal,
                       c->dense_gemm ? qgdk_dense_sigma_planes(c) : c->cp / 8,      // one plane per contributing workgroup, added in order
                       c->cpart, c->n_pcof,
                       c->g_nt ? c->g_nt : c->nt, c->g_n0);
    hipLaunchKernelGGL(k_contract_sum<false>, dim3((c->n_pcof + 15) / 16), dim3(1024), 0, c->stream, c->cpart, c->grad, c->n_pcof, chunks,
                       c->grad_accumulate, (const int *)nullptr, (double *)nullptr, mirror_of(c), ContractBatch{});
    return (int)hipGetLastError();
}

int qgdk_apply(const qgdk_ctx *c, const double *in, double *out, int n, int d, double sign)
{
    size_t shm = (size_t)c->Np * 16 * sizeof(double);
#define CALL_AP(N) hipLaunchKernelGGL((k_apply<N>), dim3(c->cp / 8), dim3(256), shm, c->stream, c->ops, c->tab, in, out, c->Np, \
                                      c->cp, c->n_ops, c->m, n, d, sign)
    DISPATCH_NOPS(c->n_ops, CALL_AP)
#undef CALL_AP
    return (int)hipGetLastError();
}

// dlam[n][j-1] = D_j(t_{max(n-1,1)})^T lambda_n for n = 1 .. nt-1 (k_adjoint_derivs); scratch: (m+1) panels per workgroup
// in HBM when they do not fit in LDS, else null
int qgdk_adjoint_derivs(const qgdk_ctx *c, double *dlam, double *scratch)
{
    if (c->nt < 2 || c->m < 1) return 0;
    size_t shm = (size_t)(c->m + 1) * c->Np * 16 * sizeof(double);
    if (scratch) shm = 0;
#define CALL_AD(N) do { if (shm > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)k_adjoint_derivs<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm)); \
        hipLaunchKernelGGL((k_adjoint_derivs<N>), dim3(c->cp / 8, c->nt - 1), dim3(256), shm, c->stream, c->ops, c->tab, c->lam, dlam, \
                           c->Np, c->cp, c->n_ops, c->m, scratch, c->n_off); } while (0)
    DISPATCH_NOPS(c->n_ops, CALL_AD)
#undef CALL_AD
    return (int)hipGetLastError();
}

int qgdk_gradient_needs_derivs(const qgdk_ctx *c)
{
    if (c->dense_gemm && !c->use_sparse) return qgdk_dense_gradient_needs_derivs(c);      // (the outer-product form through D_i needs none)
    return !(c->use_sparse || (c->Np == 64 && c->m <= 5 && c->n_ops >= 1));
}


} // extern "C"
