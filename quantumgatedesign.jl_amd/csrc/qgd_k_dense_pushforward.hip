// qgd_k_dense_pushforward.hip -- the kernel qgd_eval_dense_pushforward adds to what the grid-point pushforward and the dense
// output run: the tangent of the stage derivatives along directions in pcof, the forward-mode counterpart
// of k_dense_pullback_sweep (qgd_k_dense_pullback.hip).  (conventions and layouts: qgd_kernels_common.h)
//
// With w_0(n) = psi_n, w_j(n) = (1/j) sum_{i<j} A_{j-1-i}(t_n) w_i(n) as k_derivs left them (hist, dpsi), the state tangent
// dw_0(n) = s_v(n) of the forced scan (sv, direction `dir` in the columns dir cp ..) and
//   dA_d(t_n) = sum_o ( dq_o^(d) Asym_o - i dp_o^(d) Sym_o ),   d = 0 .. m-1,
// the dotted coefficients being the entries of the direction table of k_hvp_gv_dirs (no system term),
//   dw_j(n) = (1/j) sum_{i<j} [ A_{j-1-i}(t_n) dw_i(n) + dA_{j-1-i}(t_n) w_i(n) ],   j = 1 .. m.
// Output: dsv [nt][m][Np][2 n_dir cp], dw_1 .. dw_m of every time point in the layout of dpsi on a context whose columns are the
// n_dir cp columns of the chunk -- what qgdk_interp takes as `dpsi` beside sv as `hist`.
//
// k_tangent_derivs<NOPS>: one workgroup per (column group, time point, direction), 256 threads (four waves, a wave owns 16-row
// blocks of every target panel), on the assembled dense operator planes c->ops as k_derivs and k_dense_pullback_sweep.
//   LDS: w_0 .. w_{m-1} (m panels) and dw_0 .. dw_m (m+1 panels) of [Np][16] doubles, and the coefficients of A_d and dA_d
//   ([2][m][CF_STRIDE]): (2m+1) Np 128 + 2 m CF_STRIDE 8 bytes -- 138.1 KB at Np = 64, m = 8 (136 KB of panels), under the 160 KB of
//   a gfx950 CU.  No global-scratch route: N > 64 is refused by the entry point.
//   Products on the fp64 MFMA.  Per target j and 16-row block ONE accumulator: i ascending, the product A_{j-1-i} dw_i (k ascending)
//   before the product dA_{j-1-i} w_i (k ascending), then times 1/j.  No atomics: the same bits on every run, and the bits of a
//   direction depend neither on its neighbours nor on the width of the chunk.
//   Rows N .. Np-1 and columns c .. of the inputs are read as zeros; padding rows and columns of the output are written as zeros
//   on every call; n = 0 is written like every other point (dw_0(0) = 0 but dA w is not).  Ordinary 16-byte vector stores.
#include "qgd_kernels_common.h"

typedef double d2 __attribute__((ext_vector_type(2)));

#define TDERIV_MAX_M 8      // m = order/2 <= 8: the bound of the interpolation kernels

// index of entry (n, b) of the direction table, b = (o 2 + tau) m + d (tau = 0: p, 1: q), M = n_ops m: the layout k_hvp_gv_dirs writes
__device__ __forceinline__ size_t tderiv_gvi(int n, int b, int M, int nt) { return ((size_t)(b / M) * nt + n) * (M + 1) + b % M; }

__device__ __forceinline__ void coef_from_lds(OpCoef &cf, const double *s)
{
    cf.sys = s[0];
    #pragma unroll
    for (int o = 0; o < QGD_MAX_OPS_DEV; o++) { cf.p[o] = s[1 + 2 * o]; cf.q[o] = s[2 + 2 * o]; }
}

template <int NOPS>
__global__ __launch_bounds__(256) void k_tangent_derivs(const double *__restrict__ ops,
                                                        const double *__restrict__ tab,
                                                        const double *__restrict__ hist,
                                                        const double *__restrict__ dpsi,
                                                        const double *__restrict__ sv,
                                                        const double *__restrict__ gvt,
                                                        double *__restrict__ dsv, int N, int Np, int c, int cp,
                                                        int n_ops, int m, int nt, int n_dir)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];     // w_0..w_{m-1}, dw_0..dw_m, cfa[m][CF_STRIDE], cfd[m][CF_STRIDE]
    const int grp = blockIdx.x, n = blockIdx.y, dir = blockIdx.z;
    const int ngrp = cp >> 3, PWc = 2 * cp;
    const size_t PWs = (size_t)PWc * n_dir, hstep = (size_t)Np * PWc;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int c16 = lane & 15, kk = lane >> 4;
    const size_t ps = (size_t)Np * 16;
    double *W = smem, *T = smem + (size_t)m * ps;      // W[i * ps]: w_i, T[j * ps]: dw_j
    double *cfa = T + (size_t)(m + 1) * ps, *cfd = cfa + (size_t)m * CF_STRIDE;
    const int M = n_ops * m, nks = Np >> 2;
    const size_t dcol = 16 * ((size_t)dir * ngrp + grp);      // this direction's copy of the column group in sv and dsv

    for (int e = threadIdx.x; e < Np * 16; e += blockDim.x) {
        const int row = e >> 4, q = e & 15;
        const bool live = row < N && 8 * grp + (q & 7) < c;      // (padding rows and columns: zeros by selection, nothing is read)
        const size_t src = (size_t)row * PWc + grp * 16 + q;
        W[e] = live ? hist[(size_t)n * hstep + src] : 0.0;
        for (int i = 1; i < m; i++) W[(size_t)i * ps + e] = live ? dpsi[((size_t)n * m + (i - 1)) * hstep + src] : 0.0;
        T[e] = live ? sv[((size_t)n * Np + row) * PWs + dcol + q] : 0.0;
    }
    for (int e = threadIdx.x; e < m * CF_STRIDE; e += blockDim.x) {
        const int d = e / CF_STRIDE, q = e % CF_STRIDE, o = (q - 1) >> 1, tau = (q - 1) & 1;      // q = 0: the system flag, 1 + 2o: p_o, 2 + 2o: q_o
        const bool on = q > 0 && o < n_ops;
        cfa[e] = q == 0 ? (d == 0 ? 1.0 : 0.0) : (on ? tab[(((size_t)n * (m + 1) + d) * n_ops + o) * 2 + tau] : 0.0);
        cfd[e] = on ? gvt[tderiv_gvi(n, (o * 2 + tau) * m + d, M, nt) * n_dir + dir] : 0.0;
    }
    __syncthreads();

    for (int j = 1; j <= m; j++) {
        for (int rb = wave; rb * 16 < Np; rb += nw) {
            const int arow = rb * 16 + c16;
            d4 acc = (d4){0, 0, 0, 0};
            for (int i = 0; i < j; i++) {
                OpCoef ca, cd;
                coef_from_lds(ca, cfa + (size_t)(j - 1 - i) * CF_STRIDE);
                coef_from_lds(cd, cfd + (size_t)(j - 1 - i) * CF_STRIDE);
                const double *ti = T + (size_t)i * ps, *wi = W + (size_t)i * ps;
                for (int ks = 0; ks < nks; ks++) {      // A_{j-1-i} dw_i
                    double are, aim, b1, b2;
                    assembled_a<NOPS>(ops, Np, n_ops, ca, arow, 4 * ks + kk, are, aim);
                    panel_b(ti + (size_t)(4 * ks + kk) * 16, c16, b1, b2);
                    acc = MFMA(are, b1, acc);
                    acc = MFMA(aim, b2, acc);
                }
                for (int ks = 0; ks < nks; ks++) {      // dA_{j-1-i} w_i
                    double are, aim, b1, b2;
                    assembled_a<NOPS>(ops, Np, n_ops, cd, arow, 4 * ks + kk, are, aim);
                    panel_b(wi + (size_t)(4 * ks + kk) * 16, c16, b1, b2);
                    acc = MFMA(are, b1, acc);
                    acc = MFMA(aim, b2, acc);
                }
            }
            const double sc = 1.0 / (double)j;
            #pragma unroll
            for (int r = 0; r < 4; r++) T[(size_t)j * ps + (size_t)(rb * 16 + kk + 4 * r) * 16 + c16] = sc * acc[r];
        }
        __syncthreads();      // (dw_j is read by every wave from the next target on)
    }

    // dw_1 .. dw_m: whole panel tiles, zeros in padding rows and columns (16-byte stores, a row of the group is 128 bytes)
    for (int idx = threadIdx.x; idx < 8 * Np * m; idx += blockDim.x) {
        const int j = idx / (8 * Np), rem = idx - j * 8 * Np, row = rem >> 3, q = rem & 7, col = 8 * grp + 2 * (q & 3);
        d2 x = (d2){0.0, 0.0};
        if (row < N && col < c) {
            x = *reinterpret_cast<const d2 *>(T + (size_t)(j + 1) * ps + (size_t)row * 16 + 2 * q);
            if (col + 1 >= c) x.y = 0.0;
        }
        *reinterpret_cast<d2 *>(dsv + (((size_t)n * m + j) * Np + row) * PWs + dcol + 2 * q) = x;
    }
}

// dynamic LDS of k_tangent_derivs
static size_t tangent_derivs_lds(int Np, int m)
{
    return ((size_t)(2 * m + 1) * Np * 16 + (size_t)2 * m * CF_STRIDE) * sizeof(double);
}

extern "C" {

// the stage derivatives of c (hist, dpsi), the tangent panels sv [nt][Np][2 n_dir cp] of a chunk of n_dir directions and their
// direction table gvt (qgdk_hvp_gv_dirs) -> dsv [nt][m][Np][2 n_dir cp]
int qgdk_tangent_derivs(const qgdk_ctx *c, const double *sv, const double *gvt, double *dsv, int n_dir)
{
    if (c->m < 1 || c->m > TDERIV_MAX_M || c->n_ops < 1 || c->n_ops > QGD_MAX_OPS_DEV || c->N > 64 || c->Np > 64 || (c->Np & 15) || c->nt < 1 || c->nt > 65535 ||
        n_dir < 1 || n_dir > 65535)
        return (int)hipErrorInvalidValue;
    const size_t shm = tangent_derivs_lds(c->Np, c->m);
    if (shm > 160 * 1024) return (int)hipErrorInvalidValue;      // LDS of a gfx950 CU, all of which one workgroup may take
#define CALL_TD(NO) do { if (shm > 64 * 1024) SET_LDS_ONCE(k_tangent_derivs<NO>, shm); \
        hipLaunchKernelGGL((k_tangent_derivs<NO>), dim3(c->cp / 8, c->nt, n_dir), dim3(256), shm, c->stream, c->ops, c->tab, c->hist, \
                           c->dpsi, sv, gvt, dsv, c->N, c->Np, c->c, c->cp, c->n_ops, c->m, c->nt, n_dir); } while (0)
    DISPATCH_NOPS(c->n_ops, CALL_TD)
#undef CALL_TD
    return (int)hipGetLastError();
}

} // extern "C"
