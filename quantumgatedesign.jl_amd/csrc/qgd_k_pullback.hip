// qgd_k_pullback.hip -- cotangents of the trajectory outputs (states, level populations, expectation values) as the forcing of
// the adjoint sweep (qgd_eval_pullback).  (conventions: qgd_kernels_common.h)
//
// With the outputs of qgd_eval_states / qgd_eval_populations / qgd_eval_expectations, slot k holding time point n = k * save,
//   S[:, k, col] = [u; v],   P[g, k, col] = sum_l M[g, l] (u_l^2 + v_l^2),   E[j, k, col] = Re(psi^H O_j psi),  O_j = A_j + iB_j,
// the derivative of <Sbar, S> + <Pbar, P> + <Ebar, E> with respect to w_n = [u; v] is
//   f_n = Sbar[:, k, col] + 2 (M^T Pbar[:, k, col]) (.) [u; v] + 2 sum_j Ebar[j, k, col] [A_j u - B_j v; A_j v + B_j u]
// at the time points a slot addresses, zero at the others and at n = 0 (the initial state does not depend on pcof).  The
// gradient sum_n Re<s_k(n), f_n> is term (B) of qgd_k_hvp.hip: the adjoint scan runs with the forcing F = -f, its terminal
// value F_N, and the gradient kernels with that mu in place of lambda.
//
// k_pullback_forcing writes F [nt][Np][2cp] -- every panel on every call, padding rows and columns as zeros, so no memset and
// no stale forcing.  One (column group, time point) tile at a time per workgroup.  The expectations part runs on the f64 MFMA
// with the operand arrangement of k_expectations (qgd_k_observe.hip): the tile's 16-double rows are the B operand [u | v] as
// they lie, here with column cc scaled by Ebar[j, slot, cc], and wave rb keeps two accumulators for its 16 rows over all
// observables, sum_j A_j (e_j (.) [u | v]) and the same with the planes B_j; the epilogue pairs the halves of the second with
// those of the first through one wave shuffle.  The tile goes to LDS once, padding rows (N ..) and columns (c ..) zero by
// selection; the planes are staged once per workgroup in fragment order when they fit beside the tiles (PLANES_LDS, the rule of
// k_expectations), else every fragment is read from global memory (L2) with the same zero rule -- the same bits either way.
// Order of every sum, the same on every run: the level weights over ascending g; the accumulators over ascending j, then
// ascending k-step (one MFMA chain each); states + populations + expectations per element.  No atomics.
#include "qgd_kernels_common.h"

typedef double d2 __attribute__((ext_vector_type(2)));

struct PullbackArgs {
    const double *hist;         // state panels [nt][Np][2cp]
    double *F;                  // [nt][Np][2cp]
    const double *sbar;         // [2N, n_slots, c], or null
    const double *pbar;         // [prow, n_slots, c] (prow = n_groups with a map, else N), or null
    const double *map;          // [n_groups x N] column-major, or null
    const double *ebar;         // [n_obs, n_slots, c], or null
    const double *pre, *pim;    // [N x N x n_obs] column-major planes A and B; pim null: real observables
    int N, Np, c, cp, nt, save, n_slots, n_groups, prow, n_obs;
    int nrb, nks;               // row blocks of 16 and k-steps of 4 that cover N (nrb <= 4: one wave each)
    int total;                  // (column group, time point) tiles
};

template <bool PLANES_LDS>
__global__ __launch_bounds__(256) void k_pullback_forcing(PullbackArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, c16 = lane & 15, kk = lane >> 4;
    const int N = a.N, nrb = a.nrb, nks = a.nks, ngrp = a.cp >> 3, PWc = 2 * a.cp;
    const int npl = a.pim ? 2 : 1;
    const size_t hstep = (size_t)a.Np * PWc, NN = (size_t)N * N;
    const size_t frag = (size_t)nrb * nks * 64;      // doubles of one plane in fragment order
    double *pt = lds;                                // [16 nrb][16]  the state tile
    double *ot = pt + 256 * (size_t)nrb;             // [16 nrb][16]  sum_j e_j [A u - B v | A v + B u]
    double *eb = ot + 256 * (size_t)nrb;             // [n_obs][8]    Ebar of the tile's slot and columns
    double *pl = eb + 8 * (size_t)a.n_obs;           // [n_obs][npl][nrb][nks][64]
    if (PLANES_LDS && a.ebar) {
        const size_t cnt = (size_t)a.n_obs * npl * frag;
        for (size_t i = t; i < cnt; i += 256) {
            const int l = (int)(i & 63);
            const size_t f = i >> 6;
            const int ks = (int)(f % nks), rb = (int)((f / nks) % nrb);
            const size_t p = f / ((size_t)nks * nrb);
            const int row = 16 * rb + (l & 15), k = 4 * ks + (l >> 4);
            const double *plane = ((p % npl) ? a.pim : a.pre) + (p / npl) * NN;
            pl[i] = (row < N && k < N) ? plane[row + (size_t)N * k] : 0.0;
        }
    }
    for (int tl = blockIdx.x; tl < a.total; tl += gridDim.x) {
        const int g = tl % ngrp, n = tl / ngrp;
        const bool addressed = n > 0 && n % a.save == 0;      // (the same for the whole workgroup)
        const size_t slot = (size_t)(n / a.save);
        const double *hn = a.hist + (size_t)n * hstep;
        if (addressed && a.ebar) {
            const double *sp = hn + 16 * g;
            for (int idx = t; idx < 128 * nrb; idx += 256) {
                const int r = idx >> 3, q = idx & 7, col = 8 * g + 2 * (q & 3);
                d2 x = (d2){0.0, 0.0};
                if (r < N && col < a.c) {
                    x = *reinterpret_cast<const d2 *>(sp + (size_t)r * PWc + 2 * q);
                    if (col + 1 >= a.c) x.y = 0.0;
                }
                *reinterpret_cast<d2 *>(pt + 16 * r + 2 * q) = x;
            }
            for (int o = t; o < 8 * a.n_obs; o += 256) {
                const int j = o >> 3, col = 8 * g + (o & 7);
                eb[o] = col < a.c ? a.ebar[j + (size_t)a.n_obs * (slot + (size_t)a.n_slots * col)] : 0.0;
            }
            __syncthreads();
            if (wave < nrb) {
                const int rb = wave, row = 16 * rb + c16;
                d4 accA = (d4){0, 0, 0, 0}, accB = (d4){0, 0, 0, 0};
                for (int j = 0; j < a.n_obs; j++) {
                    const double e = eb[8 * j + (c16 & 7)];
                    const double *fa = pl + ((size_t)j * npl * nrb + rb) * nks * 64 + lane;      // plane A of j; plane B one `frag` further
                    for (int ks = 0; ks < nks; ks++) {
                        const int k = 4 * ks + kk;
                        const double b = e * pt[16 * k + c16];
                        const bool in = row < N && k < N;
                        const double av = PLANES_LDS ? fa[(size_t)ks * 64] : (in ? a.pre[j * NN + row + (size_t)N * k] : 0.0);
                        accA = MFMA(av, b, accA);
                        if (a.pim) {
                            const double bv = PLANES_LDS ? fa[frag + (size_t)ks * 64] : (in ? a.pim[j * NN + row + (size_t)N * k] : 0.0);
                            accB = MFMA(bv, b, accB);
                        }
                    }
                }
                #pragma unroll
                for (int r = 0; r < 4; r++) {      // lane (c16, kk), register r: row 16 rb + kk + 4 r, column c16
                    double v = accA[r];
                    if (a.pim) {
                        const double o = __shfl_xor(accB[r], 8);      // (B v) for a u column, (B u) for a v column
                        v += (c16 < 8) ? -o : o;
                    }
                    ot[16 * (16 * rb + kk + 4 * r) + c16] = v;
                }
            }
            __syncthreads();
        }
        // the (at most two) pairs of panel entries of this thread: 16-byte loads and stores, a row of the group is 128 bytes
        #pragma unroll
        for (int it = 0; it < 2; it++) {
            const int e2 = t + it * 256, row = e2 >> 3, q = (e2 & 7) * 2;
            if (e2 >= a.Np * 8) continue;
            const size_t off = (size_t)row * PWc + (size_t)g * 16 + q;
            const int col0 = 8 * g + (q & 7), im = q >> 3;      // im: the v half of the row
            double f[2] = {0.0, 0.0};
            if (addressed && row < N && col0 < a.c) {
                d2 x = (d2){0.0, 0.0};
                if (a.pbar) x = *reinterpret_cast<const d2 *>(hn + off);
                #pragma unroll
                for (int e = 0; e < 2; e++) {
                    const int col = col0 + e;
                    if (col >= a.c) continue;
                    const size_t sc = slot + (size_t)a.n_slots * col;
                    double acc = 0.0;
                    if (a.sbar) acc = a.sbar[row + im * N + 2 * (size_t)N * sc];
                    if (a.pbar) {
                        const double *pb = a.pbar + (size_t)a.prow * sc;
                        double w = 0.0;
                        if (a.map) for (int gi = 0; gi < a.n_groups; gi++) w = fma(a.map[gi + (size_t)a.n_groups * row], pb[gi], w);
                        else w = pb[row];
                        acc += 2.0 * w * (e ? x.y : x.x);
                    }
                    if (a.ebar) acc += 2.0 * ot[16 * row + q + e];
                    f[e] = -acc;
                }
            }
            *reinterpret_cast<d2 *>(a.F + (size_t)n * hstep + off) = (d2){f[0], f[1]};
        }
        if (addressed && a.ebar) __syncthreads();      // (the next tile overwrites pt and ot)
    }
}

// F [nt][Np][2cp] = -f of the cotangents given (each of sbar, pbar, ebar may be null; all on the device, in the layouts of the
// outputs of qgd_eval_states / qgd_eval_populations / qgd_eval_expectations with slot k at time point k * save)
extern "C" int qgdk_pullback_forcing(const qgdk_ctx *c, double *F, int save, const double *sbar, const double *pbar, const double *map_dev,
                                     int n_groups, const double *ebar, const double *obs_re, const double *obs_im, int n_obs)
{
    if (c->N > 64 || c->Np > 64 || save < 1 || (map_dev && n_groups < 1) || (ebar && (!obs_re || n_obs < 1 || n_obs > 0x00ffffff)))
        return (int)hipErrorInvalidValue;      // (two pairs of panel entries per thread, one wave per row block)
    PullbackArgs a;
    a.hist = c->hist; a.F = F; a.sbar = sbar; a.pbar = pbar; a.map = pbar ? map_dev : nullptr; a.ebar = ebar;
    a.pre = obs_re; a.pim = ebar ? obs_im : nullptr;
    a.N = c->N; a.Np = c->Np; a.c = c->c; a.cp = c->cp; a.nt = c->nt; a.save = save; a.n_slots = 1 + (c->nt - 1) / save;
    a.n_groups = a.map ? n_groups : 0; a.prow = a.map ? n_groups : c->N; a.n_obs = ebar ? n_obs : 0;
    a.nrb = (c->N + 15) / 16; a.nks = (c->N + 3) / 4;
    const long long total = (long long)(c->cp / 8) * c->nt;
    if (total > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    a.total = (int)total;
    if (!ebar) {
        hipLaunchKernelGGL(k_pullback_forcing<false>, dim3(a.total < 2048 ? a.total : 2048), dim3(256), 0, c->stream, a);
        return (int)hipGetLastError();
    }
    const size_t lds_max = 160 * 1024;      // LDS of a gfx950 CU, all of which one workgroup may take
    const size_t tile_bytes = (512 * (size_t)a.nrb + 8 * (size_t)n_obs) * sizeof(double);      // (N <= 64: 16 KB + 64 n_obs bytes)
    if (tile_bytes > lds_max) return (int)hipErrorInvalidValue;
    const size_t plane_bytes = (size_t)n_obs * (obs_im ? 2 : 1) * a.nrb * a.nks * 64 * sizeof(double);
    if (tile_bytes + plane_bytes <= lds_max && !qgd_path("planes_l2")) {      // (QGD_PATHS=planes_l2: the route of a batch that does not fit)
        const size_t bytes = tile_bytes + plane_bytes;
        const int per_cu = (int)(lds_max / bytes), grid_max = 256 * (per_cu < 8 ? per_cu : 8);
        if (bytes > 64 * 1024) SET_LDS_ONCE(k_pullback_forcing<true>, bytes);
        hipLaunchKernelGGL(k_pullback_forcing<true>, dim3(a.total < grid_max ? a.total : grid_max), dim3(256), bytes, c->stream, a);
    } else {
        if (tile_bytes > 64 * 1024) SET_LDS_ONCE(k_pullback_forcing<false>, tile_bytes);
        hipLaunchKernelGGL(k_pullback_forcing<false>, dim3(a.total < 2048 ? a.total : 2048), dim3(256), tile_bytes, c->stream, a);
    }
    return (int)hipGetLastError();
}
