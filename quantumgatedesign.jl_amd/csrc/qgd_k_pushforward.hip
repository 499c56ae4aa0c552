// qgd_k_pushforward.hip -- tangents of the level populations and the expectation values along directions in pcof
// (qgd_eval_pushforward).  (conventions and layouts: qgd_kernels_common.h)
//
// With the state panels hist [nt][Np][2cp] (w = [u; v], psi = u + iv) and the tangent panels sv [nt][Np][2 n_dir cp] of the
// forced scan (dw = [du; dv] = sum_l v_l dw/dpcof_l, direction j in the columns j cp ..), per saved time point and column:
//   pop_dot[k]    = 2 (u_k du_k + v_k dv_k),   with a level map M [n_groups x N]:  sum_k M[g, k] pop_dot[k], k ascending
//   expect_dot[j] = 2 Re(psi^H H_j dpsi),      H_j = (O_j + O_j^H) / 2 = As + i Ba of O_j = A + iB:
//                 = 2 ( u^T (As du - Ba dv) + v^T (As dv + Ba du) )
// (As = (A + A^T) / 2, Ba = (B - B^T) / 2: qgd_eval_expectations returns the expectation of the Hermitian part of what was passed,
// and this is its derivative whatever was passed).  One memory-bound pass: every panel entry is read once, with 16-byte loads.
//
// One tile = (column group, saved time point, direction), 256 threads: thread (row r = t / 4, pair pr = t % 4) holds the two
// real and the two imaginary parts of columns 2 pr, 2 pr + 1 of row r of both panels (Np <= 64: one row per thread).  A wave
// holds 16 consecutive rows.  Workgroups walk the tiles, so the map and the planes of the Hermitian parts are staged in LDS once
// per workgroup when they fit beside the tiles (STAGED); else every element is formed from global memory (L2) by the same
// expression: the same bits.  Slot 0 is written as zeros without a read.
//   Order of the sums, the same on every run and for every n_dir and n_obs: H dpsi of a row over k ascending, fused
// multiply-adds, As before Ba; u part + v part; over the 16 rows of a wave by a butterfly (lanes 4, 8, 16, 32 apart); the
// four waves in ascending order; times 2.  No atomics.
#include "qgd_kernels_common.h"

typedef double d2 __attribute__((ext_vector_type(2)));

struct PushArgs {
    const double *hist;         // state panels [nt][Np][2cp]
    const double *sv;           // tangent panels [nt][Np][2 n_dir cp]
    double *pop;                // [prow, n_slots, c, n_dir] or null
    double *expect;             // [n_obs, n_slots, c, n_dir] or null
    const double *map;          // [n_groups x N] column-major, or null
    const double *pre, *pim;    // [N x N x n_obs] column-major; pim null: real observables
    int N, Np, c, cp, n_dir, save, n_slots, n_groups, prow, n_obs;
    int total;                  // tiles: column groups x slots x directions
};

// element (r, k) of plane p of observable j's Hermitian part: p = 0 As, p = 1 Ba
__device__ __forceinline__ double herm_part(const PushArgs &a, int j, int p, int r, int k)
{
    const size_t NN = (size_t)a.N * a.N, e = (size_t)r + (size_t)a.N * k, et = (size_t)k + (size_t)a.N * r;
    return p ? 0.5 * (a.pim[j * NN + e] - a.pim[j * NN + et]) : 0.5 * (a.pre[j * NN + e] + a.pre[j * NN + et]);
}

template <bool STAGED>
__global__ __launch_bounds__(256) void k_pushforward_outputs(PushArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = t >> 2, pr = t & 3;
    const int N = a.N, G = a.n_groups, ngrp = a.cp >> 3, npl = a.pim ? 2 : 1;
    double *td = lds;                          // [Np][16]: the tangent tile
    double *pt = td + 16 * (size_t)a.Np;       // [N][8]: pop_dot of the tile (with a map)
    double *red = pt + 8 * (size_t)N;          // [4][8]: the waves' sums of one observable
    double *ml = red + 32;                     // [n_groups x N]
    double *pl = ml + (size_t)G * N;           // [n_obs][npl][N (k)][N (r)]
    if (STAGED) {
        for (int i = t; i < G * N; i += 256) ml[i] = a.map[i];
        const size_t cnt = a.expect ? (size_t)a.n_obs * npl * N * N : 0;
        for (size_t i = t; i < cnt; i += 256) {
            const int rr = (int)(i % N), k = (int)((i / N) % N);
            const size_t jp = i / ((size_t)N * N);
            pl[i] = herm_part(a, (int)(jp / npl), (int)(jp % npl), rr, k);
        }
    }
    const double *M = STAGED ? ml : a.map;
    const size_t PWc = 2 * (size_t)a.cp, PWs = PWc * a.n_dir;
    for (int tl = blockIdx.x; tl < a.total; tl += gridDim.x) {
        const int g = tl % ngrp, s = (tl / ngrp) % a.n_slots, j = tl / (ngrp * a.n_slots);
        double *po = a.pop ? a.pop + ((size_t)j * a.c * a.n_slots + s) * a.prow : nullptr;      // + col * n_slots * prow
        double *eo = a.expect ? a.expect + ((size_t)j * a.c * a.n_slots + s) * a.n_obs : nullptr;
        const size_t pcol = (size_t)a.n_slots * a.prow, ecol = (size_t)a.n_slots * a.n_obs;
        if (s == 0) {      // the initial state does not depend on pcof
            for (int o = t; po && o < 8 * a.prow; o += 256) {
                const int cc = o / a.prow, col = 8 * g + cc;
                if (col < a.c) po[col * pcol + (o - cc * a.prow)] = 0.0;
            }
            for (int o = t; eo && o < 8 * a.n_obs; o += 256) {
                const int cc = o / a.n_obs, col = 8 * g + cc;
                if (col < a.c) eo[col * ecol + (o - cc * a.n_obs)] = 0.0;
            }
            continue;
        }
        const size_t n = (size_t)s * a.save;
        const int col = 8 * g + 2 * pr;
        d2 u = (d2){0.0, 0.0}, v = u, du = u, dv = u;
        if (r < N) {      // (rows N .. Np-1 are padding: whatever the panels hold there never enters a sum)
            const double *hp = a.hist + n * a.Np * PWc + (size_t)r * PWc + 16 * g + 2 * pr;
            const double *sp = a.sv + n * a.Np * PWs + (size_t)r * PWs + 16 * ((size_t)j * ngrp + g) + 2 * pr;
            u = *reinterpret_cast<const d2 *>(hp); v = *reinterpret_cast<const d2 *>(hp + 8);
            du = *reinterpret_cast<const d2 *>(sp); dv = *reinterpret_cast<const d2 *>(sp + 8);
        }
        if (po) {
            d2 p;
            p.x = 2.0 * fma(u.x, du.x, v.x * dv.x);
            p.y = 2.0 * fma(u.y, du.y, v.y * dv.y);
            if (G > 0) {
                if (r < N) *reinterpret_cast<d2 *>(pt + 8 * r + 2 * pr) = p;
            } else if (r < N && col < a.c) {
                po[col * pcol + r] = p.x;
                if (col + 1 < a.c) po[(col + 1) * pcol + r] = p.y;
            }
        }
        if (eo && r < a.Np) {
            *reinterpret_cast<d2 *>(td + 16 * r + 2 * pr) = du;
            *reinterpret_cast<d2 *>(td + 16 * r + 8 + 2 * pr) = dv;
        }
        __syncthreads();
        if (po && G > 0)
            for (int o = t; o < 8 * G; o += 256) {
                const int cc = o / G, gi = o - cc * G, cl = 8 * g + cc;
                if (cl >= a.c) continue;
                double acc = 0.0;
                for (int k = 0; k < N; k++) acc = fma(M[gi + (size_t)G * k], pt[8 * k + cc], acc);
                po[cl * pcol + gi] = acc;
            }
        for (int jo = 0; eo && jo < a.n_obs; jo++) {
            d2 e = (d2){0.0, 0.0};
            if (r < N) {
                d2 X = (d2){0.0, 0.0}, Y = X;      // H dpsi of row r: real and imaginary part
                const double *ps = pl + (size_t)jo * npl * N * N + r;
                for (int k = 0; k < N; k++) {
                    const d2 xu = *reinterpret_cast<const d2 *>(td + 16 * k + 2 * pr), xv = *reinterpret_cast<const d2 *>(td + 16 * k + 8 + 2 * pr);
                    const double as = STAGED ? ps[(size_t)k * N] : herm_part(a, jo, 0, r, k);
                    X.x = fma(as, xu.x, X.x); X.y = fma(as, xu.y, X.y);
                    Y.x = fma(as, xv.x, Y.x); Y.y = fma(as, xv.y, Y.y);
                    if (a.pim) {
                        const double ba = STAGED ? ps[(size_t)(N + k) * N] : herm_part(a, jo, 1, r, k);
                        X.x = fma(-ba, xv.x, X.x); X.y = fma(-ba, xv.y, X.y);
                        Y.x = fma(ba, xu.x, Y.x); Y.y = fma(ba, xu.y, Y.y);
                    }
                }
                e.x = fma(u.x, X.x, v.x * Y.x);
                e.y = fma(u.y, X.y, v.y * Y.y);
            }
            #pragma unroll
            for (int o = 4; o < 64; o <<= 1) { e.x += __shfl_xor(e.x, o); e.y += __shfl_xor(e.y, o); }      // (a fixed butterfly over the wave's 16 rows)
            if (lane < 4) { red[8 * wave + 2 * lane] = e.x; red[8 * wave + 2 * lane + 1] = e.y; }
            __syncthreads();
            if (t < 8 && 8 * g + t < a.c)
                eo[(8 * g + t) * ecol + jo] = 2.0 * (((red[t] + red[8 + t]) + red[16 + t]) + red[24 + t]);
            __syncthreads();
        }
        __syncthreads();      // (the next tile overwrites td and pt)
    }
}

extern "C" int qgdk_pushforward_outputs(const qgdk_ctx *c, const double *sv, int n_dir, int save, double *pop, const double *map_dev, int n_groups,
                                        double *expect, const double *obs_re, const double *obs_im, int n_obs)
{
    if (!pop && !expect) return 0;
    if (c->N > 64 || c->Np > 64 || save < 1 || n_dir < 1 || (pop && map_dev && n_groups < 1) || (expect && (!obs_re || n_obs < 1 || n_obs > 0x00ffffff)))
        return (int)hipErrorInvalidValue;      // (one panel row per thread)
    PushArgs a;
    a.hist = c->hist; a.sv = sv; a.pop = pop; a.expect = expect; a.map = pop ? map_dev : nullptr;
    a.pre = expect ? obs_re : nullptr; a.pim = expect ? obs_im : nullptr;
    a.N = c->N; a.Np = c->Np; a.c = c->c; a.cp = c->cp; a.n_dir = n_dir; a.save = save; a.n_slots = 1 + (c->nt - 1) / save;
    a.n_groups = a.map ? n_groups : 0; a.prow = a.map ? n_groups : c->N; a.n_obs = expect ? n_obs : 0;
    const long long total = (long long)(c->cp / 8) * a.n_slots * n_dir;
    if (total > 0x7fffffffLL || (long long)a.n_groups * c->N > 0x0fffffffLL) return (int)hipErrorInvalidValue;
    a.total = (int)total;
    const size_t lds_max = 160 * 1024;      // LDS of a gfx950 CU, all of which one workgroup may take
    const size_t tile_bytes = (16 * (size_t)c->Np + 8 * (size_t)c->N + 32) * sizeof(double);      // (at most 12.3 KB)
    const size_t staged_bytes = ((size_t)a.n_groups * c->N + (size_t)a.n_obs * (a.pim ? 2 : 1) * c->N * c->N) * sizeof(double);
    if (staged_bytes && tile_bytes + staged_bytes <= lds_max && !qgd_path("planes_l2")) {      // (QGD_PATHS=planes_l2: the route of a call that does not fit)
        const size_t bytes = tile_bytes + staged_bytes;
        const int per_cu = (int)(lds_max / bytes), grid_max = 256 * (per_cu < 8 ? per_cu : 8);
        if (bytes > 64 * 1024) SET_LDS_ONCE(k_pushforward_outputs<true>, bytes);
        hipLaunchKernelGGL(k_pushforward_outputs<true>, dim3(a.total < grid_max ? a.total : grid_max), dim3(256), bytes, c->stream, a);
    } else {
        const int grid_max = staged_bytes ? 2048 : (1 << 20);      // (nothing to stage: one tile per workgroup)
        hipLaunchKernelGGL(k_pushforward_outputs<false>, dim3(a.total < grid_max ? a.total : grid_max), dim3(256), tile_bytes, c->stream, a);
    }
    return (int)hipGetLastError();
}
