// qgd_k_observe.hip -- level populations of the state history, formed on the device.
//
// The reference's get_populations (src/state_vector_helpers.jl:10-52) turns uv_history[2N, 1+m, nt, c] into
//   p[k, n, col] = u_k^2 + v_k^2                       [N, nt, c]   (Julia order)
// on the host, after the whole history came down.  Here the panels of the state history [n][Np][2cp]
// (qgd_kernels_common.h: row r of column group g holds 8 real parts and then the 8 imaginary parts of the same 8
// complex columns) are reduced where they are, and only p -- or, with a level map M[n_groups x N], the contraction
//   P[g, n, col] = sum_k M[g, k] p[k, n, col]          [n_groups, nt, c]
// -- is staged and downloaded: a (1+m)-th to a fiftieth of the bytes of uv_history, and no stage derivatives.
// Both kernels stream the panels once with 16-byte loads and are bound by HBM (16 N c bytes read per time point).
//
// Expectation values of observables that are not diagonal in the level basis (qgd_eval_expectations, no counterpart in the
// reference) come from the same panels:  E[j, n, col] = Re(psi^H O_j psi),  psi = u + iv,  O_j = A + iB,
//   = u^T A u + v^T A v + v^T B u - u^T B v
// with the products [A u | A v] and [B u | B v] on the f64 MFMA (k_expectations below).
#include "qgd_kernels_common.h"

typedef double d2 __attribute__((ext_vector_type(2)));

struct ObserveArgs {
    const double *src;          // panels of the first output slot
    double *dst;                // [rows, n_cnt, c]: rows = N, or n_groups with a map
    const double *map;          // [n_groups x N] column-major, or null
    long long src_n;            // doubles between the panels of two consecutive output slots (save_every * Np * 2cp)
    long long dst_col, dst_n;   // output strides (doubles) per column and per slot
    int N, c, cp, n_cnt, n_groups;
    int tiles_x, total;         // tiles per slot; tiles_x * n_cnt
};

// One thread per (row, pair of complex columns): the two real parts and, 64 bytes further in the same 128-byte row
// segment, the two imaginary parts -- a wave reads 16 whole row segments with its two loads and writes, per column, a
// run of 16 consecutive doubles along k (one 128-byte line); the four waves of a workgroup cover 64 consecutive rows.
// Nothing is exchanged between threads, so there is no LDS.  Nothing of a padding row or column reaches the output.
__global__ __launch_bounds__(256) void k_populations(ObserveArgs a)
{
    const int t = threadIdx.x, rl = t >> 2, pr = t & 3;
    const int ngrp = a.cp >> 3;
    const int bx = blockIdx.x % a.tiles_x, s = blockIdx.x / a.tiles_x;
    const int g = bx % ngrp, r = (bx / ngrp) * 64 + rl;
    const int col = 8 * g + 2 * pr;
    if (r >= a.N || col >= a.c) return;
    const double *row = a.src + (size_t)s * a.src_n + (size_t)r * (2 * a.cp) + 16 * g + 2 * pr;
    const d2 u = *reinterpret_cast<const d2 *>(row), v = *reinterpret_cast<const d2 *>(row + 8);
    double *dp = a.dst + (size_t)s * a.dst_n + (size_t)col * a.dst_col + r;
    dp[0] = fma(u.x, u.x, v.x * v.x);
    if (col + 1 < a.c) dp[a.dst_col] = fma(u.y, u.y, v.y * v.y);
}

// One (slot, column group) at a time per workgroup: the populations of its N x 8 elements are formed once, into LDS,
// and thread (group gi, column cc) then adds M[gi, k] p[k, cc] up over k = 0 .. N-1 in that order -- no atomics, the
// same bits on every run.  The map sits in LDS behind the populations when both fit in 64 KB (MAP_LDS), else it is read
// from global memory (L2) as it is.  A workgroup walks several tiles, so the map is staged once per workgroup.
template <bool MAP_LDS>
__global__ __launch_bounds__(256) void k_populations_grouped(ObserveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *pt = lds;                     // [N][8]
    double *ml = lds + 8 * (size_t)a.N;   // [n_groups x N]
    const int t = threadIdx.x;
    const int ngrp = a.cp >> 3, G = a.n_groups;
    if (MAP_LDS)
        for (int i = t; i < G * a.N; i += 256) ml[i] = a.map[i];
    const double *M = MAP_LDS ? ml : a.map;
    for (int tl = blockIdx.x; tl < a.total; tl += gridDim.x) {
        const int g = tl % ngrp, s = tl / ngrp;
        const double *sp = a.src + (size_t)s * a.src_n + 16 * g;
        for (int idx = t; idx < 4 * a.N; idx += 256) {
            const int r = idx >> 2, pr = idx & 3;
            const double *row = sp + (size_t)r * (2 * a.cp) + 2 * pr;
            const d2 u = *reinterpret_cast<const d2 *>(row), v = *reinterpret_cast<const d2 *>(row + 8);
            d2 p;
            p.x = fma(u.x, u.x, v.x * v.x);
            p.y = fma(u.y, u.y, v.y * v.y);
            *reinterpret_cast<d2 *>(pt + 8 * r + 2 * pr) = p;
        }
        __syncthreads();
        double *dp = a.dst + (size_t)s * a.dst_n;
        for (int o = t; o < 8 * G; o += 256) {
            const int cc = o / G, gi = o - cc * G;
            const int col = 8 * g + cc;
            if (col >= a.c) continue;
            double acc = 0.0;
            for (int k = 0; k < a.N; k++) acc = fma(M[gi + (size_t)G * k], pt[8 * k + cc], acc);
            dp[(size_t)col * a.dst_col + gi] = acc;
        }
        __syncthreads();
    }
}

// panels of n_cnt output slots, src_n doubles apart -> out[col][slot][rows] with rows = N (map_dev null: populations)
// or n_groups (level map on the device)
extern "C" int qgdk_populations(const qgdk_ctx *c, const double *panels, long long src_n, double *out, long long dst_col,
                                long long dst_n, int n_cnt, const double *map_dev, int n_groups, hipStream_t stream)
{
    if (n_cnt <= 0) return 0;
    ObserveArgs a;
    a.src = panels; a.dst = out; a.map = map_dev; a.src_n = src_n; a.dst_col = dst_col; a.dst_n = dst_n;
    a.N = c->N; a.c = c->c; a.cp = c->cp; a.n_cnt = n_cnt; a.n_groups = map_dev ? n_groups : 0;
    a.tiles_x = (map_dev ? 1 : (c->N + 63) / 64) * (c->cp / 8);
    const long long total = (long long)a.tiles_x * n_cnt;
    if (total > 0x7fffffffLL || (map_dev && ((long long)n_groups * c->N > 0x7fffffffLL || n_groups > 0x0fffffff))) return (int)hipErrorInvalidValue;
    a.total = (int)total;
    if (!map_dev) {
        hipLaunchKernelGGL(k_populations, dim3(a.total), dim3(256), 0, stream, a);
        return (int)hipGetLastError();
    }
    const size_t pt_bytes = 8 * (size_t)c->N * sizeof(double), map_bytes = (size_t)n_groups * c->N * sizeof(double);
    if (pt_bytes > 64 * 1024) return (int)hipErrorInvalidValue;      // (N <= 592: 37 KB)
    const int grid = a.total < 2048 ? a.total : 2048;
    if (pt_bytes + map_bytes <= 64 * 1024)
        hipLaunchKernelGGL(k_populations_grouped<true>, dim3(grid), dim3(256), pt_bytes + map_bytes, stream, a);
    else
        hipLaunchKernelGGL(k_populations_grouped<false>, dim3(grid), dim3(256), pt_bytes, stream, a);
    return (int)hipGetLastError();
}


struct ExpectArgs {
    const double *src;          // panels of the first output slot
    double *dst;                // [n_obs, n_cnt, c]
    const double *pre, *pim;    // [N x N x n_obs] column-major: the planes A and B of O_j = A + iB; pim null: real observables
    long long src_n;            // doubles between the panels of two consecutive output slots
    long long dst_col, dst_n;   // output strides (doubles) per column and per slot
    int N, c, cp, n_obs;
    int nrb, nks;               // row blocks of 16 and k-steps of 4 that cover N
    int jb;                     // observables per round of the cross-block sum (sizes its LDS)
    int total;                  // (slot, column group) tiles
};

// One (slot, column group) tile at a time per workgroup.  The tile's 16-double rows are an MFMA B operand as they lie: rows
// 4 ks .. 4 ks + 3 are the 4 x 16 matrix [u | v] of k-step ks, and with a 16 x 4 tile of the plane A as the A operand the
// accumulator of row block rb ends as the 16 x 16 block [A u | A v] (lane (c16, kk), register r: row 16 rb + kk + 4 r,
// column c16).  Multiplied by the same element of the tile that is u^T A u (c16 < 8) or v^T A v (c16 >= 8) of one column; with
// the plane B and the tile's other half, +v^T B u or -u^T B v.  Plain products and sums: no three-product form.
//   The tile goes to LDS once, with its padding rows (N .. ) and padding columns (c .. ) set to zero by selection -- whatever
// the panels hold there never enters a product -- and serves all observables.  The planes are staged once per workgroup in
// fragment order (64 consecutive doubles per (row block, k-step), zero beyond N: conflict-free reads) when they fit beside the
// tile (PLANES_LDS); else every fragment is read from global memory (L2) with the same zero rule.
//   Order of the sums, the same on every run and for every n_obs: four fused multiply-adds per lane and plane; A part + B part;
// the four kk lanes, then the u and the v half (wave shuffles, each pair added once); the row blocks in ascending order by one
// thread per (observable, column) from LDS.  A (observable, row block) pair is one wave's work, whatever the batch holds.
template <bool PLANES_LDS>
__global__ __launch_bounds__(256) void k_expectations(ExpectArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, c16 = lane & 15, kk = lane >> 4;
    const int N = a.N, nrb = a.nrb, nks = a.nks, ngrp = a.cp >> 3;
    const int npl = a.pim ? 2 : 1;
    const size_t frag = (size_t)nrb * nks * 64;      // doubles of one plane in fragment order
    double *pt = lds;                                // [16 nrb][16]
    double *red = pt + 256 * (size_t)nrb;            // [jb][nrb][8]
    double *pl = red + 8 * (size_t)a.jb * nrb;       // [n_obs][npl][nrb][nks][64]
    const size_t NN = (size_t)N * N;
    if (PLANES_LDS) {
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
        const int g = tl % ngrp, s = tl / ngrp;
        const double *sp = a.src + (size_t)s * a.src_n + 16 * g;
        for (int idx = t; idx < 128 * nrb; idx += 256) {
            const int r = idx >> 3, q = idx & 7, col = 8 * g + 2 * (q & 3);
            d2 x = (d2){0.0, 0.0};
            if (r < N && col < a.c) {
                x = *reinterpret_cast<const d2 *>(sp + (size_t)r * (2 * a.cp) + 2 * q);
                if (col + 1 >= a.c) x.y = 0.0;
            }
            *reinterpret_cast<d2 *>(pt + 16 * r + 2 * q) = x;
        }
        __syncthreads();
        for (int j0 = 0; j0 < a.n_obs; j0 += a.jb) {
            const int jn = (a.n_obs - j0 < a.jb) ? a.n_obs - j0 : a.jb;
            for (int w = wave; w < jn * nrb; w += 4) {
                const int jj = w / nrb, rb = w - jj * nrb, j = j0 + jj;
                const int row = 16 * rb + c16;
                d4 accA = (d4){0, 0, 0, 0}, accB = (d4){0, 0, 0, 0};
                const double *fa = pl + ((size_t)j * npl * nrb + rb) * nks * 64 + lane;      // plane A of j; plane B one `frag` further
                for (int ks = 0; ks < nks; ks++) {
                    const int k = 4 * ks + kk;
                    const double b = pt[16 * k + c16];
                    const bool in = row < N && k < N;
                    const double av = PLANES_LDS ? fa[(size_t)ks * 64] : (in ? a.pre[j * NN + row + (size_t)N * k] : 0.0);
                    accA = MFMA(av, b, accA);
                    if (a.pim) {
                        const double bv = PLANES_LDS ? fa[frag + (size_t)ks * 64] : (in ? a.pim[j * NN + row + (size_t)N * k] : 0.0);
                        accB = MFMA(bv, b, accB);
                    }
                }
                double pa = 0.0, pb = 0.0;
                #pragma unroll
                for (int r = 0; r < 4; r++) {
                    const double *prow = pt + 16 * (16 * rb + kk + 4 * r);
                    pa = fma(accA[r], prow[c16], pa);
                    if (a.pim) pb = fma(accB[r], prow[c16 ^ 8], pb);
                }
                double e = pa;
                if (a.pim) e += (c16 < 8) ? pb : -pb;
                e += __shfl_xor(e, 16);
                e += __shfl_xor(e, 32);
                e += __shfl_xor(e, 8);
                if (lane < 8) red[8 * w + lane] = e;
            }
            __syncthreads();
            double *dp = a.dst + (size_t)s * a.dst_n;
            for (int o = t; o < 8 * jn; o += 256) {
                const int cc = o / jn, jj = o - cc * jn;
                const int col = 8 * g + cc;
                if (col >= a.c) continue;
                const double *rp = red + 8 * (size_t)jj * nrb + cc;
                double e = rp[0];
                for (int rb = 1; rb < nrb; rb++) e += rp[8 * rb];
                dp[(size_t)col * a.dst_col + j0 + jj] = e;
            }
            __syncthreads();
        }
    }
}

// panels of n_cnt output slots, src_n doubles apart -> out[col][slot][n_obs]: Re(psi^H O_j psi) for the n_obs observables whose
// planes lie in obs_re / obs_im ([N x N x n_obs] column-major on the device; obs_im null: real symmetric observables)
extern "C" int qgdk_expectations(const qgdk_ctx *c, const double *panels, long long src_n, double *out, long long dst_col,
                                 long long dst_n, int n_cnt, const double *obs_re, const double *obs_im, int n_obs, hipStream_t stream)
{
    if (n_cnt <= 0) return 0;
    if (!obs_re || n_obs < 1 || n_obs > 0x0fffffff) return (int)hipErrorInvalidValue;
    ExpectArgs a;
    a.src = panels; a.dst = out; a.pre = obs_re; a.pim = obs_im; a.src_n = src_n; a.dst_col = dst_col; a.dst_n = dst_n;
    a.N = c->N; a.c = c->c; a.cp = c->cp; a.n_obs = n_obs;
    a.nrb = (c->N + 15) / 16; a.nks = (c->N + 3) / 4;
    a.jb = 256 / a.nrb < 1 ? 1 : 256 / a.nrb;
    if (a.jb > n_obs) a.jb = n_obs;
    const long long total = (long long)(c->cp / 8) * n_cnt;
    if (total > 0x7fffffffLL || (long long)a.jb * a.nrb > 0x0fffffff) return (int)hipErrorInvalidValue;
    a.total = (int)total;
    const size_t lds_max = 160 * 1024;      // LDS of a gfx950 CU, all of which one workgroup may take
    const size_t tile_bytes = (256 * (size_t)a.nrb + 8 * (size_t)a.jb * a.nrb) * sizeof(double);      // (N <= 592: 76 KB + 16 KB)
    if (tile_bytes > lds_max) return (int)hipErrorInvalidValue;
    const size_t plane_bytes = (size_t)n_obs * (obs_im ? 2 : 1) * a.nrb * a.nks * 64 * sizeof(double);
    if (tile_bytes + plane_bytes <= lds_max) {
        const size_t bytes = tile_bytes + plane_bytes;
        const int per_cu = (int)(lds_max / bytes), grid_max = 256 * (per_cu < 8 ? per_cu : 8);
        if (bytes > 64 * 1024) SET_LDS_ONCE(k_expectations<true>, bytes);
        hipLaunchKernelGGL(k_expectations<true>, dim3(a.total < grid_max ? a.total : grid_max), dim3(256), bytes, stream, a);
    } else {
        if (tile_bytes > 64 * 1024) SET_LDS_ONCE(k_expectations<false>, tile_bytes);
        hipLaunchKernelGGL(k_expectations<false>, dim3(a.total < 2048 ? a.total : 2048), dim3(256), tile_bytes, stream, a);
    }
    return (int)hipGetLastError();
}
