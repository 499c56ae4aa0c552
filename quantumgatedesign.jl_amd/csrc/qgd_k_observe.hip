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
