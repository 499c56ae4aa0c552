// qgd_k_interp.hip -- Hermite dense output: the state between the grid points, from what the sweep already holds.
//
// At every time point the device keeps the state w_0 (hist) and, once k_derivs ran, the m = order/2 scaled Taylor coefficients
// w_j = w^(j)/j! (dpsi).  The two-point Hermite interpolant of degree 2m+1 through the m+1 coefficients at
// both ends of step n (t_n .. t_n + dt) is, at t_n + theta dt with theta = s/r, s = 1 .. r-1,
//   w(theta) = sum_{j=0..m} dt^j [ A_j(theta) w_j(t_n) + (-1)^j A_j(1-theta) w_j(t_{n+1}) ]
//   A_j(theta) = theta^j (1-theta)^(m+1) sum_{k=0..m-j} C(m+k, k) theta^k
// with a local error O(dt^(2m+2)): the order of the method itself.  The 2 (m+1) (r-1) weights, dt^j and
// the sign folded in, are formed on the host in double precision (qgd_host_output.cpp: dense_weights) and read here through
// wave-uniform loads.
//
// Input: the state panels hist [nt][Np][2cp] and the stage derivatives dpsi [nt][m][Np][2cp].  Output: panels
// [1 + (nt-1) r][Np][2cp] in the same layout (qgd_kernels_common.h), slot n r + s at time (n + s/r) dt -- what qgdk_layout,
// qgdk_populations and qgdk_expectations take through their (src, stride, count) arguments.  Slot n r is the grid point n,
// copied, not evaluated.  Padding rows (N .. Np) and padding columns (c .. cp) of the output are written as zeros on every call.
//
// One workgroup per (step, column group of 8) tile, grid-stride over the tiles.  A thread owns 16-byte pairs of the tile (two
// real or two imaginary parts of two neighbouring columns of one row): it loads its pair of the 2 (m+1) input panels once --
// 18 double2 = 72 VGPRs at m = 8 -- and emits the left grid panel and the r-1 interior panels from registers; the tile of the
// last step also copies the last grid point.  Rows beyond the 32 that 256 threads cover are further passes of the same loop,
// so the kernel does not depend on N <= 64.  Every sum runs over ascending j, left end before right end: no atomics, the same
// bits on every run.  All stores are ordinary 16-byte vector stores.  Memory-bound: per tile 2 (m+1) panel tiles read (half of
// them shared with the neighbouring step through L2) and r written.
#include "qgd_kernels_common.h"

typedef double d2 __attribute__((ext_vector_type(2)));

struct InterpArgs {
    const double *hist;         // [nt][Np][2cp]
    const double *dpsi;         // [nt][m][Np][2cp]
    double *out;                // [1 + (nt-1) r][Np][2cp]
    const double *w;            // [r-1][m+1][2]: dt^j A_j(s/r), (-dt)^j A_j(1 - s/r)
    int N, Np, c, cp, nt, r;
    int total;                  // (step, column group) tiles
};

template <int M>
__global__ __launch_bounds__(256) void k_interp(InterpArgs a)
{
    const int t = threadIdx.x;
    const int ngrp = a.cp >> 3, PWc = 2 * a.cp;
    const size_t hstep = (size_t)a.Np * PWc;
    const double *__restrict__ w = a.w;
    for (int tl = blockIdx.x; tl < a.total; tl += gridDim.x) {
        const int g = tl % ngrp, n = tl / ngrp;
        const double *hl = a.hist + (size_t)n * hstep, *dl = a.dpsi + (size_t)n * M * hstep;
        double *op = a.out + (size_t)n * a.r * hstep;
        for (int idx = t; idx < 8 * a.Np; idx += 256) {
            const int row = idx >> 3, q = idx & 7, col = 8 * g + 2 * (q & 3);
            const size_t off = (size_t)row * PWc + 16 * g + 2 * q;
            const bool live = row < a.N && col < a.c;
            d2 wl[M + 1], wr[M + 1];
            #pragma unroll
            for (int j = 0; j <= M; j++) { wl[j] = (d2){0.0, 0.0}; wr[j] = (d2){0.0, 0.0}; }
            if (live) {      // (a padding row or column pair: zeros by selection, nothing is read)
                wl[0] = *reinterpret_cast<const d2 *>(hl + off);
                wr[0] = *reinterpret_cast<const d2 *>(hl + hstep + off);
                #pragma unroll
                for (int j = 1; j <= M; j++) {
                    wl[j] = *reinterpret_cast<const d2 *>(dl + (size_t)(j - 1) * hstep + off);
                    wr[j] = *reinterpret_cast<const d2 *>(dl + (size_t)(M + j - 1) * hstep + off);
                }
                if (col + 1 >= a.c) {
                    #pragma unroll
                    for (int j = 0; j <= M; j++) { wl[j].y = 0.0; wr[j].y = 0.0; }
                }
            }
            *reinterpret_cast<d2 *>(op + off) = wl[0];
            for (int s = 1; s < a.r; s++) {
                const double *ws = w + (size_t)(s - 1) * 2 * (M + 1);
                d2 acc = (d2){0.0, 0.0};
                #pragma unroll
                for (int j = 0; j <= M; j++) {
                    const double wa = ws[2 * j], wb = ws[2 * j + 1];
                    acc.x = fma(wa, wl[j].x, acc.x); acc.y = fma(wa, wl[j].y, acc.y);
                    acc.x = fma(wb, wr[j].x, acc.x); acc.y = fma(wb, wr[j].y, acc.y);
                }
                *reinterpret_cast<d2 *>(op + (size_t)s * hstep + off) = acc;
            }
            if (n == a.nt - 2) *reinterpret_cast<d2 *>(op + (size_t)a.r * hstep + off) = wr[0];
        }
    }
}

// hist, dpsi of c's nt time points -> out [1 + (nt-1) refine] panels; w_dev: the weight table [refine-1][m+1][2]
extern "C" int qgdk_interp(const qgdk_ctx *c, const double *hist, const double *dpsi, double *out, int refine,
                           const double *w_dev, hipStream_t stream)
{
    if (c->nt < 2 || refine < 1 || c->m < 1 || c->m > 8) return (int)hipErrorInvalidValue;
    const long long total = (long long)(c->nt - 1) * (c->cp / 8);
    if (total > 0x7fffffffLL || (long long)(c->nt - 1) * refine + 1 > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    InterpArgs a;
    a.hist = hist; a.dpsi = dpsi; a.out = out; a.w = w_dev;
    a.N = c->N; a.Np = c->Np; a.c = c->c; a.cp = c->cp; a.nt = c->nt; a.r = refine; a.total = (int)total;
    const int grid = a.total < 2048 ? a.total : 2048;
#define LAUNCH_INTERP(M) hipLaunchKernelGGL(k_interp<M>, dim3(grid), dim3(256), 0, stream, a)
    switch (c->m) {
    case 1: LAUNCH_INTERP(1); break; case 2: LAUNCH_INTERP(2); break; case 3: LAUNCH_INTERP(3); break; case 4: LAUNCH_INTERP(4); break;
    case 5: LAUNCH_INTERP(5); break; case 6: LAUNCH_INTERP(6); break; case 7: LAUNCH_INTERP(7); break; default: LAUNCH_INTERP(8); break;
    }
#undef LAUNCH_INTERP
    return (int)hipGetLastError();
}
