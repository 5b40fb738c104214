// Dense inverse-Hessian BFGS (scipy's fmin_bfgs restated, bioen_amd/bfgs.py) on gfx950: H lives in HBM as ld x ld FP64,
// row-major, ld = round_up(n, 16); pad rows and columns are zero and stay zero.
//
// The update  H' = H - rho (s u^T + u s^T) + c s s^T,  u = H y,  c = rho^2 y.u + rho  is applied LAZILY: the pass of
// iteration k reads H_{k-1}, applies the pending rank-2 update of step k-1 in registers, writes H_k in place (each
// element read and written by the same lane) and forms the row sums H_k [y_k, g_{k+1}] in the same sweep -- one read
// and one write of ld^2 doubles per iteration.  The first pass synthesises H_0 = I instead of reading it.
//
// Geometry.  A block owns kHRows = 16 whole rows (no second reduction stage).  Its 256 lanes walk the columns in
// 16-byte pairs; for each pair a lane loads the four column vectors (s, u, y, g) ONCE and then streams its 16 rows --
// 16 independent 16-byte loads in flight per lane, a wave reading 1 KiB contiguous per row.  The column vectors are
// re-read once per block from L2 / Infinity Cache: 4 x 8 B per column against 16 rows x 2 x 8 B of H, i.e. 1/8 of the
// H bytes.  Per lane: 32 FP64 accumulators (64 VGPRs) + 16 H pairs (64 VGPRs) + the column operands.
//
// Symmetry.  The element update is written without contraction, h - rho ((s_i u_j) + (u_i s_j)) + c (s_i s_j), so that
// (i, j) and (j, i) round identically and H stays exactly symmetric.  The row sums use FMA in a fixed order (lane walk,
// then wave_multi_reduce, then the four waves in index order): two runs give identical bits.
#include "device_utils.hpp"

namespace bioen {

constexpr int kHRows = 16;

__device__ __forceinline__ double bfgs_elem(double h, double si, double ui, double sj, double uj, double rho, double cc) {
#pragma clang fp contract(off)
    return (h - rho * ((si * uj) + (ui * sj))) + cc * (si * sj);
}

// H (ld x ld) <- H with the pending update (s, u, rho, cc); hy = H y, hg = H g (rows of this block).
// first: H_{k-1} = I (rows < n), not read.
__global__ __launch_bounds__(kBlock) void k_bfgs_hpass(double* __restrict__ H, size_t ld, int n, int first,
                                                       const double* __restrict__ s, const double* __restrict__ u,
                                                       double rho, double cc, const double* __restrict__ y,
                                                       const double* __restrict__ g, double* __restrict__ hy,
                                                       double* __restrict__ hg) {
    __shared__ double sh[kWaves][2 * kHRows];
    const size_t i0 = (size_t)blockIdx.x * kHRows;
    double si[kHRows], ui[kHRows];
#pragma unroll
    for (int r = 0; r < kHRows; ++r) {
        si[r] = s[i0 + r];
        ui[r] = u[i0 + r];
    }
    double acc[2 * kHRows];
#pragma unroll
    for (int q = 0; q < 2 * kHRows; ++q) acc[q] = 0.0;
    const size_t np = ld / 2;
    for (size_t jp = threadIdx.x; jp < np; jp += kBlock) {
        const size_t j = 2 * jp;
        const d2 sj = *reinterpret_cast<const d2*>(s + j);
        const d2 uj = *reinterpret_cast<const d2*>(u + j);
        const d2 yj = *reinterpret_cast<const d2*>(y + j);
        const d2 gj = *reinterpret_cast<const d2*>(g + j);
        d2 h[kHRows];
        if (!first) {
#pragma unroll
            for (int r = 0; r < kHRows; ++r) h[r] = *reinterpret_cast<const d2*>(H + (i0 + r) * ld + j);
        } else {
#pragma unroll
            for (int r = 0; r < kHRows; ++r) {
                const size_t i = i0 + r;
                h[r].x = (i == j && i < (size_t)n) ? 1.0 : 0.0;
                h[r].y = (i == j + 1 && i < (size_t)n) ? 1.0 : 0.0;
            }
        }
#pragma unroll
        for (int r = 0; r < kHRows; ++r) {
            d2 o;
            o.x = bfgs_elem(h[r].x, si[r], ui[r], sj.x, uj.x, rho, cc);
            o.y = bfgs_elem(h[r].y, si[r], ui[r], sj.y, uj.y, rho, cc);
            *reinterpret_cast<d2*>(H + (i0 + r) * ld + j) = o;
            acc[r] = fma(o.x, yj.x, acc[r]);
            acc[r] = fma(o.y, yj.y, acc[r]);
            acc[kHRows + r] = fma(o.x, gj.x, acc[kHRows + r]);
            acc[kHRows + r] = fma(o.y, gj.y, acc[kHRows + r]);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wave_multi_reduce<2 * kHRows>(acc, lane);          // lane l: the total of accumulator l >> 1 in acc[0]
    if ((lane & 1) == 0) sh[wave][lane >> 1] = acc[0];
    __syncthreads();
    if (threadIdx.x < 2 * kHRows) {
        const int q = threadIdx.x;
        const double t = (sh[0][q] + sh[1][q]) + (sh[2][q] + sh[3][q]);
        if (q < kHRows) hy[i0 + q] = t;
        else hg[i0 + q - kHRows] = t;
    }
}

// rows [row0, row0 + rows) of H with the pending update applied, into out (rows x ld): what the next pass would write
__global__ __launch_bounds__(kBlock) void k_bfgs_hread(const double* __restrict__ H, size_t ld, int n, int first,
                                                       const double* __restrict__ s, const double* __restrict__ u,
                                                       double rho, double cc, size_t row0, double* __restrict__ out) {
    const size_t i = row0 + blockIdx.x;
    const double si = s[i], ui = u[i];
    for (size_t j = threadIdx.x; j < ld; j += kBlock) {
        const double h = first ? ((i == j && i < (size_t)n) ? 1.0 : 0.0) : H[i * ld + j];
        out[(size_t)blockIdx.x * ld + j] = bfgs_elem(h, si, ui, s[j], u[j], rho, cc);
    }
}

// the next direction from the identity  H_{k+1} g = H_k g - rho s (u.g) - rho u (s.g) + c s (s.g):
//   p = -(((hg - a1 s) - a2 u) + a3 s),  a1 = rho u.g, a2 = rho s.g, a3 = c s.g ;  block partials of g.p and p.p
__global__ __launch_bounds__(kBlock) void k_bfgs_dir(const double* __restrict__ hg, const double* __restrict__ s,
                                                     const double* __restrict__ u, double a1, double a2, double a3,
                                                     const double* __restrict__ g, double* __restrict__ p, int n,
                                                     Xch xo) {
#pragma clang fp contract(off)
    __shared__ double sh[kWaves];
    double gp = 0.0, pp = 0.0;
    const SegPos sp = seg_pos(xo.npl, xo.segcols, n);
    for (int j = seg_first(sp); j < sp.jend; j += seg_step(xo.npl)) {
        const d2 hv = *reinterpret_cast<const d2*>(hg + j);
        const d2 sv = *reinterpret_cast<const d2*>(s + j);
        const d2 uv = *reinterpret_cast<const d2*>(u + j);
        const d2 gv = *reinterpret_cast<const d2*>(g + j);
        d2 o;
        o.x = -(((hv.x - a1 * sv.x) - a2 * uv.x) + a3 * sv.x);
        o.y = -(((hv.y - a1 * sv.y) - a2 * uv.y) + a3 * sv.y);
        *reinterpret_cast<d2*>(p + j) = o;
        gp = fma(gv.x, o.x, gp);
        gp = fma(gv.y, o.y, gp);
        pp = fma(o.x, o.x, pp);
        pp = fma(o.y, o.y, pp);
    }
    gp = block_sum(gp, sh);
    pp = block_sum(pp, sh);
    if (threadIdx.x == 0) {
        xput<4>(xo, 0, 0, gp);
        xput<4>(xo, 0, 1, pp);
    }
}

// y = a - b over ld doubles (pads: 0 - 0)
__global__ __launch_bounds__(kBlock) void k_bfgs_sub(const double* __restrict__ a, const double* __restrict__ b,
                                                     double* __restrict__ y, int n2) {
    for (int q = blockIdx.x * kBlock + threadIdx.x; q < n2; q += gridDim.x * kBlock) {
        const d2 av = *reinterpret_cast<const d2*>(a + 2 * q);
        const d2 bv = *reinterpret_cast<const d2*>(b + 2 * q);
        const d2 o = {av.x - bv.x, av.y - bv.y};
        *reinterpret_cast<d2*>(y + 2 * q) = o;
    }
}

size_t bfgs_ld(int n) { return round_up((size_t)n, kHRows); }

void launch_bfgs_hpass(bioen_hip_ctx* c, double* H, size_t ld, bool first, const double* s, const double* u, double rho,
                       double cc, const double* y, const double* g, double* hy, double* hg) {
    hipLaunchKernelGGL(k_bfgs_hpass, dim3((unsigned)(ld / kHRows)), dim3(kBlock), 0, c->stream, H, ld, c->n, first ? 1 : 0,
                       s, u, rho, cc, y, g, hy, hg);
}

void launch_bfgs_hread(bioen_hip_ctx* c, const double* H, size_t ld, bool first, const double* s, const double* u,
                       double rho, double cc, size_t row0, int rows, double* out) {
    hipLaunchKernelGGL(k_bfgs_hread, dim3((unsigned)rows), dim3(kBlock), 0, c->stream, H, ld, c->n, first ? 1 : 0, s, u,
                       rho, cc, row0, out);
}

void launch_bfgs_dir(bioen_hip_ctx* c, const double* hg, const double* s, const double* u, double a1, double a2,
                     double a3, const double* g, double* p) {      // [exchange X_GRAD, 4 * vec_grid per segment]
    hipLaunchKernelGGL(k_bfgs_dir, dim3(vec_blocks(c)), dim3(kBlock), 0, c->stream, hg, s, u, a1, a2, a3, g, p, c->n,
                       make_xch(c, X_GRAD, 4 * vec_grid(c)));
}

void launch_bfgs_sub(bioen_hip_ctx* c, const double* a, const double* b, double* y) {
    const int n2 = (int)(c->ld / 2);
    const int grid = std::max(1, std::min(1024, (n2 + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(k_bfgs_sub, dim3(grid), dim3(kBlock), 0, c->stream, a, b, y, n2);
}

}  // namespace bioen
