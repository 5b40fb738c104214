// Forces method, M <= 1024: the dense Hessian and the covariance of the observables at a kept point in ONE pass over the
// matrix (gfx950).  With Y' = Y - centre, w the point's weights, q_j - qbar what the point keeps (fpoint_q):
//   G'[u]  = sum_j u_j Y'_j Y'_j^T                       u1_j = w_j,   u2_j = w_j (q_j - qbar)
//   C      = G'[u1] - ybar' ybar'^T                      the covariance of the observables under the weights
//   G2     = G'[u2] - g ybar'^T - ybar' g^T              g = sum_j u2_j Y'_j, the point's unscaled gradient
//   H      = theta C + G2 + C C                          (affine model, S = diag(row_scale): C_A = S C S,
//                                                         H_A = S (theta C + G2) S + C_A C_A)
// The two M x M x N products share every operand: the FP64 matrix cores' only compute-bound kernel of this library.
//
// k_forces_gram reads the row-sum order strip copy (strip.hpp).  A wave's 64-row slice of a strip arrives as 8 chunks
// whose halves ARE operands of v_mfma_f64_16x16x4_f64 (row = lane & 15, k = lane >> 4) -- as A for its own row block and,
// the same registers of another slice, as B: G'_IJ += Y'_I diag(u) Y'_J^T with no transpose and no LDS image.  A wave owns
// a 64 x 64 sub-tile of BOTH matrices (2 x 16 accumulators of 4 doubles: 256 registers; one wave per SIMD), a block of
// four waves a 128 x 128 tile; only tile pairs I >= J are computed (in a diagonal tile the wave above the diagonal leaves).
// A SET is the accumulation chain from zero over the strips g, g + gs, ... of one canonical segment, in strip order; every
// (set, sub-tile) has exactly one writer; k_fgram_sum_sets adds the sets in the fixed order
//   sum over segments (in index order) of [ the segment's groups added in turn ]
// -- no floating-point atomics, and the shape of the sum is a function of (segcols, M) alone.
// The arguments, a wave's decode, its centres, the matrix fetch and the row sums' way out are fgram.hpp's: the BF16 pass
// (kernels_forces_gram_bf16.hip) runs the same ones.
#include "fgram.hpp"

namespace bioen {

struct FGramRegs {
    d2 a[kWaveRows / 8];
    d2 b[kWaveRows / 8];
    double w0[4], x[4], qv[4];       // the strip's columns 4 qq + (lane >> 4), qq = 0 .. 3
};

__global__ __launch_bounds__(256, 1) void k_forces_gram(FGramArgs q) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane >> 4, lr = lane & 15;
    FGramWave w;
    if (!fgram_decode(q, lane, wave, w)) return;
    const double logs = q.pscal[S_LOGS];
    double ca[4], cb[4];                            // the centres of the lane's rows
    fgram_centres(q, w, lr, ca, cb);

    auto fetch = [&](int i, FGramRegs& r) {
        const int s = fgram_strip(q, w, i);
        fgram_fetch(q, w, s, r.a, r.b);
        const size_t col = (size_t)s * kStripCols + lq;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            r.w0[qq] = q.w0[col + 4 * qq];
            r.x[qq] = q.x[col + 4 * qq];
            r.qv[qq] = q.qv[col + 4 * qq];
        }
    };

    d4 acc1[4][4], acc2[4][4];                      // [row block of slice si][row block of slice sj]
    double rs[4];                                   // the lane's share of the row sums of Y' u2 (slice si)
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        rs[h] = 0.0;
#pragma unroll
        for (int gb = 0; gb < 4; ++gb) {
            acc1[h][gb] = d4{0.0, 0.0, 0.0, 0.0};
            acc2[h][gb] = d4{0.0, 0.0, 0.0, 0.0};
        }
    }

    // One register set: a strip's operands are centred into registers of their own (and its weights formed) as soon as it
    // has arrived, the set is then refilled with the NEXT strip, which travels while this one is multiplied (128 matrix
    // instructions of 64 cycles each: longer than any load).
    FGramRegs pre;
    fetch(0, pre);
#pragma unroll 1
    for (int i = 0; i < w.tg; ++i) {
        // the point's weights as the SM_PRODUCT form of the strip kernels makes them; columns beyond n weigh nothing (the
        // padding of x' is zero: the exponential there is finite)
        const size_t col0 = (size_t)fgram_strip(q, w, i) * kStripCols + lq;
        double u1[4], u2[4];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const double e = exp(pre.x[qq] - logs);
            const bool valid = col0 + 4 * qq < (size_t)q.n;
            u1[qq] = valid ? pre.w0[qq] * e : 0.0;
            u2[qq] = u1[qq] * pre.qv[qq];
        }
        double ac[4][4], bc[4][4];                  // [column quad][row block]
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const d2 av = pre.a[2 * h + (qq >> 1)], bv = pre.b[2 * h + (qq >> 1)];
                ac[qq][h] = ((qq & 1) ? av.y : av.x) - ca[h];
                bc[qq][h] = ((qq & 1) ? bv.y : bv.x) - cb[h];
            }
        fetch(i + 1 < w.tg ? i + 1 : i, pre);         // unconditional
        asm volatile("" ::: "memory");              // the loads are issued HERE, in front of the products (the compiler sank them behind)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            double b1[4], b2[4];
#pragma unroll
            for (int gb = 0; gb < 4; ++gb) {
                b1[gb] = bc[qq][gb] * u1[qq];
                b2[gb] = bc[qq][gb] * u2[qq];
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                rs[h] = fma(ac[qq][h], u2[qq], rs[h]);
#pragma unroll
                for (int gb = 0; gb < 4; ++gb) {
                    acc1[h][gb] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[qq][h], b1[gb], acc1[h][gb], 0, 0, 0);
                    acc2[h][gb] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[qq][h], b2[gb], acc2[h][gb], 0, 0, 0);
                }
            }
        }
    }

    // The set leaves, accumulator by accumulator as the registers hold it: result register r of lane 16 lq + lr is row
    // 4 r + lq, column lr of the 16 x 16 block.  Row blocks beyond the strip's last one were redirected to the slice's first
    // (strip_chunk_offsets): what they leave lies beyond row m of the matrices and is never read (k_fgram_finish).
    double* const dst = q.partial + (size_t)w.set * q.set_stride + (size_t)fgram_sub(w.si, w.sj) * kFGramSubDoubles + lane;
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
        for (int gb = 0; gb < 4; ++gb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dst[((0 * 16 + h * 4 + gb) * 4 + r) * 64] = acc1[h][gb][r];
                dst[((1 * 16 + h * 4 + gb) * 4 + r) * 64] = acc2[h][gb][r];
            }
    fgram_store_row_sums(q, w, lq, lr, rs);
}

// out[e] = sum over segments (in index order) of [ the segment's gs sets added in turn ], e < count: on the sets' own
// layout (coalesced); out is one more set behind the partials
__global__ __launch_bounds__(kBlock) void k_fgram_sum_sets(const double* __restrict__ partial, size_t set_stride, size_t count,
                                                           int nlocal, int gs, double* __restrict__ out) {
    for (size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x; e < count; e += (size_t)gridDim.x * kBlock) {
        double total = 0.0;
        for (int v = 0; v < nlocal; ++v) {
            double s = 0.0;
            for (int g = 0; g < gs; ++g) s += partial[(size_t)(v * gs + g) * set_stride + e];
            total += s;
        }
        out[e] = total;
    }
}

// element (i, j), j <= i, of matrix `mat` in the summed set
__device__ __forceinline__ double fgram_elem(const double* sum, int mat, int i, int j) {
    const int h = (i >> 4) & 3, r = (i & 15) >> 2, lq = i & 3, gb = (j >> 4) & 3, lr = j & 15;
    return sum[(size_t)fgram_sub(i >> 6, j >> 6) * kFGramSubDoubles + ((mat * 16 + h * 4 + gb) * 4 + r) * 64 + 16 * lq + lr];
}

// The rank corrections, theta, the affine model's scales; the lower triangle is computed and mirrored: C and T = theta C
// + G2 (affine: S . S of both) are bitwise symmetric.  16 x 16 threads per block, blocks above the diagonal leave.
__global__ __launch_bounds__(256) void k_fgram_finish(const double* __restrict__ sum, size_t rows_at, int m, double theta,
                                                      const double* __restrict__ ybar, const double* __restrict__ row_scale,
                                                      bool affine, double* __restrict__ cov, double* __restrict__ hess) {
    if (blockIdx.x > blockIdx.y) return;
    const int i = blockIdx.y * 16 + (threadIdx.x >> 4), j = blockIdx.x * 16 + (threadIdx.x & 15);
    if (i >= m || j > i) return;
    const double yi = ybar[i], yj = ybar[j], gi = sum[rows_at + i], gj = sum[rows_at + j];
    double cv = fma(-yi, yj, fgram_elem(sum, 0, i, j));
    const double g2 = fma(-yi, gj, fma(-gi, yj, fgram_elem(sum, 1, i, j)));
    double tv = fma(theta, cv, g2);
    if (affine) {
        const double sa = row_scale[i], sb = row_scale[j];
        cv = (sa * cv) * sb;
        tv = (sa * tv) * sb;
    }
    cov[(size_t)i * m + j] = cv;
    cov[(size_t)j * m + i] = cv;
    hess[(size_t)i * m + j] = tv;
    hess[(size_t)j * m + i] = tv;
}

// hess += C C on the lower triangle, mirrored; the inner index runs 0 .. m - 1 in one fma chain per element
__global__ __launch_bounds__(256) void k_fgram_square(const double* __restrict__ cov, int m, double* __restrict__ hess) {
    __shared__ double as[16][17], bs[16][17];
    if (blockIdx.x > blockIdx.y) return;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int i = blockIdx.y * 16 + ty, j = blockIdx.x * 16 + tx;
    double s = 0.0;
    for (int k0 = 0; k0 < m; k0 += 16) {
        as[ty][tx] = (i < m && k0 + tx < m) ? cov[(size_t)i * m + k0 + tx] : 0.0;
        bs[ty][tx] = (k0 + ty < m && j < m) ? cov[(size_t)(k0 + ty) * m + j] : 0.0;
        __syncthreads();
        const int kn = min(16, m - k0);
        for (int kk = 0; kk < kn; ++kk) s = fma(as[ty][kk], bs[kk][tx], s);
        __syncthreads();
    }
    if (i < m && j <= i) {
        const double hv = hess[(size_t)i * m + j] + s;
        hess[(size_t)i * m + j] = hv;
        hess[(size_t)j * m + i] = hv;
    }
}

// ---- host side ------------------------------------------------------------------------------------
// gs: enough sets for two blocks per CU (256 CUs) over the canonical segments' tiles -- a function of (segcols, M) alone
ForcesGramPlan forces_gram_plan(const bioen_hip_ctx* c) {
    ForcesGramPlan p{};
    const int mps = panel_mps(c, 0);
    p.nsl = (mps + kWaveRows - 1) / kWaveRows;
    const int t = (p.nsl + 1) / 2;
    p.ntiles = t * (t + 1) / 2;
    p.nsub = p.nsl * (p.nsl + 1) / 2;
    const int sps = strip_sps(c);
    p.gs = std::max(1, std::min(sps, (512 + c->nseg * p.ntiles - 1) / (c->nseg * p.ntiles)));
    p.nsets = c->vr * p.gs;
    p.rows_at = (size_t)p.nsub * kFGramSubDoubles;
    p.set_stride = p.rows_at + (size_t)p.nsl * kWaveRows;
    p.cov_at = (size_t)(p.nsets + 1) * p.set_stride;
    p.hess_at = p.cov_at + (size_t)c->m * c->m;
    p.doubles = p.hess_at + (size_t)c->m * c->m;
    return p;
}

// nlocal x gs sets of set_stride doubles in buf -> their sum in the fixed order, one more set behind them (the log-weights
// Gram pass, kernels_logw_newton.hip, ends here too)
void launch_fgram_sum_sets(bioen_hip_ctx* c, double* buf, size_t set_stride, int nlocal, int gs) {
    const int sum_blocks = (int)std::min<size_t>((set_stride + kBlock - 1) / kBlock, 4096);
    hipLaunchKernelGGL(k_fgram_sum_sets, dim3(sum_blocks), dim3(kBlock), 0, c->stream, buf, set_stride, set_stride, nlocal, gs,
                       buf + (size_t)nlocal * gs * set_stride);
}

// the sets in buf -> their sum behind them, C at buf + cov_at, H at buf + hess_at (both passes end here)
void launch_fgram_tail(bioen_hip_ctx* c, const ForcesGramPlan& p, double* buf, const double* ybar, double theta) {
    double* sum = buf + (size_t)p.nsets * p.set_stride;
    launch_fgram_sum_sets(c, buf, p.set_stride, c->vr, p.gs);
    const int tb = (c->m + 15) / 16;
    hipLaunchKernelGGL(k_fgram_finish, dim3(tb, tb), dim3(256), 0, c->stream, sum, p.rows_at, c->m, theta, ybar, c->row_scale,
                       c->affine, buf + p.cov_at, buf + p.hess_at);
    hipLaunchKernelGGL(k_fgram_square, dim3(tb, tb), dim3(256), 0, c->stream, buf + p.cov_at, c->m, buf + p.hess_at);
}

// buf: forces_gram_plan's doubles; x, pscal, qv, ybar: the kept point's.  Leaves C at buf + cov_at, H at buf + hess_at.
void launch_forces_gram(bioen_hip_ctx* c, const ForcesGramPlan& p, double* buf, const double* x, const double* pscal,
                        const double* qv, const double* ybar, double theta) {
    hipLaunchKernelGGL(k_forces_gram, dim3(fgram_blocks(p)), dim3(256), 0, c->stream,
                       fgram_args(c, p, buf, x, pscal, qv));
    launch_fgram_tail(c, p, buf, ybar, theta);
}

}  // namespace bioen
