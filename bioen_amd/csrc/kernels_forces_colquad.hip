// Forces method, M <= 1024: one quadratic form per structure at a kept point, in ONE pass over the matrix (gfx950).
//   out_j = a_j^T P a_j,   a_j = (Y_:j - centre) - ybar'   (the operand is centred directly: the quadratic is never expanded)
// for a symmetric M x M matrix P (the entry has folded the affine model's scales into it: P_eff = S P S).  With P = H^-1 it
// is the Laplace variance of ln w_j, with P = C^-1 a structure's Mahalanobis distance from the refined ensemble, with P = I
// its spread.  M^2 N flops on the FP64 matrix cores: P is symmetric, its lower triangle is all that is multiplied.
//
// k_forces_colquad reads the row-sum order strip copy (strip.hpp) and no other.  A block of four waves owns a PANEL of 32
// columns (two strips) and ALL rows of it:
//   T = P A_panel contracts over ROWS, and a strip's registers (row = lane & 15, k = lane >> 4 of a column quad) contract over
//   columns.  So the panel goes through LDS, 64 rows (a slice) at a time: the waves load the slice's chunks as the forces
//   passes do (1 KiB per wave-load), centre them and store them as a plain [row][column] image; from it every wave fetches
//   the B operand of v_mfma_f64_16x16x4_f64 -- B[k = lane >> 4][n = lane & 15] = A[i0 + k][j0 + n] -- once per four rows
//   and uses it for all its row blocks of P.  The A operand is P itself, read through its symmetry so that a wave-load is
//   four runs of 128 bytes: A[row = lane & 15][k = lane >> 4] = P[i0 + k][k0 + row].
//   A wave keeps T for one 16-row block of every slice and the panel's 32 columns: 2 x NB accumulators, 256 registers at
//   M = 1024 (one wave per SIMD).  out_j = sum_k A_kj T_kj finishes inside the block, slice by slice (below): a lane's fma
//   chain over its rows in ascending order, the four row quads by two shuffles, the four waves in wave order.
// Every out_j has one writer, there are no atomics, and the order of the sum is a function of M alone.
// P's lower triangle (4 M^2 bytes, <= 4 MiB) is read once per panel from L2 / Infinity Cache, for 32 M^2 flops.
#include "strip.hpp"

namespace bioen {

constexpr int kCqStrips = kForcesColquadCols / kStripCols;      // strips of a panel
constexpr int kCqPitch = 40;                                    // doubles per row of the LDS image (32 + 8: the four row quads of an operand fetch start 16 banks apart)
constexpr int kCqChunks = kCqStrips * (kWaveRows / 8) / 4;      // chunks of a slice per wave: 4

struct ColquadArgs {
    const double* Ys;       // row-sum order strip copy
    const double* center;   // mp values
    const double* ybar;     // the point's ybar' (mp values)
    const double* P;        // mps x mps, zero beyond m, bitwise symmetric
    double* out;            // n values
    int mps, m, n;
    int sps, ilv;           // strips per segment, interleave of the copy
    int npanels;
};

// NB = ceil(mps / 64): the 64-row slices of a strip, and the 16-row blocks of T a wave holds: wave w the blocks 4 kb + w,
// kb = 0 .. NB - 1 -- one block of every slice.  With P symmetric,
//   out_j = sum_b A_b^T T'_b,    T'_b = P_bb A_b + 2 sum_{i < b} P_bi A_i     (b, i: 16-row blocks; column j throughout)
// so T'_b is complete when the contraction has reached the end of b's own slice -- while that slice still lies in LDS: the
// wave takes its A_b from the image, in the accumulators' own layout, and block b is done.  Only P's lower triangle is
// multiplied (M^2 N flops instead of 2 M^2 N), nothing is read twice, and every wave has the same work.  The weights 2, 1
// and 0 (a block of the same slice above b) are applied to the B operand: exact.
// Blocks beyond the strip's last one (mps is a multiple of 16, not of 64) read P's first row block instead (valid memory;
// straight-line code for every wave, as strip_chunk_offsets does it) and meet zeros in the image: they weigh nothing.
template <int NB>
__global__ __launch_bounds__(256, 1) void k_forces_colquad(ColquadArgs q) {
    __shared__ double tile[2][kWaveRows * kCqPitch];
    __shared__ double csh[kPanelRows], ysh[kPanelRows];
    __shared__ double red[4][kForcesColquadCols];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane >> 4, lr = lane & 15;
    const int nst = q.mps / 4;                                  // contraction steps of four rows
    const int nb16 = q.mps / 16;
    const size_t strip_doubles = (size_t)q.mps * kStripCols;

    for (int r = threadIdx.x; r < q.mps; r += 256) {
        csh[r] = r < q.m ? q.center[r] : 0.0;
        ysh[r] = r < q.m ? q.ybar[r] : 0.0;
    }
    __syncthreads();

    // P as the A operand, step st (rows 4 st .. 4 st + 3 of the contraction), block kb of the wave: through P's symmetry
    // P[4 st + lq][16 (4 kb + wave) + lr], a wave-load of four runs of 128 bytes
    // (a uniform address per block and step plus ONE lane offset: no per-block address registers)
    const int lane_off = lq * q.mps + lr;
    int poff[NB];
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) poff[kb] = __builtin_amdgcn_readfirstlane(4 * kb + wave < nb16 ? 16 * (4 * kb + wave) : 0);

    int it = 0;                                                 // slices done by this block: the LDS image alternates
#pragma unroll 1
    for (int p = blockIdx.x; p < q.npanels; p += gridDim.x) {
        const int s0 = p * kCqStrips;                           // the panel's first strip
        int lo = lane_off;                                      // (opaque once per panel: the blocks' addresses are formed where
        asm volatile("" : "+v"(lo));                            // they are used, not kept in registers across the panel loop)
        // chunk u of this wave in a slice: strip t of the panel, chunk i = 2 h + qp of the strip's slice.  A strip beyond
        // column n is redirected to the panel's first, a row block beyond the strip's last to the slice's first: the loads
        // are unconditional, what they bring is zeroed on its way into the image.
        auto fetch_slice = [&](int sl, d2 (&v)[kCqChunks]) {
#pragma unroll
            for (int u = 0; u < kCqChunks; ++u) {
                const int ci = wave + 4 * u, t = ci >> 3, i = ci & 7;
                const int s = (size_t)(s0 + t) * kStripCols < (size_t)q.n ? s0 + t : s0;
                const int ii = kWaveRows * sl + 16 * (i >> 1) < q.mps ? i : (i & 1);
                v[u] = ldg2<false>(q.Ys + (size_t)strip_phys(s, q.sps, q.ilv) * strip_doubles +
                                   (size_t)sl * kWaveRows * kStripCols + ii * 128 + lane * 2);
            }
        };
        // ... centred and laid down as image[row][column]: .x is column 8 qp + lq, .y column 8 qp + 4 + lq of the strip;
        // rows beyond m and columns beyond n are zeros
        auto store_slice = [&](int sl, const d2 (&v)[kCqChunks], double* img) {
#pragma unroll
            for (int u = 0; u < kCqChunks; ++u) {
                const int ci = wave + 4 * u, t = ci >> 3, i = ci & 7, h = i >> 1, qp = i & 1;
                const int rl = 16 * h + lr, row = kWaveRows * sl + rl;
                const int cl = kStripCols * t + 8 * qp + lq;
                const size_t col = (size_t)p * kForcesColquadCols + cl;
                const bool rv = row < q.m;
                const double cc = csh[rv ? row : 0], yy = ysh[rv ? row : 0];
                img[rl * kCqPitch + cl] = (rv && col < (size_t)q.n) ? (v[u].x - cc) - yy : 0.0;
                img[rl * kCqPitch + cl + 4] = (rv && col + 4 < (size_t)q.n) ? (v[u].y - cc) - yy : 0.0;
            }
        };

        d4 acc[NB][kCqStrips];                                  // T': [block of the wave][column block of the panel]
        double sum[kCqStrips];
#pragma unroll
        for (int jb = 0; jb < kCqStrips; ++jb) sum[jb] = 0.0;

        d2 pre[kCqChunks];
        double pc[NB];
        fetch_slice(0, pre);
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) pc[kb] = (q.P + poff[kb])[lo];
#pragma unroll
        for (int sl = 0; sl < NB; ++sl, ++it) {                 // (unrolled: slice sl feeds the blocks kb >= sl)
            double* const img = tile[it & 1];
            store_slice(sl, pre, img);
            __syncthreads();                                    // one barrier per slice: the other image is the one still read
            fetch_slice(sl + 1 < NB ? sl + 1 : sl, pre);        // travels while this slice is multiplied (unconditional)
            const int st0 = (kWaveRows / 4) * sl, cnt = min(kWaveRows / 4, nst - st0);      // (the last slice may be short)
            const double* bsrc = img + lq * kCqPitch + lr;
            // FIRST: the panel's very first step starts the accumulators from the instruction's zero operand (no zeroed
            // registers that would have to be carried into the loops)
            auto step = [&](int i4, auto FIRST) {
                double b2[kCqStrips], bd[kCqStrips];
                const int ib = i4 >> 2;                         // the step's block within the slice, against the wave's own
                const double wd = ib < wave ? 2.0 : ib == wave ? 1.0 : 0.0;
#pragma unroll
                for (int jb = 0; jb < kCqStrips; ++jb) {
                    const double b = bsrc[4 * i4 * kCqPitch + kStripCols * jb];
                    b2[jb] = 2.0 * b;
                    bd[jb] = wd * b;
                }
                // a block's P for the NEXT step is asked for as soon as this step's products with it are issued: it travels
                // for a whole step (matrix instructions of 64 cycles each) and needs no second register set
                const double* nxt = q.P + (size_t)(4 * min(st0 + i4 + 1, nst - 1)) * q.mps;
#pragma unroll
                for (int kb = sl; kb < NB; ++kb) {
#pragma unroll
                    for (int jb = 0; jb < kCqStrips; ++jb)
                        acc[kb][jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(pc[kb], kb == sl ? bd[jb] : b2[jb],
                                                                           FIRST.value ? d4{0.0, 0.0, 0.0, 0.0} : acc[kb][jb], 0, 0, 0);
                    pc[kb] = (nxt + poff[kb])[lo];
                }
            };
            int i4 = 0;
            if (sl == 0) step(i4++, std::true_type{});          // (mps >= 16: slice 0 has at least four steps)
#pragma unroll 1
            for (; i4 < cnt; ++i4) step(i4, std::false_type{});
            // block 4 sl + wave is complete and its rows lie in the image: result register r of lane 16 lq + lr is row
            // 4 r + lq, column lr of the 16 x 16 block
#pragma unroll
            for (int jb = 0; jb < kCqStrips; ++jb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    sum[jb] = fma(img[(16 * wave + 4 * r + lq) * kCqPitch + kStripCols * jb + lr], acc[sl][jb][r], sum[jb]);
        }

#pragma unroll
        for (int jb = 0; jb < kCqStrips; ++jb) {
            const double t = quad_sum(sum[jb]);
            if (lq == 0) red[wave][kStripCols * jb + lr] = t;
        }
        __syncthreads();
        if (threadIdx.x < kForcesColquadCols) {
            const size_t col = (size_t)p * kForcesColquadCols + threadIdx.x;
            const double o = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
            if (col < (size_t)q.n) q.out[col] = o;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------
// P: (strip rows)^2 doubles, zero beyond m; ybar: the kept point's ybar'; out: >= n doubles.  One block per CU (256), each
// running the panels b, b + 256, ...
ColquadGrid forces_colquad_grid(const bioen_hip_ctx* c) {
    ColquadGrid g{};
    g.npanels = (c->n + kForcesColquadCols - 1) / kForcesColquadCols;
    g.blocks = std::min(g.npanels, kForcesColquadBlocks);
    g.mps = panel_mps(c, 0);
    g.nb = (g.mps + kWaveRows - 1) / kWaveRows;               // row blocks of T per wave: 1 .. 16
    return g;
}

void launch_forces_colquad(bioen_hip_ctx* c, const double* P, const double* ybar, double* out) {
    const ColquadGrid g = forces_colquad_grid(c);
    ColquadArgs q{};
    q.Ys = c->Ys[0];
    q.center = c->strip_center;
    q.ybar = ybar;
    q.P = P;
    q.out = out;
    q.mps = g.mps;
    q.m = c->m;
    q.n = c->n;
    q.sps = strip_sps(c);
    q.ilv = strip_ilv(c);
    q.npanels = g.npanels;
    for_value<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(g.nb, [&](auto NB) {
        hipLaunchKernelGGL(k_forces_colquad<NB.value>, dim3(g.blocks), dim3(256), 0, c->stream, q);
    });
}

}  // namespace bioen
