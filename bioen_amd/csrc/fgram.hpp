// What the two dense Hessian passes of the forces method share (kernels_forces_gram.hip, kernels_forces_gram_bf16.hip;
// DESIGN 6e, 6g): their arguments, the layout of what a set leaves, and everything a wave does that is not arithmetic --
// which (set, sub-tile) it owns, its rows' centres, the matrix half of a strip's fetch, the row sums on their way out.
// A kernel keeps what is its own: how the column weights reach a lane, how an operand is formed and multiplied, and which
// (register, lane) a result leaves from.
#pragma once

#include "strip.hpp"

namespace bioen {

constexpr int kFGramSubDoubles = 2 * 16 * 4 * 64;      // a sub-tile of both matrices: [matrix 2][h 4][g 4][register 4][lane 64]

struct FGramArgs {
    const double* Ys;       // row-sum order strip copy
    const double* center;   // mp values
    int mps, mp, n;
    int sps, gs, ilv;       // strips per segment, groups per segment, interleave of the copy
    int nsets;              // local segments x gs
    int nsl, ntiles;        // 64-row slices; 128-row tile pairs I >= J
    const double* w0;       // the point: prior, x', q - qbar, scalar slot (S_LOGS)
    const double* x;
    const double* qv;
    const double* pscal;
    double* partial;        // [set][sub-tile (si, sj <= si)][kFGramSubDoubles] | [set][row]: row sums of Y' u2
    size_t set_stride;      // doubles per set
    size_t rows_at;         // where a set's row sums begin
};

// index of sub-tile (si, sj), sj <= si, among the lower triangle's
__host__ __device__ inline int fgram_sub(int si, int sj) { return si * (si + 1) / 2 + sj; }

// the copy, the plan's sets in buf, the kept point -- and the grid: a tile pair per set, the tiles of one set on one XCD
inline FGramArgs fgram_args(const bioen_hip_ctx* c, const ForcesGramPlan& p, double* buf, const double* x, const double* pscal,
                            const double* qv) {
    FGramArgs q{};
    q.Ys = c->Ys[0];
    q.center = c->strip_center;
    q.mps = panel_mps(c, 0);
    q.mp = c->mp;
    q.n = c->n;
    q.sps = strip_sps(c);
    q.gs = p.gs;
    q.ilv = strip_ilv(c);
    q.nsets = p.nsets;
    q.nsl = p.nsl;
    q.ntiles = p.ntiles;
    q.w0 = c->fixed;
    q.x = x;
    q.qv = qv;
    q.pscal = pscal;
    q.partial = buf;
    q.set_stride = p.set_stride;
    q.rows_at = p.rows_at;
    return q;
}
inline int fgram_blocks(const ForcesGramPlan& p) { return 8 * p.ntiles * ((p.nsets + 7) / 8); }

// A wave's share: the set (segment v, group g: tg strips), the 64-row slices si >= sj whose sub-tile it accumulates, and
// where the lane's halves of their chunks lie in a strip.
struct FGramWave {
    int set, v, g, tg;
    int si, sj, ra, rb;                             // slices, their first rows
    int offa[kWaveRows / 8], offb[kWaveRows / 8];
    size_t wa, wb;
};

// Blocks b and b + 8 share an XCD and its L2: the tiles of one set are numbered so that they land on one XCD, next to each
// other in dispatch order -- they read the same strips.  false: the wave has nothing to do (no barrier in these kernels:
// a wave may leave).
__device__ __forceinline__ bool fgram_decode(const FGramArgs& q, int lane, int wave, FGramWave& w) {
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    w.set = (k / q.ntiles) * 8 + xcd;
    if (w.set >= q.nsets) return false;
    int ti, tj;
    tile_pair(k % q.ntiles, ti, tj);
    w.si = 2 * ti + (wave >> 1), w.sj = 2 * tj + (wave & 1);
    if (w.si >= q.nsl || w.sj > w.si) return false; // (in a diagonal tile the wave above the diagonal leaves)
    w.v = w.set / q.gs, w.g = w.set - w.v * q.gs;
    w.tg = (q.sps - w.g + q.gs - 1) / q.gs;         // strips of the set (g < gs <= sps: at least one)
    w.ra = w.si * kWaveRows, w.rb = w.sj * kWaveRows;
    strip_chunk_offsets(q.mps, w.ra, w.offa);
    strip_chunk_offsets(q.mps, w.rb, w.offb);
    w.wa = (size_t)w.ra * kStripCols + (size_t)lane * 2, w.wb = (size_t)w.rb * kStripCols + (size_t)lane * 2;
    return true;
}

// strip i of the wave's set
__device__ __forceinline__ int fgram_strip(const FGramArgs& q, const FGramWave& w, int i) { return w.v * q.sps + w.g + q.gs * i; }

// the centres of the lane's rows (row = lane & 15 of each of a slice's four row blocks)
__device__ __forceinline__ void fgram_centres(const FGramArgs& q, const FGramWave& w, int lr, double (&ca)[4], double (&cb)[4]) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const int rowa = w.ra + 16 * h + lr, rowb = w.rb + 16 * h + lr;
        ca[h] = rowa < q.mp ? q.center[rowa] : 0.0;
        cb[h] = rowb < q.mp ? q.center[rowb] : 0.0;
    }
}

// strip s: the 8 chunks of slice si into a, of slice sj into b
__device__ __forceinline__ void fgram_fetch(const FGramArgs& q, const FGramWave& w, int s, d2 (&a)[kWaveRows / 8],
                                            d2 (&b)[kWaveRows / 8]) {
    const double* src = q.Ys + (size_t)strip_phys(s, q.sps, q.ilv) * q.mps * kStripCols;
#pragma unroll
    for (int c = 0; c < kWaveRows / 8; ++c) a[c] = ldg2<false>(src + w.wa + w.offa[c]);
#pragma unroll
    for (int c = 0; c < kWaveRows / 8; ++c) b[c] = ldg2<false>(src + w.wb + w.offb[c]);
}

// rs: the lane's share of the row sums of Y' u2 (slice si).  One writer per slice and set: the waves of sub-tile column 0.
__device__ __forceinline__ void fgram_store_row_sums(const FGramArgs& q, const FGramWave& w, int lq, int lr, const double (&rs)[4]) {
    if (w.sj != 0) return;                          // (wave-uniform)
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const double t = quad_sum(rs[h]);
        const int row = w.ra + 16 * h + lr;
        if (lq == 0) q.partial[(size_t)w.set * q.set_stride + q.rows_at + row] = row < q.mps ? t : 0.0;
    }
}

}  // namespace bioen
