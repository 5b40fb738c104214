// The dense Gram passes (kernels_forces_gram.hip, kernels_logw_newton.hip): their arguments, the
// layout of what a set leaves, and everything a wave does that is not arithmetic -- which (set, sub-tile) it owns, its rows'
// centres, the matrix half of a strip's fetch, the row sums on their way out.  The passes themselves are here too, each
// once: the FP64 pass (fgram_pass: k_forces_gram and k_logw_gram are its two instances) and the split-BF16 pass
// (fgram16_pass: k_forces_gram_bf16 and k_logw_gram_bf16), each instance with a POINT that says how many matrices a wave
// accumulates and how a column's weights come from what the point keeps.  The two methods' points are here as well, each
// once for both precisions: the FP64 pass forms the weights of four columns per lane, the BF16 pass those of one, handed
// round by shuffles.  A pass is compiled for one of two argument structs: FGramArgs, one copy with one row count (M <= 1024),
// or FGramPanelArgs, the row panels' copies (1024 < M <= 4096) -- the two differ only in where a wave's two
// slices come from, and the four kernels of the first form do not see the second.
#pragma once

#include "strip.hpp"

namespace bioen {

// doubles of a sub-tile of `mats` matrices: [matrix][h 4][g 4][register 4][lane 64]
__host__ __device__ constexpr int fgram_sub_doubles(int mats) { return mats * 16 * 4 * 64; }

struct FGramArgs {
    const double* Ys;       // row-sum order strip copy
    const double* center;   // mp values
    int mps, mp, n;
    int sps, gs, ilv;       // strips per segment, groups per segment, interleave of the copy
    int nsets;              // local segments x gs
    int nsl, ntiles;        // 64-row slices; 128-row tile pairs I >= J
    const double* w0;       // the point -- forces: prior, x', q - qbar, scalar slot (S_LOGS)
    const double* x;        //           -- log-weights: (w0 unread), e, grad, scalar slot (S_INV + segment)
    const double* qv;
    const double* pscal;
    double* partial;        // [set][sub-tile (si, sj <= si)][fgram_sub_doubles] | [set][row]: row sums of Y' u2 | (sum u2)
    size_t set_stride;      // doubles per set
    size_t rows_at;         // where a set's row sums begin
};

// index of sub-tile (si, sj), sj <= si, among the lower triangle's
__host__ __device__ inline int fgram_sub(int si, int sj) { return si * (si + 1) / 2 + sj; }

// element (i, j), j <= i, of matrix `mat` among the `mats` of a summed set
__device__ __forceinline__ double fgram_elem(const double* sum, int mats, int mat, int i, int j) {
    const int h = (i >> 4) & 3, r = (i & 15) >> 2, lq = i & 3, gb = (j >> 4) & 3, lr = j & 15;
    return sum[(size_t)fgram_sub(i >> 6, j >> 6) * fgram_sub_doubles(mats) + ((mat * 16 + h * 4 + gb) * 4 + r) * 64 + 16 * lq + lr];
}

// the copy, the plan's sets in buf, the kept point -- and the grid: a tile pair per set, the tiles of one set on one XCD
inline FGramArgs fgram_args(const bioen_hip_ctx* c, const GramPlan& p, double* buf, const double* x, const double* pscal,
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
inline int fgram_blocks(const GramPlan& p) { return 8 * p.ntiles * ((p.nsets + 7) / 8); }

// The same pass over row panels (strip.hpp: kPanelRows = 1024 rows each, the last one shorter): every panel has a strip copy
// and a row count of its own.  In every panel but the last a 64-row slice s of the matrix is local slice s & 15 of panel
// s >> 4, and a 128-row tile never straddles two panels; slices, sub-tiles, centres and row sums are numbered by GLOBAL row,
// so everything behind the sets reads them as it reads FGramArgs's.  (FGramArgs's Ys and mps are panel 0's here.)
static_assert(kDensePanelRows == kDensePanels * kPanelRows, "the dense entries' limit is whole panels");
struct FGramPanelArgs : FGramArgs {
    const double* Yp[kDensePanels];     // panel p's row-sum order strip copy
    int pmps[kDensePanels];             // its strip rows
};
inline FGramPanelArgs fgram_panel_args(const bioen_hip_ctx* c, const GramPlan& p, double* buf, const double* x,
                                       const double* pscal, const double* qv) {
    FGramPanelArgs q{};
    static_cast<FGramArgs&>(q) = fgram_args(c, p, buf, x, pscal, qv);
    for (int k = 0; k < kDensePanels; ++k) {
        const bool there = k < panel_count(c);
        q.Yp[k] = there ? c->Ys[k] : c->Ys[0];
        q.pmps[k] = there ? panel_mps(c, k) : panel_mps(c, 0);
    }
    return q;
}

// A wave's share: the set (segment v, group g: tg strips), the 64-row slices si >= sj whose sub-tile it accumulates, and
// where the lane's halves of their chunks lie in a strip.
struct FGramWave {
    int set, v, g, tg;
    int si, sj, ra, rb;                             // slices, their first rows
    int offa[kWaveRows / 8], offb[kWaveRows / 8];
    size_t wa, wb;
    const double *pa, *pb;                          // FGramPanelArgs: the copies of the slices' panels, a strip's doubles
    size_t sta, stb;                                //   there (wave-uniform: scalar registers)
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

// Over panels: the same sets, tiles and slices (counted over all panels: q.nsl); ra, rb stay GLOBAL rows (the centres, the
// row sums), the chunks' places are those of the slice's rows inside its own panel's strips
__device__ __forceinline__ bool fgram_decode(const FGramPanelArgs& q, int lane, int wave, FGramWave& w) {
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    w.set = (k / q.ntiles) * 8 + xcd;
    if (w.set >= q.nsets) return false;
    int ti, tj;
    tile_pair(k % q.ntiles, ti, tj);
    w.si = 2 * ti + (wave >> 1), w.sj = 2 * tj + (wave & 1);
    if (w.si >= q.nsl || w.sj > w.si) return false;
    w.v = w.set / q.gs, w.g = w.set - w.v * q.gs;
    w.tg = (q.sps - w.g + q.gs - 1) / q.gs;
    w.ra = w.si * kWaveRows, w.rb = w.sj * kWaveRows;
    constexpr int kSlices = kPanelRows / kWaveRows;             // 16 slices a panel
    const int pa = __builtin_amdgcn_readfirstlane(w.si / kSlices), pb = __builtin_amdgcn_readfirstlane(w.sj / kSlices);
    const int la = (w.si % kSlices) * kWaveRows, lb = (w.sj % kSlices) * kWaveRows;       // the slices' first rows in their panels
    const int ma = q.pmps[pa], mb = q.pmps[pb];
    w.pa = q.Yp[pa], w.pb = q.Yp[pb];
    w.sta = (size_t)ma * kStripCols, w.stb = (size_t)mb * kStripCols;
    strip_chunk_offsets(ma, la, w.offa);
    strip_chunk_offsets(mb, lb, w.offb);
    w.wa = (size_t)la * kStripCols + (size_t)lane * 2, w.wb = (size_t)lb * kStripCols + (size_t)lane * 2;
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
// over panels: each slice from its own panel's copy, at that panel's stride
__device__ __forceinline__ void fgram_fetch(const FGramPanelArgs& q, const FGramWave& w, int s, d2 (&a)[kWaveRows / 8],
                                            d2 (&b)[kWaveRows / 8]) {
    const size_t ph = (size_t)strip_phys(s, q.sps, q.ilv);
    const double *sa = w.pa + ph * w.sta, *sb = w.pb + ph * w.stb;
#pragma unroll
    for (int c = 0; c < kWaveRows / 8; ++c) a[c] = ldg2<false>(sa + w.wa + w.offa[c]);
#pragma unroll
    for (int c = 0; c < kWaveRows / 8; ++c) b[c] = ldg2<false>(sb + w.wb + w.offb[c]);
}

// the first row beyond the strip rows that hold slice si: rows from there on leave no row sum
__device__ __forceinline__ int fgram_row_limit(const FGramArgs& q, const FGramWave&) { return q.mps; }
__device__ __forceinline__ int fgram_row_limit(const FGramPanelArgs& q, const FGramWave& w) {
    const int p = w.ra / kPanelRows;
    return p * kPanelRows + q.pmps[p];
}

// rs: the lane's share of the row sums of Y' u2 (slice si).  One writer per slice and set: the waves of sub-tile column 0.
// limit: fgram_row_limit's
__device__ __forceinline__ void fgram_store_row_sums(const FGramArgs& q, const FGramWave& w, int lq, int lr, const double (&rs)[4],
                                                     int limit) {
    if (w.sj != 0) return;                          // (wave-uniform)
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const double t = quad_sum(rs[h]);
        const int row = w.ra + 16 * h + lr;
        if (lq == 0) q.partial[(size_t)w.set * q.set_stride + q.rows_at + row] = row < limit ? t : 0.0;
    }
}

// ---- the two methods' points ----------------------------------------------------------------------------------------------
// A Point<kCols> holds what the point keeps for kCols of a strip's columns (col, col + 4, ...) and supplies
//   static double scalar(q, w)                 the wave's scalar of the point
//   void load(q, col)                          its registers from the point's vectors
//   void weights(scalar, k, valid, u1, u2)     the two weights of its column k; `valid`: the column lies below n
// Matrix 0 of a pass is weighted by u1, matrix 1 (kMats = 2) by u2; the row sums of Y' u2 ride along, and with kSumU2
// sum u2 itself.  The FP64 pass takes four columns per lane (4 qq + (lane >> 4)), the BF16 pass one (lane & 15).

// The forces point: the weights as the SM_PRODUCT form of the strip kernels makes them, u1 = w0 exp(x' - log s), u2 = u1
// (q - qbar); columns beyond n weigh nothing (the padding of x' is zero: the exponential there is finite)
template <int kCols>
struct ForcesGramPoint {
    static constexpr int kMats = 2;
    static constexpr bool kSumU2 = false;
    double w0[kCols], x[kCols], qv[kCols];
    __device__ __forceinline__ static double scalar(const FGramArgs& q, const FGramWave&) { return q.pscal[S_LOGS]; }
    __device__ __forceinline__ void load(const FGramArgs& q, size_t col) {
#pragma unroll
        for (int k = 0; k < kCols; ++k) {
            w0[k] = q.w0[col + 4 * k];
            x[k] = q.x[col + 4 * k];
            qv[k] = q.qv[col + 4 * k];
        }
    }
    __device__ __forceinline__ void weights(double logs, int k, bool valid, double& u1, double& u2) const {
        const double e = exp(x[k] - logs);
        u1 = valid ? w0[k] * e : 0.0;
        u2 = u1 * qv[k];
    }
};

// The log-weights point, in FGramArgs x = e, qv = grad, pscal = the point's scalar slot, w0 unread: the weights are slot 0's
// e times the softmax factor of the set's segment (S_INV), u2 = grad; columns beyond n weigh nothing
template <int kCols>
struct LogwGramPoint {
    static constexpr int kMats = 1;
    static constexpr bool kSumU2 = true;
    double e[kCols], gr[kCols];
    __device__ __forceinline__ static double scalar(const FGramArgs& q, const FGramWave& w) { return q.pscal[S_INV + w.v]; }
    __device__ __forceinline__ void load(const FGramArgs& q, size_t col) {
#pragma unroll
        for (int k = 0; k < kCols; ++k) {
            e[k] = q.x[col + 4 * k];
            gr[k] = q.qv[col + 4 * k];
        }
    }
    __device__ __forceinline__ void weights(double inv, int k, bool valid, double& u1, double& u2) const {
        u1 = valid ? e[k] * inv : 0.0;
        u2 = valid ? gr[k] : 0.0;
    }
};

// a strip's registers: the chunks of the wave's two slices and the point's columns
template <class Point>
struct FGramRegs {
    d2 a[kWaveRows / 8];
    d2 b[kWaveRows / 8];
    Point pt;
};

// ---- the split-BF16 pass's operands -----------------------------------------------------------------------
typedef float fl4 __attribute__((ext_vector_type(4)));
typedef short bh4 __attribute__((ext_vector_type(4)));      // four bfloat16: an operand fragment of the 16-deep instruction
typedef unsigned u2v __attribute__((ext_vector_type(2)));   // the same two registers as they are filled: elements (0, 1) | (2, 3)
typedef __bf16 bfp __attribute__((ext_vector_type(2)));
typedef float flp __attribute__((ext_vector_type(2)));

// two floats -> two bfloat16 in one register (v0 in the low half), round to nearest even: v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned bf_pack(float v0, float v1) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(flp{v0, v1}, bfp));
}

// v0, v1 = hi + lo + (what the split drops), both bfloat16: a register of two his and one of two los -- half a fragment
__device__ __forceinline__ void bf_split2(double v0, double v1, unsigned& hi, unsigned& lo) {
    const float f0 = (float)v0, f1 = (float)v1;
    hi = bf_pack(f0, f1);
    lo = bf_pack(f0 - __uint_as_float(hi << 16), f1 - __uint_as_float(hi & 0xffff0000u));       // exact in f32
}

__device__ __forceinline__ fl4 mfma16(u2v a, u2v b, fl4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(bh4, a), __builtin_bit_cast(bh4, b), c, 0, 0, 0);
}

// ---- the FP64 pass -------------------------------------------------------------------------------------------------------
// A wave's 64-row slice of a strip arrives as 8 chunks whose halves ARE operands of v_mfma_f64_16x16x4_f64 (row = lane & 15,
// k = lane >> 4) -- as A for its own row block and, the same registers of another slice, as B: G'_IJ += Y'_I diag(u) Y'_J^T
// with no transpose and no LDS image.  A wave owns a 64 x 64 sub-tile of Point::kMats matrices (16 accumulators of 4 doubles
// each), matrix 0 weighted by u1, matrix 1 by u2; the row sums of Y' u2 ride along, and with Point::kSumU2 sum u2 itself.
// Point: a four-column point, the strip's columns 4 qq + (lane >> 4), qq = 0 .. 3.
// Args: FGramArgs, or FGramPanelArgs -- decode, fetch and the row sums' limit are chosen by it, nothing else differs.
template <class Point, class Args>
__device__ __forceinline__ void fgram_pass(const Args& q) {
    constexpr int kMats = Point::kMats;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane >> 4, lr = lane & 15;
    FGramWave w;
    if (!fgram_decode(q, lane, wave, w)) return;
    const double scal = Point::scalar(q, w);
    double ca[4], cb[4];                            // the centres of the lane's rows
    fgram_centres(q, w, lr, ca, cb);

    auto fetch = [&](int i, FGramRegs<Point>& r) {
        const int s = fgram_strip(q, w, i);
        fgram_fetch(q, w, s, r.a, r.b);
        r.pt.load(q, (size_t)s * kStripCols + lq);
    };

    d4 acc[kMats][4][4];                            // [matrix][row block of slice si][row block of slice sj]
    double rs[4], sg = 0.0;                         // the lane's share of the row sums of Y' u2 (slice si), of sum u2
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        rs[h] = 0.0;
#pragma unroll
        for (int gb = 0; gb < 4; ++gb)
#pragma unroll
            for (int mat = 0; mat < kMats; ++mat) acc[mat][h][gb] = d4{0.0, 0.0, 0.0, 0.0};
    }

    // One register set: a strip's operands are centred into registers of their own (and its weights formed) as soon as it
    // has arrived, the set is then refilled with the NEXT strip, which travels while this one is multiplied (64 matrix
    // instructions of 64 cycles each per matrix: longer than any load).
    FGramRegs<Point> pre;
    fetch(0, pre);
#pragma unroll 1
    for (int i = 0; i < w.tg; ++i) {
        const size_t col0 = (size_t)fgram_strip(q, w, i) * kStripCols + lq;
        double u1[4], u2[4];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            pre.pt.weights(scal, qq, col0 + 4 * qq < (size_t)q.n, u1[qq], u2[qq]);
            if constexpr (Point::kSumU2) sg += u2[qq];
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
        fetch(i + 1 < w.tg ? i + 1 : i, pre);       // unconditional
        asm volatile("" ::: "memory");              // the loads are issued HERE, in front of the products (the compiler sank them behind)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            double bu[kMats][4];
#pragma unroll
            for (int gb = 0; gb < 4; ++gb) {
                bu[0][gb] = bc[qq][gb] * u1[qq];
                if constexpr (kMats == 2) bu[1][gb] = bc[qq][gb] * u2[qq];
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                rs[h] = fma(ac[qq][h], u2[qq], rs[h]);
#pragma unroll
                for (int gb = 0; gb < 4; ++gb)
#pragma unroll
                    for (int mat = 0; mat < kMats; ++mat)
                        acc[mat][h][gb] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[qq][h], bu[mat][gb], acc[mat][h][gb], 0, 0, 0);
            }
        }
    }

    // The set leaves, accumulator by accumulator as the registers hold it: result register r of lane 16 lq + lr is row
    // 4 r + lq, column lr of the 16 x 16 block (fgram_elem).  Row blocks beyond the strip's last one were redirected to the
    // slice's first (strip_chunk_offsets): what they leave lies beyond row m of the matrices and is never read.
    double* const set = q.partial + (size_t)w.set * q.set_stride;
    double* const dst = set + (size_t)fgram_sub(w.si, w.sj) * fgram_sub_doubles(kMats) + lane;
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
        for (int gb = 0; gb < 4; ++gb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int mat = 0; mat < kMats; ++mat) dst[((mat * 16 + h * 4 + gb) * 4 + r) * 64] = acc[mat][h][gb][r];
    fgram_store_row_sums(q, w, lq, lr, rs, fgram_row_limit(q, w));
    if constexpr (Point::kSumU2)
        if (w.si == 0) {                            // (sj = 0 too) over the set's columns: the four quarters hold four columns each
            const double t = quad_sum(sg);
            if (lane == 0) set[q.rows_at + (size_t)q.nsl * kWaveRows] = t;
        }
}

// ---- the split-BF16 pass ------------------------------------------------------------------------------------
// fgram_pass with the M x M x N products from SPLIT-BF16 operands on the BF16 matrix cores; the sets, their order and the
// layout of what a set leaves are fgram_pass's:
//   a = Y_ij - centre_i (FP64)        a_hi = bf(a),  a_lo = bf((float)a - a_hi)          bf: float, then bfloat16, both
//   t = a u_j           (FP64)        t_hi = bf(t),  t_lo = bf((float)t - t_hi)              round-to-nearest-even
//   G'[u]_ik = sum_j (a_hi t_hi + a_hi t_lo + a_lo t_hi)        v_mfma_f32_16x16x16_bf16, f32 accumulators
// The row sums of Y' u2 (and sum u2) stay fgram_pass's FP64 fma chains in its column order (they feed cancellations): the
// same bits.  The strip copy's registers (row = lane & 15, the strip's columns 4 qq + (lane >> 4) in qq = 0 .. 3) are a
// 16-row, 16-deep BF16 operand as they stand: element qq of a lane's fragment is depth index 4 (lane >> 4) + qq of the
// instruction, for the A and the B operand alike, so the instruction contracts over the strip's 16 columns in a permuted
// order.  A wave owns a 64 x 64 sub-tile of Point::kMats matrices (16 accumulators of 4 floats each).  A set's f32 sums
// leave as doubles on fgram_elem's layout, so k_fgram_sum_sets adds the sets IN FP64 in its fixed order and the FP64 pass's
// finishing kernels take them as they are.
// Point: a one-column point, the strip's column lane & 15 -- a lane forms the weights of ONE column with the operations of
// the four-column point (the same bits), the lanes that multiply with them receive them by shuffles.
template <class Point, class Args>
__device__ __forceinline__ void fgram16_pass(const Args& q) {
    constexpr int kMats = Point::kMats;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane >> 4, lr = lane & 15;
    FGramWave w;
    if (!fgram_decode(q, lane, wave, w)) return;
    const double scal = Point::scalar(q, w);
    double ca[4], cb[4];                            // the centres of the lane's rows
    fgram_centres(q, w, lr, ca, cb);

    auto fetch = [&](int i, FGramRegs<Point>& r) {
        const int s = fgram_strip(q, w, i);
        fgram_fetch(q, w, s, r.a, r.b);
        r.pt.load(q, (size_t)s * kStripCols + lr);
    };

    fl4 acc[kMats][4][4];                           // [matrix][row block of slice si][row block of slice sj]
    double rs[4], sg = 0.0;                         // the lane's share of the row sums of Y' u2 (slice si), of sum u2
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        rs[h] = 0.0;
#pragma unroll
        for (int gb = 0; gb < 4; ++gb)
#pragma unroll
            for (int mat = 0; mat < kMats; ++mat) acc[mat][h][gb] = fl4{0.f, 0.f, 0.f, 0.f};
    }

    // One register set, as in fgram_pass: a strip's operands are centred, weighted and split into registers of their own
    // as soon as it has arrived, the set is refilled with the NEXT strip, which travels while this one is multiplied.
    FGramRegs<Point> pre;
    fetch(0, pre);
#pragma unroll 1
    for (int i = 0; i < w.tg; ++i) {
        // formed once per column (lane & 15) and handed to the lanes that multiply with them: lane 4 qq + lq formed column
        // 4 qq + lq -- fgram_pass's columns and order
        const size_t colc = (size_t)fgram_strip(q, w, i) * kStripCols + lr;
        double uc[2], u[2][4];                      // [u1 | u2]
        pre.pt.weights(scal, 0, colc < (size_t)q.n, uc[0], uc[1]);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            u[0][qq] = __shfl(uc[0], 4 * qq + lq, 64);
            u[1][qq] = __shfl(uc[1], 4 * qq + lq, 64);
            if constexpr (Point::kSumU2) sg += u[1][qq];
        }
        u2v ah[4], al[4], bh[kMats][4], bl[kMats][4];           // [row block]: the fragments, element qq = column quad qq
#pragma unroll
        for (int h = 0; h < 4; ++h)
#pragma unroll
            for (int qp = 0; qp < 2; ++qp) {                    // the column quads 2 qp (.x) and 2 qp + 1 (.y)
                const d2 av = pre.a[2 * h + qp], bv = pre.b[2 * h + qp];
                const double a0 = av.x - ca[h], a1 = av.y - ca[h];
                const double b0 = bv.x - cb[h], b1 = bv.y - cb[h];
                rs[h] = fma(a0, u[1][2 * qp], rs[h]);
                rs[h] = fma(a1, u[1][2 * qp + 1], rs[h]);
                unsigned hi, lo;
                bf_split2(a0, a1, hi, lo);
                ah[h][qp] = hi;
                al[h][qp] = lo;
#pragma unroll
                for (int mat = 0; mat < kMats; ++mat) {
                    bf_split2(b0 * u[mat][2 * qp], b1 * u[mat][2 * qp + 1], hi, lo);
                    bh[mat][h][qp] = hi;
                    bl[mat][h][qp] = lo;
                }
            }
        fetch(i + 1 < w.tg ? i + 1 : i, pre);       // unconditional
        asm volatile("" ::: "memory");              // the loads are issued HERE, in front of the products
#pragma unroll
        for (int h = 0; h < 4; ++h)
#pragma unroll
            for (int gb = 0; gb < 4; ++gb) {        // hi hi, hi lo, lo hi: the matrices alternate inside each group
#pragma unroll
                for (int mat = 0; mat < kMats; ++mat) acc[mat][h][gb] = mfma16(ah[h], bh[mat][gb], acc[mat][h][gb]);
#pragma unroll
                for (int mat = 0; mat < kMats; ++mat) acc[mat][h][gb] = mfma16(ah[h], bl[mat][gb], acc[mat][h][gb]);
#pragma unroll
                for (int mat = 0; mat < kMats; ++mat) acc[mat][h][gb] = mfma16(al[h], bh[mat][gb], acc[mat][h][gb]);
            }
    }

    // The set leaves as doubles on fgram_pass's layout (fgram_elem: element (i, j) of a 16 x 16 block at register
    // (i & 15) >> 2 of lane 16 (i & 3) + j).  Result register r of lane 16 lq + lr of THIS instruction is row 4 lq + r,
    // column lr of the block: it goes to register slot lq, lane 16 r + lr.  Row blocks beyond the strip's last one were
    // redirected (strip_chunk_offsets): what they leave lies beyond row m and is never read.
    double* const set = q.partial + (size_t)w.set * q.set_stride;
    double* const dst = set + (size_t)fgram_sub(w.si, w.sj) * fgram_sub_doubles(kMats) + lr;
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
        for (int gb = 0; gb < 4; ++gb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int mat = 0; mat < kMats; ++mat)
                    dst[((mat * 16 + h * 4 + gb) * 4 + lq) * 64 + 16 * r] = (double)acc[mat][h][gb][r];
    fgram_store_row_sums(q, w, lq, lr, rs, fgram_row_limit(q, w));
    if constexpr (Point::kSumU2)
        if (w.si == 0) {                            // (sj = 0 too) as fgram_pass leaves it
            const double t = quad_sum(sg);
            if (lane == 0) set[q.rows_at + (size_t)q.nsl * kWaveRows] = t;
        }
}

}  // namespace bioen
