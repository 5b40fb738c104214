// Forces method, M <= 1024: the dense Hessian for a Newton minimizer from SPLIT-BF16 operands on the BF16 matrix cores
// (gfx950).  The mathematics, the sets, their order and the layout of what a set leaves are k_forces_gram's
// (kernels_forces_gram.hip); only the two M x M x N products change precision:
//   a = Y_ij - centre_i (FP64)        a_hi = bf(a),  a_lo = bf((float)a - a_hi)          bf: float, then bfloat16, both
//   t = a u_j           (FP64)        t_hi = bf(t),  t_lo = bf((float)t - t_hi)              round-to-nearest-even
//   G'[u]_ik = sum_j (a_hi t_hi + a_hi t_lo + a_lo t_hi)        v_mfma_f32_16x16x16_bf16, f32 accumulators
// The row sums g = sum_j u2_j Y'_j stay k_forces_gram's FP64 fma chains (they feed a cancellation): the same bits.
//
// The strip copy's registers (row = lane & 15, the strip's columns 4 qq + (lane >> 4) in qq = 0 .. 3) are a 16-row, 16-deep
// BF16 operand as they stand: element qq of a lane's fragment is depth index 4 (lane >> 4) + qq of the instruction, for the A
// and the B operand alike, so the instruction contracts over the strip's 16 columns in a permuted order.  A wave owns a
// 64 x 64 sub-tile of both matrices (2 x 16 accumulators of 4 floats), a block of four waves a 128 x 128 tile pair I >= J, as
// in k_forces_gram.  A set's f32 sums leave as doubles on k_forces_gram's layout, so the sets are added IN FP64 in its
// fixed order by its k_fgram_sum_sets, and k_fgram_finish / k_fgram_square finish them: launch_fgram_tail, that file's,
// launches those three kernels as they are.  What a wave does around its arithmetic is fgram.hpp's, shared with that kernel.
#include "fgram.hpp"

namespace bioen {

// (the split and the 16-deep instruction -- bf_split2, mfma16 -- are fgram.hpp's, shared with k_logw_gram_bf16)
struct FGram16Regs {
    d2 a[kWaveRows / 8];
    d2 b[kWaveRows / 8];
    double w0, x, qv;                // the strip's column lane & 15: a lane forms the weights of ONE column, the others arrive by shuffles
};

__global__ __launch_bounds__(256, 1) void k_forces_gram_bf16(FGramArgs q) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lq = lane >> 4, lr = lane & 15;
    FGramWave w;
    if (!fgram_decode(q, lane, wave, w)) return;
    const double logs = q.pscal[S_LOGS];
    double ca[4], cb[4];                            // the centres of the lane's rows
    fgram_centres(q, w, lr, ca, cb);

    auto fetch = [&](int i, FGram16Regs& r) {
        const int s = fgram_strip(q, w, i);
        fgram_fetch(q, w, s, r.a, r.b);
        const size_t col = (size_t)s * kStripCols + lr;
        r.w0 = q.w0[col];
        r.x = q.x[col];
        r.qv = q.qv[col];
    };

    fl4 acc1[4][4], acc2[4][4];                     // [row block of slice si][row block of slice sj]
    double rs[4];                                   // the lane's share of the row sums of Y' u2 (slice si)
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        rs[h] = 0.0;
#pragma unroll
        for (int gb = 0; gb < 4; ++gb) {
            acc1[h][gb] = fl4{0.f, 0.f, 0.f, 0.f};
            acc2[h][gb] = fl4{0.f, 0.f, 0.f, 0.f};
        }
    }

    // One register set, as in k_forces_gram: a strip's operands are centred, weighted and split into registers of their own
    // as soon as it has arrived, the set is refilled with the NEXT strip, which travels while this one is multiplied.
    FGram16Regs pre;
    fetch(0, pre);
#pragma unroll 1
    for (int i = 0; i < w.tg; ++i) {
        // the point's weights as k_forces_gram forms them (the same operations, so the same bits), columns beyond n weigh
        // nothing -- formed once per column (lane & 15) and handed to the lanes that multiply with them: 4 qq + lq
        const size_t colc = (size_t)fgram_strip(q, w, i) * kStripCols + lr;
        const double e = exp(pre.x - logs);
        const double u1c = colc < (size_t)q.n ? pre.w0 * e : 0.0;
        const double u2c = u1c * pre.qv;
        double u1[4], u2[4];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            u1[qq] = __shfl(u1c, 4 * qq + lq, 64);
            u2[qq] = __shfl(u2c, 4 * qq + lq, 64);
        }
        u2v ah[4], al[4], b1h[4], b1l[4], b2h[4], b2l[4];       // [row block]: the fragments, element qq = column quad qq
#pragma unroll
        for (int h = 0; h < 4; ++h)
#pragma unroll
            for (int qp = 0; qp < 2; ++qp) {                    // the column quads 2 qp (.x) and 2 qp + 1 (.y)
                const d2 av = pre.a[2 * h + qp], bv = pre.b[2 * h + qp];
                const double a0 = av.x - ca[h], a1 = av.y - ca[h];
                const double b0 = bv.x - cb[h], b1 = bv.y - cb[h];
                rs[h] = fma(a0, u2[2 * qp], rs[h]);
                rs[h] = fma(a1, u2[2 * qp + 1], rs[h]);
                unsigned hi, lo;
                bf_split2(a0, a1, hi, lo);
                ah[h][qp] = hi;
                al[h][qp] = lo;
                bf_split2(b0 * u1[2 * qp], b1 * u1[2 * qp + 1], hi, lo);
                b1h[h][qp] = hi;
                b1l[h][qp] = lo;
                bf_split2(b0 * u2[2 * qp], b1 * u2[2 * qp + 1], hi, lo);
                b2h[h][qp] = hi;
                b2l[h][qp] = lo;
            }
        fetch(i + 1 < w.tg ? i + 1 : i, pre);         // unconditional
        asm volatile("" ::: "memory");              // the loads are issued HERE, in front of the products
#pragma unroll
        for (int h = 0; h < 4; ++h)
#pragma unroll
            for (int gb = 0; gb < 4; ++gb) {
                acc1[h][gb] = mfma16(ah[h], b1h[gb], acc1[h][gb]);
                acc2[h][gb] = mfma16(ah[h], b2h[gb], acc2[h][gb]);
                acc1[h][gb] = mfma16(ah[h], b1l[gb], acc1[h][gb]);
                acc2[h][gb] = mfma16(ah[h], b2l[gb], acc2[h][gb]);
                acc1[h][gb] = mfma16(al[h], b1h[gb], acc1[h][gb]);
                acc2[h][gb] = mfma16(al[h], b2h[gb], acc2[h][gb]);
            }
    }

    // The set leaves as doubles on k_forces_gram's layout (fgram_elem: element (i, j) of a 16 x 16 block at register
    // (i & 15) >> 2 of lane 16 (i & 3) + j).  Result register r of lane 16 lq + lr of THIS instruction is row 4 lq + r,
    // column lr of the block: it goes to register slot lq, lane 16 r + lr.  Row blocks beyond the strip's last one were
    // redirected (strip_chunk_offsets): what they leave lies beyond row m and is never read (k_fgram_finish).
    double* const dst = q.partial + (size_t)w.set * q.set_stride + (size_t)fgram_sub(w.si, w.sj) * fgram_sub_doubles(2) + lr;
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
        for (int gb = 0; gb < 4; ++gb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dst[((0 * 16 + h * 4 + gb) * 4 + lq) * 64 + 16 * r] = (double)acc1[h][gb][r];
                dst[((1 * 16 + h * 4 + gb) * 4 + lq) * 64 + 16 * r] = (double)acc2[h][gb][r];
            }
    fgram_store_row_sums(q, w, lq, lr, rs);
}

// ---- host side ------------------------------------------------------------------------------------
// buf: forces_gram_plan's doubles (a buffer of this entry's own); x, pscal, qv, ybar: the kept point's.  Leaves C~ at
// buf + cov_at, H~ at buf + tail_at.
void launch_forces_gram_bf16(bioen_hip_ctx* c, const GramPlan& p, double* buf, const double* x, const double* pscal,
                             const double* qv, const double* ybar, double theta) {
    hipLaunchKernelGGL(k_forces_gram_bf16, dim3(fgram_blocks(p)), dim3(256), 0, c->stream,
                       fgram_args(c, p, buf, x, pscal, qv));
    launch_fgram_tail(c, p, buf, ybar, theta);
}

}  // namespace bioen
