// k_strip_fwd / k_strip_adj: the two matrix passes of the log-weights method on the strip copies (layout and kernel
// arguments: strip.hpp).
#include "strip.hpp"

namespace bioen {

// ---- log-weights forward pass on the strip copy: partial[set mp K + row K + k] = sum_{j in the set's strips} Y'[row][j] e_k[j]
// (A4, c_bioen_common.c:70-108; replaces k_fwd_partial for M <= 1024).  The copy is stored in the operand
// order of this product, so the matrix goes HBM -> registers -> matrix cores: no LDS image, no shuffles, and the
// K vectors e_k enter once per BLOCK and strip (16 K doubles through LDS, loaded one strip ahead) instead of once
// per wave and KiB as in the streaming kernel, whose K = 8 launch took 1.28 x its K = 1 time for that reason.
// Geometry: a wave owns 64 rows of one strip (128 registers: 16 waves per CU).  A block is `spb` strip slots of
// `wps` waves each -- the whole CU for every M (M = 1024: 1 x 16, 512: 2 x 8, 256: 4 x 4, <= 128: 4 x 2) -- and does
// `spb` strips per iteration behind ONE barrier: with one strip per block a 256-row problem ran 4 blocks of 4 waves
// per CU, four times the barriers and per-strip bookkeeping per byte, at 4.8 TB/s instead of 6.9.  Slot `sub` of
// block B is partial set B spb + sub and takes the strips set + it * (sets): the assignment, and therefore every
// bit of the result, is that of one block per set.  A 64-row strip keeps a second, idle wave per slot (the 16 K
// threads that stage e need up to two waves): it re-reads the first one's rows and stores nothing.
// One register set (one strip in flight per wave, 128 KB per CU).  r03 tried two (110-126 VGPRs, no spill, loop
// unrolled by two as in k_strip): 2418-2443 vs 2432-2438 us of matrix kernels per headline round, 84.7 vs 82 us at
// N = 1e5 x M = 256 -- no gain: the ~7 TB/s these passes reach is the memory system's rate for this stream, not a
// shortage of bytes in flight.
template <int K, bool NT, int STORE = 0>
__global__ __launch_bounds__(1024) void k_strip_fwd(StripArgs q, Vec8 v) {
    constexpr int NK = (K + 3) / 4;
    __shared__ double tv[2][4][8 * kStripCols];                   // [parity][slot][problem][column]
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int sub = wave / q.wps, rw = wave - sub * q.wps;
    const int rbase = rw * kWaveRows;
    const int rsrc = rbase < q.mps ? rbase : 0;
    const int lq = lane >> 4, lj = lane & 3;

    double acc[kWaveRows / 16][NK];
#pragma unroll
    for (int h = 0; h < kWaveRows / 16; ++h)
#pragma unroll
        for (int kq = 0; kq < NK; ++kq) acc[h][kq] = 0.0;
    for (int i = t; i < 2 * 4 * 8 * kStripCols; i += blockDim.x) (&tv[0][0][0])[i] = 0.0;   // problems k >= K of a quad stay zero

    const bool p2 = t < q.spb * kStripCols * K;                   // slot t / 16 K, problem (t % 16 K) / 16, column t % 16
    const int psub = p2 ? t / (kStripCols * K) : 0;
    const int pk = p2 ? (t - psub * kStripCols * K) >> 4 : 0, pc = t & 15;
    const double* vk = v.p[0];                                    // chosen by comparison, not by a lane-indexed (vector) load
#pragma unroll
    for (int k = 1; k < K; ++k)
        if (pk == k) vk = v.p[k];
    d2 pre[kWaveRows / 8];
    f4 rhi[4];                                                     // reduced formats (STORE != 0): the wave's slice as it is stored
    u4 rlo[2];
    double cen[kWaveRows / 16];                                    // centre of the lane's row in each of its four row blocks
#pragma unroll
    for (int h = 0; h < kWaveRows / 16; ++h) {
        const int row = rsrc + 16 * h + (lane & 15);
        cen[h] = (STORE == 0 && row < q.mp) ? q.center[row] : 0.0;     // the reduced copies hold the centred operand
    }
    const size_t wave_off = (size_t)rsrc * kStripCols + (size_t)lane * 2;
    int choff[kWaveRows / 8];
    strip_chunk_offsets(q.mps, rsrc, choff);
    auto fetch = [&](int strip) {
        if constexpr (STORE == 0) {
            const double* src = q.Ys + (size_t)strip_phys(strip, q.sps, q.ilv) * q.mps * kStripCols + wave_off;
#pragma unroll
            for (int i = 0; i < kWaveRows / 8; ++i) pre[i] = ldg2<NT>(src + choff[i]);
        } else {
            constexpr int SB = reduced_slice_bytes<STORE>();
            const unsigned char* src = reinterpret_cast<const unsigned char*>(q.Ys) +
                                       ((size_t)strip * (q.mps / kWaveRows) + (size_t)(rsrc / kWaveRows)) * SB + (size_t)lane * 16;
#pragma unroll
            for (int u = 0; u < 4; ++u) rhi[u] = ldg16<NT, f4>(src + u * 1024);
            if constexpr (STORE == 1) {
#pragma unroll
                for (int u = 0; u < 2; ++u) rlo[u] = ldg16<NT, u4>(src + 4096 + u * 1024);
            }
        }
    };
    // canonical sets (kernels.hpp: StripSets): the wave's slot and the slot this thread stages e for
    const SlotWork mw = strip_slot(q, blockIdx.x * q.spb + sub);
    const SlotWork pw = strip_slot(q, blockIdx.x * q.spb + psub);
    int trips = 0;                                                 // the block's iterations: its longest slot's (block-uniform)
    for (int i = 0; i < q.spb; ++i) trips = max(trips, strip_slot(q, blockIdx.x * q.spb + i).count);
    const int safe = mw.count > 0 ? mw.first : 0;                  // a strip the wave may touch when it has none of its own left
    double ecur = (p2 && pw.count > 0) ? vk[(size_t)pw.first * kStripCols + pc] : 0.0;
    fetch(safe);
    __syncthreads();
    // fold: the slot runs a whole group and adds up its chunks (tc strips each) in turn, from +0.0 -- what the consumer
    // does with the sets of a launch that runs one chunk per slot (k_fwd_rows_local_t): the same bits either way
    double tot[kWaveRows / 16][NK];
#pragma unroll
    for (int h = 0; h < kWaveRows / 16; ++h)
#pragma unroll
        for (int kq = 0; kq < NK; ++kq) tot[h][kq] = 0.0;
    int tcnt = 0;
    for (int it = 0, par = 0; it < trips; ++it, par ^= 1) {
        if (p2) tv[par][psub][pk * 16 + pc] = ecur;               // loaded during the previous strip
        ecur = (p2 && it + 1 < pw.count) ? vk[(size_t)(pw.first + q.gs * (it + 1)) * kStripCols + pc] : 0.0;   // (without these loads: -2 %; nontemporal: +1 %)
        __syncthreads();                                           // this strip's e is in place; the buffer of parity
                                                                   // `par` is rewritten two strips on, behind another barrier
        double bv[4][NK];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
#pragma unroll
            for (int kq = 0; kq < NK; ++kq) bv[qq][kq] = tv[par][sub][(4 * kq + lj) * 16 + 4 * qq + lq];
        // consecutive instructions go to different accumulators (a result is ready three issue slots later)
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
#pragma unroll
            for (int h = 0; h < kWaveRows / 16; ++h) {
                double a;
                if constexpr (STORE == 0) {
                    const d2 y = pre[2 * h + (qq >> 1)];
#if STRIP_PRECENTERED
                    a = (qq & 1) ? y.y : y.x;
#else
                    a = ((qq & 1) ? y.y : y.x) - cen[h];               // the centring (r02: stored in the copy)
#endif
                } else {
                    a = reduced_elem<STORE, 4>(rhi, rlo, 2 * h + (qq >> 1), qq & 1);
                }
#pragma unroll
                for (int kq = 0; kq < NK; ++kq)
                    acc[h][kq] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, bv[qq][kq], acc[h][kq], 0, 0, 0);
            }
        // unconditional (see k_strip_adj); the operands are consumed at issue.  Past its last strip a wave re-reads a
        // strip it may touch (its last one, or strip 0) against e = 0
#if FWD_DIAG & 1
        fetch(min((int)(blockIdx.x * q.spb + sub + (it + 1) * gridDim.x * q.spb), q.nstrips - 1));
#else
        fetch(it + 1 < mw.count ? mw.first + q.gs * (it + 1) : (mw.count > 0 ? mw.first + q.gs * (mw.count - 1) : 0));
#endif
        if (!(FWD_DIAG & 2) && q.fold && ++tcnt == q.tc) {                            // a chunk ends (block-uniform; registers only)
            tcnt = 0;
#pragma unroll
            for (int h = 0; h < kWaveRows / 16; ++h)
#pragma unroll
                for (int kq = 0; kq < NK; ++kq) {
                    tot[h][kq] += acc[h][kq];
                    acc[h][kq] = 0.0;
                }
        }
    }
    if (q.fold) {                                                  // the group's last, shorter chunk (or + 0.0)
#pragma unroll
        for (int h = 0; h < kWaveRows / 16; ++h)
#pragma unroll
            for (int kq = 0; kq < NK; ++kq) acc[h][kq] = tot[h][kq] + acc[h][kq];
    }
    {
        // result lane 16 i + 4 blk + j: row rbase + 16 h + 4 blk + i, problem 4 kq + j
        const int rr = rbase + 4 * ((lane >> 2) & 3) + lq;
#pragma unroll
        for (int h = 0; h < kWaveRows / 16; ++h)
#pragma unroll
            for (int kq = 0; kq < NK; ++kq) {
                const int row = rr + 16 * h, k = 4 * kq + lj;
                if (mw.live && row < q.mp && k < K)     // transposed: a set's sums are one run; rows beyond the strip: zero
                    q.partial[(size_t)mw.set * q.pstride * K + (size_t)row * K + k] = row < q.mps ? acc[h][kq] : 0.0;
            }
    }
}

// ---- log-weights adjoint pass on the strip copy (column-sum operand order):
//   out_k[j] = sum_i u_ik (Y_ij - ybar_ik) = sum_i Y'_ij u_ik + shift_k,   shift_k = sum_i u_ik (center_i - ybar_ik)
// (A6, c_bioen_kernels_logw.c:185-205; replaces k_adj for M <= 1024).  HBM -> registers -> matrix cores and the block
// geometry as in the forward pass; u = r (compact [row K + k]) sits in an LDS table in B-operand reach, the partial
// column sums of a slot's waves meet in LDS (two buffers by strip parity: one barrier per iteration), 16 K threads per
// slot add the shift and store.
// One register set, as in the forward pass.  r06 tried two here (the strip after next requested before the products of the
// next one start, loop unrolled by two, same bits; profiles/r06_adj_depth_ab.txt): K <= 4: 1.18-1.21 ms per launch at
// N = 1e6 x M = 1024 against 1.17-1.21 (nothing), K > 4: 1.71 ms against 1.21-1.26 (the second set does not fit beside
// 2 x 16 operand registers of u).  What a launch takes moves by 4-5 % with the process and the box (the first 0.2 s of a
// process, where the copy landed in HBM: tools/pass_probe.py shows it for both passes and for the plain read probe alike),
// not with bytes in flight.  Nor does it help at K > 4 to move the 16 centred operands out of the load registers first and
// request the next strip before the 32 products (what the one-copy form k_strip2<ADJ> gains 4 % from, below): 1.231-1.258 ms
// either way at N = 1e6 x M = 1024, K = 8 (three alternations, one box).
template <int K, bool NT, int STORE = 0>
__global__ __launch_bounds__(1024) void k_strip_adj(StripArgs q, MVec8 out, MVec8 scal) {
    constexpr int NK = (K + 3) / 4;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nwaves = blockDim.x >> 6;
    const int lrows = q.wps * kWaveRows;                          // the table holds 64 rows per wave of a slot
    double* ul = lds;                                             // u[row][8], zero beyond K and mp
    double* cl = ul + (size_t)lrows * 8;                          // centre[row] (16 per lane in registers would spill at K = 8)
    double* red = cl + lrows;                                     // [parity][wave][problem 8][column 16]
    const int sub = wave / q.wps, rw = wave - sub * q.wps;
    const int rbase = rw * kWaveRows;
    const int rsrc = rbase < q.mps ? rbase : 0;                   // the idle second wave of a 64-row strip re-reads the first one's rows
    const int lq = lane >> 4, lj = lane & 3;
    const int stride = gridDim.x * q.spb;
    for (int i = t; i < lrows * 8; i += blockDim.x) {
        const int row = i >> 3, k = i & 7;
        ul[i] = (row < q.mp && k < K) ? q.u_c[(size_t)row * K + k] : 0.0;
    }
    for (int i = t; i < lrows; i += blockDim.x) cl[i] = i < q.mp ? q.center[i] : 0.0;
    const bool p2 = t < q.spb * kStripCols * K;                   // slot t / 16 K, problem (t % 16 K) / 16, column t % 16
    const int psub = p2 ? t / (kStripCols * K) : 0;
    const int pk = p2 ? (t - psub * kStripCols * K) >> 4 : 0, pc = t & 15;
    double shift = 0.0;
    double* outk = out.p[0];                                      // chosen by comparison, not by a lane-indexed (vector) load
    const double* sck = scal.p[0];
#pragma unroll
    for (int k = 1; k < K; ++k)
        if (pk == k) {
            outk = out.p[k];
            sck = scal.p[k];
        }
    if (p2 && q.accumulate == 0) shift = sck[S_B0] - sck[S_UY];
    d2 pre[kWaveRows / 8];
    f4 rhi[4];                                                     // reduced formats (STORE != 0)
    u4 rlo[2];
    const size_t wave_off = (size_t)rsrc * kStripCols + (size_t)lane * 2;
    int choff[kWaveRows / 8];
    strip_chunk_offsets(q.mps, rsrc, choff);
    auto fetch = [&](int strip) {
        if constexpr (STORE == 0) {
            const double* src = q.Ys + (size_t)strip * q.mps * kStripCols + wave_off;
#pragma unroll
            for (int i = 0; i < kWaveRows / 8; ++i) pre[i] = ldg2<NT>(src + choff[i]);
        } else {
            constexpr int SB = reduced_slice_bytes<STORE>();
            const unsigned char* src = reinterpret_cast<const unsigned char*>(q.Ys) +
                                       ((size_t)strip * (q.mps / kWaveRows) + (size_t)(rsrc / kWaveRows)) * SB + (size_t)lane * 16;
#pragma unroll
            for (int u = 0; u < 4; ++u) rhi[u] = ldg16<NT, f4>(src + u * 1024);
            if constexpr (STORE == 1) {
#pragma unroll
                for (int u = 0; u < 2; ++u) rlo[u] = ldg16<NT, u4>(src + 4096 + u * 1024);
            }
        }
    };
    int base = blockIdx.x * q.spb;                                 // strip of slot 0: < nstrips for every block
    int sw = base + sub, sp = base + psub;                         // this wave's strip / the strip this thread stores for
    fetch(sw < q.nstrips ? sw : base);
    __syncthreads();                                              // ul in place
    const double* pu = ul + (size_t)(rbase + lq) * 8 + lj;
    const double* pc_ = cl + (rsrc + lq);                         // the centre of row group g: pc_[4 g]
    const int nown = (q.mps + kWaveRows - 1) / kWaveRows;
    for (int par = 0; base < q.nstrips; base += stride, sw += stride, sp += stride, par ^= 1) {
        double* redw = red + (size_t)par * nwaves * 128;
        {
            double d[4][NK];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch)
#pragma unroll
                for (int kq = 0; kq < NK; ++kq) d[ch][kq] = 0.0;
            double b1[kWaveRows / 4][NK];
#pragma unroll
            for (int g = 0; g < kWaveRows / 4; ++g)
#pragma unroll
                for (int kq = 0; kq < NK; ++kq) b1[g][kq] = pu[g * 32 + 4 * kq];
#pragma unroll
            for (int g = 0; g < kWaveRows / 4; ++g) {
                double a;
                if constexpr (STORE == 0) {
#if STRIP_PRECENTERED
                    a = (g & 1) ? pre[g >> 1].y : pre[g >> 1].x;
#else
                    a = ((g & 1) ? pre[g >> 1].y : pre[g >> 1].x) - pc_[4 * g];   // the centring (r02: stored in the copy)
#endif
                } else {
                    a = reduced_elem<STORE, 4>(rhi, rlo, g >> 1, g & 1);
                }
#pragma unroll
                for (int kq = 0; kq < NK; ++kq)
                    d[g & 3][kq] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b1[g][kq], d[g & 3][kq], 0, 0, 0);
            }
            // unconditional (past its last strip a wave re-reads one it may touch): a conditional prefetch makes the
            // compiler's vmcnt bookkeeping assume the loads may not exist, and every wait then drains them all
            const int nxt = sw + stride;
            fetch(nxt < q.nstrips ? nxt : (sw < q.nstrips ? sw : base));   // the operands are consumed at issue
            const int c = 4 * ((lane >> 2) & 3) + lq;             // result lane 16 i + 4 blk + j: column 4 blk + i, problem 4 kq + j
#pragma unroll
            for (int kq = 0; kq < NK; ++kq)
                redw[wave * 128 + (4 * kq + lj) * 16 + c] = (d[0][kq] + d[1][kq]) + (d[2][kq] + d[3][kq]);
        }
        __syncthreads();            // the buffer of this parity is rewritten two strips on, behind the next barrier
        if (p2 && sp < q.nstrips) {
            double colsum = 0.0;
            for (int wv = 0; wv < nown; ++wv) colsum += redw[(psub * q.wps + wv) * 128 + pk * 16 + pc];
#if ADJ_DIAG & 1
            if (colsum == 1.2345e300) outk[(size_t)sp * kStripCols + pc] = colsum + shift;
#else
            // streamed past the L2 (no write-allocate): a plain store here cost 3 % of the pass -- the 8 K bytes per
            // column are 0.8 % of the traffic, without any store the pass runs at the forward pass's time.  (r03, tried
            // and dropped: contiguous runs of strips per block with the outputs staged in LDS and written as KiB runs --
            // which strip a block takes changes no bit here.  One run per block: 1 % SLOWER at N = 1e6 x M = 1024, the
            // blocks' reads no longer sweep the HBM channels together; runs of 8 strips dealt round-robin: +0.2..0.7 %,
            // within the noise, and the uneven last run costs as much.)
            // (a row panel behind the first one of a matrix taller than 1024 rows continues its predecessors' sums)
            const double start = q.accumulate == 1 ? outk[(size_t)sp * kStripCols + pc] : shift;     // (2: shift stayed 0)
            __builtin_nontemporal_store(colsum + start, outk + (size_t)sp * kStripCols + pc);
#endif
        }
    }
}

void run_k_strip_fwd(bioen_hip_ctx* c, const StripArgs& q, const Vec8& v, dim3 block, const StripForm& f) {
    const dim3 grid((q.nslots + q.spb - 1) / q.spb);
    for_width(f.K, [&](auto k) {
        for_value<1, 0>(f.nt, [&](auto nt) {
            for_value<1, 2, 0>(f.store, [&](auto st) {
                constexpr int K = decltype(k)::value, STORE = decltype(st)::value;
                constexpr bool NT = decltype(nt)::value != 0;
                BIOEN_LAUNCH_TIMED(c, (k_strip_fwd<K, NT, STORE>), grid, block, 0, q, v);
            });
        });
    });
}

void run_k_strip_adj(bioen_hip_ctx* c, const StripArgs& q, const MVec8& out, const MVec8& scal, dim3 block, size_t lds,
                     const StripForm& f) {
    const dim3 grid((q.nblk + q.spb - 1) / q.spb);
    for_width(f.K, [&](auto k) {
        for_value<1, 0>(f.nt, [&](auto nt) {
            for_value<1, 2, 0>(f.store, [&](auto st) {
                constexpr int K = decltype(k)::value, STORE = decltype(st)::value;
                constexpr bool NT = decltype(nt)::value != 0;
                allow_big_lds<&k_strip_adj<K, NT, STORE>>(c);
                BIOEN_LAUNCH_TIMED(c, (k_strip_adj<K, NT, STORE>), grid, block, lds, q, out, scal);
            });
        });
    });
}

}  // namespace bioen
