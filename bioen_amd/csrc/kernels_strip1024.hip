// k_strip2: the forces passes and the one-copy log-weights adjoint for 512 < M <= 1024 (design, layout and kernel
// arguments: strip.hpp; the kernel it is the taller sibling of: kernels_strip512.hip).
#include "strip.hpp"

namespace bioen {

// ---- the same two passes for 512 < M <= 1024 (r03; until then the r01 kernels on the row-major matrix: 4.8 TB/s at K = 1,
// spilling at K = 8).  Sixteen waves of 64 rows would leave 128 registers per wave and need a 128-KB image beside the
// 64-KB operand table; instead EIGHT waves own 128 rows each (256 registers, as k_strip): a wave keeps its 16 KB of
// the strip in registers as the row-sum operands (a3) and passes it through its 8-KB slice of the LDS image in two
// halves of 64 rows for the column sums (P1 over the first half, rewrite, P1 over the second half, one chain of
// accumulators).  One register set in flight (the prefetch is issued as soon as a3 holds the strip): 8 waves x 16 KB =
// the 128 KB per CU the other strip kernels keep in flight.  Everything else -- operand maps, swizzle, P2, P3, the
// straight-line rules about vmcnt -- is k_strip's; kept as a kernel of its own so that the tuned M <= 512 code does not
// move by an instruction.
#ifndef STRIP2_GB2
#define STRIP2_GB2 2
#endif
template <int K, bool NT, int MODE, int STORE = 0, bool ADJ = false>        // MODE, ADJ: as in k_strip
__global__ __launch_bounds__(512, 2) void k_strip2(StripArgs q, ForcesRound fr) {
    constexpr bool XY = MODE == SM_XY;
    constexpr bool HP = MODE == SM_TANGENT || MODE == SM_PRODUCT;
    constexpr int RH = 2;                           // 64-row halves per wave
    constexpr int WR = 64 * RH;                     // rows per wave
    constexpr int NK = (K + 3) / 4;                 // problem quads
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nwaves = blockDim.x >> 6;
    const int lrows = nwaves * WR;
    double* tile = lds;                              // [wave][64 rows][16]: one half of a wave's rows at a time
    double* ul = tile + (size_t)nwaves * 64 * kStripCols;  // u[row][8]: forces | residuals, zero beyond K and mp
    double* red = ul + (size_t)lrows * 8;           // [wave][problem 8][column 16]: the waves' partial column sums
    double* tv = red + nwaves * 128;                // v[problem 8][column 16]: e | t of the strip
    double* scale = tv + 128;
    double* cl = scale + 16;                        // centre[row]
    const int rbase = wave * WR;
    const int rsrc = rbase < q.mps ? rbase : 0;     // rows the wave loads
    const int lq = lane >> 4, lr = lane & 15, lj = lane & 3;
    const ForcesSlot wk = forces_slot(q, blockIdx.x, ADJ);

    for (int i = t; i < lrows * 8; i += blockDim.x) {
        const int row = i >> 3, k = i & 7;
        ul[i] = (row < q.mp && k < K) ? q.u_c[(size_t)row * K + k] : 0.0;
    }
    for (int i = t; i < 128; i += blockDim.x) tv[i] = 0.0;         // problems k >= K of a quad stay zero
    for (int i = t; i < lrows; i += blockDim.x) cl[i] = i < q.mp ? q.center[i] : 0.0;
    if (!HP && t < 8) scale[t] = 1.0;

    // P3 accumulators: row block h (16 rows), problem quad kq: lane 16 i + 4 blk + j holds
    // row rbase + 16 h + 4 blk + i, problem 4 kq + j
    double acc[WR / 16][NK];
#pragma unroll
    for (int h = 0; h < WR / 16; ++h)
#pragma unroll
        for (int kq = 0; kq < NK; ++kq) acc[h][kq] = 0.0;

    // P2 state (threads t < 16 K: problem k = t / 16, column c = t % 16 -- a problem's 16 columns sit in one
    // 16-lane group, so the strip's maximum needs no LDS and no barrier)
    const bool p2 = t < kStripCols * K;
    const int pk = p2 ? t >> 4 : 0, pc = t & 15;
    double m_run = -DBL_MAX, zacc = 0.0, pxacc = 0.0;             // xy: running maximum, sum e, sum e x | bt: zacc = sum t
    double logs = 0.0, theta = 0.0, b0 = 0.0;
    // per-lane choice among the K kernel arguments by comparison (indexing the argument block with a lane value is
    // a vector load whose pending state forces vmcnt(0) -- a drain of the prefetch -- wherever the pointer is used)
    double* ak = fr.a[0];
    double* sck = fr.scal[0];
    double* pak = fr.part[0];
    double thk = fr.theta[0];
#pragma unroll
    for (int k = 1; k < K; ++k)
        if (pk == k) {
            if constexpr (!HP) ak = fr.a[k];        // (the product's forms: every direction reads the point's x, theta, S_LOGS)
            sck = fr.scal[k];
            pak = fr.part[k];
            if constexpr (!HP) thk = fr.theta[k];
        }
    if constexpr (HP) {
        logs = fr.scal[0][S_LOGS];
        theta = thk;
    } else if (!XY && p2) {
        logs = sck[S_LOGS];
        b0 = sck[S_B0];
        theta = thk;
    }
    // The product's forms (k_strip has the arguments' meaning).  This kernel has no register to spare beside a3 and the
    // prefetch: what is the same for every direction stays wave-uniform (above), and the direction's two constants of
    // SM_PRODUCT, dxbar and -cbar, wait in `scale`, which only the XY form uses otherwise.
    // ... and the direction's dx vector is chosen among the kernel arguments where it is used, not held across the strips.
    auto dx_of = [&]() {
        double* p = fr.w[0];
#pragma unroll
        for (int k = 1; k < K; ++k)
            if (pk == k) p = fr.w[k];
        return p;
    };
    if constexpr (HP) {
        if (MODE == SM_PRODUCT && p2 && pc == 0) {
            scale[2 * pk] = sck[S_SPARE0];
            scale[2 * pk + 1] = sck[S_B0];
        }
    }
    double shift = 0.0;                             // ADJ: k_strip_adj's constant (k_strip)
    if constexpr (ADJ) {                            // (accumulate: 0 = start at the shift, 1 = continue the panels before, 2 = start at 0)
        if (p2 && q.accumulate == 0) shift = sck[S_B0] - sck[S_UY];
    }

    // the wave's 16 KB of the next strip travel in registers
    StripRegs<WR / 8> pre;
    const size_t wave_off = (size_t)rsrc * kStripCols + (size_t)lane * 2;      // the wave's slice is contiguous in the copy
    int choff[WR / 8];                                                          // chunk -> chunk actually loaded (wave-uniform)
    {
        const int nh = min(WR / 16, (q.mps - rsrc) / 16);                       // row blocks of this wave's slice
#pragma unroll
        for (int i = 0; i < WR / 8; ++i) choff[i] = __builtin_amdgcn_readfirstlane(((i >> 1) < nh ? i : (i & 1)) * 128);
    }
    auto fetch_part = [&](int strip, int lo, int hi) {
        if constexpr (STORE == 0) {
            const double* src = q.Ys + (size_t)strip_phys(strip, q.sps, q.ilv) * q.mps * kStripCols + wave_off;
#pragma unroll
            for (int i = 0; i < WR / 8; ++i)
                if (i >= lo && i < hi) pre.v[i] = ldg2<NT>(src + choff[i]);
        } else {      // reduced-storage experiment: centred, rows padded to 128 here; a wave's two 64-row slices are adjacent
            constexpr int SB = reduced_slice_bytes<STORE>();
            const unsigned char* src = reinterpret_cast<const unsigned char*>(q.Ys) +
                                       ((size_t)strip * (q.mps / 64) + (size_t)(rsrc / 64)) * SB + (size_t)lane * 16;
#pragma unroll
            for (int u = 0; u < WR / 16; ++u)
                if (2 * u >= lo && 2 * u < hi) pre.hi[u] = ldg16<NT, f4>(src + (u >> 2) * SB + (u & 3) * 1024);
            if constexpr (STORE == 1) {
#pragma unroll
                for (int u = 0; u < WR / 32; ++u)
                    if (4 * u >= lo && 4 * u < hi) pre.lo[u] = ldg16<NT, u4>(src + (u >> 1) * SB + 4096 + (u & 1) * 1024);
            }
        }
    };
    auto fetch = [&](int strip) { fetch_part(strip, 0, WR / 8); };
    // K > 4: the operand batches of the column-sum product do not fit beside a3 AND the whole prefetch (7-12 registers
    // spilled per strip); the second half of the prefetch is issued behind that product instead
    // (r06) The ADJ form has no row-sum accumulators and no second operand table: the WHOLE prefetch fits in front of the
    // product at every K (174 registers, no spill) -- K = 5 / 8 at N = 1e6 x M = 1024: 1.167 / 1.19 ms per launch against
    // 1.222 / 1.235 with the split (three alternations, one box: profiles/r06_adj_prefetch_ab.txt); -DSTRIP2_ADJ_SPLIT=1
    // brings the split back for an A/B.  The order of the loads changes no bit.
#ifndef STRIP2_ADJ_SPLIT
#define STRIP2_ADJ_SPLIT 0
#endif
    constexpr int SPLIT = (NK > 1 && (!ADJ || STRIP2_ADJ_SPLIT)) ? WR / 16 : WR / 8;
    auto flush = [&](int set) {                                    // a segment's sums leave as one set; then everything starts from zero (k_strip)
        // result lane 16 i + 4 blk + j: row rbase + 16 h + 4 blk + i, problem 4 kq + j.  Row block by row block (16 rows x K
        // sums = one run of <= 128 doubles of the set) through the wave's own slice of `red` -- free here: the column sums of
        // the strip before have been consumed -- so that the sums leave as contiguous stores: as 8-byte stores 8 K bytes apart
        // (r02-r04, once per launch) eight flushes per block cost 7 % of a pass at K = 4 (partial-line writes: 0.75 TB/s)
        int lz = lane;
        asm volatile("" : "+v"(lz));      // opaque: keeps the address arithmetic of these stores out of the strip loop's registers
        double* const stg = red + wave * 128;
        const int rl = 4 * ((lz >> 2) & 3) + (lz >> 4);
#pragma unroll
        for (int h = 0; h < WR / 16; ++h) {
#pragma unroll
            for (int kq = 0; kq < NK; ++kq) {
                const int k = 4 * kq + (lz & 3);
                // rows between the strip's last row block and mp exist only in the M-vectors: their sums are zero (the
                // wave computed a redirected row block's there)
                if (k < K) stg[rl * K + k] = rbase + 16 * h + rl < q.mps ? acc[h][kq] : 0.0;
                acc[h][kq] = 0.0;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int nrun = min(16, q.mp - (rbase + 16 * h)) * K;          // (<= 0: rows beyond the operands; the idle second wave of a 64-row strip)
            double* const dst = q.partial + ((size_t)set * q.mp + rbase + 16 * h) * K;
            for (int i = lz; i < nrun; i += 64) __builtin_nontemporal_store(stg[i], dst + i);   // streamed: see k_strip_adj's outputs
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        double z = zacc, px = pxacc;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            z += __shfl_xor(z, o, 64);
            px += __shfl_xor(px, o, 64);
        }
        if (p2 && pc == 0) {
            double* pa = pak;
            if (XY) {
                pa[(size_t)P_MAX * kPartStride + set] = m_run;
                pa[(size_t)P_SUM * kPartStride + set] = z;
                pa[(size_t)P_PP * kPartStride + set] = px;
            } else {
                pa[(size_t)P_KL * kPartStride + set] = z;        // this set's share of sum_j t_j
            }
        }
        m_run = -DBL_MAX;
        zacc = 0.0;
        pxacc = 0.0;
    };
    auto one_strip = [&](int si, int flush_set) {   // si: number of the strip in the slot's sequence (k_strip)
        const int s = wk.strip(si);
        // the strip's centred values: the row-sum operands of P3, and the source of the LDS image below
        double a3[4][WR / 16];
        {
#pragma unroll
            for (int i = 0; i < WR / 8; ++i) {
                const int h = i >> 1, qp = i & 1;
                if constexpr (STORE == 0) {
                    const double ch = cl[rsrc + 16 * h + lr];
                    a3[2 * qp][h] = pre.v[i].x - ch;                              // the centring
                    a3[2 * qp + 1][h] = pre.v[i].y - ch;
                } else {
                    a3[2 * qp][h] = reduced_elem<STORE, WR / 16>(pre.hi, pre.lo, i, 0);
                    a3[2 * qp + 1][h] = reduced_elem<STORE, WR / 16>(pre.hi, pre.lo, i, 1);
                }
            }
        }
        if constexpr (!ADJ)
            if (flush_set >= 0) flush(flush_set);  // (block-uniform) a segment's first strip: the set of the segment before it,
                                                   // behind the wait for this strip's data and in front of its prefetch (k_strip)
        // P2's operands first, THEN the prefetch: vmcnt retires in order, a load issued behind the
        // prefetch would wait for the whole strip after next
        const size_t col = (size_t)s * kStripCols + pc;
        double w0v = 0.0, xv = 0.0;
        double dxv = 0.0, qv = 0.0;                 // PRODUCT: the direction's dx_j, the point's q_j - qbar
        double* dxp = nullptr;                      // TANGENT: where dx_j goes (formed here: `col` need not outlive P1)
        if constexpr (MODE == SM_TANGENT) dxp = dx_of() + col;
        const bool validc = col < (size_t)q.n;
        if constexpr (!ADJ) {
            if (p2) {
                w0v = q.w0[col];
                if (!XY) xv = ak[col];
                if constexpr (MODE == SM_PRODUCT) {
                    dxv = dx_of()[col];
                    qv = fr.t[0][col];
                }
            }
        } else {
            if (p2 && q.accumulate == 1) xv = ak[col];            // the column sums of the row panels before this one
        }
        const int nxt = si + 1 < wk.total ? wk.strip(si + 1) : s;
        fetch_part(nxt, 0, SPLIT);                 // unconditional, see k_strip_adj; `pre` is free: a3 holds the strip
        // ---- P1: D1[c][k] = sum_{i in the wave's rows} Y'[i][c] u[i][k], half by half through the LDS image ----
        {
            // four chains over the row groups (the result latency is 3 issues) for EVERY K: a problem's sums must not
            // depend on the width of its batch
            double d[4][NK];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch)
#pragma unroll
                for (int kq = 0; kq < NK; ++kq) d[ch][kq] = 0.0;
            const int sw3 = strip_swz(lr);          // row 16 h + lr of the half: only bit 0 of its swizzle depends on h
            double* img = tile + (size_t)(wave * 64 + lr) * kStripCols;
            const double* p1 = tile + (size_t)(wave * 64 + lq) * kStripCols;
#pragma unroll
            for (int half = 0; half < RH; ++half) {
                // registers -> image (row-major, swizzled: the same 16 rows x 2 columns per 32 lanes as a row-sum operand
                // fetch: conflict-free); the wave's own program order is the synchronisation of its private slice
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int hl = 0; hl < 4; ++hl)
#pragma unroll
                    for (int qp = 0; qp < 2; ++qp) {
                        img[hl * 256 + (((8 * qp + lq) ^ sw3) ^ (hl & 1))] = a3[2 * qp][4 * half + hl];
                        img[hl * 256 + (((8 * qp + 4 + lq) ^ sw3) ^ (hl & 1))] = a3[2 * qp + 1][4 * half + hl];
                    }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                // A: lane (kk = lq, blk, i) = Y'[r0 + lq][c = 4 blk + i = lr]; B: lane (kk = lq, blk, j) = u[r0 + lq][4 kq + j]
                const double* pu = ul + (size_t)(rbase + 64 * half + lq) * 8 + lj;
                // operand batches that fit beside a3 and the prefetch (K > 4 with the WHOLE prefetch in flight here, batches of
                // 4 | 2 | 1: 27-31 | 7-12 | 8-9 registers spilled; pass 1 / pass 2 at N = 1e6 x M = 1024, K = 8: 1.66 / 1.45 |
                // 1.50 / 1.39 | 1.51 / 1.41 ms; with the prefetch split around this product (SPLIT): none, 1.30 / 1.19 ms)
                constexpr int GB = NK > 1 ? STRIP2_GB2 : 8, NB = 16 / GB;
#pragma unroll
                for (int hb = 0; hb < NB; ++hb) {
                    double a1[GB], b1[GB][NK];
#pragma unroll
                    for (int gg = 0; gg < GB; ++gg) {
                        const int g = hb * GB + gg;
                        a1[gg] = p1[g * 64 + (lr ^ (((((lq >> 1) + 2 * g) & 7) << 1) ^ ((g >> 2) & 1)))];
#pragma unroll
                        for (int kq = 0; kq < NK; ++kq) b1[gg][kq] = pu[g * 32 + 4 * kq];
                    }
#pragma unroll
                    for (int gg = 0; gg < GB; ++gg)
#pragma unroll
                        for (int kq = 0; kq < NK; ++kq)
                            d[(hb * GB + gg) & 3][kq] =
                                __builtin_amdgcn_mfma_f64_4x4x4f64(a1[gg], b1[gg][kq], d[(hb * GB + gg) & 3][kq], 0, 0, 0);
                }
            }
            // result lane 16 i + 4 blk + j: column c = 4 blk + i, problem 4 kq + j
            const int c = 4 * ((lane >> 2) & 3) + lq;
#pragma unroll
            for (int kq = 0; kq < NK; ++kq)
                red[wave * 128 + (4 * kq + lj) * 16 + c] = (d[0][kq] + d[1][kq]) + (d[2][kq] + d[3][kq]);
        }
        if (SPLIT < WR / 8) fetch_part(nxt, SPLIT, WR / 8);
        __syncthreads();
        // ---- P2 ----
        if constexpr (ADJ) {
            if (p2) {                               // the waves' partial column sums in wave order, the constant, out
                double colsum = 0.0;
                const int nown = (q.mps + WR - 1) / WR;
                for (int wv = 0; wv < nown; ++wv) colsum += red[wv * 128 + pk * 16 + pc];
                __builtin_nontemporal_store(col < (size_t)q.n ? colsum + (q.accumulate == 1 ? xv : shift) : 0.0, ak + col);
            }
        } else if (t < kStripCols * K || (XY && wave < (kStripCols * K + 63) / 64)) {      // whole waves: the shuffles below
            double colsum = 0.0;
            if (p2) {
                const int nown = (q.mps + WR - 1) / WR;
                for (int wv = 0; wv < nown; ++wv) colsum += red[wv * 128 + pk * 16 + pc];
            }
            if (XY) {
                const bool valid = p2 && col < (size_t)q.n;
                if (p2) __builtin_nontemporal_store(valid ? colsum : 0.0, ak + col);   // streamed, see k_strip_adj (plain: +3..5 %)
                double smax = valid ? colsum : -DBL_MAX;          // the strip's maximum: over the 16 lanes of the problem
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) smax = fmax(smax, __shfl_xor(smax, o, 64));
                const double m_new = fmax(m_run, smax);
                // the running maximum rarely moves after the first strips: exp(0) = 1 exactly, skip it wave-wide
                double sc = 1.0;
                if (__any(m_new != m_run)) sc = exp(m_run - m_new);   // 0 the first time
                const double e = valid ? w0v * exp(colsum - m_new) : 0.0;
                zacc = fma(zacc, sc, e);
                pxacc = fma(pxacc, sc, valid ? e * colsum : 0.0);
                m_run = m_new;
                if (p2) {
                    if (pc == 0) scale[pk] = sc;
                    tv[pk * 16 + pc] = e;
                }
            } else if constexpr (HP) {                            // k_strip's forms of the same name
                if (p2) {
                    const bool valid = validc;
                    const double wv = w0v * exp(xv - logs);
                    double tval;
                    if constexpr (MODE == SM_TANGENT) {
                        __builtin_nontemporal_store(valid ? colsum : 0.0, dxp);
                        tval = valid ? wv * colsum : 0.0;
                    } else {
                        tval = valid ? wv * fma(dxv - scale[2 * pk], qv + theta, colsum + scale[2 * pk + 1]) : 0.0;
                    }
                    tv[pk * 16 + pc] = tval;
                    zacc += tval;
                }
            } else if (p2) {
                const double lrat = xv - logs;                    // log(w / w0)
                const double wv = w0v * exp(lrat);
                double dd = 1.0;
                if (wv >= DBL_MIN && w0v >= DBL_MIN) dd += lrat;  // c_bioen_kernels_forces.c:320-328
                const double tval = (dd * theta + (colsum + b0)) * wv;
                tv[pk * 16 + pc] = tval;
                zacc += tval;
            }
        }
        __syncthreads();
        // ---- P3: acc[row][k] (+)= sum_c Y'[row][c] v[c][k] ----
        // A: lane (kk = lq, blk, i) = Y'[r0 + 4 blk + i = r0 + lr][c = 4 qq + lq]; B: lane (kk, blk, j) = v[4 qq + lq][4 kq + j]
        if constexpr (!ADJ) {
            if (XY) {
#pragma unroll
                for (int kq = 0; kq < NK; ++kq) {
                    const double sc = scale[4 * kq + lj];
#pragma unroll
                    for (int h = 0; h < WR / 16; ++h) acc[h][kq] *= sc;
                }
            }
            double bv[4][NK];
#pragma unroll
            for (int qq = 0; qq < 4; ++qq)
#pragma unroll
                for (int kq = 0; kq < NK; ++kq) bv[qq][kq] = tv[(4 * kq + lj) * 16 + 4 * qq + lq];
#pragma unroll
            for (int qq = 0; qq < 4; ++qq)
#pragma unroll
                for (int h = 0; h < WR / 16; ++h)
#pragma unroll
                    for (int kq = 0; kq < NK; ++kq)
                        acc[h][kq] = __builtin_amdgcn_mfma_f64_4x4x4f64(a3[qq][h], bv[qq][kq], acc[h][kq], 0, 0, 0);
        }
        // no barrier here: the next strip's copy goes to the wave's own slice; red is rewritten only after
        // every wave has finished P2 of this strip (second barrier above), v only after the next first barrier.
    };
    fetch(wk.strip(0));                                            // total >= 1: the slot has a first strip
    __syncthreads();                                              // ul / tv / scale / cl initialised
    // straight through the local segments; a segment's first strip carries the flush of the segment before it (k_strip)
    int cnt = 0, vloc = 0;
    for (int i = 0; i < wk.total; ++i) {
        one_strip(i, (i > 0 && cnt == 0) ? (vloc - 1) * q.gs + wk.g : -1);
        if (++cnt == wk.tg) {
            cnt = 0;
            ++vloc;
        }
    }
    if constexpr (!ADJ) flush((vloc - 1) * q.gs + wk.g);           // the last segment's set
}

template <int K, bool NT, int MODE, int STORE, bool ADJ>
static void launch(bioen_hip_ctx* c, const StripArgs& q, const ForcesRound& fr, dim3 block, size_t lds) {
    allow_big_lds<&k_strip2<K, NT, MODE, STORE, ADJ>>(c);
    BIOEN_LAUNCH_TIMED(c, (k_strip2<K, NT, MODE, STORE, ADJ>), dim3(q.nblk), block, lds, q, fr);
}

void run_k_strip2(bioen_hip_ctx* c, const StripArgs& q, const ForcesRound& fr, dim3 block, size_t lds, const StripForm& f) {
    for_width(f.K, [&](auto k) {
        for_value<1, 0>(f.nt, [&](auto nt) {
            constexpr int K = decltype(k)::value;
            constexpr bool NT = decltype(nt)::value != 0;
            if (f.adj) return launch<K, NT, SM_XY, 0, true>(c, q, fr, block, lds);      // (FP64 copy only)
            if (f.mode == SM_TANGENT) return launch<K, NT, SM_TANGENT, 0, false>(c, q, fr, block, lds);      // the product's forms: FP64 copy only
            if (f.mode == SM_PRODUCT) return launch<K, NT, SM_PRODUCT, 0, false>(c, q, fr, block, lds);
            for_value<1, 0>(f.xy, [&](auto xy) {
                constexpr int XY = decltype(xy)::value != 0 ? SM_XY : SM_BT;
                for_value<1, 2, 0>(f.store, [&](auto st) { launch<K, NT, XY, decltype(st)::value, false>(c, q, fr, block, lds); });
            });
        });
    });
}

}  // namespace bioen
