// k_strip: the two matrix passes of the forces method for M <= 512 and, in its ADJ form, the log-weights adjoint on ONE
// strip copy (design, layout and kernel arguments: strip.hpp).
#include "strip.hpp"

namespace bioen {

// dynamic LDS: tile[mps * 16] | ul[mps * 8] | red[waves][8][16] | v[8][16] | scale[8]
//
// v_mfma_f64_4x4x4_4b_f64 (four independent 4x4x4 products per instruction, 16 cycles; maps measured with
// one-hot operands, tools/mfma_f64_4x4_probe.hip): lane l = 16 kk + 4 blk + r holds A_blk[i = r][kk],
// B_blk[kk][j = r]; the result lane 16 i + 4 blk + j holds D_blk[i][j].  Unlike the 16x16x4 form nothing is
// padded: K <= 4 problems take one instruction per operand fetch, K <= 8 two, at 32 FLOP/clk/SIMD either way.
// DEPTH: 2 = two register sets in flight (K <= 4), 1 = one; 3 (r04, K > 4) = one register set AND the row-sum product of
// strip s deferred behind the first barrier of strip s + 1, where it runs beside P2 of that strip on the waves P2 leaves
// idle: ONE barrier per strip, P3 off the serial chain (the partial-sum, e | t and rescale buffers are doubled by strip
// parity).  Same operands, same order of every sum: the bits of a problem do not depend on which form served it.
// ADJ (r05): the column-sum half of pass 1 alone -- out_k[j] = sum_i Y'_ij u_ik + shift_k, the log-weights ADJOINT
// (k_strip_adj's product) on the ROW-sum order copy: what lets the log-weights method run with ONE strip copy of the
// matrix (ctx.hpp: one_copy).  No softmax, no row sums, no sets; instantiated with MODE = SM_XY, DEPTH 2.
// MODE (strip.hpp: StripMode): SM_BT / SM_XY the two passes of the evaluation; SM_TANGENT / SM_PRODUCT the two passes of a
// Hessian-vector product at a kept point -- P2 forms of their own on the BT skeleton (no running maximum, no
// rescale, the set's share of sum_j tv_j in P_KL); P1, P3, the fetch, the flush and the strip loop are shared.
template <int K, bool NT, int MODE, int DEPTH = STRIP_DEPTH, int STORE = 0, bool ADJ = false>
__global__ __launch_bounds__(512, STRIP_WAVES_PER_SIMD) void k_strip(StripArgs q, ForcesRound fr) {
    constexpr bool XY = MODE == SM_XY;
    constexpr bool HP = MODE == SM_TANGENT || MODE == SM_PRODUCT;
    constexpr int NK = (K + 3) / 4;                 // problem quads
    constexpr bool DEFER = DEPTH == 3;
    constexpr int SETS = DEPTH == 2 ? 2 : 1;        // register sets (strips in flight per wave)
    constexpr int NBUF = DEFER ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int nwaves = blockDim.x >> 6;
    // Every wave of the block runs the same straight-line code (a branch around the prefetch makes the compiler's
    // vmcnt bookkeeping drain BOTH register sets at every wait, see k_strip_adj): LDS regions are sized for
    // 64 rows per wave, and the second wave of a 64-row strip (blocks have at least two waves: P2 needs up to 128
    // threads) re-reads the first wave's rows against zero operands and stores nothing.
    const int lrows = nwaves * kWaveRows;
    double* tile = lds;
    double* ul = tile + (size_t)lrows * kStripCols;  // u[row][8]: forces | residuals, zero beyond K and mp
    double* red = ul + (size_t)lrows * 8;           // [parity][wave][problem 8][column 16]: the waves' partial column sums
    double* tv = red + NBUF * nwaves * 128;         // [parity] v[problem 8][column 16]: e | t of the strip
    double* scale = tv + NBUF * 128;
    double* cl = scale + NBUF * 16;                 // centre[row]
    const int rbase = wave * kWaveRows;
    const int rsrc = rbase < q.mps ? rbase : 0;     // rows the wave loads
    const int lq = lane >> 4, lr = lane & 15, lj = lane & 3;
    const ForcesSlot wk = forces_slot(q, blockIdx.x, ADJ);

    for (int i = t; i < lrows * 8; i += blockDim.x) {
        const int row = i >> 3, k = i & 7;
        ul[i] = (row < q.mp && k < K) ? q.u_c[(size_t)row * K + k] : 0.0;
    }
    for (int i = t; i < NBUF * 128; i += blockDim.x) tv[i] = 0.0;  // problems k >= K of a quad stay zero
    for (int i = t; i < lrows; i += blockDim.x) cl[i] = i < q.mp ? q.center[i] : 0.0;
    if (t < NBUF * 16) scale[t] = 1.0;

    // P3 accumulators: row block h (16 rows), problem quad kq: lane 16 i + 4 blk + j holds
    // row rbase + 16 h + 4 blk + i, problem 4 kq + j
    double acc[kWaveRows / 16][NK];
#pragma unroll
    for (int h = 0; h < kWaveRows / 16; ++h)
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
            ak = fr.a[k];
            sck = fr.scal[k];
            pak = fr.part[k];
            thk = fr.theta[k];
        }
    if (!XY && p2) {
        logs = sck[S_LOGS];
        b0 = sck[S_B0];
        theta = thk;
    }
    // the product's forms: fr.a = the point's x (every direction the same), fr.w[k] = the direction's dx (TANGENT: out,
    // PRODUCT: in), fr.t = the point's q - qbar; the direction's scalars: S_LOGS (the point's), S_SPARE0 = dxbar, S_B0 = -cbar
    double* dxk = nullptr;
    double dxbar = 0.0;
    if constexpr (HP) {
        dxk = fr.w[0];
#pragma unroll
        for (int k = 1; k < K; ++k)
            if (pk == k) dxk = fr.w[k];
        if (MODE == SM_PRODUCT && p2) dxbar = sck[S_SPARE0];
    }
    double shift = 0.0;                             // ADJ: sum_i u_ik (center_i - ybar_ik), k_strip_adj's constant
    if constexpr (ADJ) {                            // (accumulate: 0 = start at the shift, 1 = continue the panels before, 2 = start at 0)
        if (p2 && q.accumulate == 0) shift = sck[S_B0] - sck[S_UY];
    }

    // the wave's 8 KB of the next TWO strips travel in registers (two sets, used alternately)
    using Regs = StripRegs<kWaveRows / 8>;
    Regs preA;
    Regs preB;                                      // (SETS == 1: never touched)
    double a3old[4][kWaveRows / 16];                // DEFER: the row-sum operands of the strip before this one
    const size_t wave_off = (size_t)rsrc * kStripCols + (size_t)lane * 2;      // the wave's slice is contiguous in the copy
    int choff[kWaveRows / 8];                                                   // chunk -> chunk actually loaded (wave-uniform)
    strip_chunk_offsets(q.mps, rsrc, choff);
    auto fetch = [&](int strip, Regs& pre) {
#if !(STRIP_DIAG & 2)
        if constexpr (STORE == 0) {
            const double* src = q.Ys + (size_t)strip_phys(strip, q.sps, q.ilv) * q.mps * kStripCols + wave_off;
#pragma unroll
            for (int i = 0; i < kWaveRows / 8; ++i) pre.v[i] = ldg2<NT>(src + choff[i]);
        } else {                                    // reduced-storage experiment: centred, rows padded to 64
            constexpr int SB = reduced_slice_bytes<STORE>();
            const unsigned char* src = reinterpret_cast<const unsigned char*>(q.Ys) +
                                       ((size_t)strip * (q.mps / kWaveRows) + (size_t)(rsrc / kWaveRows)) * SB + (size_t)lane * 16;
#pragma unroll
            for (int u = 0; u < 4; ++u) pre.hi[u] = ldg16<NT, f4>(src + u * 1024);
            if constexpr (STORE == 1) {
#pragma unroll
                for (int u = 0; u < 2; ++u) pre.lo[u] = ldg16<NT, u4>(src + 4096 + u * 1024);
            }
        }
#endif
    };
#if STRIP_DIAG & 4
    long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long tlast = __builtin_amdgcn_s_memtime();
#define STAMP(i) { const long long now_ = __builtin_amdgcn_s_memtime(); tacc[i] += now_ - tlast; tlast = now_; }
#else
#define STAMP(i)
#endif
    // ---- P3: acc[row][k] (+)= sum_c Y'[row][c] v[c][k] ----
    // A: lane (kk = lq, blk, i) = Y'[r0 + 4 blk + i = r0 + lr][c = 4 qq + lq]; B: lane (kk, blk, j) = v[4 qq + lq][4 kq + j]
    auto p3 = [&](double (&a3x)[4][kWaveRows / 16], const double* tvp, const double* scp) {
        if (XY) {
#pragma unroll
            for (int kq = 0; kq < NK; ++kq) {
                const double sc = scp[4 * kq + lj];
#pragma unroll
                for (int h = 0; h < kWaveRows / 16; ++h) acc[h][kq] *= sc;
            }
        }
#if !(STRIP_DIAG & 1)
        double bv[4][NK];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
#pragma unroll
            for (int kq = 0; kq < NK; ++kq) bv[qq][kq] = tvp[(4 * kq + lj) * 16 + 4 * qq + lq];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
#pragma unroll
            for (int h = 0; h < kWaveRows / 16; ++h)
#pragma unroll
                for (int kq = 0; kq < NK; ++kq)
                    acc[h][kq] = __builtin_amdgcn_mfma_f64_4x4x4f64(a3x[qq][h], bv[qq][kq], acc[h][kq], 0, 0, 0);
#else
        acc[0][0] += a3x[0][0] * tvp[lj * 16];
#endif
    };
    // A segment's sums leave as one set: the row sums and the set statistics; then everything starts from zero again
    // (pass 1: running maximum -DBL_MAX, so the next strip rescales by exp(-DBL_MAX - m) = 0 exactly as a block's first).
    // WHERE it is issued matters (r05, measured): the wave has two strips of loads in flight and waits for them with
    // vmcnt(N), N = the loads the compiler counts behind the one it needs.  Stores it does not count (they sit under a
    // block-uniform branch) issued BEHIND those loads make every such wait longer by as many of the YOUNGER loads -- the
    // strip after next -- as there are stores: 3-4 us per flush and block, 5-10 % of a pass with eight segments per block.
    // So the set of a finished segment leaves at the start of the NEXT segment's first strip, behind the wait for that
    // strip's own data and in front of its prefetch: then only the (fast) stores themselves stand in the way of a wait.
    auto flush = [&](int set) {
        // result lane 16 i + 4 blk + j: row rbase + 16 h + 4 blk + i, problem 4 kq + j.  Row block by row block (16 rows x K
        // sums = one run of <= 128 doubles of the set) through the wave's own slice of `red` -- free here: the column sums of
        // the strip before have been consumed -- so that the sums leave as contiguous stores: as 8-byte stores 8 K bytes apart
        // (r02-r04, once per launch) eight flushes per block cost 7 % of a pass at K = 4 (partial-line writes: 0.75 TB/s)
        int lz = lane;
        asm volatile("" : "+v"(lz));      // opaque: keeps the address arithmetic of these stores out of the strip loop's registers
        double* const stg = red + wave * 128;
        const int rl = 4 * ((lz >> 2) & 3) + (lz >> 4);
#pragma unroll
        for (int h = 0; h < kWaveRows / 16; ++h) {
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
        // set statistics per problem: sums over the problem's 16 columns (its 16-lane group)
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
    auto one_strip = [&](int si, Regs& pre, int par, bool first, int flush_set) {      // si: number of the strip in the slot's sequence
        const int s = wk.strip(si);
        double* const redp = red + (DEFER ? par * nwaves * 128 : 0);
        double* const tvp = tv + (DEFER ? par * 128 : 0);
        double* const scp = scale + (DEFER ? par * 16 : 0);
        // registers -> LDS image (row-major, swizzled) for the column sums; the same 16 rows x 2 columns per
        // 32 lanes as the row-sum operand fetch used to read: conflict-free.  The registers themselves ARE the
        // row-sum operands: kept in a3 until P3 (the prefetch below reuses `pre`).
        double a3[4][kWaveRows / 16];
        {
            const int sw3 = strip_swz(lr);          // row rbase + 16 h + lr: only bit 0 of its swizzle depends on h
            double* img = tile + (size_t)(rbase + lr) * kStripCols;
#pragma unroll
            for (int i = 0; i < kWaveRows / 8; ++i) {
                const int h = i >> 1, qp = i & 1;
                double vx, vy;
                if constexpr (STORE == 0) {
                    const double ch = cl[rsrc + 16 * h + lr];
#if STRIP_PRECENTERED
                    vx = pre.v[i].x, vy = pre.v[i].y;
#else
                    vx = pre.v[i].x - ch, vy = pre.v[i].y - ch;                   // the centring (r02: stored in the copy)
#endif
                } else {
                    vx = reduced_elem<STORE, 4>(pre.hi, pre.lo, i, 0);
                    vy = reduced_elem<STORE, 4>(pre.hi, pre.lo, i, 1);
                }
                a3[2 * qp][h] = vx;
                a3[2 * qp + 1][h] = vy;
                img[h * 256 + (((8 * qp + lq) ^ sw3) ^ (h & 1))] = vx;
                img[h * 256 + (((8 * qp + 4 + lq) ^ sw3) ^ (h & 1))] = vy;
            }
        }
        // wave-private slice of the tile: the wave's own program order is the synchronisation
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        STAMP(0)    // waited for the strip, copied it to LDS
        if constexpr (!ADJ) {
            if (flush_set >= 0) {                   // (block-uniform) the first strip of a segment: the set of the one before it
                if constexpr (DEFER) {              // ... whose last strip's deferred row sums run now
                    __syncthreads();                // its e | t are in place
                    p3(a3old, tv + (par ^ 1) * 128, scale + (par ^ 1) * 16);
                }
                flush(flush_set);
            }
        }
        // P2's operands first, THEN the prefetch: vmcnt retires in order, a load issued behind the
        // prefetch would wait for the whole strip after next
        const size_t col = (size_t)s * kStripCols + pc;
        double w0v = 0.0, xv = 0.0;
        double dxv = 0.0, qv = 0.0;                 // PRODUCT: the direction's dx_j, the point's q_j - qbar
        if constexpr (!ADJ) {
            if (p2) {
                w0v = q.w0[col];
                if (!XY) xv = ak[col];
                if constexpr (MODE == SM_PRODUCT) {
                    dxv = dxk[col];
                    qv = fr.t[0][col];
                }
            }
        } else {
            if (p2 && q.accumulate == 1) xv = ak[col];            // the column sums of the row panels before this one
        }
        fetch(si + SETS < wk.total ? wk.strip(si + SETS) : s, pre);   // unconditional, see k_strip_adj
        // ---- P1: D1[c][k] = sum_{i in the wave's rows} Y'[i][c] u[i][k] ----
        // A: lane (kk = lq, blk, i) = Y'[r0 + lq][c = 4 blk + i = lr]; B: lane (kk = lq, blk, j) = u[r0 + lq][4 kq + j]
        {
            double d[4][NK];                        // four chains over the row groups: the result latency is 3 issues
#pragma unroll
            for (int ch = 0; ch < 4; ++ch)
#pragma unroll
                for (int kq = 0; kq < NK; ++kq) d[ch][kq] = 0.0;
            // row rbase + 4 g + lq: its swizzle has period 8 in g (rbase is a multiple of 64): compile-time
            // offsets on four per-lane bases address all of P1
            const double* p1 = tile + (size_t)(rbase + lq) * kStripCols;
            const double* pu = ul + (size_t)(rbase + lq) * 8 + lj;
#if !(STRIP_DIAG & 1)
            // all operand fetches of a batch first (one LDS round trip instead of sixteen), then its matrix
            // instructions; K > 4 takes two batches of eight row groups: one batch of 16 x 3 operands does not fit
            // beside the two register sets in flight (the compiler spilled 2..22 values per strip)
            constexpr int NB = NK > 1 ? 2 : 1, GB = kWaveRows / 4 / NB;
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
                        d[gg & 3][kq] = __builtin_amdgcn_mfma_f64_4x4x4f64(a1[gg], b1[gg][kq], d[gg & 3][kq], 0, 0, 0);
            }
#else
            d[0][0] = p1[lr] * pu[0];
#endif
            // result lane 16 i + 4 blk + j: column c = 4 blk + i, problem 4 kq + j
            const int c = 4 * ((lane >> 2) & 3) + lq;
            double* redw = redp;
#pragma unroll
            for (int kq = 0; kq < NK; ++kq)
                redw[wave * 128 + (4 * kq + lj) * 16 + c] = (d[0][kq] + d[1][kq]) + (d[2][kq] + d[3][kq]);
        }
        STAMP(1)    // issued the prefetch, P1
        __syncthreads();
        STAMP(2)    // first barrier
        // ---- P2 ----
        if constexpr (ADJ) {
            if (p2) {                               // the waves' partial column sums in wave order, the constant, out
                double colsum = 0.0;
                const int nown = (q.mps + kWaveRows - 1) / kWaveRows;
                for (int wv = 0; wv < nown; ++wv) colsum += redp[wv * 128 + pk * 16 + pc];
                __builtin_nontemporal_store(col < (size_t)q.n ? colsum + (q.accumulate == 1 ? xv : shift) : 0.0, ak + col);
            }
        } else if (t < kStripCols * K || (XY && wave < (kStripCols * K + 63) / 64)) {      // whole waves: the shuffles below
            double colsum = 0.0;
            if (p2) {
                const int nown = (q.mps + kWaveRows - 1) / kWaveRows;
                for (int wv = 0; wv < nown; ++wv) colsum += redp[wv * 128 + pk * 16 + pc];
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
                    if (pc == 0) scp[pk] = sc;
                    tvp[pk * 16 + pc] = e;
                }
            } else if constexpr (HP) {
                if (p2) {
                    const bool valid = col < (size_t)q.n;
                    const double wv = w0v * exp(xv - logs);       // the point's weight, as the BT form makes it
                    double tval;
                    if constexpr (MODE == SM_TANGENT) {           // dx_j out, tv = w_j dx_j
                        __builtin_nontemporal_store(valid ? colsum : 0.0, dxk + col);
                        tval = valid ? wv * colsum : 0.0;
                    } else {                                      // tv = s_j = w_j [(dx_j - dxbar)(q_j - qbar + theta) + c_j - cbar]
                        tval = valid ? wv * fma(dxv - dxbar, qv + theta, colsum + b0) : 0.0;
                    }
                    tvp[pk * 16 + pc] = tval;
                    zacc += tval;
                }
            } else if (p2) {
                const double lrat = xv - logs;                    // log(w / w0)
                const double wv = w0v * exp(lrat);
                double dd = 1.0;
                if (wv >= DBL_MIN && w0v >= DBL_MIN) dd += lrat;  // c_bioen_kernels_forces.c:320-328
                const double tval = (dd * theta + (colsum + b0)) * wv;
                tvp[pk * 16 + pc] = tval;
                zacc += tval;
            }
        }
        STAMP(3)    // P2
        if constexpr (DEFER) {
            // no second barrier: the row sums of the strip BEFORE this one run here, beside P2 of this strip (its e | t and
            // rescale factors sit in the other parity's buffers, complete since the barrier above); this strip's own
            // row-sum operands wait in a3old for the next turn
            if (!first) p3(a3old, tv + (par ^ 1) * 128, scale + (par ^ 1) * 16);
#pragma unroll
            for (int qq = 0; qq < 4; ++qq)
#pragma unroll
                for (int h = 0; h < kWaveRows / 16; ++h) a3old[qq][h] = a3[qq][h];
            STAMP(4)
        } else {
            __syncthreads();
            STAMP(4)    // second barrier (ADJ: `red` may be rewritten)
            if constexpr (!ADJ) p3(a3, tvp, scp);
        }
        STAMP(5)    // P3
        // no barrier here: the next strip's copy goes to the wave's own slice; red is rewritten only after
        // every wave has finished P2 of this strip (second barrier above), v only after the next first barrier.
    };
    // The slot's strips, number 0 .. total - 1, straight through the local segments.  The two register sets of DEPTH 2
    // alternate strip by strip whatever the segments' lengths; the first strip of a segment carries the flush of the
    // segment before it (above), the last segment's set leaves behind the loop.
    int cnt = 0, vloc = 0;
    auto pending = [&](int i) { return (i > 0 && cnt == 0) ? (vloc - 1) * q.gs + wk.g : -1; };   // the set to flush at strip i
    auto count = [&]() {
        if (++cnt == wk.tg) {
            cnt = 0;
            ++vloc;
        }
    };
    fetch(wk.strip(0), preA);                                      // total >= 1: the slot has a first strip
    if constexpr (DEPTH == 2) fetch(wk.total > 1 ? wk.strip(1) : wk.strip(0), preB);
    __syncthreads();                                              // ul / tv / scale initialised
    if constexpr (DEPTH == 2) {
        // both halves and both prefetches unconditional inside the loop (see k_strip_adj); an odd last strip is peeled
        int i = 0;
        for (; i + 1 < wk.total; i += 2) {
            one_strip(i, preA, 0, false, pending(i));
            count();
            one_strip(i + 1, preB, 1, false, pending(i + 1));
            count();
        }
        if (i < wk.total) {
            one_strip(i, preA, 0, false, pending(i));
            count();
        }
    } else if constexpr (DEFER) {
        int par = 0;
        for (int i = 0; i < wk.total; ++i, par ^= 1) {
            const int fs = pending(i);
            one_strip(i, preA, par, i == 0 || fs >= 0, fs);       // (a segment's first strip: the deferred row sums of the strip
            count();                                              //  before it have run with the flush)
        }
        __syncthreads();                                          // the last strip's e | t are in place
        p3(a3old, tv + (par ^ 1) * 128, scale + (par ^ 1) * 16);
    } else {
        for (int i = 0, par = 0; i < wk.total; ++i, par ^= 1) {
            one_strip(i, preA, par, false, pending(i));
            count();
        }
    }
    if constexpr (!ADJ) flush((vloc - 1) * q.gs + wk.g);           // the last segment's set
#if STRIP_DIAG & 4
    if (q.stamps && lane == 0)
        for (int i = 0; i < 8; ++i) q.stamps[((size_t)blockIdx.x * 16 + wave) * 8 + i] = tacc[i];
#endif
}

template <int K, bool NT, int MODE, int DEPTH, int STORE, bool ADJ>
static void launch(bioen_hip_ctx* c, const StripArgs& q, const ForcesRound& fr, dim3 block, size_t lds) {
    allow_big_lds<&k_strip<K, NT, MODE, DEPTH, STORE, ADJ>>(c);
    BIOEN_LAUNCH_TIMED(c, (k_strip<K, NT, MODE, DEPTH, STORE, ADJ>), dim3(q.nblk), block, lds, q, fr);
}

// Instantiated: the ADJ form with two register sets on the FP64 copy; K <= 4: two register sets; K > 4: the deferred form
// (DEPTH 3) and, on the FP64 copy only, the two r03 forms it replaced (f.depth 1 / 2: strip_plan.cpp, BIOEN_HIP_STRIP_DEPTH5)
void run_k_strip(bioen_hip_ctx* c, const StripArgs& q, const ForcesRound& fr, dim3 block, size_t lds, const StripForm& f) {
    for_width(f.K, [&](auto k) {
        for_value<1, 0>(f.nt, [&](auto nt) {
            constexpr int K = decltype(k)::value;
            constexpr bool NT = decltype(nt)::value != 0;
            if (f.adj) return launch<K, NT, SM_XY, 2, 0, true>(c, q, fr, block, lds);
            // the product's forms: the FP64 copy, the width's default depth
            if (f.mode == SM_TANGENT) return launch<K, NT, SM_TANGENT, (K > 4 ? 3 : 2), 0, false>(c, q, fr, block, lds);
            if (f.mode == SM_PRODUCT) return launch<K, NT, SM_PRODUCT, (K > 4 ? 3 : 2), 0, false>(c, q, fr, block, lds);
            for_value<1, 0>(f.xy, [&](auto xy) {
                constexpr int XY = decltype(xy)::value != 0 ? SM_XY : SM_BT;
                if constexpr (K > 4) {
                    if (!f.store && f.depth != 3)
                        return for_value<1, 2>(f.depth, [&](auto d) { launch<K, NT, XY, decltype(d)::value, 0, false>(c, q, fr, block, lds); });
                }
                for_value<1, 2, 0>(f.store, [&](auto st) { launch<K, NT, XY, (K > 4 ? 3 : 2), decltype(st)::value, false>(c, q, fr, block, lds); });
            });
        });
    });
}

}  // namespace bioen
