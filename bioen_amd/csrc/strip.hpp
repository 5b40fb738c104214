// Strip-major matrix passes: what their translation units share -- the layout of the copies, the kernel arguments and the
// small host interface between the files:
//   kernels_strip512.hip   k_strip      forces passes M <= 512, one-copy log-weights adjoint      } one kernel family each,
//   kernels_strip1024.hip  k_strip2     the same for 512 < M <= 1024                              } with the launcher that
//   kernels_strip_logw.hip k_strip_fwd, k_strip_adj   log-weights forward / adjoint pass          } instantiates it
//   kernels_strip_copy.hip the copies: construction, layouts, life cycle, read-back
//   strip_plan.cpp         geometry and launch planning: the public launch_* functions of kernels.hpp
//
// Forces method, M <= 1024 (k_strip: M <= 512; k_strip2: 512 < M <= 1024): the whole evaluation in TWO passes over a strip-major copy of yTilde, with both
// products of each pass on the FP64 matrix cores (v_mfma_f64_4x4x4_4b_f64).
//
// Reference: _get_weights_from_forces (c_bioen_kernels_forces.c:111-224), _bioen_log_posterior_forces
// (:227-277), _grad_bioen_log_posterior_forces (:280-340) -- five passes over the matrix there.
//
// Layout.  The row-major matrix serves the log-weights kernels (whole rows / 128-column strips of rows
// stream at 6.8 TB/s).  The forces evaluation needs whole COLUMNS (x_j = sum_i Y_ij f_i) and whole ROWS
// (ybar_i = sum_j Y_ij e_j) of the same data in one pass, i.e. a block must hold all rows of a few
// columns: 128-byte row segments 8 MB apart in the row-major matrix, which reach 4.9 TB/s at best (r01).
// So the matrix passes for M <= 1024 (log-weights: any M, over row panels of <= 1024 rows) read strip-major copies,
// built on first use:
//     Ys[strip s][row][c ^ swz(row)] = Y[row][16 s + c]          (raw numbers; rows padded to 16)
// * strip-major: the 16 columns x all rows a block works on are ONE contiguous chunk (64 KB at
//   M = 512) -- every wave-load is a contiguous KiB, as in the streaming kernels;
// * the kernels subtract center = YTilde (the targets, identical on every rank of a sharded context) from every
//   operand on its way from the load registers into the products: Y' = Y - center.  The softmax is invariant under
//   x_j -> x_j + const, ybar_i = center_i + sum_j Y'_ij w_j, the adjoint picks up the constant
//   B0 = sum_i center_i r_i, and the reference's centred gradient sum becomes
//       sum_j (Y_ij - ybar_i) t_j  =  sum_j Y'_ij t_j  -  (ybar_i - center_i) sum_j t_j
//   with BOTH terms at the scale of the data's spread instead of its offset: the plain matrix product
//   the matrix cores compute loses nothing to cancellation, and no per-problem centring is needed
//   inside the product.  (r02 stored Y' in the copies; the raw copies of r03 give the same operands -- the same
//   subtraction, a register later -- and let the copies REPLACE the row-major matrix: read_ytilde is exact from them.)
// * the XOR swizzle (columns permuted by bits 1..4 of the row) makes the LDS image of a strip -- a plain
//   copy, 16 doubles per row, no padding -- conflict-free for both operand fetch patterns below.
//
// Kernel (K = batch width as a template parameter, both passes from one template):
//   a wave owns 64 rows of the strip: it prefetches them two strips ahead (2 x 8 KiB in registers: 128 KB
//   in flight per CU), copies them to its slice of the LDS tile and is the only reader of that slice (no
//   block barrier around the tile);
//   P1  column sums  D1[c][k] = sum_i Y'[i][c] u[i][k]:  16 x ceil(K/4) matrix instructions per wave; A = 4 rows
//       x 16 columns from the tile, B = 4 rows x 4 problems of u = forces | residuals from an LDS table;
//       the waves' partial D1 meet in LDS                                                        -> barrier
//   P2  16 K threads (a problem's 16 columns in one 16-lane group): xy: x_j out, online softmax (running
//       maximum per block), e_j;   bt: t_j = (theta (1 + log w_j/w0_j) + b_j) w_j                 -> barrier
//   P3  row sums  D3[i][k] += sum_c Y'[i][c] v[c][k]:  16 x ceil(K/4) matrix instructions per wave into
//       persistent accumulators; A = 16 rows x 4 columns from the tile (fetched BEFORE the barriers: it does
//       not depend on P2), B = v (e | t) from LDS.
//   The 4x4x4 four-block form computes exactly the K <= 4 (or 8) problems -- the 16x16x4 form pads them to 16
//   at the same 32 FLOP/clk/SIMD, which is also the vector ALU's FP64 rate -- and delivers the cross-lane sums
//   of P1 without a single shuffle; all operand fetches of a phase are issued before its first instruction.
//   Measured (r02, N = 1e6 x M = 512, 4.1 GB per pass): 0.60 / 0.62 ms per pass at K = 1 (6.7 TB/s), 0.68 /
//   0.78 ms at K = 8, against 0.81 / 0.85 ms and 2.28 / 1.61 ms for the r01 kernels on the row-major matrix.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <type_traits>

#include "device_utils.hpp"

#ifndef STRIP_WAVES_PER_SIMD
#define STRIP_WAVES_PER_SIMD 2
#endif
#ifndef STRIP_DEPTH
#define STRIP_DEPTH 2      // strips in flight per wave (register sets)
#endif
#ifndef ADJ_DIAG
#define ADJ_DIAG 0      // diagnostic builds: 1 = no output stores in k_strip_adj (timing only: results are garbage)
#endif
#ifndef STRIP_DIAG
#define STRIP_DIAG 0      // diagnostic builds: 1 = no MFMAs, 2 = no matrix loads
#endif
#ifndef FWD_DIAG
#define FWD_DIAG 0        // diagnostic builds of k_strip_fwd (timing only, results are garbage): 1 = the blocks sweep the copy as ONE
#endif                    // front (slot s takes strips s, s + slots, ...: the r04 pattern), 2 = no chunk fold
#ifndef STRIP_PRECENTERED
#define STRIP_PRECENTERED 0   // diagnostic builds: 1 = the r02 layout (copies hold Y - centre, no subtraction in the kernels;
#endif                        // read_ytilde is then off by the centre): A/B of what the in-kernel centring costs

namespace bioen {

constexpr int kStripCols = 16;
constexpr int kWaveRows = 64;

// physical column of logical column c in row r:  c ^ strip_swz(r)
__device__ __forceinline__ int strip_swz(int row) { return (((row >> 1) & 7) << 1) ^ ((row >> 4) & 1); }

// Where strip s of the row-sum order copy lives (r06).  A context that holds ilv > 1 canonical segments (one GPU: all
// eight) stores the strips of its segments INTERLEAVED: strip r of local segment v at position r ilv + v.  The row-sum
// passes give every slot the strips g, g + gs, ... of ONE segment (kernels.hpp: StripSets), so in segment order the 256
// slots of a launch read eight windows of the copy a segment (1 GB at the headline) apart; interleaved, the same slots at
// the same moment read ONE contiguous window, as the whole-matrix sweep of r04 did -- which strips a set is summed over,
// and in which order, does not change (same bits), only where they lie.  Measured (tools/pass_probe.py, profiles/
// r06_fwd_ab.txt): 1.5-3 % of the forward pass on boxes whose memory system does not mind the eight windows, 7 % on those
// that do (r04's kernel 1.155-1.169 ms in the headline sweep against 1.247-1.253 ms for r05's on the same box).
__device__ __forceinline__ int strip_phys(int s, int sps, int ilv) {
    if (ilv <= 1) return s;
    const int v = s / sps;
    return (s - v * sps) * ilv + v;
}

// ---- one-time construction of the strip-major copy -------------------------------------------------
// Within a strip the 64-row slice of wave w is stored in the order the ROW-SUM product wants its matrix
// operand, so a wave-load (1 KiB, 16 B per lane) lands in the operand registers with no further movement:
//   chunk i = 2 h + qp (h = 16-row block 0..3, qp = column octet 0..1), lane l = 16 lq + lr:
//     .x = Y'[64 w + 16 h + lr][8 qp + lq]        (operand of column quad qq = 2 qp)
//     .y = Y'[64 w + 16 h + lr][8 qp + 4 + lq]    (                      qq = 2 qp + 1)
// The column-sum product reads the same data through an LDS image (row-major, 16 doubles per row, columns
// XOR-swizzled by strip_swz(row)), which the waves fill from those registers.
__device__ __forceinline__ size_t strip_pos(int row, int col) {          // index inside a strip (doubles)
    const int w = row >> 6, h = (row >> 4) & 3, lr = row & 15;
    const int qp = col >> 3, hi = (col >> 2) & 1, lq = col & 3;
    return ((size_t)((w * 4 + h) * 2 + qp) * 64 + (lq * 16 + lr)) * 2 + hi;
}

// The same strips in the operand order of the COLUMN-SUM product (the log-weights adjoint streams this one):
//   chunk i (row groups 2 i, 2 i + 1 of the wave's 64 rows), lane l = 16 lq + lr:
//     .x = Y'[64 w + 8 i + lq][lr]      .y = Y'[64 w + 8 i + 4 + lq][lr]
__device__ __forceinline__ size_t strip_pos_colsum(int row, int col) {
    const int w = row >> 6, g = (row >> 2) & 15, lq = row & 3;
    return ((size_t)(w * 8 + (g >> 1)) * 64 + (lq * 16 + col)) * 2 + (g & 1);
}

// A wave loads its 64-row slice of a strip as 8 chunks of 1 KiB; chunks 2 h and 2 h + 1 hold row block h (16 rows)
// in both operand orders.  Row blocks beyond the strip's last one (mps is a multiple of 16, not of 64) do not exist in
// the copy: their chunks are redirected to the slice's first row block.  Offsets in doubles, wave-uniform.
__device__ __forceinline__ void strip_chunk_offsets(int mps, int rsrc, int (&off)[kWaveRows / 8]) {
    const int nh = min(kWaveRows / 16, (mps - rsrc) / 16);       // row blocks of this wave's slice
#pragma unroll
    for (int i = 0; i < kWaveRows / 8; ++i) off[i] = __builtin_amdgcn_readfirstlane(((i >> 1) < nh ? i : (i & 1)) * 128);
}

// ---- reduced-byte storage EXPERIMENT (r04; SURVEY 7 "treat FP32/BF16-split as an experiment", 8 f4; never the default,
// never the headline): the log-weights matrix passes can stream copies that hold the CENTRED operand Y' = Y - centre as
//   STORE 1: fp32 high part + bf16 residual (6 bytes per element, |error| <= 2^-33 |Y'|), reassembled in FP64 registers,
//   STORE 2: fp32 (4 bytes, 2^-25 |Y'|),
// in the same operand orders.  A wave's 64-row slice of a strip (rows padded to 64 here) is one contiguous run: four
// 1-KiB loads of the high parts -- load u, lane l: {chunk 2u .x, .y, chunk 2u+1 .x, .y} of the FP64 layout above -- and,
// STORE 1, two 1-KiB loads of the residuals behind them -- load v, lane l, word w: chunk 4v + w, .x in the low half,
// .y in the high half.  Every load is 16 bytes per lane as in the FP64 stream; measured, tools/split_read_probe.hip:
// 6.87 TB/s for the 6-byte stream reassembled to FP64 = 1.31 x the elements per second of the 8-byte stream, 2.0 x for fp32.
typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned int u4 __attribute__((ext_vector_type(4)));
template <int STORE>
__host__ __device__ constexpr int reduced_slice_bytes() { return STORE == 1 ? 6144 : 4096; }

template <bool NT, class T>
__device__ __forceinline__ T ldg16(const void* p) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const T*>(p));
    return *reinterpret_cast<const T*>(p);
}
// element (.x | .y) of chunk i of the wave's slice(s), back in FP64; NH loads of high parts (chunks 2u, 2u + 1 in load u),
// NH / 2 loads of residuals (chunks 4v .. 4v + 3 in load v) -- NH = 4: one 64-row slice, 8: the two slices of 128 rows
template <int STORE, int NH>
__device__ __forceinline__ double reduced_elem(const f4 (&hi)[NH], const u4 (&lo)[NH / 2], int i, int xy) {
    const f4 h = hi[i >> 1];
    const int e = (i & 1) * 2 + xy;
    double d = (double)(e == 0 ? h.x : e == 1 ? h.y : e == 2 ? h.z : h.w);
    if (STORE == 1) {
        const u4 l = lo[i >> 2];
        const int wsel = i & 3;
        const unsigned w = wsel == 0 ? l.x : wsel == 1 ? l.y : wsel == 2 ? l.z : l.w;
        d += (double)__uint_as_float(xy ? (w & 0xffff0000u) : (w << 16));
    }
    return d;
}
// a wave's strip in flight: FP64 chunks, or the reduced formats' loads (the members a format does not use never exist)
template <int NCH>
struct StripRegs {
    d2 v[NCH];
    f4 hi[NCH / 2];
    u4 lo[NCH / 4];
};

struct StripArgs {
    const double* Ys;       // strip-major copy (raw matrix; the reduced formats: bytes, centred)
    const double* center;   // mp values subtracted from the rows on the way into the products (a zero vector: none)
    int mps;                // rows of a strip (multiple of 16)
    int mp;                 // rows of the operands u_c / outputs
    int nstrips;
    int n;                  // valid columns
    int K;
    int nblk;               // k_strip_adj: strip slots of the launch
    int wps, spb;           // k_strip_fwd / k_strip_adj: waves per strip slot, strips per block and iteration
    // canonical partial sets (kernels.hpp: StripSets) of the row-sum passes: k_strip_fwd, k_strip, k_strip2
    int sps, gs, tc, nch, fold, slots;
    int nslots;             // physical slots of the launch = slots x local segments (forces passes: = gs)
    int nlocal;             // local segments (forces passes: a block runs its group through all of them)
    int ilv;                // row-sum order FP64 copies: segments interleaved by this many (strip_phys); <= 1: strip order
    const double* u_c;      // [row * K + k]: forces (xy) | residuals (bt)
    const double* w0;
    double* partial;        // [block * mp K + row * K + k]  (transposed: device_utils.hpp, tiles_sum16)
    int pstride;            // k_strip_fwd: rows of the partial layout (= mp; a row panel of a taller matrix: the matrix's)
    int accumulate;         // k_strip_adj: 0 = start at `shift`, 1 = add to the outputs of the panels before this one, 2 = start at 0
    long long* stamps;      // diagnostic builds (STRIP_DIAG & 4): per wave 8 phase-cycle sums
};

// What physical slot `ps` of a row-sum pass works on (kernels.hpp: StripSets): the strips first, first + gs, ... (count
// of them) of local segment v = ps / slots -- a whole group (fold), or chunk cg of group g (slot r = cg gs + g of the
// segment: consecutive blocks read consecutive strips) -- and the set its sums go to.  count = 0: an empty chunk (a
// short group's last one) or a slot beyond the launch; its set is all zeros.
struct SlotWork {
    int first, count, set;
    int nsets, set_stride;      // forces passes: the sets the slot writes (set, set + set_stride, ...: one per chunk)
    bool live;
};
__device__ __forceinline__ SlotWork strip_slot(const StripArgs& q, int ps) {
    SlotWork w;
    w.live = ps < q.nslots;
    const int pss = w.live ? ps : 0;
    const int v = pss / q.slots, r = pss - v * q.slots;
    const int cg = r / q.gs, g = r - cg * q.gs;                 // fold: cg = 0
    const int tg = (q.sps - g + q.gs - 1) / q.gs;               // strips of group g (g < gs <= sps: at least one)
    const int t0 = q.fold ? 0 : cg * q.tc;
    const int t1 = q.fold ? tg : min(tg, t0 + q.tc);
    w.first = v * q.sps + g + q.gs * t0;
    w.count = (w.live && t1 > t0) ? t1 - t0 : 0;
    w.set = q.fold ? v * q.gs + g : (v * q.gs + g) * q.nch + cg;
    w.nsets = 1;
    w.set_stride = 0;
    return w;
}
// Forces passes: set (v, g) = the matrix-core chain over the strips g, g + gs, ... of segment v (gs = min(sps, full
// grid) groups per segment; no chunks).  Block g runs its group through the context's local segments one after the other
// -- all eight on one GPU, the 256 blocks sweeping one segment's strips side by side as they swept the whole matrix
// before r05; one on each of eight GPUs -- and writes a set at every segment's end.  Its strips as ONE sequence:
// number i is strip (i / tg) sps + g + gs (i % tg), tg = the group's strips per segment.
struct ForcesSlot {
    int g, tg, total, sps, gs;
    int flat;           // > 1 (ADJ on an interleaved copy): the slot's strips are POSITIONS g, g + gs, ... of the copy
    __device__ __forceinline__ int strip(int i) const {
        if (flat > 1) {                             // position p holds strip p / flat of local segment p % flat (strip_phys)
            const int p = g + gs * i;
            return (p % flat) * sps + p / flat;
        }
        const int v = i / tg;
        return v * sps + g + gs * (i - v * tg);
    }
};
// adj: the column-sum form on the one-copy path -- no sum over strips, so any assignment of strips to blocks gives the same
// bits; on a copy whose segments are interleaved (strip_phys) the blocks take the copy's positions in order, and at any
// moment read one contiguous window of it instead of every ilv-th strip of a window ilv times as wide
__device__ __forceinline__ ForcesSlot forces_slot(const StripArgs& q, int ps, bool adj = false) {
    ForcesSlot w;
    w.g = ps;
    w.sps = q.sps;
    w.gs = q.gs;
    w.flat = (adj && q.ilv > 1) ? q.ilv : 0;
    if (w.flat > 1) {
        w.total = (q.nstrips - ps + q.gs - 1) / q.gs;      // (ps < gs <= nstrips: at least one)
        w.tg = w.total + 1;                                 // never a segment's end: nothing is flushed in this form
        return w;
    }
    w.tg = (q.sps - ps + q.gs - 1) / q.gs;      // (ps < gs <= sps: at least one)
    w.total = w.tg * q.nlocal;
    return w;
}

// ---- host side ------------------------------------------------------------------------------------
// (internal to the strip translation units: kept out of the library's dynamic symbol table)
#pragma GCC visibility push(hidden)
inline int env_flag(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}

// Rows of a strip: M padded to the 16-row block of a matrix-core operand (r02 padded to a wave's 64 rows: M = 205
// streamed 256 rows, 20 % of the traffic for nothing; M = 28 streamed 64).  A wave still owns 64 rows of a strip; the
// last wave of a strip owns the 1..4 row blocks that exist, and the chunks of the others are redirected to its first
// row block (cache hits, multiplied with zero operands or never stored), so that every wave runs the same
// straight-line code and every sum is formed from the same terms in the same order as before.
// Matrices taller than 1024 rows (r03): the matrix passes run over row PANELS of <= 1024 rows -- the same two
// kernels once per panel, the forward pass writing its panel's rows of the partial sums, the adjoint pass continuing
// the column sums of the panels before it.  Until r03 that range ran the r01 streaming kernels (K = 8 forward pass 1.28 x
// its K = 1 time).  The panels are cut from the row-major matrix, which is freed once they exist (read-back and the
// fallback kernels gather it back from them: gather_block / ensure_rowmajor).  M <= 1024 is the one-panel case.
constexpr int kPanelRows = 1024;
inline bool paneled(const bioen_hip_ctx* c) { return c->mp > kPanelRows; }
inline int panel_count(const bioen_hip_ctx* c) { return paneled(c) ? (c->m + kPanelRows - 1) / kPanelRows : 1; }
inline int panel_m(const bioen_hip_ctx* c, int p) { return paneled(c) ? std::min(kPanelRows, c->m - p * kPanelRows) : c->m; }     // valid rows
inline int panel_mp(const bioen_hip_ctx* c, int p) { return paneled(c) ? std::min(kPanelRows, c->mp - p * kPanelRows) : c->mp; }  // operand rows
inline int panel_mps(const bioen_hip_ctx* c, int p) { return (int)round_up((size_t)panel_m(c, p), 16); }                          // strip rows
inline int strip_count(const bioen_hip_ctx* c) { return (int)(c->ld / kStripCols); }
inline int strip_sps(const bioen_hip_ctx* c) { return c->segcols / kStripCols; }
inline int strip_ilv(const bioen_hip_ctx* c) { return std::max(1, c->strip_ilv); }      // the layout the row-sum order copies ARE in
// reduced-storage experiment: rows of a reduced strip -- whole 64-row slices; 512 < M <= 1024: pairs of them (k_strip2's waves own 128 rows)
inline int reduced_rows(const bioen_hip_ctx* c) { return (int)round_up((size_t)c->m, c->mp > 512 ? 2 * kWaveRows : kWaveRows); }
bool one_copy_by_default(const bioen_hip_ctx* c);      // strip_plan.cpp

// P2 of the forces kernels (k_strip, k_strip2): what a strip's column sums become before the row-sum product takes them
enum StripMode : int {
    SM_BT = 0,          // pass 2 of the evaluation: b, t
    SM_XY = 1,          // pass 1: x out, online softmax, e
    SM_TANGENT = 2,     // pass 1 of a Hessian-vector product at a kept point: dx out, w dx
    SM_PRODUCT = 3,     // pass 2 of it: s
};

// Which instantiation of its family a launch runs: all the template parameters ever decide.
struct StripForm {
    int K;              // batch width 1 .. 8
    bool nt;            // nontemporal matrix loads
    bool xy;            // forces kernels: pass 1 (x, softmax, ybar) | pass 2 (b, t, Y' t)
    int mode;           // forces kernels: SM_TANGENT / SM_PRODUCT, the product's forms (else 0: xy decides)
    bool adj;           // forces kernels: the column-sum half alone (the one-copy log-weights adjoint)
    int depth;          // k_strip: 2 = two register sets, 1 = one, 3 = one + deferred row sums (the default at K > 4)
    int store;          // 0 FP64 | 1, 2: the reduced-storage experiment's copies
};
void run_k_strip(bioen_hip_ctx* c, const StripArgs& q, const ForcesRound& fr, dim3 block, size_t lds, const StripForm& f);
void run_k_strip2(bioen_hip_ctx* c, const StripArgs& q, const ForcesRound& fr, dim3 block, size_t lds, const StripForm& f);
void run_k_strip_fwd(bioen_hip_ctx* c, const StripArgs& q, const Vec8& v, dim3 block, const StripForm& f);
void run_k_strip_adj(bioen_hip_ctx* c, const StripArgs& q, const MVec8& out, const MVec8& scal, dim3 block, size_t lds, const StripForm& f);

// f(std::integral_constant<int, V>{}) for the V of the list that equals v; the LAST one serves every other value.
// The one dispatcher from run-time choices to template parameters: batch widths (for_width), flags, storage formats.
template <int V, int... Rest, class F>
void for_value(int v, F&& f) {
    if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, V>{});
    else if (v == V) f(std::integral_constant<int, V>{});
    else for_value<Rest...>(v, f);
}
template <class F>
void for_width(int K, F&& f) { for_value<1, 2, 3, 4, 5, 6, 7, 8>(K, f); }

// More than 64 KB of dynamic LDS needs an opt-in -- on the CURRENT device's copy of the kernel: once per (kernel, device),
// contexts of one process may sit on different devices
template <auto Kernel>
void allow_big_lds(const bioen_hip_ctx* c) {
    static std::atomic<unsigned long long> done{0};
    const unsigned long long bit = 1ull << (c->device & 63);
    if (done.load(std::memory_order_relaxed) & bit) return;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    done.fetch_or(bit, std::memory_order_relaxed);
}
#pragma GCC visibility pop

}  // namespace bioen
