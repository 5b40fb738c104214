// Strip-major matrix passes, host side: geometry (which kernel, how many blocks, which canonical sets) and the launch
// functions of kernels.hpp.  The kernels and their launchers: kernels_strip512.hip, kernels_strip1024.hip,
// kernels_strip_logw.hip; the copies: kernels_strip_copy.hip; layout and kernel arguments: strip.hpp.
#include "strip.hpp"

namespace bioen {

// ---- geometry ------------------------------------------------------------------------------------
// The regimes: M <= 512 k_strip (a wave owns 64 rows), 512 < M <= 1024 k_strip2 (128 rows per wave), beyond that row
// panels (strip.hpp), on which only the log-weights kernels and the ADJ forms run.
bool strip_panels(const bioen_hip_ctx* c) { return paneled(c); }
static bool strip_tall(int mp) { return mp > 512; }

// block shape of the forces kernels (k_strip / k_strip2) on strips of mps rows with mp operand rows
struct ForcesBlock {
    int threads;
    size_t lds;
};
static ForcesBlock forces_block(int mps, int mp, bool deferred = false) {
    const int per_wave = strip_tall(mp) ? 2 * kWaveRows : kWaveRows;
    const size_t waves = std::max(2, (mps + per_wave - 1) / per_wave);
    // image: 64 rows per wave (k_strip2: one half at a time) | operand table and centres: the wave's rows | partial column
    // sums per wave | e or t | rescale factors
    size_t doubles = waves * kWaveRows * kStripCols + waves * per_wave * (8 + 1) + waves * 128 + 128 + 16;
    if (deferred) doubles += waves * 128 + 128 + 16;        // k_strip, DEPTH 3: the last three doubled by strip parity
    return {(int)(64 * waves), doubles * sizeof(double)};
}
static ForcesBlock forces_block(const bioen_hip_ctx* c) { return forces_block(panel_mps(c, 0), c->mp); }

static int forces_per_cu(const bioen_hip_ctx* c) {
    // blocks per CU: LDS (160 KiB) and the waves per SIMD the kernel's register budget admits
    const ForcesBlock b = forces_block(c);
    const int by_lds = (int)((size_t)160 * 1024 / b.lds);
    const int by_waves = 4 * STRIP_WAVES_PER_SIMD / (b.threads / 64);
    return std::max(1, std::min(std::min(by_lds, by_waves), 4));
}
// the one-copy adjoint: as many blocks per CU as the forces passes run (M <= 128: four of two waves, <= 256: two of four,
// else one); on row panels one
static int one_copy_adj_per_cu(const bioen_hip_ctx* c) { return paneled(c) ? 1 : forces_per_cu(c); }

// canonical sets of a row-sum pass whose full grid is `gs_nominal` slots per segment (kernels.hpp: StripSets)
static StripSets make_sets(const bioen_hip_ctx* c, int gs_nominal, bool may_fold) {
    StripSets ss{};
    ss.sps = strip_sps(c);
    ss.gs = std::max(1, std::min(ss.sps, gs_nominal));
    const int tmax = (ss.sps + ss.gs - 1) / ss.gs;
    ss.tc = (tmax + 7) / 8;
    ss.nch = (tmax + ss.tc - 1) / ss.tc;
    // a context that holds all eight segments runs whole groups per slot (8 x gs slots: the full grid) and adds up the
    // chunks in registers; BIOEN_HIP_STRIP_FOLD=0: one chunk per slot there too (the same bits:
    // tests/test_hip_strip_loops.py::test_unfolded_forward_pass_gives_the_folded_bits, at chunks of two strips)
    ss.fold = (may_fold && c->vr >= 8 && env_flag("BIOEN_HIP_STRIP_FOLD", 1) != 0) ? 1 : 0;
    ss.slots = ss.gs * (ss.fold ? 1 : ss.nch);
    ss.sets = ss.slots;
    return ss;
}

StripSets forces_sets(const bioen_hip_ctx* c) {        // gs = 0: the strip passes do not apply to this context
    static const bool tall_off = env_flag("BIOEN_HIP_STRIP_TALL", 1) == 0;     // the streaming kernels for 512 < M <= 1024 (A/B)
    if (paneled(c) || (strip_tall(c->mp) && tall_off) || c->strips_unavailable) return StripSets{};
    // one set per (segment, group): gs = the full grid of a GPU holding ONE segment (or every strip of the segment); a
    // block runs its group through the local segments (strip.hpp: ForcesSlot)
    StripSets ss{};
    ss.sps = strip_sps(c);
    ss.gs = std::max(1, std::min(ss.sps, 256 * forces_per_cu(c)));
    ss.tc = (ss.sps + ss.gs - 1) / ss.gs;
    ss.nch = 1;
    ss.fold = 0;
    ss.slots = ss.gs;
    ss.sets = ss.gs;
    return ss;
}

int forces_fused_blocks(const bioen_hip_ctx* c) {      // sets per SEGMENT of the forces strip passes; 0: not applicable
    return forces_sets(c).sets;
}

// geometry of the 16-wave kernels (k_strip_fwd / k_strip_adj): waves per strip slot, slots per block -- on row panels
// every panel uses that of a full 1024-row panel
static int fa_wps_rows(int mps) { return std::max(2, (mps + kWaveRows - 1) / kWaveRows); }
static int fa_spb_rows(int mps) { return std::max(1, std::min(16 / fa_wps_rows(mps), 4)); }
static int fa_spb(const bioen_hip_ctx* c) { return fa_spb_rows(paneled(c) ? kPanelRows : panel_mps(c, 0)); }

// forward pass of the log-weights method on the strip copy (all K <= 8): the number of partial sets
StripSets strip_sets(const bioen_hip_ctx* c) { return make_sets(c, 32 * fa_spb(c), true); }

// > 0: the log-weights matrix passes run on the strip copies; the value = sets of the forward pass that reach memory
// on this context (all local segments: what a consumer that totals them as one run is given)
int fwd_strip_blocks(const bioen_hip_ctx* c) {
    if (c->fwd_stream || c->strips_unavailable) return 0;
    if (paneled(c) && (c->panel_off || panel_count(c) > bioen_hip_ctx::kMaxPanels)) return 0;
    return strip_sets(c).sets * c->vr;
}

// ONE strip copy or two?  (r06: the default depends on the size.)  one_copy_wanted: 1 / 0 = asked for / refused
// (BIOEN_HIP_ONE_COPY, bioen_hip_ctx_set_one_copy), -1 = by size: a second copy of more than 1 GiB is not made.  With the
// one-copy adjoint taking the copy's positions in order (forces_slot: flat) it runs at the two-copy kernel's time wherever
// the matrix is large (profiles/r06_onecopy_ab.txt: headline sweep 1.306-1.316 s on one copy against 1.307-1.315 s on two,
// adjoint 1.203-1.209 against 1.201-1.212 ms; M = 512 x 1e6, 1024 x 1.25e5, 256 x 1e5: equal; M <= 128: a launch of the
// LDS-image kernel costs 12 us against 6), so the 8.2 GB the headline's second copy took are no longer spent by default;
// small problems keep the faster dedicated kernel.  Decided on the GLOBAL matrix (every rank of a sharded context takes
// the same form: the bits of a result must not depend on the GPU count).
bool one_copy_by_default(const bioen_hip_ctx* c) {
    if (c->one_copy_wanted >= 0) return c->one_copy_wanted == 1;
    const double global_copy_bytes = (double)round_up((size_t)c->m, 16) * (double)c->n_global * sizeof(double);
    return global_copy_bytes > 1024.0 * 1024.0 * 1024.0;
}

// ---- launch plans ----------------------------------------------------------------------------------
// What every strip launch shares: panel p of the row-sum (colsum: column-sum) order copy, its centre (plain: none -- the
// product with the matrix itself) and its extent; the reduced-storage experiment's copies instead where they are on.
static StripArgs strip_args(const bioen_hip_ctx* c, int p, bool colsum, int K, bool plain) {
    StripArgs q{};
    q.Ys = colsum ? c->Ys1[p] : c->Ys[p];
    q.center = (plain ? c->zero_center : c->strip_center) + p * kPanelRows;
    q.mps = panel_mps(c, p);
    q.ilv = strip_ilv(c);
    if (c->storage) {               // centred copies in strip order, rows padded to whole slices
        q.Ys = static_cast<const double*>(colsum ? c->Yr1 : c->Yr);
        q.mps = reduced_rows(c);
        q.ilv = 1;
    }
    q.mp = panel_mp(c, p);
    q.nstrips = strip_count(c);
    q.n = c->n;
    q.K = K;
    return q;
}
static void use_sets(StripArgs& q, const StripSets& ss) {
    q.sps = ss.sps; q.gs = ss.gs; q.tc = ss.tc; q.nch = ss.nch; q.fold = ss.fold; q.slots = ss.slots;
}
static StripForm strip_form(const bioen_hip_ctx* c, int K) {
    StripForm f{};
    f.K = K;
    f.nt = c->nontemporal;
    f.store = c->storage;
    return f;
}

// partial[(row K + a) nblk + block] of Y' . v_a; the caller adds the centre back (k_rows_combine's `center`);
// plain = true: Y . v_a itself (no centring: bioen_hip_chi_squared takes any w, not only normalised ones)
void launch_fwd_strip(bioen_hip_ctx* c, int K, const Vec8& v, bool plain) {
    const StripSets ss = strip_sets(c);
    for (int p = 0; p < panel_count(c); ++p) {
        TimedLaunch tl(c, 0, K);
        StripArgs q = strip_args(c, p, false, K, plain);
        use_sets(q, ss);                                // the sets are those of the context's geometry in every panel
        q.nslots = ss.slots * c->vr;
        q.partial = c->fwd_partial + (size_t)p * kPanelRows * K;
        q.pstride = c->mp;
        q.spb = fa_spb(c);
        q.wps = std::min(fa_wps_rows(q.mps), 16 / q.spb);    // (the bound cannot bind: a shorter last panel needs fewer waves per slot)
        run_k_strip_fwd(c, q, v, dim3(64 * q.wps * q.spb), strip_form(c, K));
    }
}

// the forces kernels' arguments on row-sum order panel p: one block per group of `per_cu` x 256, running the context's
// local segments in turn
static StripArgs forces_args(const bioen_hip_ctx* c, int p, int K, bool plain, int gs, const double* u_c) {
    StripArgs q = strip_args(c, p, false, K, plain);
    q.sps = strip_sps(c);
    q.gs = gs;
    q.tc = (q.sps + q.gs - 1) / q.gs;
    q.nch = 1; q.fold = 0; q.slots = q.gs;
    q.nslots = q.nblk = q.gs;
    q.nlocal = c->vr;
    q.u_c = u_c;
    q.w0 = c->fixed;
    q.partial = c->fwd_partial;
    return q;
}

// out_a[j] = sum_i u_c[i K + a] (Y_ij - ybar_c[i K + a]) with the RAW ybar in ybar_c; needs S_B0 / S_UY of this
// round in the problems' scalars (k_rows_combine with the strip centre).  plain: out = Y^T u itself (forces method, M > 1024).
// A matrix taller than 1024 rows: panel by panel, continuing the column sums.  No sum over columns here: any assignment
// of strips to blocks gives the same bits.
void launch_adj_strip(bioen_hip_ctx* c, int K, const double* u_c, const MVec8& out, const MVec8& scal, bool plain) {
    StripForm f = strip_form(c, K);
    for (int p = 0; p < panel_count(c); ++p) {
        TimedLaunch tl(c, 1, K);
        const int accumulate = p > 0 ? 1 : (plain ? 2 : 0);
        const double* u_p = u_c + (size_t)p * kPanelRows * K;
        if (c->one_copy && !c->storage) {
            // ONE strip copy (r05): the product runs on the row-sum order copy through the forces kernels' LDS image
            // (k_strip / k_strip2 in their ADJ form)
            const int gs = std::max(1, std::min(strip_sps(c), 256 * one_copy_adj_per_cu(c)));
            StripArgs q = forces_args(c, p, K, plain, gs, u_p);
            q.accumulate = accumulate;
            ForcesRound fr{};
            fr.n = K;
            for (int a = 0; a < K; ++a) {
                fr.a[a] = out.p[a];
                fr.scal[a] = scal.p[a];
            }
            const ForcesBlock b = forces_block(q.mps, q.mp);
            f.adj = true;
            if (strip_tall(q.mp)) run_k_strip2(c, q, fr, dim3(b.threads), b.lds, f);
            else run_k_strip(c, q, fr, dim3(b.threads), b.lds, f);
            continue;
        }
        StripArgs q = strip_args(c, p, true, K, plain);          // the column-sum order copy and its own kernel
        q.nblk = std::min(256 * fa_spb(c), q.nstrips);
        q.u_c = u_p;
        q.accumulate = accumulate;
        q.wps = fa_wps_rows(q.mps);
        q.spb = fa_spb(c);
        // u table of one slot's rows | their centres | two parity buffers of partial sums
        const size_t lds = ((size_t)q.wps * kWaveRows * 9 + (size_t)2 * q.wps * q.spb * 128) * sizeof(double);
        run_k_strip_adj(c, q, out, scal, dim3(64 * q.wps * q.spb), lds, f);
    }
}

// A forces pass (M <= 1024).  Strips in flight per wave of k_strip: two register sets, except at K > 4, where the second
// one does not fit (pass 1: the compiler spilled): one set + the row-sum product deferred behind the next strip's barrier
// (DEPTH 3, r04).  BIOEN_HIP_STRIP_DEPTH5=2 / 1: the r03 forms (A/B; FP64 copies only; read at every launch).
// mode: SM_TANGENT / SM_PRODUCT, the forms of a Hessian-vector product (FP64 copy, the width's default depth), else 0
static void forces_pass(bioen_hip_ctx* c, const ForcesRound& fr, bool xy, const double* u_c, int mode = 0) {
    StripArgs q = forces_args(c, 0, fr.n, false, forces_sets(c).gs, u_c);
    q.stamps = reinterpret_cast<long long*>(c->strip_stamps);
    StripForm f = strip_form(c, fr.n);
    f.xy = xy;
    f.mode = mode;
    const int depth5 = (c->storage || mode) ? 3 : env_flag("BIOEN_HIP_STRIP_DEPTH5", 3);
    f.depth = fr.n <= 4 ? 2 : (depth5 == 1 || depth5 == 2) ? depth5 : 3;
    const bool tall = strip_tall(c->mp);
    const ForcesBlock b = forces_block(panel_mps(c, 0), c->mp, !tall && f.depth == 3);
    if (tall) run_k_strip2(c, q, fr, dim3(b.threads), b.lds, f);
    else run_k_strip(c, q, fr, dim3(b.threads), b.lds, f);
}

// pass 1: x' = Y'^T f, online softmax, raw ybar' per block; then the block merge and ybar' -> X_YBAR
void launch_forces_xy(bioen_hip_ctx* c, const ForcesRound& fr, int seg_sets) {
    {
        TimedLaunch tl(c, 1, fr.n);
        forces_pass(c, fr, true, c->um);
    }
    launch_forces_blockmerge(c, fr, seg_sets);
}

// pass 2: b' = Y'^T r, t, Y' . t
void launch_forces_bt(bioen_hip_ctx* c, const ForcesRound& fr) {
    TimedLaunch tl(c, 0, fr.n);
    forces_pass(c, fr, false, c->r_c);
}

// ---- Hessian-vector products of the forces objective at a kept point (M <= 1024) ---------------------------
// pass 1: dx = Y'^T (v o s) -> fr.w, w dx, Y' . (w dx); fr.a = the point's x, fr.scal = the directions' scalars
void launch_forces_hp_tangent(bioen_hip_ctx* c, const ForcesRound& fr) {
    TimedLaunch tl(c, 6, fr.n);
    forces_pass(c, fr, false, c->um, SM_TANGENT);
}

// pass 2: c = Y'^T (dy' o s o s), s_j, Y' . s; fr.t = the point's q - qbar
void launch_forces_hp_product(bioen_hip_ctx* c, const ForcesRound& fr) {
    TimedLaunch tl(c, 7, fr.n);
    forces_pass(c, fr, false, c->r_c, SM_PRODUCT);
}

// out_j = sum_i Y'_ij u_i on the forces passes' copy (one operand): the ADJ form of the forces kernels, from zero
void launch_forces_colsum(bioen_hip_ctx* c, const double* u_c, double* out) {
    TimedLaunch tl(c, 1, 1);
    const int gs = std::max(1, std::min(strip_sps(c), 256 * forces_per_cu(c)));
    StripArgs q = forces_args(c, 0, 1, false, gs, u_c);
    q.accumulate = 2;
    ForcesRound fr{};
    fr.n = 1;
    fr.a[0] = out;
    fr.scal[0] = c->scal;           // (not read: the sum starts at zero)
    StripForm f = strip_form(c, 1);
    f.adj = true;
    const ForcesBlock b = forces_block(q.mps, q.mp);
    if (strip_tall(q.mp)) run_k_strip2(c, q, fr, dim3(b.threads), b.lds, f);
    else run_k_strip(c, q, fr, dim3(b.threads), b.lds, f);
}

}  // namespace bioen
