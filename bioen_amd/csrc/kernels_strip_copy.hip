// The strip-major copies of the matrix (layout: strip.hpp): the kernels that build, move and read them back, and their
// life cycle on a context -- one list of row panels per operand order (ctx.hpp: Ys, Ys1; M <= 1024 is the one-panel case).
#include "strip.hpp"

namespace bioen {

// ---- construction -------------------------------------------------------------------------------
// The copies hold the RAW matrix (r03; r02 stored Y - centre): the centring is applied to the operand registers
// inside the kernels -- the same subtraction, hence the same bits in every product -- so that the strip copies can
// REPLACE the row-major matrix instead of standing beside it: bioen_hip_ctx_read_ytilde gathers the caller's numbers
// back out of them bit for bit, and the row-major copy is freed once the row-sum copy exists (ctx.hpp: Y).
template <bool COLSUM>
__global__ __launch_bounds__(256) void k_build_strips(const double* __restrict__ Y, size_t ld, int mp, int mps, int n,
                                                      double* __restrict__ Ys, int nstrips,
                                                      const double* __restrict__ center_diag, int sps, int ilv) {
    for (int s = blockIdx.x; s < nstrips; s += gridDim.x) {
        double* dst = Ys + (size_t)strip_phys(s, sps, ilv) * mps * kStripCols;
        for (int p = threadIdx.x; p < mps * 8; p += 256) {
            const int row = p >> 3, part = p & 7;
            d2 v{0.0, 0.0};
            if (row < mp) {
                const size_t col = (size_t)s * kStripCols + part * 2;
                v = *reinterpret_cast<const d2*>(Y + (size_t)row * ld + col);
                v.x = col < (size_t)n ? v.x : 0.0;
                v.y = col + 1 < (size_t)n ? v.y : 0.0;
#if STRIP_PRECENTERED
                if (col < (size_t)n) v.x -= center_diag[row];
                if (col + 1 < (size_t)n) v.y -= center_diag[row];
#endif
            }
            dst[COLSUM ? strip_pos_colsum(row, part * 2) : strip_pos(row, part * 2)] = v.x;
            dst[COLSUM ? strip_pos_colsum(row, part * 2 + 1) : strip_pos(row, part * 2 + 1)] = v.y;
        }
    }
}

// row-sum order copy -> column-sum order copy (the log-weights adjoint's), strip by strip through LDS-free index maps
__global__ __launch_bounds__(256) void k_restripe(const double* __restrict__ Ys, int mps, double* __restrict__ Ys1,
                                                  int nstrips, int sps, int ilv) {
    for (int s = blockIdx.x; s < nstrips; s += gridDim.x) {
        const double* src = Ys + (size_t)strip_phys(s, sps, ilv) * mps * kStripCols;    // (the column-sum copy: strip order)
        double* dst = Ys1 + (size_t)s * mps * kStripCols;
        for (int p = threadIdx.x; p < mps * kStripCols; p += 256) {
            const int row = p >> 4, col = p & 15;
            dst[strip_pos_colsum(row, col)] = src[strip_pos(row, col)];
        }
    }
}

// row-sum order copy, segments interleaved by ilv_from -> the same strips interleaved by ilv_to (whole strips move)
__global__ __launch_bounds__(256) void k_relayout(const double* __restrict__ from, double* __restrict__ to, int mps, int nstrips,
                                                  int sps, int ilv_from, int ilv_to) {
    for (int s = blockIdx.x; s < nstrips; s += gridDim.x) {
        const d2* src = reinterpret_cast<const d2*>(from + (size_t)strip_phys(s, sps, ilv_from) * mps * kStripCols);
        d2* dst = reinterpret_cast<d2*>(to + (size_t)strip_phys(s, sps, ilv_to) * mps * kStripCols);
        for (int p = threadIdx.x; p < mps * (kStripCols / 2); p += 256) dst[p] = src[p];
    }
}

// row-sum order copy -> row-major block out[rows][cols] (device), rows [row0, row0 + rows), columns [col0, col0 + cols)
__global__ __launch_bounds__(256) void k_gather_strips(const double* __restrict__ Ys, int mps, int row0, int rows,
                                                       size_t col0, int cols, double* __restrict__ out, size_t ldo,
                                                       int sps, int ilv) {
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < (size_t)rows * cols; p += (size_t)gridDim.x * 256) {
        const int r = (int)(p / cols);
        const size_t cc = col0 + (p - (size_t)r * cols);
        out[(size_t)r * ldo + (p - (size_t)r * cols)] =
            Ys[(size_t)strip_phys((int)(cc / kStripCols), sps, ilv) * mps * kStripCols + strip_pos(row0 + r, (int)(cc % kStripCols))];
    }
}

// row-major matrix -> reduced strip copy (centred); COLSUM selects the operand order (strip_pos / strip_pos_colsum)
template <bool COLSUM, int STORE>
__global__ __launch_bounds__(256) void k_build_strips_reduced(const double* __restrict__ Y, size_t ld, int mp, int mps64, int n,
                                                              unsigned char* __restrict__ out, int nstrips,
                                                              const double* __restrict__ center) {
    constexpr int SB = reduced_slice_bytes<STORE>();
    const size_t strip_bytes = (size_t)(mps64 / kWaveRows) * SB;
    for (int s = blockIdx.x; s < nstrips; s += gridDim.x) {
        unsigned char* dst = out + (size_t)s * strip_bytes;
        for (int p = threadIdx.x; p < mps64 * kStripCols; p += 256) {
            const int row = p >> 4, cc = p & 15;
            const size_t col = (size_t)s * kStripCols + cc;
            double v = 0.0;
            if (row < mp && col < (size_t)n) v = Y[(size_t)row * ld + col] - center[row];
            const size_t pos = COLSUM ? strip_pos_colsum(row, cc) : strip_pos(row, cc);     // ((wave 8 + chunk) 64 + lane) 2 + xy
            const int xy = (int)(pos & 1), lane = (int)((pos >> 1) & 63), chunk = (int)((pos >> 7) & 7), w = (int)(pos >> 10);
            unsigned char* sl = dst + (size_t)w * SB;
            const float hi = (float)v;
            reinterpret_cast<float*>(sl)[((chunk >> 1) * 64 + lane) * 4 + (chunk & 1) * 2 + xy] = hi;
            if (STORE == 1) {
                const float r = (float)(v - (double)hi);
                unsigned b = __float_as_uint(r);
                b += 0x7fffu + ((b >> 16) & 1u);                        // bf16, round to nearest even
                reinterpret_cast<unsigned short*>(sl + 4096)[(((chunk >> 2) * 64 + lane) * 4 + (chunk & 3)) * 2 + xy] =
                    (unsigned short)(b >> 16);
            }
        }
    }
}

// ---- life cycle ----------------------------------------------------------------------------------
static size_t panel_bytes(const bioen_hip_ctx* c, int p) { return (size_t)strip_count(c) * panel_mps(c, p) * kStripCols * sizeof(double); }
static dim3 copy_grid(const bioen_hip_ctx* c) { return dim3(std::min(strip_count(c), 4096)); }
static void free_panels(double* const* made, int np) {
    for (int p = 0; p < np; ++p)
        if (made[p]) (void)hipFree(made[p]);
}

// the layout a method wants: the log-weights passes (k_strip_fwd's folded groups, one slot per (segment, group)) the
// interleaved one; the forces passes (a block runs its group through the segments one after the other: already one window)
// strip order -- interleaved they read every ilv-th strip of an ilv times wider window, 2-4 % slower at K >= 6.
// BIOEN_HIP_STRIP_INTERLEAVE=0: strip order as until r05 (A/B; read at the first copy and at every method change)
static int strip_ilv_wanted(const bioen_hip_ctx* c, bool forces) {
    if (forces) return 1;
    return env_flag("BIOEN_HIP_STRIP_INTERLEAVE", 1) != 0 ? std::max(1, c->vr) : 1;
}

// Every allocation of a strip copy goes through here.  Tests: BIOEN_HIP_TEST_FAIL_STRIP_ALLOC=k makes the k-th one of a
// context fail as an exhausted device would (the fallback to the streaming kernels is otherwise never exercised).
static hipError_t strip_malloc(bioen_hip_ctx* c, double** p, size_t bytes) {
    ++c->strip_allocs;
    if (env_flag("BIOEN_HIP_TEST_FAIL_STRIP_ALLOC", 0) == c->strip_allocs) return hipErrorOutOfMemory;
    return hipMalloc(reinterpret_cast<void**>(p), bytes);
}

// A failed allocation leaves the context WITHOUT strip copies (strips_unavailable): fwd_strip_blocks /
// forces_fused_blocks then answer 0 and every caller takes the streaming kernels on the row-major matrix, which
// need no extra memory.  The copy pointers are published only after the build kernels are enqueued.
static int strip_copy_failed(bioen_hip_ctx* c, hipError_t e, const char* what) {
    (void)hipGetLastError();                       // an out-of-memory error must not surface at the next launch check
    c->strips_unavailable = 1;
    return hip_fail(e, what, __FILE__, __LINE__);
}

// The row-major matrix is the form data ARRIVE in (upload, device-side assembly, generator) and the operand of the
// streaming kernels.  Once the row-sum order copy exists it is redundant for every other path -- the copy holds the same
// numbers -- and is freed (bioen_hip_ctx_read_ytilde, bioen_hip_chi_squared and the column-sum order copy are served by
// the strip copy); a later call that needs it gets it back from the strip copy (ensure_rowmajor) and then keeps it.
// Footprint of the matrix: log-weights 2 x (both strip copies; 1 x on one copy), forces method 1 x.
int ensure_rowmajor(bioen_hip_ctx* c) {
    if (c->Y) return 0;
    if (!c->Ys[0]) return BIOEN_HIP_ESTATE;
    int rc = 0;
    double* y = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&y), (size_t)c->mp * c->ld * sizeof(double));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        hip_fail(e, "hipMalloc (row-major matrix back from the strip copy)", __FILE__, __LINE__);
        return BIOEN_HIP_ENOMEM;
    }
    e = hipMemsetAsync(y, 0, (size_t)c->mp * c->ld * sizeof(double), c->stream);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemsetAsync", __FILE__, __LINE__);
    for (int p = 0; p < panel_count(c) && !rc; ++p) {
        const int mps = panel_mps(c, p);
        hipLaunchKernelGGL(k_gather_strips, dim3(4096), dim3(256), 0, c->stream, c->Ys[p], mps, 0, std::min(mps, panel_mp(c, p)),
                           (size_t)0, (int)c->ld, y + (size_t)p * kPanelRows * c->ld, c->ld, strip_sps(c), strip_ilv(c));
        e = hipGetLastError();
        if (e != hipSuccess) rc = hip_fail(e, "k_gather_strips", __FILE__, __LINE__);
    }
    if (rc) {
        (void)hipFree(y);
        return rc;
    }
    c->Y = y;
    c->rowmajor_rebuilt = 1;
    return 0;
}

// block of the matrix -> device buffer out[rows][cols], whichever form is resident
int gather_block(bioen_hip_ctx* c, int row0, int rows, size_t col0, int cols, double* out) {
    if (c->Y) {
        hipError_t e = hipMemcpy2DAsync(out, (size_t)cols * sizeof(double), c->Y + (size_t)row0 * c->ld + col0,
                                        c->ld * sizeof(double), (size_t)cols * sizeof(double), (size_t)rows,
                                        hipMemcpyDeviceToDevice, c->stream);
        return e == hipSuccess ? 0 : hip_fail(e, "hipMemcpy2DAsync", __FILE__, __LINE__);
    }
    if (!c->Ys[0]) return BIOEN_HIP_ESTATE;
    for (int p = row0 / kPanelRows; p < panel_count(c) && p * kPanelRows < row0 + rows; ++p) {     // panel by panel
        const int lo = std::max(row0, p * kPanelRows), hi = std::min(row0 + rows, (p + 1) * kPanelRows);
        const size_t total = (size_t)(hi - lo) * cols;
        hipLaunchKernelGGL(k_gather_strips, dim3((unsigned)std::min<size_t>(4096, (total + 255) / 256)), dim3(256), 0,
                           c->stream, c->Ys[p], panel_mps(c, p), lo - p * kPanelRows, hi - lo, col0, cols,
                           out + (size_t)(lo - row0) * cols, (size_t)cols, strip_sps(c), strip_ilv(c));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "k_gather_strips", __FILE__, __LINE__);
    }
    return 0;
}

// the centres: mp zeros ("no centring": bioen_hip_chi_squared, the plain products) and YTilde at the time of the copy
static int ensure_zero_center(bioen_hip_ctx* c) {
    if (c->zero_center) return 0;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->zero_center), (size_t)c->mp * sizeof(double));
    if (e != hipSuccess) {
        c->zero_center = nullptr;
        return hip_fail(e, "hipMalloc", __FILE__, __LINE__);
    }
    e = hipMemsetAsync(c->zero_center, 0, (size_t)c->mp * sizeof(double), c->stream);
    return e == hipSuccess ? 0 : hip_fail(e, "hipMemsetAsync", __FILE__, __LINE__);
}

static int ensure_center(bioen_hip_ctx* c) {
    if (c->strip_center) return 0;
    double* cen = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&cen), (size_t)c->mp * sizeof(double));
    if (e != hipSuccess) return strip_copy_failed(c, e, "hipMalloc (strip centre)");
    e = hipMemcpyAsync(cen, c->YT, (size_t)c->mp * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
    if (e != hipSuccess) {
        (void)hipFree(cen);
        return strip_copy_failed(c, e, "hipMemcpyAsync (strip centre)");
    }
    c->strip_center = cen;
    return 0;
}

// reduced-byte storage experiment: the centred copies of c->storage's format, both operand orders, from the row-major
// FP64 matrix (which stays resident: read-back, chi_squared and the forces method keep using it)
static size_t reduced_copy_bytes(const bioen_hip_ctx* c) {
    const size_t slices = (size_t)strip_count(c) * (reduced_rows(c) / kWaveRows);
    return slices * (c->storage == 1 ? reduced_slice_bytes<1>() : reduced_slice_bytes<2>());
}
static int ensure_reduced_copy(bioen_hip_ctx* c, bool colsum) {
    void*& slot = colsum ? c->Yr1 : c->Yr;
    if (slot) return 0;
    if (paneled(c)) return BIOEN_HIP_ESTATE;
    int rc = ensure_rowmajor(c);                        // (gathered back exactly if the FP64 strip copy had replaced it)
    if (rc) return rc;
    if ((rc = ensure_center(c))) return rc;
    if (ensure_zero_center(c)) return BIOEN_HIP_ENOMEM;
    void* buf = nullptr;
    hipError_t e = hipMalloc(&buf, reduced_copy_bytes(c));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        hip_fail(e, "hipMalloc (reduced-storage strip copy)", __FILE__, __LINE__);
        return BIOEN_HIP_ENOMEM;
    }
    const int nstrips = strip_count(c), mps64 = reduced_rows(c);
    unsigned char* out = static_cast<unsigned char*>(buf);
    for_value<1, 2>(c->storage, [&](auto st) {
        for_value<1, 0>(colsum, [&](auto cs) {
            hipLaunchKernelGGL((k_build_strips_reduced<(decltype(cs)::value != 0), decltype(st)::value>), copy_grid(c), dim3(256), 0,
                               c->stream, c->Y, c->ld, c->mp, mps64, c->n, out, nstrips, c->strip_center);
        });
    });
    e = hipGetLastError();
    if (e != hipSuccess) {
        (void)hipFree(buf);
        return hip_fail(e, "k_build_strips_reduced", __FILE__, __LINE__);
    }
    slot = buf;
    return 0;
}

// bioen_hip_ctx_set_storage: switch the format of the log-weights passes' copies (0 = FP64).  Copies of another format
// are dropped; the row-major FP64 matrix is made resident again and kept from now on.
int set_storage_format(bioen_hip_ctx* c, int fmt) {
    if (fmt == c->storage) return 0;
    if (fmt != 0 && paneled(c)) return BIOEN_HIP_ESTATE;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
    if (fmt != 0) {
        const int rc = ensure_rowmajor(c);
        if (rc && !(rc == BIOEN_HIP_ESTATE && c->Y)) return rc;
        c->keep_rowmajor = 1;
    }
    if (c->Yr) (void)hipFree(c->Yr);
    if (c->Yr1) (void)hipFree(c->Yr1);
    c->Yr = c->Yr1 = nullptr;
    c->storage = fmt;
    return 0;
}

// The existing row-sum order copies into the layout `want` (strip_phys), best effort: new buffers, whole strips moved, the old
// ones freed -- 2 x the copy's bytes of traffic (3 ms at the headline) and, for the moment of the move, a second copy's
// memory; if that is not to be had the copies stay as they are (every kernel reads either layout).
static void relayout_strip_copies(bioen_hip_ctx* c, int want) {
    if (strip_ilv(c) == want) return;
    const int np = panel_count(c);
    double* made[bioen_hip_ctx::kMaxPanels] = {};
    hipError_t e = hipSuccess;
    for (int p = 0; p < np && e == hipSuccess; ++p) {
        e = strip_malloc(c, &made[p], panel_bytes(c, p));
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_relayout, copy_grid(c), dim3(256), 0, c->stream, c->Ys[p], made[p], panel_mps(c, p), strip_count(c),
                           strip_sps(c), strip_ilv(c), want);
        e = hipGetLastError();
    }
    if (e != hipSuccess) (void)hipGetLastError();
    if (hipStreamSynchronize(c->stream) != hipSuccess || e != hipSuccess) {       // (a failed move is reported by the next launch check)
        free_panels(made, np);
        return;
    }
    for (int p = 0; p < np; ++p) {
        (void)hipFree(c->Ys[p]);
        c->Ys[p] = made[p];
    }
    c->strip_ilv = want;
    ++c->strip_relayouts;
}

// The row-sum order copy, built on first use from the row-major matrix, which has then served: every path of the context
// that still wants it (forces_weights' streaming kernels, the r01 kernels of an A/B run) gets it back through
// ensure_rowmajor.  BIOEN_HIP_KEEP_ROWMAJOR=1 keeps it (A/B).
// method: 0 = the log-weights passes are about to run on the copy, 1 = the forces passes, -1 = any layout will do
int ensure_strip_copy(bioen_hip_ctx* c, int method) {
    if (c->storage) return ensure_reduced_copy(c, false);
    if (c->Ys[0]) {
        if (method >= 0) relayout_strip_copies(c, strip_ilv_wanted(c, method == 1));
        return 0;
    }
    c->strip_ilv = strip_ilv_wanted(c, method == 1);              // the layout they are built in
    if (c->strips_unavailable) return BIOEN_HIP_ENOMEM;
    if (!c->Y) return BIOEN_HIP_ESTATE;
    double* made[bioen_hip_ctx::kMaxPanels] = {};
    const int np = panel_count(c);
    hipError_t e = hipSuccess;
    for (int p = 0; p < np && e == hipSuccess; ++p) e = strip_malloc(c, &made[p], panel_bytes(c, p));
    if (e != hipSuccess) {
        free_panels(made, np);
        return strip_copy_failed(c, e, "hipMalloc (strip-major copy of yTilde)");
    }
    int rc = ensure_center(c);
    if (!rc && ensure_zero_center(c)) rc = strip_copy_failed(c, hipErrorOutOfMemory, "zero centre");
    if (rc) {
        free_panels(made, np);
        return rc;
    }
    for (int p = 0; p < np && e == hipSuccess; ++p) {
        hipLaunchKernelGGL(k_build_strips<false>, copy_grid(c), dim3(256), 0, c->stream, c->Y + (size_t)p * kPanelRows * c->ld, c->ld,
                           panel_mp(c, p), panel_mps(c, p), c->n, made[p], strip_count(c), c->strip_center + (size_t)p * kPanelRows,
                           strip_sps(c), strip_ilv(c));
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        free_panels(made, np);
        return strip_copy_failed(c, e, "k_build_strips");
    }
    std::copy(made, made + np, c->Ys);
    if (!c->keep_rowmajor) {
        e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipFree(c->Y);
        if (e != hipSuccess) return hip_fail(e, "release of the row-major matrix", __FILE__, __LINE__);
        c->Y = nullptr;
    }
    return 0;
}

// The column-sum order copy of the log-weights adjoint, cut from the row-sum order one on first use (the centre is shared)
// -- unless ONE strip copy serves (r05; ctx.hpp: one_copy): asked for (BIOEN_HIP_ONE_COPY=1), the default of a large
// matrix (r06: one_copy_by_default), or taken when the second copy does not fit.  The adjoint then runs on the row-sum
// order copy (launch_adj_strip) at the forces kernels' rate, instead of the whole context falling back to the streaming
// kernels on the row-major matrix.
int ensure_strip_copy_colsum(bioen_hip_ctx* c) {
    if (c->storage) {
        const int rc = ensure_reduced_copy(c, false);
        return rc ? rc : ensure_reduced_copy(c, true);
    }
    if (c->Ys1[0]) return 0;
    const int rc = ensure_strip_copy(c);
    if (rc) return rc;
    if (!c->one_copy && one_copy_by_default(c)) c->one_copy = 1;
    if (c->one_copy) return 0;
    double* made[bioen_hip_ctx::kMaxPanels] = {};
    const int np = panel_count(c);
    for (int p = 0; p < np; ++p) {
        hipError_t e = strip_malloc(c, &made[p], panel_bytes(c, p));
        if (e != hipSuccess) {                                   // no room for a second copy:
            (void)hipGetLastError();                             // (the error must not surface at the next launch check)
            free_panels(made, np);
            c->one_copy = 1;                                     // the row-sum order copy serves both products
            return 0;
        }
        hipLaunchKernelGGL(k_restripe, copy_grid(c), dim3(256), 0, c->stream, c->Ys[p], panel_mps(c, p), made[p], strip_count(c),
                           strip_sps(c), strip_ilv(c));
        e = hipGetLastError();
        if (e != hipSuccess) {                                   // a launch that fails is no memory shortage: reported
            free_panels(made, np);
            return strip_copy_failed(c, e, "k_restripe");
        }
    }
    std::copy(made, made + np, c->Ys1);
    return 0;
}

}  // namespace bioen
