// The host side's internal interface: what the translation units behind the C ABI call across their boundaries, and nothing
// more -- api.hip (contexts, evaluations, the engines and the multimin drivers), comm.cpp (the exchange), and the
// second-order and session entries, one unit each: api_hessp.cpp, api_forces_*.cpp, api_logw_newton.cpp, api_bfgs.cpp (what
// those share among themselves is dense.hpp).  Everything here is hidden: none of it is a dynamic symbol of the library,
// and the link refuses a name declared here that no unit defines.  What is still part of api.hip's unit (the engine_*.inl
// files, api_multimin.inl) becomes a translation unit of its own by including this header instead of api.hip's static
// helpers; what it needs beyond these names is declared here first.
#pragma once

#include <chrono>
#include <cstdio>
#include <string>
#include <thread>

#include "ctx.hpp"

#pragma GCC visibility push(hidden)
namespace bioen {

// ---- error reporting (api.hip; set_last_error and hip_fail: ctx.hpp) ------------------------------------------------------
int fail(int code, const char* msg);      // the thread's last error <- msg; -> code
const std::string& last_error();          // the thread's last error (what bioen_hip_last_error hands out)

// ---- the entry guard (api.hip) --------------------------------------------------------------------------------------------
// The entry guard: the first statement of every extern "C" function that takes a context (bioen_hip_ctx_destroy, which
// accepts NULL, has none) says there what the call does to the state other calls rely on (DESIGN 6c has the table):
//   FX_DEVICE         it works on the device: the context's device becomes the thread's current one
//   FX_DROPS_POINT    it evaluates on the context or changes the matrix state: the products' point is gone
//   FX_ENDS_SESSION   it evaluates or optimises: a live BFGS session ends, and its next call returns BIOEN_HIP_ESTATE
//   FX_NEEDS_SESSION  it is a call of the BFGS session: BIOEN_HIP_ESTATE without one
// A NULL context is BIOEN_HIP_EINVAL.  The effects come before the entry looks at its other arguments: a call rejected
// for those has had them all the same.
enum : unsigned {
    FX_NONE = 0,             // queries and settings: host fields only (the entries that take a const context pass this)
    FX_DEVICE = 1,
    FX_DROPS_POINT = 2,
    FX_ENDS_SESSION = 4,
    FX_NEEDS_SESSION = 8,
    FX_CHANGES_MATRIX = FX_DEVICE | FX_DROPS_POINT,
    FX_EVALUATES = FX_DEVICE | FX_DROPS_POINT | FX_ENDS_SESSION,
    FX_SESSION_CALL = FX_DEVICE | FX_DROPS_POINT | FX_NEEDS_SESSION,
};

int enter(const bioen_hip_ctx* ctx, unsigned fx, const char* who);

// ---- point and session (point_drop: api.hip; hessp_free: api_hessp.cpp; bfgs_free: api_bfgs.cpp) ---------------------------
// The point a Hessian-vector product refers to is gone; `by`: an entry's name, or what failed
void point_drop(bioen_hip_ctx* c, const char* by);
void hessp_free(bioen_hip_ctx* c);        // the buffers of the kept point and of the products on it; the point with them
void bfgs_free(bioen_hip_ctx* c);         // the dense inverse-Hessian BFGS session, if one is live (BfgsSession: api_bfgs.cpp only)

// ---- allocation and transfers (api.hip) -------------------------------------------------------------------------------------
int dalloc_zero(double** p, size_t count, hipStream_t s);      // count doubles on the device, zeroed on s
// the pinned staging buffer of the forces method, c->host_m (2 x mp x kMaxBatch doubles: forces up | gradients down), on first need
int forces_staging(bioen_hip_ctx* c);
// Copies between the device and a CALLER's (pageable) buffer, on the context's stream: directly, or, where the runtime
// refuses to pin the buffer, through pinned staging buffers of the library's own (the device-to-host forms are synchronous then)
int h2d_user(bioen_hip_ctx* c, void* dst, const void* src, size_t bytes);
hipError_t d2h_user(hipStream_t stream, void* dst, const void* src, size_t bytes);
hipError_t d2h_user_2d(hipStream_t stream, char* dst, size_t dpitch, const char* src, size_t spitch, size_t width, size_t height);
// host N-vectors are always GLOBAL (n_global long); a sharded context takes its slice
int upload_n(bioen_hip_ctx* c, double* dst, const double* src);
// gather a sharded device N-vector into a GLOBAL host vector (world == 1: plain download)
int download_n(bioen_hip_ctx* c, double* dst_global, const double* src_local);
// the scalars of the first nslots slots -> c->host_scal, synchronised; scalars behind a failed exchange are not results
int read_scalars(bioen_hip_ctx* c, int nslots = 1);

// ---- launch check (api.hip) -------------------------------------------------------------------------------------------------
int check_launch();                       // hipGetLastError behind a run of kernel launches -> 0 | BIOEN_HIP_EHIP

// ---- log-weights evaluation (api.hip; all asynchronous on c->stream) --------------------------------------------------------
struct Round;                             // kernels.hpp
// the round of the k problems in `slots`: their vectors, scalars and partials, stp and theta (NULL: zeros)
Round make_round(bioen_hip_ctx* c, const int* slots, int k, const double* stp, const double* theta);
// The pass family of a product with the matrix on the log-weights side, decided and made ready: *nblk > 0, the strip kernels
// (with `colsum` the column-sum order copy too), or *nblk = 0, the streaming kernels on the row-major matrix.
// strips_ok = false: the caller has reasons of its own against the strips.
int choose_logw_passes(bioen_hip_ctx* c, bool strips_ok, int method, bool colsum, int* nblk);
// r.x must hold the points and P_MAX their block maxima (launch_trial does both)
int enqueue_logw_eval(bioen_hip_ctx* c, const Round& r, bool with_grad);
// second half of an evaluation; needs w, scal[S_P] and the compact ybar_c / r_c of the SAME round still in place
int enqueue_logw_adjoint(bioen_hip_ctx* c, const Round& r);
// One evaluation of the round's single point, start to finish; keep_point: and what the Hessian-vector products keep of it.
// -> *f; grad_out (a caller's global N-vector) if given; the round's scalars in host_scal
int eval_logw_point(bioen_hip_ctx* c, const Round& r, bool with_grad, bool keep_point, double* f, double* grad_out);

// ---- forces evaluation (api.hip) --------------------------------------------------------------------------------------------
// what the forces method refuses on this context: a sharded one without canonical segments (strip_path_ok = false: without
// exception), the affine model or anything but the strip passes on the reduced-storage experiment's copies
int forces_guard(const bioen_hip_ctx* c, bool strip_path_ok = true);
// k evaluations that share every matrix pass (slots 0 .. k-1); forces [k][m], grad [k][m]
int forces_eval(bioen_hip_ctx* c, int k, const double* forces, const double* w0, const double* thetas, double* f, double* grad);

// ---- the exchange interface (comm.cpp) ------------------------------------------------------------------------------------
// One in-place all-gather of an exchange stage ([world][payload] doubles).  world == 1: nothing.  Three transports, in
// this order of precedence: the peer-to-peer mailboxes (kernels_p2p.hip: one kernel, no collective launch, no host), RCCL
// (ncclAllGather on the context's stream), the host callback (D2H, the caller's all-gather, H2D: processes that share
// neither).  All three leave the same bytes in the stage buffer.
// world == 1 with force_exchange (bioen_hip_ctx_set_force_exchange / BIOEN_HIP_FORCE_EXCHANGE=1) and a communicator
// or callback in place: the one-rank all-gather is executed all the same -- a copy of the rank's segment onto
// itself, same bits -- so the stage path can run under test on a single GPU.
bool exchanges_forced(const bioen_hip_ctx* c);
// `seg_payload` = doubles per SEGMENT (what the kernels' stage views are built with); a rank ships its vr segments
int exchange(bioen_hip_ctx* c, int stage, size_t seg_payload);
int exchange_raw(bioen_hip_ctx* c, int stage, size_t payload);      // payload = doubles per RANK

// What went wrong asynchronously on this context's transports since the last look: the error word of the peer-to-peer
// exchange kernels (kernels_p2p.hip) and the RCCL communicator's own.  0 = nothing.
int transport_error(bioen_hip_ctx* c);

void rccl_abort(bioen_hip_ctx* c);        // ncclCommAbort: kernels of a collective a dead peer left hanging return
// what bioen_hip_p2p_detach and bioen_hip_comm_destroy do, for the callers inside the library
void p2p_release(bioen_hip_ctx* c);
void comm_release(bioen_hip_ctx* c);

// A bounded host wait on a word a kernel publishes (the live pages of the engines).  tick() is called once per look at
// the word: it spins politely (pause, later yield), and every 4096 looks asks the stream (a failed launch ends the wait
// with its error), the transports (above) and the clock: past c->wait_timeout_s the wait fails with BIOEN_HIP_ERCCL
// on a context that exchanges (a peer is gone: the communicator is aborted so that its kernel returns) and BIOEN_HIP_EHIP
// otherwise -- never a hang.
struct BoundedWait {
    bioen_hip_ctx* c;
    const char* what;
    unsigned spins = 0;
    bool armed = false;
    std::chrono::steady_clock::time_point deadline;
    BoundedWait(bioen_hip_ctx* ctx, const char* w) : c(ctx), what(w) {}
    // published(): re-reads the word; -> 0 keep waiting, 1 it is there, < 0 failure
    template <class Pred>
    int tick(Pred published) {
        ++spins;
        if ((spins & 0xfffu) == 0) {
            const hipError_t q = hipStreamQuery(c->stream);
            if (q == hipSuccess) {
                if (published()) return 1;
                const int te = transport_error(c);
                if (te) return te;
                return fail(BIOEN_HIP_ESTATE, "round finished without publishing its results");
            }
            if (q != hipErrorNotReady) return hip_fail(q, "hipStreamQuery", __FILE__, __LINE__);
            const int te = transport_error(c);
            if (te) return te;
            const auto now = std::chrono::steady_clock::now();
            if (!armed) {
                armed = true;
                deadline = now + std::chrono::duration_cast<std::chrono::steady_clock::duration>(
                                     std::chrono::duration<double>(c->wait_timeout_s + (c->p2p_on ? 2.0 : 0.0)));
            } else if (now > deadline) {
                char buf[200];
                std::snprintf(buf, sizeof buf, "timed out after %g s waiting for %s (BIOEN_HIP_WAIT_TIMEOUT)",
                              c->wait_timeout_s, what);
                c->failed = 1;
                if (c->fail_msg.empty()) c->fail_msg = buf;
                const bool exchanging = c->world > 1 || c->comm || c->exchange_cb || c->p2p_on;
                if (c->comm) rccl_abort(c);
                return fail(exchanging ? BIOEN_HIP_ERCCL : BIOEN_HIP_EHIP, buf);
            }
        }
        if (spins < 20000u) {
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#else
            std::this_thread::yield();
#endif
        } else {
            std::this_thread::yield();
        }
        return 0;
    }
};

}  // namespace bioen
#pragma GCC visibility pop
