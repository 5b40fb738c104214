// The host side's internal interface: what the translation units behind the C ABI (api.hip, comm.cpp) call across their
// boundary, and nothing more.  Everything here is hidden: none of it is a dynamic symbol of the library.  A part of api.hip's
// unit (an .inl file) becomes a translation unit of its own by including this header instead of api.hip's static helpers;
// what it needs beyond these names is declared here first.
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
