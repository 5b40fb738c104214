// The communication layer: the stage exchange of sharded contexts over its three transports (the peer-to-peer mailboxes
// of kernels_p2p.hip, RCCL, the host callback), what watches them for failures, and the extern "C" entries that set them
// up, drive them and take them down.  No kernels here; the interface towards the rest of the host side is host.hpp.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "host.hpp"
#include "kernels.hpp"

namespace bioen {

// ---- RCCL (resolved lazily so single-GPU use never needs librccl) ---------------------------
namespace {
struct Rccl {
    void* h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;                         // optional
    ncclResult_t (*CommGetAsyncError)(ncclComm_t, ncclResult_t*) = nullptr;  // optional
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;

int load_rccl() {
    if (g_rccl.h) return 0;
    const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void* h = nullptr;
    for (const char* nm : names) {
        h = dlopen(nm, RTLD_NOW | RTLD_NOLOAD);
        if (h) break;
    }
    for (const char* nm : names) {
        if (h) break;
        h = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
    }
    if (!h) return fail(BIOEN_HIP_ERCCL, "librccl.so not found");
    g_rccl.GetUniqueId = reinterpret_cast<decltype(g_rccl.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    g_rccl.CommInitRank = reinterpret_cast<decltype(g_rccl.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
    g_rccl.AllGather = reinterpret_cast<decltype(g_rccl.AllGather)>(dlsym(h, "ncclAllGather"));
    g_rccl.CommDestroy = reinterpret_cast<decltype(g_rccl.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    g_rccl.GetErrorString = reinterpret_cast<decltype(g_rccl.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
    g_rccl.CommAbort = reinterpret_cast<decltype(g_rccl.CommAbort)>(dlsym(h, "ncclCommAbort"));
    g_rccl.CommGetAsyncError = reinterpret_cast<decltype(g_rccl.CommGetAsyncError)>(dlsym(h, "ncclCommGetAsyncError"));
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy)
        return fail(BIOEN_HIP_ERCCL, "librccl.so lacks a required symbol");
    g_rccl.h = h;
    return 0;
}

int rccl_fail(ncclResult_t r, const char* what) {
    std::string s = std::string(what) + " failed: " +
                    (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "(no error string)");
    set_last_error(s);
    return BIOEN_HIP_ERCCL;
}
}  // namespace

static int rccl_allgather_inplace(bioen_hip_ctx* c, double* base, size_t count) {
    ncclResult_t r = g_rccl.AllGather(base + (size_t)c->rank * count, base, count, ncclDouble,
                                      static_cast<ncclComm_t>(c->comm), c->stream);
    if (r != ncclSuccess) return rccl_fail(r, "ncclAllGather");
    return 0;
}

// the communicator's asynchronous state (a peer that died, a transport error): polled from the bounded waits
// (!= 0: the communicator reports a failure, last_error set)
static int rccl_async_error(bioen_hip_ctx* c) {
    if (!c->comm || !g_rccl.CommGetAsyncError) return 0;
    ncclResult_t st = ncclSuccess;
    const ncclResult_t r = g_rccl.CommGetAsyncError(static_cast<ncclComm_t>(c->comm), &st);
    if (r != ncclSuccess) return rccl_fail(r, "ncclCommGetAsyncError");
    if (st != ncclSuccess && st != ncclInProgress) {
        const int rc = rccl_fail(st, "RCCL communicator (asynchronous error)");
        rccl_abort(c);
        return rc;
    }
    return 0;
}

static std::atomic<int> g_comm_init_abandoned{0};      // helper threads of given-up (bounded) ncclCommInitRank calls that are still inside RCCL

void rccl_abort(bioen_hip_ctx* c) {
    if (!c->comm) return;
    if (g_rccl.CommAbort) g_rccl.CommAbort(static_cast<ncclComm_t>(c->comm));    // frees the communicator as well
    else if (g_rccl.CommDestroy) g_rccl.CommDestroy(static_cast<ncclComm_t>(c->comm));
    c->comm = nullptr;
}

// ---- the stage exchange and its failures (host.hpp says what each of these is) ---------------
int transport_error(bioen_hip_ctx* c) {
    if (c->p2p_err) {
        const unsigned long long w = __atomic_load_n(c->p2p_err, __ATOMIC_ACQUIRE);
        if (w) {
            static const char* const why[] = {"?", "timed out waiting for", "received an ABORT flag from", "an earlier exchange failed; peer",
                                              "is OUT OF STEP (another stage or payload under this exchange number) with"};
            char buf[256];
            std::snprintf(buf, sizeof buf, "peer-to-peer exchange %llu (stage %d): %s rank %d (BIOEN_HIP_WAIT_TIMEOUT = %g s)",
                          w & 0xffffffffffull, (int)((w >> 52) & 0xff), why[std::min<unsigned long long>(4, w >> 60)],
                          (int)((w >> 40) & 0xfff), c->wait_timeout_s);
            if (!c->failed) c->failed_p2p = 1;
            c->failed = 1;
            if (c->fail_msg.empty()) c->fail_msg = buf;
            return fail(BIOEN_HIP_ERCCL, c->fail_msg.c_str());
        }
    }
    if (c->comm) {
        const int rc = rccl_async_error(c);
        if (rc) {
            c->failed = 1;
            if (c->fail_msg.empty()) c->fail_msg = last_error();
            return rc;
        }
    }
    return 0;
}

bool exchanges_forced(const bioen_hip_ctx* c) {
    return c->world == 1 && c->force_exchange && (c->comm || c->exchange_cb || c->p2p_on);
}

int exchange(bioen_hip_ctx* c, int stage, size_t seg_payload) {
    return exchange_raw(c, stage, seg_payload * (size_t)c->vr);
}
int exchange_raw(bioen_hip_ctx* c, int stage, size_t payload) {      // payload = doubles per RANK
    if (c->world == 1 && !exchanges_forced(c)) return 0;
    if (c->failed) {
        const std::string m = "this context failed earlier and must be destroyed: " + c->fail_msg;
        return fail(BIOEN_HIP_ESTATE, m.c_str());
    }
    double* base = c->xbuf[stage];
    if (c->mirror_exchange) {      // measurement aid: this rank's part over every other rank's (one kernel)
        launch_xch_mirror(c, stage, payload);
        return 0;
    }
    if (c->p2p_on) {          // stores into the peers' mailboxes + flags, one kernel (kernels_p2p.hip)
        if (payload > c->p2p_cap) return fail(BIOEN_HIP_EINVAL, "exchange payload exceeds the mailbox slot");
        ++c->n_p2p_exchanges;
        launch_p2p_exchange(c, stage, payload);
        return 0;
    }
    if (c->comm) {
        ++c->n_rccl_exchanges;
        return rccl_allgather_inplace(c, base, payload);
    }
    if (!c->exchange_cb) return fail(BIOEN_HIP_ESTATE, "sharded context without a communicator");
    ++c->n_host_exchanges;
    // host-staged path (processes that cannot share an RCCL communicator, e.g. tests on one GPU)
    const size_t total = payload * c->world;
    if (c->exchange_host_count < total) {
        if (c->exchange_host) hipHostFree(c->exchange_host);
        c->exchange_host = nullptr;
        BIOEN_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&c->exchange_host), total * sizeof(double),
                                      hipHostMallocDefault));
        c->exchange_host_count = total;
    }
    BIOEN_HIP_CHECK(hipMemcpyAsync(c->exchange_host + (size_t)c->rank * payload, base + (size_t)c->rank * payload,
                                   payload * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (c->exchange_cb(c->exchange_user, c->exchange_host, payload) != 0) {
        c->exchange_error = 1;
        c->failed = 1;
        if (c->fail_msg.empty()) c->fail_msg = "the host-staged exchange callback failed (a peer gone, or its transport timed out)";
        return fail(BIOEN_HIP_ERCCL, c->fail_msg.c_str());
    }
    BIOEN_HIP_CHECK(hipMemcpyAsync(base, c->exchange_host, total * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return 0;
}

void p2p_release(bioen_hip_ctx* c) {      // (the context's device is the current one)
    if (c->stream) hipStreamSynchronize(c->stream);
    c->p2p_on = 0;
    if (c->failed_p2p) {     // the failure was this transport's own; the stream has drained and the transport goes: the
        c->failed = 0;       // context (and an RCCL communicator it may hold) is usable again
        c->failed_p2p = 0;
        c->fail_msg.clear();
    }
    for (int r = 0; r < 128; ++r)
        if (c->p2p_mapped[r]) {
            hipIpcCloseMemHandle(c->p2p_mapped[r]);
            c->p2p_mapped[r] = nullptr;
        }
    if (c->p2p_peers) hipFree(c->p2p_peers);
    c->p2p_peers = nullptr;
    if (c->p2p_box) hipFree(c->p2p_box);
    c->p2p_box = nullptr;
    if (c->p2p_err) hipHostFree(c->p2p_err);
    c->p2p_err = nullptr;
    if (c->p2p_dev_err) hipFree(c->p2p_dev_err);
    c->p2p_dev_err = nullptr;
    if (c->p2p_cnt) hipFree(c->p2p_cnt);
    c->p2p_cnt = nullptr;
    c->p2p_seq = 0;
    (void)hipGetLastError();
}

void comm_release(bioen_hip_ctx* c) {
    if (c->comm && c->failed) rccl_abort(c);      // a destroy would wait for peers that may be gone
    if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(static_cast<ncclComm_t>(c->comm));
    c->comm = nullptr;
    if (c->comm_buf) hipFree(c->comm_buf);
    c->comm_buf = nullptr;
    c->comm_buf_count = 0;
}

}  // namespace bioen

using namespace bioen;

// =====================================================================================
// C ABI
// =====================================================================================
extern "C" {

int bioen_hip_ctx_set_exchange_callback(bioen_hip_ctx* c, bioen_hip_exchange_fn fn, void* user) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;
    c->exchange_cb = fn;
    c->exchange_user = user;
    return 0;
}

int bioen_hip_ctx_set_force_exchange(bioen_hip_ctx* c, int on) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;
    c->force_exchange = on ? 1 : 0;
    return 0;
}

int bioen_hip_ctx_set_mirror_exchange(bioen_hip_ctx* c, int on) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;
    c->mirror_exchange = on ? 1 : 0;
    return 0;
}

int bioen_hip_exchange_counts(const bioen_hip_ctx* c, long long* rccl, long long* host_staged) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;
    if (rccl) *rccl = c->n_rccl_exchanges;
    if (host_staged) *host_staged = c->n_host_exchanges;
    return 0;
}

int bioen_hip_comm_unique_id(unsigned char id[128]) {
    if (!id) return fail(BIOEN_HIP_EINVAL, "id is NULL");
    int rc = load_rccl();
    if (rc) return rc;
    ncclUniqueId u;
    ncclResult_t r = g_rccl.GetUniqueId(&u);
    if (r != ncclSuccess) return rccl_fail(r, "ncclGetUniqueId");
    std::memcpy(id, u.internal, 128);
    return 0;
}

int bioen_hip_comm_init(bioen_hip_ctx* c, const unsigned char id[128], int rank, int nranks) {
    if (int rc = enter(c, FX_DEVICE, __func__)) return rc;
    if (!id || nranks <= 0 || rank < 0 || rank >= nranks) return fail(BIOEN_HIP_EINVAL, "bad argument");
    if (c->comm) return fail(BIOEN_HIP_ESTATE, "communicator already initialised");
    if (c->world > 1 && (rank != c->rank || nranks != c->world))
        return fail(BIOEN_HIP_EINVAL, "communicator rank/size must match the context's shard");
    int rc = load_rccl();
    if (rc) return rc;
    ncclUniqueId u;
    std::memcpy(u.internal, id, 128);
    // ncclCommInitRank is a collective of all ranks and has no time limit of its own: a rank that never calls it (it failed
    // before, or died) would keep the others here for good.  It runs on a helper thread; this thread waits for it for three
    // times the context's wait bound (topology detection on a full node takes seconds) and then gives the transport up --
    // the helper stays behind, blocked, in a process that goes on without RCCL (the callers fall back).
    // One state word per job decides who owns the outcome (two release / acquire flags read crosswise are a
    // Dekker pattern -- both sides could miss each other, and a late-successful communicator was then neither adopted nor
    // aborted): RUNNING -> DONE by the helper, RUNNING -> ABANDONED by the caller, one sequentially consistent
    // compare-exchange each -- whoever LOSES the exchange knows the other side's move and acts on it.  The process-wide
    // count of helpers still blocked inside RCCL goes up when a job is abandoned and down whenever such a helper returns,
    // successful or not.
    struct InitJob {
        enum { RUNNING = 0, DONE = 1, ABANDONED = 2 };
        ncclComm_t comm = nullptr;
        ncclResult_t r = ncclSuccess;
        std::atomic<int> state{RUNNING};
    };
    auto job = std::make_shared<InitJob>();
    const int dev = c->device;
    try {
        std::thread([job, nranks, u, rank, dev]() {
            if (hipSetDevice(dev) != hipSuccess) (void)hipGetLastError();
            job->r = g_rccl.CommInitRank(&job->comm, nranks, u, rank);
            int expected = InitJob::RUNNING;
            if (job->state.compare_exchange_strong(expected, InitJob::DONE)) return;      // the caller is still waiting: it adopts the result
            // ABANDONED: the caller walked away (and counted this helper as blocked).  A peer that arrived late completes
            // the init now: the orphan is aborted here, so that the peers' collectives on it fail fast instead of waiting
            // for a rank that will never join them; then this helper is no longer inside RCCL, whatever the init returned
            if (job->r == ncclSuccess && job->comm) {
                if (g_rccl.CommAbort) g_rccl.CommAbort(job->comm);
                else if (g_rccl.CommDestroy) g_rccl.CommDestroy(job->comm);
            }
            g_comm_init_abandoned.fetch_sub(1);
        }).detach();
    } catch (...) {
        return fail(BIOEN_HIP_ERCCL, "could not start the thread that initialises the RCCL communicator");
    }
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration<double>(3.0 * std::max(c->wait_timeout_s, 1.0));
    while (job->state.load() == InitJob::RUNNING) {
        if (std::chrono::steady_clock::now() > deadline) {
            // A helper thread stays behind, blocked inside RCCL: static destructors of librccl / HIP running under it at
            // interpreter teardown can hang or crash.  The process-wide count (bioen_hip_comm_init_abandoned) tells the
            // host layer to leave through os._exit after flushing its output (bioen_amd/_lib.py: leave_process).
            g_comm_init_abandoned.fetch_add(1);                      // before the exchange: the helper's decrement comes after it
            int expected = InitJob::RUNNING;
            if (job->state.compare_exchange_strong(expected, InitJob::ABANDONED)) {
                char buf[200];
                std::snprintf(buf, sizeof buf, "ncclCommInitRank (rank %d of %d) did not return within %g s: a rank is missing "
                              "(3 x BIOEN_HIP_WAIT_TIMEOUT)", rank, nranks, 3.0 * std::max(c->wait_timeout_s, 1.0));
                return fail(BIOEN_HIP_ERCCL, buf);
            }
            g_comm_init_abandoned.fetch_sub(1);                      // the helper finished in that very moment: its result is ours
            break;
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    ncclComm_t comm = job->comm;
    const ncclResult_t r = job->r;
    if (r != ncclSuccess) return rccl_fail(r, "ncclCommInitRank");
    c->comm = comm;
    c->comm_rank = rank;
    c->comm_nranks = nranks;
    return 0;
}

int bioen_hip_comm_init_abandoned(void) { return g_comm_init_abandoned.load() > 0 ? 1 : 0; }

int bioen_hip_comm_allgather(bioen_hip_ctx* c, const double* send, size_t count, double* recv) {
    if (int rc = enter(c, FX_DEVICE, __func__)) return rc;
    if (!send || !recv || count == 0) return fail(BIOEN_HIP_EINVAL, "bad argument");
    if (!c->comm) return fail(BIOEN_HIP_ESTATE, "communicator not initialised");
    const size_t need = count * (size_t)(c->comm_nranks + 1);
    if (c->comm_buf_count < need) {
        if (c->comm_buf) hipFree(c->comm_buf);
        c->comm_buf = nullptr;
        c->comm_buf_count = 0;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->comm_buf), need * sizeof(double));
        if (e != hipSuccess) {
            hip_fail(e, "hipMalloc", __FILE__, __LINE__);
            return BIOEN_HIP_ENOMEM;
        }
        c->comm_buf_count = need;
    }
    double* dsend = c->comm_buf;
    double* drecv = c->comm_buf + count;
    BIOEN_HIP_CHECK(hipMemcpyAsync(dsend, send, count * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ncclResult_t r = g_rccl.AllGather(dsend, drecv, count, ncclDouble, static_cast<ncclComm_t>(c->comm), c->stream);
    if (r != ncclSuccess) return rccl_fail(r, "ncclAllGather");
    BIOEN_HIP_CHECK(hipMemcpyAsync(recv, drecv, count * c->comm_nranks * sizeof(double), hipMemcpyDeviceToHost,
                                   c->stream));
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int bioen_hip_exchange_probe(bioen_hip_ctx* c, size_t count, int reps, double* usec_per_exchange) {
    if (int rc = enter(c, FX_DEVICE, __func__)) return rc;
    if (!usec_per_exchange || reps <= 0 || count == 0) return fail(BIOEN_HIP_EINVAL, "bad argument");
    if (count > c->xcap[X_YBAR]) count = c->xcap[X_YBAR];
    int rc = 0;
    for (int i = 0; i < 5 && !rc; ++i) rc = exchange_raw(c, X_YBAR, count);   // warm-up (connection set-up)
    if (rc) return rc;
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < reps && !rc; ++i) rc = exchange_raw(c, X_YBAR, count);
    if (rc) return rc;
    BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    if ((rc = transport_error(c))) return rc;
    *usec_per_exchange = 1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / reps;
    return 0;
}

int bioen_hip_exchange_selftest(bioen_hip_ctx* c, int reps, long long* mismatches) {
    if (int rc = enter(c, FX_DEVICE, __func__)) return rc;
    if (!mismatches || reps <= 0) return fail(BIOEN_HIP_EINVAL, "bad argument");
    unsigned long long* bad = nullptr;
    BIOEN_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&bad), sizeof *bad));
    hipError_t e = hipMemsetAsync(bad, 0, sizeof *bad, c->stream);
    int rc = e == hipSuccess ? 0 : hip_fail(e, "memset", __FILE__, __LINE__);
    // payloads of every shape the stages use: odd and even counts, a few doubles to the whole slot, back to back
    const size_t cap = c->xcap[X_YBAR];
    const size_t sizes[] = {1, 2, 3, 42, 169, 336, 1027, cap / 2, cap > 1 ? cap - 1 : 1, cap};
    for (int rep = 0; rep < reps && !rc; ++rep) {
        const size_t payload = std::max<size_t>(1, std::min(cap, sizes[rep % (sizeof sizes / sizeof *sizes)]));
        launch_xch_fill(c, X_YBAR, (int)payload, rep);
        rc = exchange_raw(c, X_YBAR, payload);
        if (!rc) launch_xch_check(c, X_YBAR, (int)payload, rep, bad);
        if (!rc && c->xcap[X_VEC] && rep % 8 == 7) {       // the result gathers' shape: a whole N-vector share per rank
            const size_t pv = rep % 16 == 7 ? c->xcap[X_VEC] : std::max<size_t>(1, c->xcap[X_VEC] - 1);
            launch_xch_fill(c, X_VEC, (int)pv, rep);
            rc = exchange_raw(c, X_VEC, pv);
            if (!rc) launch_xch_check(c, X_VEC, (int)pv, rep, bad);
        }
    }
    unsigned long long h = 0;
    if (!rc) {
        e = hipMemcpyAsync(&h, bad, sizeof h, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = hip_fail(e, "exchange self-test", __FILE__, __LINE__);
    }
    if (!rc) rc = transport_error(c);
    (void)hipFree(bad);
    *mismatches = (long long)h;
    return rc;
}

// ---- peer-to-peer stage exchange (kernels_p2p.hip) ------------------------------------------------------------
int bioen_hip_p2p_export(bioen_hip_ctx* c, unsigned char handle[64]) {
    if (int rc = enter(c, FX_DEVICE, __func__)) return rc;
    if (!handle) return fail(BIOEN_HIP_EINVAL, "NULL argument");
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t");
    if (c->p2p_on) return fail(BIOEN_HIP_ESTATE, "peer-to-peer exchange already attached");
    if (!c->p2p_box) {
        size_t cap = 0;
        for (int st = 0; st < X_COUNT; ++st) cap = std::max(cap, c->xcap[st]);
        cap = round_up(cap, 2);
        const size_t doubles = p2p_mailbox_doubles(c->world, cap);
        void* p = nullptr;
        // uncached: a polling wave must see what a peer's store put into this GPU's memory, not a line its L2 kept
        hipError_t e = hipExtMallocWithFlags(&p, doubles * sizeof(double), hipDeviceMallocUncached);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            e = hipExtMallocWithFlags(&p, doubles * sizeof(double), hipDeviceMallocFinegrained);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            hip_fail(e, "hipExtMallocWithFlags (mailbox)", __FILE__, __LINE__);
            return BIOEN_HIP_ENOMEM;
        }
        c->p2p_box = static_cast<double*>(p);
        c->p2p_cap = cap;
        c->p2p_bytes = doubles * sizeof(double);
        BIOEN_HIP_CHECK(hipMemsetAsync(c->p2p_box, 0, c->p2p_bytes, c->stream));
        BIOEN_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    hipIpcMemHandle_t h;
    BIOEN_HIP_CHECK(hipIpcGetMemHandle(&h, c->p2p_box));
    std::memcpy(handle, &h, 64);
    return 0;
}

int bioen_hip_p2p_detach(bioen_hip_ctx* c) {
    if (int rc = enter(c, FX_DEVICE, __func__)) return c ? rc : 0;      // (NULL: nothing to detach)
    p2p_release(c);
    return 0;
}

int bioen_hip_p2p_attach(bioen_hip_ctx* c, const unsigned char* handles) {
    if (int rc = enter(c, FX_DEVICE, __func__)) return rc;
    if (!handles && c->world > 1) return fail(BIOEN_HIP_EINVAL, "NULL argument");
    if (c->p2p_on) return fail(BIOEN_HIP_ESTATE, "peer-to-peer exchange already attached");
    if (!c->p2p_box) return fail(BIOEN_HIP_ESTATE, "bioen_hip_p2p_export first");
    std::vector<double*> peers((size_t)c->world, nullptr);
    int rc = 0;
    for (int r = 0; r < c->world && !rc; ++r) {
        if (r == c->rank) {
            peers[r] = c->p2p_box;
            continue;
        }
        hipIpcMemHandle_t h;
        std::memcpy(&h, handles + (size_t)r * 64, 64);
        void* p = nullptr;
        const hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            char buf[160];
            std::snprintf(buf, sizeof buf, "hipIpcOpenMemHandle of rank %d's mailbox failed: %s", r, hipGetErrorString(e));
            rc = fail(BIOEN_HIP_ERCCL, buf);
            break;
        }
        c->p2p_mapped[r] = p;
        peers[r] = static_cast<double*>(p);
        // a mailbox on ANOTHER device is only usable where this device reaches that one's memory: ask before the first kernel
        // does (a store the fabric cannot route is a GPU fault, not an error code); where the runtime cannot tell, the
        // self-test decides
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, p) == hipSuccess && at.device != c->device) {
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, c->device, at.device) == hipSuccess && !can) {
                char buf[160];
                std::snprintf(buf, sizeof buf, "device %d has no peer access to device %d (rank %d's mailbox)", c->device, at.device, r);
                rc = fail(BIOEN_HIP_ERCCL, buf);
                break;
            }
        }
        (void)hipGetLastError();
    }
    if (!rc && !c->p2p_err) {
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&c->p2p_err), 64, hipHostMallocCoherent | hipHostMallocMapped);
        if (e == hipSuccess) {
            std::memset(c->p2p_err, 0, 64);
            e = hipMalloc(reinterpret_cast<void**>(&c->p2p_dev_err), 64);
        }
        if (e == hipSuccess) e = hipMemset(c->p2p_dev_err, 0, 64);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->p2p_cnt), 128 * sizeof(unsigned int));
        if (e == hipSuccess) e = hipMemset(c->p2p_cnt, 0, 128 * sizeof(unsigned int));
        if (e != hipSuccess) rc = hip_fail(e, "error words of the peer-to-peer exchange", __FILE__, __LINE__);
    }
    if (!rc) {
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->p2p_peers), (size_t)c->world * sizeof(double*));
        if (e == hipSuccess)
            e = hipMemcpy(c->p2p_peers, peers.data(), (size_t)c->world * sizeof(double*), hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = hip_fail(e, "peer table", __FILE__, __LINE__);
    }
    if (rc) {
        p2p_release(c);      // (reports nothing: the failure's message stays)
        return rc;
    }
    c->p2p_seq = 0;
    c->p2p_on = 1;
    return 0;
}

int bioen_hip_exchange_transport(const bioen_hip_ctx* c) {
    if (enter(c, FX_NONE, __func__)) return -1;
    if (c->p2p_on) return 3;
    if (c->comm) return 1;
    if (c->exchange_cb) return 2;
    return 0;
}

int bioen_hip_exchange_counts3(const bioen_hip_ctx* c, long long* rccl, long long* host_staged, long long* p2p) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;
    if (rccl) *rccl = c->n_rccl_exchanges;
    if (host_staged) *host_staged = c->n_host_exchanges;
    if (p2p) *p2p = c->n_p2p_exchanges;
    return 0;
}

int bioen_hip_ctx_set_wait_timeout(bioen_hip_ctx* c, double seconds) {
    if (int rc = enter(c, FX_NONE, __func__)) return rc;
    if (!(seconds > 0.0)) return fail(BIOEN_HIP_EINVAL, "bad argument");
    c->wait_timeout_s = seconds;
    return 0;
}

int bioen_hip_comm_destroy(bioen_hip_ctx* c) {
    if (enter(c, FX_NONE, __func__)) return 0;      // (NULL: nothing to destroy)
    comm_release(c);
    return 0;
}

}  // extern "C"
