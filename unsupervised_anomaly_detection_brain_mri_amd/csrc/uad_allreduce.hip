// Library-issued RCCL all-reduce, shared by the VAE-family handle (uad_model.hip: uad_allreduce_attach / uad_backward_allreduce) and the GAN handle
// (uad_gan.hip: uad_gan_allreduce_attach / uad_gan_phase): the run-time binding of librccl, the uad_rccl_* exports of include/uad_hip.h, and the lane
// (uad_allreduce.h) that owns a handle's collective stream, events and buckets.
#include <stdlib.h>
#include <string.h>

#include <dlfcn.h>
// RCCL: types only -- the library is bound at run time (rccl_api below), libuad_hip.so does not link it.  Without the development header (a single-GPU ROCm
// install) the few opaque types are declared here and the uad_rccl_* entry points still work whenever librccl.so.1 itself can be loaded.
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclChar = 0, ncclUint8 = 1, ncclInt32 = 2, ncclInt = 2, ncclUint32 = 3, ncclInt64 = 4, ncclUint64 = 5, ncclFloat16 = 6, ncclHalf = 6, ncclFloat32 = 7, ncclFloat = 7, ncclFloat64 = 8, ncclDouble = 8 } ncclDataType_t;
typedef enum { ncclSum = 0, ncclProd = 1, ncclMax = 2, ncclMin = 3, ncclAvg = 4 } ncclRedOp_t;
#endif
#include "../../include/uad_hip.h"
#include "uad_allreduce.h"
#include "uad_kernels.h"      // uad_fail, HIP_TRY

#define fail uad_fail

// RCCL is bound at run time: librccl.so.1 as the process already has it (the copy PyTorch-ROCm loads), else from the loader path.  libuad_hip.so
// itself has no link-time dependency on it -- single-GPU users and the CPU-side symbol tests never touch it.
namespace {
struct RcclApi {
    void* h = nullptr;
    decltype(&ncclGetUniqueId) getUniqueId = nullptr;
    decltype(&ncclCommInitRank) commInitRank = nullptr;
    decltype(&ncclCommDestroy) commDestroy = nullptr;
    decltype(&ncclAllReduce) allReduce = nullptr;
    decltype(&ncclGetErrorString) errString = nullptr;
    bool ok = false;
};
RcclApi* rccl_api() {
    static RcclApi api;
    static bool tried = false;
    if (tried) return api.ok ? &api : nullptr;
    tried = true;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    if (const char* over = getenv("UAD_RCCL_LIB")) api.h = dlopen(over, RTLD_NOW | RTLD_LOCAL);      // explicit override wins (tests: a stub whose "all-reduce" doubles)
    for (const char* nm : names) {
        if (api.h) break;
        api.h = dlopen(nm, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);       // the copy the process already uses (torch's), if any
    }
    for (const char* nm : names) {
        if (api.h) break;
        api.h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
    }
    if (!api.h) return nullptr;
    api.getUniqueId = reinterpret_cast<decltype(api.getUniqueId)>(dlsym(api.h, "ncclGetUniqueId"));
    api.commInitRank = reinterpret_cast<decltype(api.commInitRank)>(dlsym(api.h, "ncclCommInitRank"));
    api.commDestroy = reinterpret_cast<decltype(api.commDestroy)>(dlsym(api.h, "ncclCommDestroy"));
    api.allReduce = reinterpret_cast<decltype(api.allReduce)>(dlsym(api.h, "ncclAllReduce"));
    api.errString = reinterpret_cast<decltype(api.errString)>(dlsym(api.h, "ncclGetErrorString"));
    api.ok = api.getUniqueId && api.commInitRank && api.commDestroy && api.allReduce && api.errString;
    return api.ok ? &api : nullptr;
}
int rccl_missing() { return fail(UAD_ERR_UNSUPPORTED, "librccl.so.1 could not be loaded or lacks the nccl* entry points (set UAD_RCCL_LIB to its path)"); }
#define RCCL_API(A)          \
    RcclApi* A = rccl_api(); \
    if (!A) return rccl_missing()
#define RCCL_TRY(A, expr)                                                                              \
    do {                                                                                               \
        ncclResult_t r_ = (expr);                                                                      \
        if (r_ != ncclSuccess) return fail(UAD_ERR_HIP, "%s failed: %s", #expr, (A)->errString(r_));   \
    } while (0)

int make_event(hipEvent_t* e) {
    if (*e || hipEventCreateWithFlags(e, hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess) return UAD_OK;
    HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return UAD_OK;
}
}  // namespace

// ------------------------------------------------------------------------------------------------ lane
int uad_ar_open(UadArLane* l, void* comm, int world, float* grads, UadArPlacement where, hipStream_t borrow) {
    if (!rccl_api()) return rccl_missing();
    if (where == UAD_AR_BORROW) {
        if (l->owned) return fail(UAD_ERR_INVALID, "all-reduce lane: already runs on a stream of its own");
        l->stream = borrow;
    } else if (!l->owned) {
        if (where == UAD_AR_OWN_HIGH) {
            int lo = 0, hi = 0;
            HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
            HIP_TRY(hipStreamCreateWithPriority(&l->stream, hipStreamNonBlocking, hi));
        } else {
            HIP_TRY(hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking));
        }
        l->owned = true;
    }
    for (hipEvent_t& e : l->ev_in)
        if (const int rc = make_event(&e)) return rc;
    if (const int rc = make_event(&l->ev_out)) return rc;
    l->comm = comm; l->world = world; l->grads = grads;
    return UAD_OK;
}

int uad_ar_reduce(UadArLane* l, int b, hipStream_t st) {
    static const bool skip = getenv("UAD_AR_SKIP") != nullptr;       // measurement: everything but the ncclAllReduce call itself
    if (skip) return UAD_OK;
    RCCL_API(api);
    float* g = l->grads + l->off[b];
    RCCL_TRY(api, api->allReduce(g, g, (size_t)l->cnt[b], ncclFloat, ncclSum, (ncclComm_t)l->comm, st));
    return UAD_OK;
}

int uad_ar_issue(UadArLane* l, int b, hipStream_t producer) {
    if (producer != l->stream) {
        HIP_TRY(hipEventRecord(l->ev_in[b], producer));
        HIP_TRY(hipStreamWaitEvent(l->stream, l->ev_in[b], 0));
    }
    l->pending = true;
    return uad_ar_reduce(l, b, l->stream);
}

int uad_ar_join(UadArLane* l, hipStream_t consumer) {
    if (l->pending && consumer != l->stream) {
        HIP_TRY(hipEventRecord(l->ev_out, l->stream));
        HIP_TRY(hipStreamWaitEvent(consumer, l->ev_out, 0));
    }
    l->pending = false;
    return UAD_OK;
}

int uad_ar_close(UadArLane* l) {
    int rc = UAD_OK;
    auto note = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == UAD_OK) rc = fail(UAD_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    };
    if (l->owned) {
        note(hipStreamSynchronize(l->stream), "hipStreamSynchronize(all-reduce stream)");      // a queued collective still reads the gradients
        note(hipStreamDestroy(l->stream), "hipStreamDestroy(all-reduce stream)");
    }
    for (hipEvent_t e : l->ev_in) if (e) note(hipEventDestroy(e), "hipEventDestroy");
    if (l->ev_out) note(hipEventDestroy(l->ev_out), "hipEventDestroy");
    *l = UadArLane();
    return rc;
}

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" {

int uad_rccl_unique_id(void* id_out, int cap) {
    if (!id_out || cap < (int)sizeof(ncclUniqueId)) return fail(UAD_ERR_INVALID, "uad_rccl_unique_id: need a buffer of %d bytes", (int)sizeof(ncclUniqueId));
    RCCL_API(api);
    ncclUniqueId id;
    RCCL_TRY(api, api->getUniqueId(&id));
    memcpy(id_out, &id, sizeof id);
    return UAD_OK;
}
int uad_rccl_comm_create(const void* id_bytes, int world, int rank, void** comm_out) {
    if (!id_bytes || !comm_out || world < 1 || rank < 0 || rank >= world) return fail(UAD_ERR_INVALID, "uad_rccl_comm_create: bad arguments");
    RCCL_API(api);
    ncclUniqueId id;
    memcpy(&id, id_bytes, sizeof id);
    ncclComm_t c = nullptr;
    // (RCCL prints a start-up banner -- version / host / library path -- to STDOUT from rank 0's first communicator.  A caller whose stdout is a protocol
    // points its file descriptor 1 elsewhere itself, as bench.py's claim_stdout() does: the library does not touch process-wide descriptors -- ADVICE r5.)
    const ncclResult_t r = api->commInitRank(&c, world, id, rank);        // collective over the ranks: every rank calls it with rank 0's id, on its own device
    if (r != ncclSuccess) return fail(UAD_ERR_HIP, "ncclCommInitRank failed: %s", api->errString(r));
    *comm_out = (void*)c;
    return UAD_OK;
}
int uad_rccl_comm_destroy(void* comm) {
    if (!comm) return UAD_OK;
    RCCL_API(api);
    RCCL_TRY(api, api->commDestroy((ncclComm_t)comm));
    return UAD_OK;
}
int uad_rccl_allreduce(void* comm, float* buf, long long count, void* stream) {
    if (!comm || !buf || count <= 0) return fail(UAD_ERR_INVALID, "uad_rccl_allreduce: bad arguments");
    RCCL_API(api);
    RCCL_TRY(api, api->allReduce(buf, buf, (size_t)count, ncclFloat, ncclSum, (ncclComm_t)comm, (hipStream_t)stream));
    return UAD_OK;
}

}  // extern "C"
