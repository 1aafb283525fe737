// Internal interface of uad_allreduce.hip: the library-issued gradient all-reduce both handle types share (not the public C-ABI).
// A lane owns the collective side of one handle: the RCCL communicator it was attached to, the stream its collectives run on, the events that
// order that stream against the handle's own streams, and up to four buckets (contiguous slices of the handle's flat gradient buffer).
#pragma once
#include <hip/hip_runtime.h>

enum UadArPlacement {
    UAD_AR_BORROW,       // run on a stream the handle already has (the VAE handle's side stream)
    UAD_AR_OWN,          // a non-blocking stream of the lane's own (VAE handle, UAD_AR_STREAM=own)
    UAD_AR_OWN_HIGH,     // a non-blocking stream of the lane's own at the highest priority (GAN handle)
};

struct UadArLane {
    void* comm = nullptr;              // RCCL communicator (uad_rccl_comm_create); null: detached
    int world = 1;
    float* grads = nullptr;            // the handle's flat gradient buffer the buckets index
    hipStream_t stream = nullptr;      // where the collectives run
    bool owned = false;                // the lane created `stream` (and destroys it in uad_ar_close)
    bool pending = false;              // a collective was issued on `stream` that no consumer has joined yet
    hipEvent_t ev_in[4] = {}, ev_out = nullptr;
    int nb = 0;
    long long off[4] = {}, cnt[4] = {};
};

// Attaches `comm` and picks where the collectives run (`borrow` for UAD_AR_BORROW).  The stream and the events are created once per lane;
// the buckets are the caller's to fill in (nb, off, cnt).
int uad_ar_open(UadArLane* l, void* comm, int world, float* grads, UadArPlacement where, hipStream_t borrow);
// Bucket b's in-place sum on the lane's stream, ordered behind everything enqueued on `producer` so far.  UAD_AR_SKIP: everything but the collective.
int uad_ar_issue(UadArLane* l, int b, hipStream_t producer);
// Bucket b's in-place sum straight on `st` (the caller has ordered `st` itself).
int uad_ar_reduce(UadArLane* l, int b, hipStream_t st);
// `consumer` waits once for the collectives issued on the lane so far (nothing to do on the lane's own stream).
int uad_ar_join(UadArLane* l, hipStream_t consumer);
// Synchronizes and destroys a stream the lane owns, destroys its events.  Call it before the gradient buffer is freed.
int uad_ar_close(UadArLane* l);
