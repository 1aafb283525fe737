// What the two model handles (uad_model.hip: AE / VAE family, uad_gan.hip: materialised-graph family) share: the tensor table over the flat fp32
// parameter / gradient / Adam-slot buffers, the packed weight copies, the allocation list, and the argument checks and copies behind the
// *_tensor_info / *_set_buffer / *_get_buffer entry points.  Host-only; each handle struct derives from UadHandleCore and keeps what differs
// (how a parameter write invalidates the packs, extra optimizer slots, segments / groups, step counters) to itself.
#pragma once
#include <string.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/uad_hip.h"
#include "uad_allreduce.h"
#include "uad_kernels.h"

#define fail uad_fail

constexpr float kBnEps = 1e-3f;     // tf.layers.BatchNormalization default epsilon (frozen statistics)
constexpr float kLrelu = 0.3f;      // keras LeakyReLU() default (customlayers.py:23,36)

struct UadTensor {
    std::string name;
    long long off;
    int rank;
    int shape[4];
    long long count() const { return (long long)shape[0] * shape[1] * shape[2] * shape[3]; }
};

struct UadHandleCore {
    std::vector<UadTensor> tensors;
    long long nparams;
    float *params, *grads, *adam_m, *adam_v;
    float *wpack_f, *wpack_d;          // k-quad-interleaved fp32 copies of the packed kernels
    float *wpack16_f, *wpack16_d;      // bf16 hi | lo planes of the same kernels (bf16x3); 2 * nparams ushorts each
    float *wpack3_f, *wpack3_d;        // three bf16 planes (bf16x6 products); 4 * nparams ushorts each, null until a mode needs them
    int math;                          // UAD_MATH_*
    bool packed_valid;                 // the packs hold the current `params`
    UadGemmWs ws;                      // split-K slabs for the GEMMs that cannot fill the chip on their own
    UadArLane ar;                      // library-issued gradient all-reduce (uad_allreduce.h)
    std::vector<void*> allocs;         // every dev_alloc of the handle: freed by core_free
    std::map<std::string, std::pair<float*, long long>> dbg;      // the allocations that were given a name (debug_buffer lookup)
};

inline float* P(UadHandleCore* c, long long off) { return c->params + off; }
inline float* Gr(UadHandleCore* c, long long off) { return c->grads + off; }

inline long long add_tensor(UadHandleCore* c, const std::string& name, int rank, int s0, int s1, int s2, int s3) {
    UadTensor t;
    t.name = name; t.off = c->nparams; t.rank = rank;
    t.shape[0] = s0; t.shape[1] = s1; t.shape[2] = s2; t.shape[3] = s3;
    c->nparams += t.count();
    c->tensors.push_back(t);
    return t.off;
}

// zero-filled device floats owned by the handle; a name makes them visible to the debug_buffer lookup
inline int dev_alloc(UadHandleCore* c, float** p, size_t floats, const char* name = nullptr) {
    void* q = nullptr;
    if (floats == 0) floats = 4;
    HIP_TRY(hipMalloc(&q, floats * sizeof(float)));
    HIP_TRY(hipMemset(q, 0, floats * sizeof(float)));
    c->allocs.push_back(q);
    *p = (float*)q;
    if (name) c->dbg[name] = std::make_pair((float*)q, (long long)floats);
    return UAD_OK;
}

// closes the all-reduce lane (it may still read `grads`), then frees every allocation; the caller deletes the handle
inline int core_free(UadHandleCore* c) {
    const int rc = uad_ar_close(&c->ar);
    for (void* p : c->allocs) (void)hipFree(p);
    c->allocs.clear();
    return rc;
}

inline int core_tensor_info(const UadHandleCore* c, int idx, char* name, int name_cap, long long* offset, int* rank, int* shape4) {
    if (!c || idx < 0 || idx >= (int)c->tensors.size()) return fail(UAD_ERR_INVALID, "tensor index out of range");
    const UadTensor& t = c->tensors[idx];
    if (name && name_cap > 0) { strncpy(name, t.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
    if (offset) *offset = t.off;
    if (rank) *rank = t.rank;
    if (shape4) for (int i = 0; i < 4; ++i) shape4[i] = t.shape[i];
    return UAD_OK;
}

// the four buffers both engines have; no side effect (a caller that may WRITE through the pointer runs its engine's invalidation itself)
inline float* core_buffer_ptr(const UadHandleCore* c, int which) {
    if (!c) return nullptr;
    switch (which) {
        case UAD_BUF_PARAMS: return c->params;
        case UAD_BUF_GRADS: return c->grads;
        case UAD_BUF_ADAM_M: return c->adam_m;
        case UAD_BUF_ADAM_V: return c->adam_v;
    }
    return nullptr;
}

// host <-> device copies of one flat buffer `p` (null: the engine has no such buffer).  The engine's hook runs once the arguments are known to be
// good: before_write in front of the copy into the handle, after_sync (returns a status) between the device synchronize and the copy out.
template <class Hook>
int core_set_buffer(UadHandleCore* c, const char* who, float* p, const float* host, long long count, Hook before_write) {
    if (!p || !host || count != c->nparams) return fail(UAD_ERR_INVALID, "%s: bad arguments (count=%lld, expected %lld)", who, count, c ? c->nparams : -1);
    before_write();
    HIP_TRY(hipMemcpy(p, host, (size_t)count * sizeof(float), hipMemcpyHostToDevice));
    return UAD_OK;
}
template <class Hook>
int core_get_buffer(UadHandleCore* c, const char* who, const float* p, float* host, long long count, Hook after_sync) {
    if (!p || !host || count != c->nparams) return fail(UAD_ERR_INVALID, "%s: bad arguments (count=%lld, expected %lld)", who, count, c ? c->nparams : -1);
    HIP_TRY(hipDeviceSynchronize());
    if (const int rc = after_sync()) return rc;
    HIP_TRY(hipMemcpy(host, p, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
    return UAD_OK;
}

inline UadXform no_xform() { UadXform x; x.scale = nullptr; x.shift = nullptr; x.alpha = 1.f; x.mult = 1.f; return x; }
inline UadEpilogue epi_bias(const float* bias, const float* mul = nullptr, const float* add = nullptr) {
    UadEpilogue e;
    memset(&e, 0, sizeof e);
    e.kind = UAD_EPI_BIAS; e.bias = bias; e.mul = mul; e.add = add;
    return e;
}
inline UadConvDesc dense_desc(int n, int in, int out) { return UadConvDesc{n, 1, 1, in, 1, 1, out, 1, 1, 0}; }
inline UadConvDesc conv1x1_desc(int n, int h, int w, int cin, int cout) { return UadConvDesc{n, h, w, cin, h, w, cout, 1, 1, 0}; }
inline int ilog2i(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
inline unsigned blocks256(size_t n) { return (unsigned)((n + 255) / 256); }
