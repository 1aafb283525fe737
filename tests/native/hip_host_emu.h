// The host-emulation shim of the tests/native/*_emu.cpp programs: everything a kernel source of csrc/ needs to compile for the CPU and run
// there.  An emulator includes this header, then the .hip file (whose launch layer UAD_HOST_EMULATION leaves out), and drives the kernels
// with the library's own launch geometry through launch_loop / launch_threads.  `__shared__` is a static here, so LDS objects are plain
// globals that an emulator's poison callable can name.
#pragma once
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#define UAD_HOST_EMULATION
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __restrict__

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
thread_local dim3 threadIdx, blockIdx;
dim3 blockDim, gridDim;
std::barrier<>* block_barrier = nullptr;
static inline void __syncthreads() { block_barrier->arrive_and_wait(); }

struct alignas(16) float4 { float x, y, z, w; };
struct alignas(16) int4 { int x, y, z, w; };
struct alignas(16) uint4 { unsigned x, y, z, w; };
struct alignas(4) uchar4 { unsigned char x, y, z, w; };
static inline float4 make_float4(float a, float b, float c, float d) { return float4{a, b, c, d}; }
static inline uint4 make_uint4(unsigned a, unsigned b, unsigned c, unsigned d) { return uint4{a, b, c, d}; }

static inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline int atomicCAS(int* p, int expected, int desired) {
    __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expected;                                              // the old value, as the device function returns it
}

// a kernel without a barrier: every thread of every workgroup in turn, as a plain loop
template <class F>
static void launch_loop(dim3 g, dim3 b, F kernel) {
    gridDim = g; blockDim = b;
    for (unsigned bz = 0; bz < g.z; ++bz)
        for (unsigned by = 0; by < g.y; ++by)
            for (unsigned bx = 0; bx < g.x; ++bx)
                for (unsigned ty = 0; ty < b.y; ++ty)
                    for (unsigned tx = 0; tx < b.x; ++tx) { blockIdx = dim3(bx, by, bz); threadIdx = dim3(tx, ty, 0); kernel(); }
}

static inline void no_poison() {}

// a kernel with barriers: the block.x * block.y threads of a workgroup are real threads around a std::barrier and live for the whole launch;
// the workgroups of the grid.x * grid.y * grid.z grid run one after the other.  LDS does not survive a workgroup and holds nothing known at
// its start: thread 0 runs `poison` before each workgroup, between two barrier arrivals, so nobody reads LDS any more when it is poisoned
// again.  A kernel thread that returns early simply reaches the end-of-workgroup barrier.
template <class F, class P = void (*)()>
static void launch_threads(dim3 g, dim3 b, F kernel, P poison = no_poison) {
    gridDim = g; blockDim = b;
    std::barrier<> bar(b.x * b.y);
    block_barrier = &bar;
    std::vector<std::thread> threads;
    for (unsigned ty = 0; ty < b.y; ++ty)
        for (unsigned tx = 0; tx < b.x; ++tx)
            threads.emplace_back([=, &bar] {
                threadIdx = dim3(tx, ty, 0);
                for (unsigned bz = 0; bz < g.z; ++bz)
                    for (unsigned by = 0; by < g.y; ++by)
                        for (unsigned bx = 0; bx < g.x; ++bx) {
                            if (tx == 0 && ty == 0) poison();
                            bar.arrive_and_wait();
                            blockIdx = dim3(bx, by, bz);
                            kernel();
                            bar.arrive_and_wait();
                        }
            });
    for (auto& t : threads) t.join();
}

template <class T>
static bool read_all(const char* path, T* p, size_t count) {
    FILE* f = fopen(path, "rb");
    const bool ok = f && fread(p, sizeof(T), count, f) == count;
    if (f) fclose(f);
    return ok;
}

template <class T>
static bool read_all(const char* path, std::vector<T>& v) { return read_all(path, v.data(), v.size()); }

template <class T>
static bool write_all(const char* path, const T* p, size_t count) {
    FILE* f = fopen(path, "wb");
    const bool ok = f && fwrite(p, sizeof(T), count, f) == count;
    if (f) fclose(f);
    return ok;
}

// a 16-byte aligned allocation of count + off elements; the array starts off elements in
template <class T>
struct Shifted {
    void* raw;
    T* p;
    Shifted(size_t count, size_t off) {
        raw = std::aligned_alloc(16, ((count + off) * sizeof(T) + 31) / 16 * 16);
        p = static_cast<T*>(raw) + off;
    }
    ~Shifted() { std::free(raw); }
};

// an output of count elements, off elements off its 16-byte alignment, between two runs of GUARD elements (a multiple of 16 bytes: p keeps
// the alignment off gives) that hold GUARD_VALUE and must come back untouched
template <class T, T GUARD_VALUE>
struct Guarded {
    static constexpr size_t GUARD = 64;
    Shifted<T> buf;
    size_t count;
    T* p;
    explicit Guarded(size_t count_, size_t off = 0) : buf(count_ + 2 * GUARD, off), count(count_), p(buf.p + GUARD) {
        std::fill(buf.p, buf.p + count + 2 * GUARD, GUARD_VALUE);
    }
    bool intact() const {
        for (size_t i = 0; i < GUARD; ++i)
            if (buf.p[i] != GUARD_VALUE || buf.p[GUARD + count + i] != GUARD_VALUE) return false;
        return true;
    }
};
