// hip_host.h -- host-side HIP helpers that know nothing of the engine: the device scope of every entry point (engine and trainer) and
// the owners of device / pinned memory.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

// Every entry point works on its object's device and leaves the caller's current HIP device as it found it (PyTorch and
// other engines in the same process keep theirs).
struct DeviceScope {
    int prev;
    bool ok;
    explicit DeviceScope(int dev) : prev(-1) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (prev == dev) || hipSetDevice(dev) == hipSuccess;
        if (prev == dev) prev = -1;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// The device allocations of one lifetime: handed out by alloc, freed together by clear() or with the owner (whose device must be
// current then).  A buffer that is replaced on its own gets an owner of its own.
struct DeviceAllocs {
    std::vector<void*> ptrs;
    hipError_t last = hipSuccess;   // why the last alloc returned nullptr
    DeviceAllocs() = default;
    DeviceAllocs(const DeviceAllocs&) = delete;
    DeviceAllocs& operator=(const DeviceAllocs&) = delete;
    template <typename T>
    T* alloc(size_t n) {   // n elements, at least 16 bytes
        void* q = nullptr;
        last = hipMalloc(&q, n * sizeof(T) > 0 ? n * sizeof(T) : 16);
        if (last != hipSuccess) return nullptr;
        ptrs.push_back(q);
        return (T*)q;
    }
    void clear() { for (void* p : ptrs) (void)hipFree(p); ptrs.clear(); }
    ~DeviceAllocs() { clear(); }
};

// One device buffer whose size depends on the call: a larger one replaces it (the owner's stream is idle between calls).  Freed with
// the owner, whose device must be current then.
struct DeviceBuffer {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t last = hipSuccess;   // why the last reserve returned false
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    bool reserve(size_t n) {   // the new buffer first: a failure leaves the old one in place
        if (p && bytes >= n) return true;
        void* q = nullptr;
        last = hipMalloc(&q, n);
        if (last != hipSuccess) return false;
        if (p) (void)hipFree(p);
        p = q;
        bytes = n;
        return true;
    }
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
};

// One block of pinned host memory (hipHostMalloc)
struct PinnedBlock {   // (only ever a member of an object that cannot be copied)
    void* p = nullptr;
    ~PinnedBlock() { if (p) (void)hipHostFree(p); }
};
