// smcsmc_amd/csrc/pf_devmem.h -- the error text of the C-ABI and the owner of device memory on the host side of pf_hip.hip.
// Nothing else in pf_hip.hip, pf_run.h or the host headers allocates or frees device memory.
#pragma once

static thread_local std::string g_err;
const char* pf_last_error(void) { return g_err.c_str(); }

#define HIPCHK(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            g_err = std::string(#call) + ": " + hipGetErrorString(e_);                    \
            return -1;                                                                    \
        }                                                                                 \
    } while (0)

// bytes held by all DevMem of the process (pf_test_live_bytes: a leak shows without asking a shared device how much memory is free)
static std::atomic<long long> g_live_bytes{0};

// Owns device allocations, one per array, and frees them when it goes: a member of pf_handle for the handle's arrays, a local of the entry
// points without a handle.  Every call returns 0, or -1 with g_err set.
struct DevMem {
    struct Block { void* p; size_t bytes; };
    std::vector<Block> blocks;
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { clear(); }
    void clear() {
        for (const Block& b : blocks) { hipFree(b.p); g_live_bytes -= (long long)b.bytes; }
        blocks.clear();
    }
    // max(count, 1) elements, not initialised
    template <class T>
    int reserve(T** p, size_t count) {
        void* q = nullptr;
        HIPCHK(hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
        blocks.push_back({q, std::max<size_t>(count, 1) * sizeof(T)});
        g_live_bytes += (long long)blocks.back().bytes;
        *p = (T*)q;
        return 0;
    }
    // ... zeroed on `stream`
    template <class T>
    int alloc(T** p, size_t count, hipStream_t stream) {
        if (reserve(p, count)) return -1;
        HIPCHK(hipMemsetAsync(*p, 0, std::max<size_t>(count, 1) * sizeof(T), stream));
        return 0;
    }
    // ... filled from the host on `stream`, behind the memset: a plain hipMemcpy is not ordered with a non-blocking stream, and the memset,
    // queued behind those of larger arrays, could land after it and leave zeros.  The caller synchronises the stream, once, before `src` goes
    // away or the data is needed.
    template <class T>
    int upload(const T** p, const T* src, size_t count, hipStream_t stream) {
        T* q = nullptr;
        if (alloc(&q, count, stream)) return -1;
        if (count) HIPCHK(hipMemcpyAsync(q, src, count * sizeof(T), hipMemcpyHostToDevice, stream));
        *p = q;
        return 0;
    }
};

// `count` elements from the device into v (the getters; the caller has synchronised)
template <class T>
static int download(std::vector<T>& v, const T* dev, size_t count) {
    v.resize(count);
    if (count) HIPCHK(hipMemcpy(v.data(), dev, count * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}
