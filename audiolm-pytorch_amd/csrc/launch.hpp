// Host-side launch plumbing shared by every launcher that needs more dynamic LDS than the default 64 KB limit.
// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (kernel, device): it is set once per pair and raised when a launcher asks for more.
// The table below is the library's only process state: one per process, guarded by a mutex, so the C ABI stays callable from any thread.
#pragma once
#include <mutex>
#include <vector>

// (kernel function pointer, device ordinal) -> bytes already granted.  Plain C++ (no HIP): tests/launch_table_main.cpp builds it with the host compiler.
class AlmLdsTable {
public:
    // must the attribute be set?  yes when (fn, dev) is unseen or was granted fewer bytes (a smaller request never shrinks the limit)
    bool needs_set(const void* fn, int dev, int bytes) {
        std::lock_guard<std::mutex> g(mu_);
        const Entry* e = find(fn, dev);
        return !e || e->bytes < bytes;
    }
    // a set that SUCCEEDED: a failed one is not recorded, so the next call tries again and returns the error again
    void record(const void* fn, int dev, int bytes) {
        std::lock_guard<std::mutex> g(mu_);
        if (Entry* e = find(fn, dev)) e->bytes = e->bytes < bytes ? bytes : e->bytes;
        else entries_.push_back(Entry{fn, dev, bytes});
    }
    size_t size() {
        std::lock_guard<std::mutex> g(mu_);
        return entries_.size();
    }

private:
    struct Entry { const void* fn; int dev, bytes; };
    Entry* find(const void* fn, int dev) {                              // a few dozen entries at most: linear scan
        for (Entry& e : entries_) if (e.fn == fn && e.dev == dev) return &e;
        return nullptr;
    }
    std::mutex mu_;
    std::vector<Entry> entries_;
};

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

inline AlmLdsTable g_alm_lds_table;

// allow `bytes` of dynamic LDS for kernel `kfn` on the current device -> 0 or the hipError_t.  Every launcher asks one fixed size per kernel, so two threads
// that race on the first call set the same value twice.
inline int alm_lds_limit(const void* kfn, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (!g_alm_lds_table.needs_set(kfn, dev, bytes)) return 0;
    e = hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return (int)e;
    g_alm_lds_table.record(kfn, dev, bytes);
    return 0;
}

template <class K, class... Args>
int alm_launch_lds(K kfn, dim3 grid, dim3 block, int lds_bytes, hipStream_t st, const Args&... args) {
    const int rc = alm_lds_limit(reinterpret_cast<const void*>(kfn), lds_bytes);
    if (rc) return rc;
    hipLaunchKernelGGL(kfn, grid, block, lds_bytes, st, args...);
    return 0;
}

// the tile GEMMs' grid: (tiles_m * tiles_n, ny, nz), or with `raster` the 1-D XCD-panel order of 8 * PL * Q * nz workgroups (PL = panel length / 8: `plimit`
// when > 0, else the longer tile dimension x ny; Q = the shorter tile dimension).  P: the kernel's parameter block (M, N read here)
template <int BM, int BN, int THREADS, int LDS, class K, class P>
int alm_launch_raster(K kfn, const P& p, bool raster, int plimit, int ny, int nz, hipStream_t st) {
    const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
    if (!raster) return alm_launch_lds(kfn, dim3(tiles_m * tiles_n, ny, nz), dim3(THREADS), LDS, st, p);
    const int tmaj = tiles_m >= tiles_n ? tiles_m : tiles_n, Q = tiles_m >= tiles_n ? tiles_n : tiles_m;
    const int PL = ((plimit > 0 ? plimit : tmaj * ny) + 7) / 8;
    return alm_launch_lds(kfn, dim3(8 * PL * Q * nz), dim3(THREADS), LDS, st, p);
}
#endif
