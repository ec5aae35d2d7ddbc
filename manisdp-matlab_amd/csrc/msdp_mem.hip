// msdp_mem.hip -- device memory of a handle (msdp_dev_alloc_bytes and its kin), the per-process pool of fine-grained
// exchange memory (arenas with a coalescing sub-allocator) and the per-process cache of streams + pinned control blocks.
#include "msdp_common.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

int msdp_dev_alloc_bytes(msdp_handle h, void** out, size_t bytes) {
    void* p = nullptr;
    *out = nullptr;
    if (bytes == 0) bytes = 1;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        msdp_set_error("hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        return MSDP_ENOMEM;
    }
    h->allocs.push_back(p);
    *out = p;
    return 0;
}
// Uncached (MTYPE UC) device memory for the words that workgroups on different XCDs exchange inside one launch:
// sc1 accesses to it skip the L2 look-up on both ends (tools/microbench_sync.hip: grid reduction 1.99 -> 1.24 us;
// 12.8 -> 10.0 us per tCG trip).  Falls back to plain hipMalloc where the flag is not supported.
// Uncached blocks come from a per-process pool and go back to it, never to the driver, while the process lives
// (msdp_release_cache frees the pool).  Round 3: uncached memory that was allocated and hipFree'd per handle left LATER handles
// of the process with corrupted buffers (a fresh handle's eG read back as garbage in two runs out of three of
// tests/test_gpu_blockeig.py once the block eigen-solver added a 20-MB uncached allocation per handle; the same tests pass with
// plain memory, and with this pool) -- memory whose caching attribute changes between owners is not safe to recycle here.
// Round 4: the pool is a set of ARENAS with a coalescing first-fit sub-allocator instead of one driver block per request.  A
// long-lived host (MATLAB) that cycles handles of varying sizes re-uses the same arenas -- freed blocks merge with their
// neighbours, so the pool grows to the high-water mark of what was live together, not with the number of distinct sizes
// (the per-request pool matched sizes within 2 x only and grew without bound).  Arenas go back to the driver only when NO
// uncached block of the process is live any more: then, beyond MSDP_UC_POOL_CAP bytes, largest first (msdp_destroy of the last
// handle), or all of them (msdp_release_cache) -- uncached pages never change owner while a handle that could be handed
// them lives.  tests/test_gpu_edge_cases.py::test_handle_churn_keeps_results_and_pool_bounded.
struct UcArena { char* base; size_t bytes; int dev; std::map<size_t, size_t> freemap; size_t live; };   // freemap: offset -> size
static std::mutex g_uc_mutex;
static std::vector<UcArena> g_uc_arenas;
static std::map<void*, std::pair<int, size_t>> g_uc_live;     // block -> (arena index, size)
static const size_t UC_ALIGN = 256, UC_ARENA_MIN = (size_t)32 << 20;
static size_t g_uc_cap = (size_t)1 << 30;                     // pool bytes kept when nothing is live (MSDP_UC_POOL_CAP, bytes)
static int g_uc_release = 0;                                  // MSDP_UC_RELEASE=1: arenas may go back to the driver (see msdp_uc_free)
static size_t uc_pool_bytes_locked() { size_t t = 0; for (auto& a : g_uc_arenas) t += a.bytes; return t; }
static int g_uc_direct = 0;                                   // MSDP_UC_POOL=0: one driver block per request, hipFree'd at once (the round-3
                                                              //   arrangement that corrupted later handles; kept for tools/uc_pool_stress.py only)
// Round 5: the exchange memory is FINE-GRAINED device memory (hipDeviceMallocFinegrained), not uncached (hipDeviceMallocUncached) any more.
// tools/uc_pool_stress.py, 300 handles per mode: uncached blocks that went back to the driver corrupt whoever receives their pages next --
// the same three handles wrong whether the block was hipFree'd as it was (mode 0), hipMemset + synchronised first (4), or rewritten line
// by line with cached stores and an L2 write-back / invalidate (5): a formerly-uncached page keeps something of its memory type that no
// access from user space clears.  Fine-grained blocks freed the same way: 0 of 300 wrong (mode 6), and the persistent trip is FASTER on
// them (G81, p = 32: 6.41 against 6.55 us; 146 100 against 142 500 Hess-vec/s per trustregions() call, profiles/r5_finegrained_vs_uncached.log).
// MSDP_UC_MEM=uncached restores the old memory type (then the arenas never go back to the driver, as in round 4).
static unsigned g_uc_flags = hipDeviceMallocFinegrained;     // MSDP_UC_MEM=uncached: hipDeviceMallocUncached; MSDP_UC_POOL=6 / 7: fine-grained (direct / arenas)
// Round 5 probes (tools/uc_pool_stress.py): what has to happen to a formerly-uncached block before hipFree for its pages to be safe in
// somebody else's hands?  4: hipMemset of the whole block + hipDeviceSynchronize; 5: every 128-byte line written by a kernel with plain
// (cached) stores, then an L2 write-back + invalidate by every wave (buffer_wbl2 sc1 / buffer_inv sc1), then hipDeviceSynchronize.
__global__ void k_uc_scrub(unsigned long long* p, size_t words) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) p[i] = 0ULL;
    asm volatile("s_waitcnt vmcnt(0)\n\tbuffer_wbl2 sc1\n\ts_waitcnt vmcnt(0)\n\tbuffer_inv sc1" ::: "memory");
}
void* msdp_uc_alloc(size_t bytes) {
    if (bytes == 0) bytes = 8;
    bytes = (bytes + UC_ALIGN - 1) / UC_ALIGN * UC_ALIGN;
    int dev = -1;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_uc_mutex);
    static bool env_read = false;
    if (!env_read) {
        env_read = true;
        const char* e = getenv("MSDP_UC_POOL_CAP"); if (e && *e) g_uc_cap = (size_t)strtoull(e, nullptr, 10);
        e = getenv("MSDP_UC_MEM"); if (e && !strcmp(e, "uncached")) g_uc_flags = hipDeviceMallocUncached;
        e = getenv("MSDP_UC_POOL"); if (e && *e >= '0' && *e <= '5' && *e != '1') g_uc_flags = hipDeviceMallocUncached;   // the probes of the old memory type
        e = getenv("MSDP_UC_RELEASE"); if (e && *e == '1') g_uc_release = 1; else if (e && *e == '0') g_uc_release = 0;
        else g_uc_release = g_uc_flags == hipDeviceMallocFinegrained ? 1 : 0;   // fine-grained pages are safe in anybody's hands
        // probes of tools/uc_pool_stress.py: 0 = direct (hipFree at destroy), 2 = direct + hipDeviceSynchronize before every free,
        // 3 = direct, uncached blocks never freed
        // round 5: 4 / 5 = direct, the block scrubbed before hipFree (see k_uc_scrub); 6 = direct, fine-grained instead of uncached memory;
        // 7 = the arenas, of fine-grained memory
        e = getenv("MSDP_UC_POOL");
        if (e && *e >= '0' && *e <= '7' && *e != '1') g_uc_direct = *e == '0' ? 1 : (*e == '7' ? 0 : *e - '0');
        if (e && (*e == '6' || *e == '7')) g_uc_flags = hipDeviceMallocFinegrained;
    }
    if (g_uc_direct) {
        void* p = nullptr;
        if (hipExtMallocWithFlags(&p, bytes, g_uc_flags) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        if (g_uc_direct == 3) g_uc_live[p] = {-1, bytes};     // registered with no arena: msdp_uc_free keeps it for ever
        if (g_uc_direct == 4 || g_uc_direct == 5) g_uc_live[p] = {-2, bytes};   // registered for its size: scrubbed in msdp_uc_free, hipFree'd by the caller
        return p;                                             // else not registered: msdp_uc_free returns false and the caller hipFree's it
    }
    for (int pass = 0; pass < 2; ++pass) {
        // best fit over the free ranges of this device's arenas
        int ba = -1; size_t boff = 0, bsz = (size_t)-1;
        for (size_t ai = 0; ai < g_uc_arenas.size(); ++ai) {
            UcArena& a = g_uc_arenas[ai];
            if (a.dev != dev) continue;
            for (auto& fr : a.freemap)
                if (fr.second >= bytes && fr.second < bsz) { ba = (int)ai; boff = fr.first; bsz = fr.second; }
        }
        if (ba >= 0) {
            UcArena& a = g_uc_arenas[ba];
            a.freemap.erase(boff);
            if (bsz > bytes) a.freemap[boff + bytes] = bsz - bytes;
            a.live += bytes;
            void* p = a.base + boff;
            g_uc_live[p] = {ba, bytes};
            return p;
        }
        if (pass == 1) break;
        void* p = nullptr;
        const size_t ab = std::max(bytes, UC_ARENA_MIN);
        if (hipExtMallocWithFlags(&p, ab, g_uc_flags) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        UcArena a; a.base = (char*)p; a.bytes = ab; a.dev = dev; a.live = 0; a.freemap[0] = ab;
        g_uc_arenas.push_back(a);
    }
    return nullptr;
}
static void uc_trim_locked(size_t keep) {                     // only ever called with no live block anywhere
    std::sort(g_uc_arenas.begin(), g_uc_arenas.end(), [](const UcArena& x, const UcArena& y) { return x.bytes > y.bytes; });
    while (!g_uc_arenas.empty() && uc_pool_bytes_locked() > keep) { (void)hipFree(g_uc_arenas.front().base); g_uc_arenas.erase(g_uc_arenas.begin()); }
}
bool msdp_uc_free(void* p) {                                  // true: p was an uncached block (now back in its arena)
    if (!p) return false;
    std::lock_guard<std::mutex> lk(g_uc_mutex);
    auto it = g_uc_live.find(p);
    if (it == g_uc_live.end()) { if (g_uc_direct == 2) (void)hipDeviceSynchronize(); return false; }
    if (it->second.first == -2) {                             // probe modes 4 / 5: scrub, then the caller hipFree's
        const size_t sz = it->second.second;
        (void)hipDeviceSynchronize();
        if (g_uc_direct == 4) (void)hipMemset(p, 0, sz);
        else hipLaunchKernelGGL(k_uc_scrub, dim3(256), dim3(256), 0, 0, (unsigned long long*)p, sz / 8);
        (void)hipDeviceSynchronize();
        g_uc_live.erase(it);
        return false;
    }
    if (it->second.first < 0) return true;                    // probe mode 3: leaked on purpose
    UcArena& a = g_uc_arenas[it->second.first];
    size_t off = (size_t)((char*)p - a.base), sz = it->second.second;
    a.live -= sz;
    auto nx = a.freemap.lower_bound(off);
    if (nx != a.freemap.end() && off + sz == nx->first) { sz += nx->second; nx = a.freemap.erase(nx); }
    if (nx != a.freemap.begin()) { auto pv = std::prev(nx); if (pv->first + pv->second == off) { off = pv->first; sz += pv->second; a.freemap.erase(pv); } }
    a.freemap[off] = sz;
    g_uc_live.erase(it);
    // Round 5: arenas of UNCACHED memory are never handed back to the driver while the process lives -- such pages corrupt whoever
    // receives them next (torch, a MATLAB gpuArray in the same process included), and no scrub of tools/uc_pool_stress.py is clean.
    // Arenas of fine-grained memory (the default now) go back beyond MSDP_UC_POOL_CAP when nothing is live and on msdp_release_cache.
    if (g_uc_release && g_uc_live.empty() && uc_pool_bytes_locked() > g_uc_cap) uc_trim_locked(g_uc_cap);   // indices are free to change: nothing is live
    return true;
}
void msdp_uc_release_pool() {
    std::lock_guard<std::mutex> lk(g_uc_mutex);
    if (!g_uc_release || !g_uc_live.empty()) return;          // a live handle owns uncached blocks: its arenas stay
    uc_trim_locked(0);
}
// Pool statistics: bytes the arenas hold, bytes handed out, number of arenas (tests)
extern "C" int msdp_debug_pool_stats(int64_t* pool_bytes, int64_t* live_bytes, int64_t* arenas) {
    std::lock_guard<std::mutex> lk(g_uc_mutex);
    size_t live = 0;
    for (auto& a : g_uc_arenas) live += a.live;
    if (pool_bytes) *pool_bytes = (int64_t)uc_pool_bytes_locked();
    if (live_bytes) *live_bytes = (int64_t)live;
    if (arenas) *arenas = (int64_t)g_uc_arenas.size();
    return 0;
}
extern "C" int msdp_debug_mem_info(int64_t* free_bytes, int64_t* total_bytes) {
    size_t f = 0, t = 0;
    if (hipMemGetInfo(&f, &t) != hipSuccess) { (void)hipGetLastError(); msdp_set_error("hipMemGetInfo failed"); return MSDP_EHIP; }
    if (free_bytes) *free_bytes = (int64_t)f;
    if (total_bytes) *total_bytes = (int64_t)t;
    return 0;
}
int msdp_dev_alloc_uncached_bytes(msdp_handle h, void** out, size_t bytes) {
    void* p = msdp_uc_alloc(bytes);
    if (!p) return msdp_dev_alloc_bytes(h, out, bytes);
    h->allocs.push_back(p);
    *out = p;
    return 0;
}
void msdp_dev_free(msdp_handle h, void* p) {
    if (!p) return;
    for (size_t i = 0; i < h->allocs.size(); ++i)
        if (h->allocs[i] == p) { h->allocs.erase(h->allocs.begin() + i); break; }
    if (!msdp_uc_free(p)) (void)hipFree(p);
}

// The stream and the four pinned control blocks of a handle come from a small cache of the process (round 6): hipStreamCreate 2.8 ms,
// hipStreamDestroy 3.9 - 4.5 ms and the hipHostMalloc / hipHostFree pairs were 8 of the 163 ms of a G81 solve to KKT 1e-8, paid by every
// handle a host opens (rocprofv3 --hip-trace, tools/hip_api_totals.py).  A kit goes back when its handle is destroyed (the stream
// synchronised), at most HOST_KIT_MAX per process are kept, msdp_release_cache frees them.
struct HostKit { int dev; hipStream_t stream; Ctl* h_ctl; Frame* h_frame; volatile int* h_flags; volatile unsigned long long* h_status; };
static std::mutex g_kit_mutex;
static std::vector<HostKit> g_kits;
static const size_t HOST_KIT_MAX = 8;
static void host_kit_free(HostKit& k) {
    if (k.h_ctl) (void)hipHostFree(k.h_ctl);
    if (k.h_frame) (void)hipHostFree(k.h_frame);
    if (k.h_status) (void)hipHostFree((void*)k.h_status);
    if (k.h_flags) (void)hipHostFree((void*)k.h_flags);
    if (k.stream) (void)hipStreamDestroy(k.stream);
}
bool msdp_host_kit_take(msdp_handle h) {
    int dev = -1;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_kit_mutex);
    for (size_t i = 0; i < g_kits.size(); ++i) {
        if (g_kits[i].dev != dev) continue;
        HostKit k = g_kits[i];
        g_kits.erase(g_kits.begin() + i);
        h->stream = k.stream; h->h_ctl = k.h_ctl; h->h_frame = k.h_frame; h->h_flags = k.h_flags; h->h_status = k.h_status;
        memset(h->h_ctl, 0, sizeof(Ctl)); memset(h->h_frame, 0, 2 * sizeof(Frame)); memset((void*)h->h_flags, 0, 64); memset((void*)h->h_status, 0, 64);
        return true;
    }
    return false;
}
void msdp_host_kit_give(msdp_handle h) {
    HostKit k = {-1, h->stream, h->h_ctl, h->h_frame, h->h_flags, h->h_status};
    h->stream = nullptr; h->h_ctl = nullptr; h->h_frame = nullptr; h->h_flags = nullptr; h->h_status = nullptr;
    (void)hipGetDevice(&k.dev);
    const bool whole = k.stream && k.h_ctl && k.h_frame && k.h_flags && k.h_status;
    if (whole && hipStreamSynchronize(k.stream) == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_kit_mutex);
        if (g_kits.size() < HOST_KIT_MAX) { g_kits.push_back(k); return; }
    }
    (void)hipGetLastError();
    host_kit_free(k);
}
void msdp_host_kits_release() {                               // msdp_release_cache
    std::lock_guard<std::mutex> lk(g_kit_mutex);
    for (auto& k : g_kits) host_kit_free(k);
    g_kits.clear();
}
