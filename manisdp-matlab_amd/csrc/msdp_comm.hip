// msdp_comm.hip -- row sharding: the RCCL communicator and its two stand-ins (handles of one process, processes that share
// memory through HIP IPC), the collectives and the halo exchange above them, the host side of the cross-rank persistent tCG
// (xr_*), and the row partition (msdp_comm_init*).  The only unit that includes RCCL and the POSIX shared-memory headers.
#include "msdp_common.h"
#include <rccl/rccl.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

// send / receive lists of the halo exchange ("Halo exchange" below)
struct Halo {
    int N = 0;
    std::vector<int> send_cnt, send_off, recv_cnt, recv_off;     // per peer, in rows
    int send_rows = 0, recv_rows = 0;
    int* send_idx = nullptr;       // device: local row index of every row to send (peer-major)
    int* recv_idx = nullptr;       // device: global row index of every row to receive (peer-major)
    double* sendbuf = nullptr;     // device: send_rows x ldcap
    double* recvbuf = nullptr;     // device: recv_rows x ldcap
    int ldcap = 0;
    // cross-rank persistent kernels, round 5 ("push" exchange): every member's exchange buffer = [its own rows (cap)] [a slot for
    // every foreign row its rows of C reference, in the order of recv_idx].  A member stores its rows into its own buffer AND into the
    // halo slots of the members that reference them, so every gather is a local load with buffer-local indices:
    int* xr_colind = nullptr;      // device: the local CSR column indices remapped to buffer positions (c - row0, or cap + halo slot)
    int* xr_ellc = nullptr;        // device: the same for the ELL copy ([w][cap])
    int* xr_pq = nullptr;          // device: [2][n_loc] member that needs local row i (-1: none), up to two per row
    int* xr_pidx = nullptr;        // device: [2][n_loc] its buffer position there (cap_of_that_member + slot)
    bool xr_ok = false;            // false: some row is referenced by more than two other members -> lock-step trips
};

// ------------------------------------------------------------------ in-process stand-in for the communicator
// N handles of ONE process on ONE GPU, each driven by its own host thread, stand in for N ranks: the three collectives the
// library uses (all-reduce of a device array, all-gather of equal slabs) are carried out with a host barrier and device
// copies / a summation kernel between the handles' buffers.  Everything else -- the row partition, the row offsets into the
// replicated operator state, the lock-step tCG driver, the order and number of collective calls on every rank -- is the
// code of the RCCL run, so one GPU can execute the N-rank paths (tests/test_gpu_local_ranks.py).  Sums run in rank order on
// every member: all members obtain the same bits, as with ncclAllReduce.
#define LOCAL_MAX_RANKS 8
// Round 5: the same group, with its members in DIFFERENT PROCESSES (msdp_comm_init_ipc) -- ranks on one GPU, or one rank per GPU of a
// node with peer access.  What the in-process members share through their common address space travels through two shared blocks here:
// a POSIX shared-memory segment for the host side (barrier, votes, halo list sizes, the IPC handle) and ONE device allocation of rank 0
// that every member maps through hipIpcOpenMemHandle (the ARENA: the slot regions and exchange buffer of the cross-rank persistent tCG,
// and one staging slab per rank for the collectives: a member copies its contribution into its slab, the others read it there).  The
// collectives, the lock-step driver and the cross-rank persistent tCG above them are the code of the in-process group, call for call.
#define IPC_MAGIC 0x4d53445049504331ULL   // "MSDPIPC1": written by rank 0 when the cleared segment is ready
struct IpcShared {
    std::atomic<unsigned long long> magic;
    std::atomic<int> arrived; std::atomic<unsigned long long> gen; std::atomic<int> broken;
    std::atomic<int> attached; std::atomic<int> arena_ready;
    hipIpcMemHandle_t arena;
    unsigned long long arena_bytes, stage_bytes, rows_doubles, slot_bytes;
    hipIpcMemHandle_t rows_handle[LOCAL_MAX_RANKS];          // every member's exchange buffer (its own allocation, on its own device)
    hipIpcMemHandle_t blk_handle[LOCAL_MAX_RANKS];           // every member's two-level synchronisation block (msdp_psync.h psync2; round 6)
    char devid[LOCAL_MAX_RANKS][32];                         // the PCI bus id of every member's device
    int vote[LOCAL_MAX_RANKS];
    int plan[LOCAL_MAX_RANKS][4];
    int halo_off[LOCAL_MAX_RANKS][LOCAL_MAX_RANKS], halo_cnt[LOCAL_MAX_RANKS][LOCAL_MAX_RANKS];
};
struct LocalGroup {
    // members in other processes (msdp_comm_init_ipc): the host segment, the arena as this process maps it, this member's rank
    bool ipc = false;
    IpcShared* shm = nullptr;
    std::string shm_name;
    char* arena = nullptr;
    char* stage = nullptr;         // arena + slots + exchange buffer: n slabs of stage_bytes
    size_t stage_bytes = 0;
    int my_rank = 0;
    int ipc_ew = 0;                // the ELL width the members agreed on for the running call (0: CSR form)
    int n = 0;
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0;
    unsigned long long gen = 0;
    bool broken = false;
    const double* ptr[LOCAL_MAX_RANKS] = {nullptr};
    const Halo* halo[LOCAL_MAX_RANKS] = {nullptr};
    int members = 0;
    int vote[LOCAL_MAX_RANKS] = {0};
    // cross-rank persistent tCG (msdp_persist.hip XR): what the members' launches share -- two slot regions of the grid
    // synchronisation, the error word (fine-grained device memory); the exchange buffers: xr_rows below
    unsigned long long* xr_slots = nullptr;
    int* xr_err = nullptr;
    // the combined launch (member 0 issues it for everybody): every member's Dev and plan, the events that order it behind the
    // members' streams and the members' streams behind it
    Dev xr_dev[LOCAL_MAX_RANKS];
    int xr_plan[3 * LOCAL_MAX_RANKS] = {0};
    hipEvent_t xr_ready[LOCAL_MAX_RANKS] = {nullptr};
    hipEvent_t xr_done = nullptr;
    // the members' exchange buffers of the cross-rank kernels: xr_rows[q] = member q's rows (in-process: all in this address space;
    // process group: this process's own allocation for q = my_rank, the IPC mappings of the others'), xr_rows_doubles each
    double* xr_rows[LOCAL_MAX_RANKS] = {nullptr};
    size_t xr_rows_doubles = 0;
    int xr_halo_max = 0;          // halo slots behind a member's rows in every buffer (the largest halo of the group)
    // two-level reductions (process group): the members' blocks as this process maps them (mine: my own allocation), the device copy of
    // that table
    unsigned long long* xr2_blk[LOCAL_MAX_RANKS] = {nullptr};
    unsigned long long** xr2_table = nullptr;
};
static std::mutex g_groups_mutex;
static std::map<int, LocalGroup*> g_groups;
// false: a member did not arrive within the time limit (it failed or never made the matching call) -- the group is broken and
// every later collective fails at once instead of hanging the process.  The limit is 120 s unless MSDP_LOCAL_BARRIER_TIMEOUT
// (seconds) says otherwise: eight replicated 60000-step verification runs sharing one loaded GPU are legitimately slow.
static double local_barrier_timeout() {
    static const double t = [] {
        const char* e = getenv("MSDP_LOCAL_BARRIER_TIMEOUT");
        const double v = e ? atof(e) : 0.0;
        return v > 0.0 ? v : 120.0;
    }();
    return t;
}
// a member that fails between two barriers marks the group broken at once, so that its peers do not wait out the time limit
static void local_break(LocalGroup* g) {
    if (!g) return;
    if (g->ipc) { g->shm->broken.store(1); return; }
    std::lock_guard<std::mutex> lk(g->m);
    g->broken = true;
    g->cv.notify_all();
}
static bool local_barrier(LocalGroup* g) {
    if (g->ipc) {
        // sense-reversing barrier on the shared segment; polite polling (a collective on this path lasts tens of microseconds at least)
        IpcShared* sh = g->shm;
        if (sh->broken.load()) return false;
        const unsigned long long my = sh->gen.load();
        if (sh->arrived.fetch_add(1) + 1 == g->n) { sh->arrived.store(0); sh->gen.fetch_add(1); return true; }
        const auto t0 = std::chrono::steady_clock::now();
        long spins = 0;
        while (sh->gen.load() == my) {
            if (sh->broken.load()) return false;
            if (++spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(20));
            if ((spins & 1023) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > local_barrier_timeout()) { sh->broken.store(1); return false; }
        }
        return true;
    }
    std::unique_lock<std::mutex> lk(g->m);
    if (g->broken) return false;
    const unsigned long long my = g->gen;
    if (++g->arrived == g->n) { g->arrived = 0; ++g->gen; g->cv.notify_all(); return true; }
    if (!g->cv.wait_for(lk, std::chrono::duration<double>(local_barrier_timeout()), [&] { return g->gen != my || g->broken; }) || g->broken) {
        g->broken = true;
        g->cv.notify_all();
        return false;
    }
    return true;
}
#define LOCAL_BARRIER(g) do { if (!local_barrier(g)) { msdp_set_error("in-process communicator: a member did not reach the collective (group broken)"); return MSDP_ECOMM; } } while (0)
// minimum of one int per member (an agreement: every member takes the branch only if all of them can)
int msdp_local_vote_min(msdp_handle h, int v, int* out) {
    LocalGroup* g = h->lgroup;
    if (g->ipc) g->shm->vote[h->rank] = v;
    else { std::lock_guard<std::mutex> lk(g->m); g->vote[h->rank] = v; }
    LOCAL_BARRIER(g);
    int m = v;
    for (int r = 0; r < g->n; ++r) m = std::min(m, g->ipc ? g->shm->vote[r] : g->vote[r]);
    LOCAL_BARRIER(g);                                      // nobody overwrites its vote before everyone has read it
    *out = m;
    return 0;
}
// The shared block of the group: allocated by member 0 the first time (and again when the factor outgrows the exchange buffer)
static int xr_ensure_shared(msdp_handle h) {
    LocalGroup* g = h->lgroup;
    size_t need = (g->ipc ? 4 : 1) * ((size_t)msdp_rows_capacity(h) + (size_t)(g->ipc ? g->xr_halo_max : h->xr_halo_rows)) * (size_t)std::max(h->ldcap, 64);   // per member: its rows + halo slots (process group: four regions)
    if (g->ipc) {                                            // the buffers were cut at msdp_comm_init_ipc
        if (g->xr_rows_doubles < need) { msdp_set_error("cross-rank persistent tCG: the factor outgrew the exchange buffers of this communicator (ld %d)", h->ldcap); return MSDP_ENOMEM; }
        return 0;
    }
    // the members agree on the LARGEST halo and the largest need (member 0's alone decided, a member with a wider
    // factor failed)
    {
        int m = 0;
        int rcv = msdp_local_vote_min(h, -h->xr_halo_rows, &m);
        if (rcv) return rcv;
        const int hmax = -m;
        need = ((size_t)msdp_rows_capacity(h) + (size_t)hmax) * (size_t)std::max(h->ldcap, 64);
        if ((rcv = msdp_local_vote_min(h, -(int)((need + 1023) / 1024), &m))) return rcv;
        need = (size_t)(-m) * 1024;
        if (h->rank == 0) g->xr_halo_max = hmax;
    }
    int rc = 0;
    if (h->rank == 0 && (!g->xr_slots || g->xr_rows_doubles < need)) {
        if (!g->xr_slots) {
            g->xr_slots = (unsigned long long*)msdp_uc_alloc(msdp_xpersist_slot_bytes() + 256);
            if (g->xr_slots) {
                g->xr_err = (int*)((char*)g->xr_slots + msdp_xpersist_slot_bytes());
                if (hipMemset(g->xr_err, 0, 256) != hipSuccess) rc = MSDP_EHIP;
                if (hipEventCreateWithFlags(&g->xr_done, hipEventDisableTiming) != hipSuccess) rc = MSDP_EHIP;
            }
        }
        g->xr_rows_doubles = 0;
        for (int q = 0; q < g->n; ++q) {
            if (g->xr_rows[q]) { if (!msdp_uc_free(g->xr_rows[q])) (void)hipFree(g->xr_rows[q]); g->xr_rows[q] = nullptr; }
            g->xr_rows[q] = (double*)msdp_uc_alloc(need * sizeof(double));
            if (!g->xr_rows[q]) { rc = MSDP_ENOMEM; break; }
            if (hipMemset(g->xr_rows[q], 0, need * sizeof(double)) != hipSuccess) rc = MSDP_EHIP;
        }
        if (!rc) g->xr_rows_doubles = need;
        if (!g->xr_slots) rc = MSDP_ENOMEM;
    }
    LOCAL_BARRIER(g);
    if (!g->xr_slots || g->xr_rows_doubles < need) { msdp_set_error("cross-rank persistent tCG: shared buffers unavailable"); return rc ? rc : MSDP_ENOMEM; }
    return 0;
}
// Start of a trustregions() call on the cross-rank path: member 0 clears both slot regions and the error word; nobody goes on before
int msdp_xr_begin(msdp_handle h, bool* use) {
    LocalGroup* g = h->lgroup;
    *use = false;
    int rc = xr_ensure_shared(h);
    if (rc) return rc;
    if (!h->xr_ev) HIPCHK(hipEventCreateWithFlags(&h->xr_ev, hipEventDisableTiming));
    *use = true;
    if (g->ipc) {
        // the plan of the call: lanes per row and row slots must agree, a differing ELL width sends everybody to the CSR form
        Dev dv; int pl[3];
        if ((rc = msdp_xpersist_member(h, h->nranks, h->rank, g->xr_rows, g->xr_halo_max, &dv, pl))) { local_break(g); return rc; }
        for (int q = 0; q < 3; ++q) g->shm->plan[h->rank][q] = pl[q];
        LOCAL_BARRIER(g);
        g->ipc_ew = pl[1];
        for (int r = 0; r < g->n; ++r) {
            if (g->shm->plan[r][0] != pl[0] || g->shm->plan[r][2] != pl[2]) { msdp_set_error("cross-rank persistent tCG: the members' plans differ"); local_break(g); return MSDP_ESTATE; }
            if (g->shm->plan[r][1] != pl[1]) g->ipc_ew = 0;
        }
    }
    if (h->rank == 0) {
        if ((rc = msdp_xpersist_reset(h->stream, g->xr_slots, g->xr_err))) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (g->ipc && h->xr2_blk) {
        // two-level form: every member clears ITS block (slots, member lines, error word); nobody posts before everybody has
        if ((rc = msdp_xr2_reset(h->stream, h->xr2_blk))) { local_break(g); return rc; }
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    LOCAL_BARRIER(g);
    return 0;
}
static int* xr2_err(msdp_handle h) { return reinterpret_cast<int*>(reinterpret_cast<char*>(h->xr2_blk) + msdp_xr2_err_offset()); }
// One tCG for all members: each hands its Dev and plan to the group and marks its stream; member 0 makes its stream wait for
// the others', launches the combined kernel and marks its end; the others' streams wait for that mark.
int msdp_xr_launch(msdp_handle h) {
    LocalGroup* g = h->lgroup;
    int rc;
    if (g->ipc) {
        // members in different processes: every member launches ITS workgroups itself (separate processes have separate hardware
        // queues; the launches meet in the first grid synchronisation, a bounded spin turns a member that never comes into MSDP_ECOMM).
        // The members agreed on the plan in msdp_xr_begin: no host exchange per launch.
        Dev dv; int pl[3];
        if ((rc = msdp_xpersist_member(h, h->nranks, h->rank, g->xr_rows, g->xr_halo_max, &dv, pl))) { local_break(g); return rc; }
        pl[1] = g->ipc_ew;
        if (h->tune.fail_xr) { h->tune.fail_xr = 0; dv.xr_gtot += 8; dv.xr2_skip = 8; }
        if ((rc = msdp_launch_tcg_xpersist_one(h->stream, dv, pl, g->xr_slots, dv.xr2_on ? xr2_err(h) : g->xr_err))) { local_break(g); return rc; }
        return 0;
    }
    {
        Dev dv; int pl[3];
        if ((rc = msdp_xpersist_member(h, h->nranks, h->rank, g->xr_rows, g->xr_halo_max, &dv, pl))) { local_break(g); return rc; }
        HIPCHK(hipEventRecord(h->xr_ev, h->stream));
        std::lock_guard<std::mutex> lk(g->m);
        g->xr_dev[h->rank] = dv;
        for (int q = 0; q < 3; ++q) g->xr_plan[3 * h->rank + q] = pl[q];
        g->xr_ready[h->rank] = h->xr_ev;
    }
    LOCAL_BARRIER(g);
    if (h->rank == 0) {
        for (int q = 1; q < g->n; ++q) HIPCHK(hipStreamWaitEvent(h->stream, g->xr_ready[q], 0));
        if (h->tune.fail_xr) {                                 // test hook: the workgroups wait for eight more than exist -> bounded spin -> error word
            h->tune.fail_xr = 0;
            for (int q = 0; q < g->n; ++q) g->xr_dev[q].xr_gtot += 8;
        }
        if ((rc = msdp_launch_tcg_xpersist_all(h->stream, g->n, g->xr_dev, g->xr_plan, g->xr_slots, g->xr_err))) { local_break(g); return rc; }
        HIPCHK(hipEventRecord(g->xr_done, h->stream));
    }
    LOCAL_BARRIER(g);
    if (h->rank != 0) HIPCHK(hipStreamWaitEvent(h->stream, g->xr_done, 0));
    return 0;
}
int msdp_xr_tail(msdp_handle h) {
    LocalGroup* g = h->lgroup;
    Dev dv; int pl[3];
    int rc = msdp_xpersist_member(h, h->nranks, h->rank, g->xr_rows, g->xr_halo_max, &dv, pl);
    if (!rc) rc = msdp_launch_tr_tail_xr(h->stream, dv, g->xr_slots, dv.xr2_on ? xr2_err(h) : g->xr_err);
    if (rc) local_break(g);
    return rc;
}
int msdp_xr_check(msdp_handle h) {
    int e = 0;
    HIPCHK(msdp_memcpy(&e, h->lgroup->xr_err, sizeof(int), hipMemcpyDeviceToHost));
    if (!e && h->xr2_blk) HIPCHK(msdp_memcpy(&e, xr2_err(h), sizeof(int), hipMemcpyDeviceToHost));    // (the two-level form's word lives in the member's own block)
    if (e) {
        msdp_set_error("cross-rank persistent tCG: a grid synchronisation timed out (a member's launch did not arrive or the workgroups were not co-resident)");
        local_break(h->lgroup);                              // the other members' host-side collectives fail at once instead of waiting for this one
        return MSDP_ECOMM;
    }
    return 0;
}
struct LocalPtrs { const double* p[LOCAL_MAX_RANKS]; };
__global__ void k_local_sum(LocalPtrs src, int n, size_t count, double* __restrict__ out) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        double acc = 0.0;
        for (int r = 0; r < n; ++r) acc += src.p[r][i];
        out[i] = acc;
    }
}
// A member's contribution to a collective: in one process the others read it where it lies; across processes it is copied into the
// member's staging slab of the arena first (the caller has synchronised its stream: the source is complete)
static int group_publish(msdp_handle h, const double* buf, size_t count) {
    LocalGroup* g = h->lgroup;
    if (!g->ipc) { std::lock_guard<std::mutex> lk(g->m); g->ptr[h->rank] = buf; return 0; }
    if (count * sizeof(double) > g->stage_bytes) { msdp_set_error("inter-process communicator: a contribution of %zu bytes exceeds the staging slab (%zu)", count * sizeof(double), g->stage_bytes); local_break(g); return MSDP_ENOMEM; }
    HIPCHK(msdp_memcpy_async(g->stage + (size_t)h->rank * g->stage_bytes, buf, count * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
static const double* group_peer(LocalGroup* g, int r) { return g->ipc ? (const double*)(g->stage + (size_t)r * g->stage_bytes) : g->ptr[r]; }
static int local_allreduce(msdp_handle h, double* buf, size_t count) {
    LocalGroup* g = h->lgroup;
    if (h->lc_tmp_cap < count) {
        if (h->lc_tmp) (void)hipFree(h->lc_tmp);
        h->lc_tmp = nullptr; h->lc_tmp_cap = 0;
        if (hipMalloc((void**)&h->lc_tmp, count * sizeof(double)) != hipSuccess) { msdp_set_error("local all-reduce: scratch allocation failed"); return MSDP_ENOMEM; }
        h->lc_tmp_cap = count;
    }
    HIPCHK(hipStreamSynchronize(h->stream));               // my contribution is complete
    { int rcp = group_publish(h, buf, count); if (rcp) return rcp; }
    LOCAL_BARRIER(g);
    LocalPtrs src;
    for (int r = 0; r < LOCAL_MAX_RANKS; ++r) src.p[r] = r < g->n ? group_peer(g, r) : nullptr;
    int blocks = (int)std::min<size_t>(1024, (count + 255) / 256);
    hipLaunchKernelGGL(k_local_sum, dim3(blocks), dim3(256), 0, h->stream, src, g->n, count, h->lc_tmp);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    LOCAL_BARRIER(g);                                      // every member has read every contribution
    HIPCHK(msdp_memcpy_async(buf, h->lc_tmp, count * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return 0;
}
static int local_allgather(msdp_handle h, const double* local, double* all, size_t count_per_rank) {
    LocalGroup* g = h->lgroup;
    HIPCHK(hipStreamSynchronize(h->stream));
    { int rcp = group_publish(h, local, count_per_rank); if (rcp) return rcp; }
    LOCAL_BARRIER(g);
    for (int r = 0; r < g->n; ++r)
        HIPCHK(msdp_memcpy_async(all + (size_t)r * count_per_rank, group_peer(g, r), count_per_rank * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    LOCAL_BARRIER(g);                                      // nobody overwrites its slab before everyone has copied it
    return 0;
}
// halo rows between in-process members: every member publishes its packed send buffer and its per-peer offsets
static int local_halo(msdp_handle h, Halo* ha, int ld) {
    LocalGroup* g = h->lgroup;
    HIPCHK(hipStreamSynchronize(h->stream));               // my send buffer is packed
    if (g->ipc) {
        for (int q = 0; q < g->n; ++q) { g->shm->halo_cnt[h->rank][q] = ha->send_cnt[q]; g->shm->halo_off[h->rank][q] = ha->send_off[q]; }
        int rcp = group_publish(h, ha->sendbuf, (size_t)ha->send_rows * ld); if (rcp) return rcp;
    } else { std::lock_guard<std::mutex> lk(g->m); g->ptr[h->rank] = ha->sendbuf; g->halo[h->rank] = ha; }
    LOCAL_BARRIER(g);
    for (int q = 0; q < g->n; ++q) {
        if (q == h->rank || ha->recv_cnt[q] == 0) continue;
        const int q_cnt = g->ipc ? g->shm->halo_cnt[q][h->rank] : g->halo[q]->send_cnt[h->rank];
        const int q_off = g->ipc ? g->shm->halo_off[q][h->rank] : g->halo[q]->send_off[h->rank];
        if (q_cnt != ha->recv_cnt[q]) {
            msdp_set_error("halo exchange: rank %d sends %d rows, rank %d expects %d", q, q_cnt, h->rank, ha->recv_cnt[q]);
            local_break(g);                                    // the peers learn at once, not after the barrier's time limit
            return MSDP_ECOMM;
        }
        HIPCHK(msdp_memcpy_async(ha->recvbuf + (size_t)ha->recv_off[q] * ld, group_peer(g, q) + (size_t)q_off * ld,
                              (size_t)ha->recv_cnt[q] * ld * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    LOCAL_BARRIER(g);
    return 0;
}
void msdp_local_leave(msdp_handle h) {
    if (!h->lgroup) return;
    std::lock_guard<std::mutex> lk(g_groups_mutex);
    LocalGroup* g = h->lgroup;
    h->lgroup = nullptr;
    if (g->ipc) {
        // the arena belongs to rank 0 (the mappings of the others keep its memory alive until they close them)
        if (g->arena) { if (g->my_rank == 0) (void)hipFree(g->arena); else (void)hipIpcCloseMemHandle(g->arena); }
        for (int q = 0; q < g->n; ++q) if (g->xr_rows[q]) { if (q == g->my_rank) (void)hipFree(g->xr_rows[q]); else (void)hipIpcCloseMemHandle(g->xr_rows[q]); }
        for (int q = 0; q < g->n; ++q) if (g->xr2_blk[q]) { if (q == g->my_rank) (void)hipFree(g->xr2_blk[q]); else (void)hipIpcCloseMemHandle(g->xr2_blk[q]); }
        if (g->xr2_table) (void)hipFree(g->xr2_table);
        h->xr2_blk = nullptr; h->xr2_peers = nullptr; h->lgroup_is_ipc = false;
        if (g->shm) (void)munmap((void*)g->shm, sizeof(IpcShared));
        if (g->my_rank == 0 && !g->shm_name.empty()) (void)shm_unlink(g->shm_name.c_str());
        delete g;
        return;
    }
    if (--g->members == 0) {
        for (auto it = g_groups.begin(); it != g_groups.end(); ++it) if (it->second == g) { g_groups.erase(it); break; }
        if (g->xr_slots && !msdp_uc_free(g->xr_slots)) (void)hipFree(g->xr_slots);
        for (int q = 0; q < LOCAL_MAX_RANKS; ++q) if (g->xr_rows[q] && !msdp_uc_free(g->xr_rows[q])) (void)hipFree(g->xr_rows[q]);
        if (g->xr_done) (void)hipEventDestroy(g->xr_done);
        delete g;
    }
}
void msdp_comm_release(msdp_handle h) { if (h->comm) (void)ncclCommDestroy((ncclComm_t)h->comm); }   // msdp_destroy: the RCCL communicator
int msdp_local_barrier(msdp_handle h) { LOCAL_BARRIER(h->lgroup); return 0; }                           // for the callers that do not see LocalGroup

// ------------------------------------------------------------------ Halo exchange (sparse C)
// The all-gather of the n x p direction moves (N-1)/N * n*p*8 bytes into every rank before every S*U -- for the G81 family
// on eight ranks 35 MB per trip where the rows of C a rank owns reference 400 rows of other ranks (100 KB).  With the option
// "halo_exchange" a rank packs, for every peer, the rows that peer's rows of C reference, one grouped ncclSend / ncclRecv
// per peer moves them, and an unpack kernel scatters the received rows to their global positions in the gather buffer, which
// the S*U kernels read exactly as after an all-gather.  Every rank holds the whole CSR structure on the host, so all send /
// receive lists are computed locally and agree by construction.  Only for sparse C and only for the two exchanges in front
// of the cost/gradient and Hess-vec kernels; msdp_get_point_all and the replicated escape keep the all-gather (they need
// every row).
__global__ void k_halo_pack(int rows, int ld, const int* __restrict__ idx, const double* __restrict__ local, double* __restrict__ buf) {
    const int64_t tot = (int64_t)rows * ld;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = e / ld; const int c = (int)(e - k * ld);
        buf[e] = local[(int64_t)idx[k] * ld + c];
    }
}
__global__ void k_halo_unpack(int rows, int ld, const int* __restrict__ idx, const double* __restrict__ buf, double* __restrict__ full) {
    const int64_t tot = (int64_t)rows * ld;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = e / ld; const int c = (int)(e - k * ld);
        full[(int64_t)idx[k] * ld + c] = buf[e];
    }
}
void msdp_halo_release(msdp_handle h) {
    Halo* ha = h->halo;
    if (!ha) return;
    if (ha->send_idx) (void)hipFree(ha->send_idx);
    if (ha->recv_idx) (void)hipFree(ha->recv_idx);
    if (ha->sendbuf) (void)hipFree(ha->sendbuf);
    if (ha->recvbuf) (void)hipFree(ha->recvbuf);
    if (ha->xr_colind) (void)hipFree(ha->xr_colind);
    if (ha->xr_ellc) (void)hipFree(ha->xr_ellc);
    if (ha->xr_pq) (void)hipFree(ha->xr_pq);
    if (ha->xr_pidx) (void)hipFree(ha->xr_pidx);
    delete ha;
    h->halo = nullptr;
    h->d.xr_colind = h->d.xr_ellc = h->d.xr_pq = h->d.xr_pidx = nullptr; h->xr_ok = false; h->xr_halo_rows = 0;
    h->xr_paddr_pq = nullptr; h->d.xr_paddr = nullptr;   // (the push addresses are rebuilt from the next partition's lists)
}
// Lists for the current partition (called by comm_partition for sparse C); buffers follow the vectors' capacity
static int halo_setup(msdp_handle h) {
    msdp_halo_release(h);
    if (h->d.costkind != COST_SPARSE || h->h_rowptr.empty() || h->nranks < 2) return 0;
    const int N = h->nranks, n = h->d.n, cap = msdp_rows_capacity(h), me = h->rank;
    Halo* ha = new Halo();
    ha->N = N;
    ha->send_cnt.assign(N, 0); ha->send_off.assign(N + 1, 0); ha->recv_cnt.assign(N, 0); ha->recv_off.assign(N + 1, 0);
    // needs[q]: rows outside q's range that q's rows of C reference (sorted, unique)
    std::vector<std::vector<int>> send_rows(N);          // what I send to q (local indices), in the order q will unpack
    std::vector<int> recv_rows;
    std::vector<char> mark((size_t)n, 0);
    const int my0 = std::min(n, me * cap), my1 = std::min(n, my0 + cap), nloc = my1 - my0;
    std::vector<int> pq((size_t)2 * std::max(nloc, 1), -1), pidx((size_t)2 * std::max(nloc, 1), 0);
    bool push_ok = true;
    for (int q = 0; q < N; ++q) {
        const int q0 = std::min(n, q * cap), q1 = std::min(n, q0 + cap);
        std::vector<int> need;
        for (int i = q0; i < q1; ++i)
            for (int t = h->h_rowptr[i]; t < h->h_rowptr[i + 1]; ++t) {
                const int c = h->h_colind[t];
                if ((c < q0 || c >= q1) && !mark[c]) { mark[c] = 1; need.push_back(c); }
            }
        std::sort(need.begin(), need.end());
        for (int c : need) mark[c] = 0;
        if (q == me) {
            recv_rows = need;                            // sorted by global row = grouped by owning peer
            for (int c : need) ha->recv_cnt[c / cap]++;
        } else {
            const int m0 = std::min(n, me * cap), m1 = std::min(n, m0 + cap);
            for (int c : need) if (c >= m0 && c < m1) send_rows[q].push_back(c - m0);
            ha->send_cnt[q] = (int)send_rows[q].size();
            // push exchange: my row c sits at position cap + (index of c in q's sorted need list) of q's buffer
            for (size_t k = 0; k < need.size(); ++k) {
                const int c = need[k];
                if (c < m0 || c >= m1) continue;
                const int i = c - m0;
                if (pq[i] < 0) { pq[i] = q; pidx[i] = cap + (int)k; }
                else if (pq[(size_t)nloc + i] < 0) { pq[(size_t)nloc + i] = q; pidx[(size_t)nloc + i] = cap + (int)k; }
                else push_ok = false;
            }
        }
    }
    std::vector<int> sidx;
    for (int q = 0; q < N; ++q) { ha->send_off[q + 1] = ha->send_off[q] + ha->send_cnt[q]; ha->recv_off[q + 1] = ha->recv_off[q] + ha->recv_cnt[q]; sidx.insert(sidx.end(), send_rows[q].begin(), send_rows[q].end()); }
    ha->send_rows = ha->send_off[N]; ha->recv_rows = ha->recv_off[N];
    ha->ldcap = h->ldcap > 0 ? h->ldcap : ((h->pcap + 1) / 2) * 2;
    auto upi = [&](const std::vector<int>& v, int** out) -> int {
        if (hipMalloc((void**)out, (v.size() ? v.size() : 1) * sizeof(int)) != hipSuccess) return MSDP_ENOMEM;
        if (!v.empty() && msdp_memcpy(*out, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return MSDP_EHIP;
        return 0;
    };
    int rc = upi(sidx, &ha->send_idx);
    if (!rc) rc = upi(recv_rows, &ha->recv_idx);
    // push exchange: buffer-local column indices of my rows (CSR and ELL copies), push targets
    if (!rc) {
        std::vector<int> gmap((size_t)n, -1);
        for (int c = my0; c < my1; ++c) gmap[c] = c - my0;
        for (size_t k = 0; k < recv_rows.size(); ++k) gmap[recv_rows[k]] = cap + (int)k;
        const int base = nloc > 0 ? h->h_rowptr[my0] : 0, nnzl = nloc > 0 ? h->h_rowptr[my1] - base : 0;
        std::vector<int> xcol((size_t)std::max(nnzl, 1), 0);
        for (int t = 0; t < nnzl; ++t) xcol[t] = gmap[h->h_colind[base + t]];
        rc = upi(xcol, &ha->xr_colind);
        if (!rc && h->d.ellW > 0) {
            const int W = h->d.ellW;
            std::vector<int> ec((size_t)W * cap);
            for (int w = 0; w < W; ++w) for (int i = 0; i < cap; ++i) ec[(size_t)w * cap + i] = std::min(i, nloc > 0 ? nloc - 1 : 0);    // padding: (own row, 0.0)
            for (int i = 0; i < nloc; ++i)
                for (int t = h->h_rowptr[my0 + i]; t < h->h_rowptr[my0 + i + 1] && t - h->h_rowptr[my0 + i] < W; ++t)
                    ec[(size_t)(t - h->h_rowptr[my0 + i]) * cap + i] = gmap[h->h_colind[t]];
            rc = upi(ec, &ha->xr_ellc);
        }
        if (!rc) rc = upi(pq, &ha->xr_pq);
        if (!rc) rc = upi(pidx, &ha->xr_pidx);
        ha->xr_ok = push_ok && !rc;
        h->d.xr_colind = ha->xr_colind; h->d.xr_ellc = ha->xr_ellc; h->d.xr_pq = ha->xr_pq; h->d.xr_pidx = ha->xr_pidx;
        h->xr_ok = ha->xr_ok; h->xr_halo_rows = (int)recv_rows.size();
    }
    if (!rc && hipMalloc((void**)&ha->sendbuf, (size_t)std::max(ha->send_rows, 1) * ha->ldcap * sizeof(double)) != hipSuccess) rc = MSDP_ENOMEM;
    if (!rc && hipMalloc((void**)&ha->recvbuf, (size_t)std::max(ha->recv_rows, 1) * ha->ldcap * sizeof(double)) != hipSuccess) rc = MSDP_ENOMEM;
    h->halo = ha;
    if (rc) { msdp_set_error("halo exchange: set-up allocation failed"); msdp_halo_release(h); }
    return rc;
}
// rows of `local` the other ranks reference -> their gather buffers; mine + what I reference -> my gather buffer
static int halo_exchange(msdp_handle h, const double* local_rows, bool with_sums = false) {
    Halo* ha = h->halo;
    const int ld = h->d.ld;
    ++h->coll_calls;
    if (ld > ha->ldcap) {                                  // the vectors were re-allocated for a wider factor: follow
        const int cap = h->ldcap;
        if (ha->sendbuf) (void)hipFree(ha->sendbuf);
        if (ha->recvbuf) (void)hipFree(ha->recvbuf);
        ha->sendbuf = ha->recvbuf = nullptr;
        if (hipMalloc((void**)&ha->sendbuf, (size_t)std::max(ha->send_rows, 1) * cap * sizeof(double)) != hipSuccess ||
            hipMalloc((void**)&ha->recvbuf, (size_t)std::max(ha->recv_rows, 1) * cap * sizeof(double)) != hipSuccess) { msdp_set_error("halo exchange: buffer allocation failed"); return MSDP_ENOMEM; }
        ha->ldcap = cap;
    }
    h->d.full = h->full_buf;
    const size_t own = (size_t)msdp_rows_capacity(h) * ld;
    HIPCHK(msdp_memcpy_async(h->full_buf + (size_t)h->rank * own, local_rows, own * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (ha->send_rows > 0) {
        const int64_t tot = (int64_t)ha->send_rows * ld;
        hipLaunchKernelGGL(k_halo_pack, dim3((int)std::min<int64_t>(1024, (tot + 255) / 256)), dim3(256), 0, h->stream, ha->send_rows, ld,
                           (const int*)ha->send_idx, local_rows, ha->sendbuf);
        HIPCHK(hipGetLastError());
    }
    if (h->lgroup) { int rc = local_halo(h, ha, ld); if (rc) return rc; }
    else {
        // with_sums (msdp_trip1.hip): every pair of ranks also swaps its four sums in the same group
        if (with_sums) HIPCHK(msdp_memcpy_async(h->d.xs_all + 4 * (size_t)h->rank, h->d.xs, 4 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        ncclResult_t r = ncclGroupStart();
        for (int q = 0; q < ha->N && r == ncclSuccess; ++q) {
            if (q == h->rank) continue;
            if (ha->send_cnt[q] > 0) r = ncclSend(ha->sendbuf + (size_t)ha->send_off[q] * ld, (size_t)ha->send_cnt[q] * ld, ncclDouble, q, (ncclComm_t)h->comm, h->stream);
            if (r == ncclSuccess && ha->recv_cnt[q] > 0) r = ncclRecv(ha->recvbuf + (size_t)ha->recv_off[q] * ld, (size_t)ha->recv_cnt[q] * ld, ncclDouble, q, (ncclComm_t)h->comm, h->stream);
            if (with_sums && r == ncclSuccess) r = ncclSend(h->d.xs, 4, ncclDouble, q, (ncclComm_t)h->comm, h->stream);
            if (with_sums && r == ncclSuccess) r = ncclRecv(h->d.xs_all + 4 * (size_t)q, 4, ncclDouble, q, (ncclComm_t)h->comm, h->stream);
        }
        ncclResult_t r2 = ncclGroupEnd();
        if (r != ncclSuccess || r2 != ncclSuccess) { msdp_set_error("halo exchange: ncclSend/ncclRecv failed: %s", ncclGetErrorString(r != ncclSuccess ? r : r2)); return MSDP_ECOMM; }
    }
    if (ha->recv_rows > 0) {
        const int64_t tot = (int64_t)ha->recv_rows * ld;
        hipLaunchKernelGGL(k_halo_unpack, dim3((int)std::min<int64_t>(1024, (tot + 255) / 256)), dim3(256), 0, h->stream, ha->recv_rows, ld,
                           (const int*)ha->recv_idx, (const double*)ha->recvbuf, h->full_buf);
        HIPCHK(hipGetLastError());
    }
    return 0;
}
extern "C" int msdp_debug_p2p_self(msdp_handle h, int64_t count, const double* in_host, double* out_host) {
    if (!h || !h->use_comm || h->lgroup || !h->comm || count <= 0) { msdp_set_error("debug_p2p_self: needs an RCCL communicator"); return MSDP_ESTATE; }
    double *a = nullptr, *b = nullptr;
    if (hipMalloc((void**)&a, count * sizeof(double)) != hipSuccess || hipMalloc((void**)&b, count * sizeof(double)) != hipSuccess) {
        if (a) (void)hipFree(a);
        msdp_set_error("debug_p2p_self: allocation failed"); return MSDP_ENOMEM;
    }
    int rc = 0;
    if (msdp_memcpy_async(a, in_host, count * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess) rc = MSDP_EHIP;
    if (!rc) {
        ncclResult_t r = ncclGroupStart();
        if (r == ncclSuccess) r = ncclSend(a, (size_t)count, ncclDouble, h->rank, (ncclComm_t)h->comm, h->stream);
        if (r == ncclSuccess) r = ncclRecv(b, (size_t)count, ncclDouble, h->rank, (ncclComm_t)h->comm, h->stream);
        ncclResult_t r2 = ncclGroupEnd();
        if (r != ncclSuccess || r2 != ncclSuccess) { msdp_set_error("debug_p2p_self: %s", ncclGetErrorString(r != ncclSuccess ? r : r2)); rc = MSDP_ECOMM; }
    }
    if (!rc && msdp_memcpy_async(out_host, b, count * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc = MSDP_EHIP;
    if (hipStreamSynchronize(h->stream) != hipSuccess && !rc) rc = MSDP_EHIP;
    (void)hipFree(a); (void)hipFree(b);
    return rc;
}

int msdp_exchange_rows(msdp_handle h, const double* local_rows) {
    if (h->use_comm && h->halo && h->tune.halo_exchange && h->nranks > 1) return halo_exchange(h, local_rows);
    return msdp_allgather_rows(h, local_rows);
}

// The exchange of msdp_trip1.hip: the rows as above AND d.xs (4 doubles) of every rank into d.xs_all, in ONE grouped
// collective call -- RCCL fuses the operations between ncclGroupStart / ncclGroupEnd into one launch.
int msdp_exchange_rows_sums(msdp_handle h, const double* local_rows) {
    Dev& d = h->d;
    if (!h->use_comm) {                                   // one rank, no communicator: the kernels read the rows and the sums in place
        if (h->nranks != 1) { msdp_set_error("exchange_rows_sums: no communicator"); return MSDP_ESTATE; }
        d.full = const_cast<double*>(local_rows);
        d.xs_all = d.xs;
        return 0;
    }
    const bool halo = h->halo && h->tune.halo_exchange && h->nranks > 1;
    if (h->lgroup) {
        // in-process stand-in: the two parts one after the other, counted as the one call they are under RCCL
        int rc = halo ? halo_exchange(h, local_rows) : msdp_allgather_rows(h, local_rows);      // (counted there)
        if (!rc) rc = local_allgather(h, d.xs, d.xs_all, 4);
        return rc;
    }
    if (halo) return halo_exchange(h, local_rows, true);
    ++h->coll_calls;
    const size_t cnt = (size_t)msdp_rows_capacity(h) * d.ld;
    d.full = h->full_buf;
    ncclResult_t r = ncclGroupStart();
    if (r == ncclSuccess) r = ncclAllGather(local_rows, h->full_buf, cnt, ncclDouble, (ncclComm_t)h->comm, h->stream);
    if (r == ncclSuccess) r = ncclAllGather(d.xs, d.xs_all, 4, ncclDouble, (ncclComm_t)h->comm, h->stream);
    ncclResult_t r2 = ncclGroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess) { msdp_set_error("grouped ncclAllGather failed: %s", ncclGetErrorString(r != ncclSuccess ? r : r2)); return MSDP_ECOMM; }
    return 0;
}

// ------------------------------------------------------------------ collectives
int msdp_allreduce_partials(msdp_handle h, int first, int count) {
    if (!h->use_comm) return 0;
    ++h->coll_calls;
    if (h->lgroup) return local_allreduce(h, h->d.P + (size_t)first * MSDP_MAX_GRID, (size_t)count * MSDP_MAX_GRID);
    double* buf = h->d.P + (size_t)first * MSDP_MAX_GRID;
    ncclResult_t r = ncclAllReduce(buf, buf, (size_t)count * MSDP_MAX_GRID, ncclDouble, ncclSum,
                                   (ncclComm_t)h->comm, h->stream);
    if (r != ncclSuccess) { msdp_set_error("ncclAllReduce failed: %s", ncclGetErrorString(r)); return MSDP_ECOMM; }
    return 0;
}

// Make all rows of a row-sharded vector visible to the gather kernels: one RCCL
// all-gather of the thin n x p factor (each rank sends its slab to its 7 peers,
// one message per xGMI link).  With one rank the local buffer is used directly.
int msdp_allgather_rows(msdp_handle h, const double* local_rows) {
    if (!h->use_comm) {
        if (h->nranks > 1) {        // a lone process standing in for one shard (tests / per-shard measurement)
            const size_t cnt1 = (size_t)msdp_rows_capacity(h) * h->d.ld;
            HIPCHK(msdp_memcpy_async(h->full_buf + (size_t)h->rank * cnt1, local_rows, cnt1 * sizeof(double),
                                  hipMemcpyDeviceToDevice, h->stream));
            h->d.full = h->full_buf;
            return 0;
        }
        h->d.full = const_cast<double*>(local_rows);
        return 0;
    }
    const size_t cnt = (size_t)msdp_rows_capacity(h) * h->d.ld;
    // slabs are packed with the CURRENT ld so the full buffer is n_pad x ld row-major
    h->d.full = h->full_buf;
    ++h->coll_calls;
    if (h->lgroup) return local_allgather(h, local_rows, h->full_buf, cnt);
    ncclResult_t r = ncclAllGather(local_rows, h->full_buf, cnt, ncclDouble, (ncclComm_t)h->comm, h->stream);
    if (r != ncclSuccess) { msdp_set_error("ncclAllGather failed: %s", ncclGetErrorString(r)); return MSDP_ECOMM; }
    return 0;
}

// sum of a device array over the ranks, in place (not counted in coll_calls: msdp_factor_gram runs outside the solve)
int msdp_allreduce_array(msdp_handle h, double* buf, size_t count) {
    if (h->lgroup) return local_allreduce(h, buf, count);
    ncclResult_t r = ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, (ncclComm_t)h->comm, h->stream);
    if (r != ncclSuccess) { msdp_set_error("ncclAllReduce failed: %s", ncclGetErrorString(r)); return MSDP_ECOMM; }
    return 0;
}

// count_per_rank doubles from every rank, in rank order
int msdp_allgather_vec(msdp_handle h, const double* local, double* all, size_t count_per_rank) {
    if (!h->use_comm) { msdp_set_error("allgather_vec: no communicator"); return MSDP_ESTATE; }
    ++h->coll_calls;
    if (h->lgroup) return local_allgather(h, local, all, count_per_rank);
    ncclResult_t r = ncclAllGather(local, all, count_per_rank, ncclDouble, (ncclComm_t)h->comm, h->stream);
    if (r != ncclSuccess) { msdp_set_error("ncclAllGather failed: %s", ncclGetErrorString(r)); return MSDP_ECOMM; }
    return 0;
}

extern "C" int msdp_comm_unique_id(void* id128) {
    if (!id128) return MSDP_EINVAL;
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) { msdp_set_error("ncclGetUniqueId failed: %s", ncclGetErrorString(r)); return MSDP_ECOMM; }
    static_assert(sizeof(ncclUniqueId) == 128, "RCCL unique id is 128 bytes");
    memcpy(id128, &id, 128);
    return 0;
}

static int comm_partition(msdp_handle h, int32_t nranks, int32_t rank);

// Test / diagnostic: member `rank` of the in-process group `group_id` of `nranks` handles (one process, one GPU, one host
// thread per handle).  Same partition, same code paths as msdp_comm_init; the collectives are the local stand-ins above.
extern "C" int msdp_comm_init_local(msdp_handle h, int32_t nranks, int32_t rank, int32_t group_id) {
    MSDP_CHECK_H(h);
    if (nranks < 1 || nranks > LOCAL_MAX_RANKS || rank < 0 || rank >= nranks) { msdp_set_error("comm_init_local: bad arguments"); return MSDP_EINVAL; }
    if (h->d.costkind == COST_HERM) { msdp_set_error("comm_init_local: a Hermitian handle joins no communicator (row-sharded complex factors are not implemented)"); return MSDP_EUNSUPPORTED; }
    if (h->d.costkind == COST_BLOCK) { msdp_set_error("comm_init_local: a %s handle joins no communicator (row-sharded block rows are not implemented)", msdp_block_kind_name(h->d.efree)); return MSDP_EUNSUPPORTED; }
    if (h->d.costkind == COST_SPLR) { msdp_set_error("comm_init_local: a sparse-plus-low-rank handle joins no communicator (row-sharded low-rank terms are not implemented)"); return MSDP_EUNSUPPORTED; }
    if (h->have_point || h->use_comm) { msdp_set_error("comm_init_local must precede set_point / comm_init"); return MSDP_ESTATE; }
    if (h->presharded && (nranks != h->nranks || rank != h->rank)) { msdp_set_error("comm_init_local: shard was created as rank %d of %d", h->rank, h->nranks); return MSDP_EINVAL; }
    if (h->kind == MSDP_KIND_MULTIBLOCK || msdp_dual_kind(h)) { msdp_set_error("row sharding is not implemented for the multiblock and dual kinds"); return MSDP_EUNSUPPORTED; }
    {
        std::lock_guard<std::mutex> lk(g_groups_mutex);
        LocalGroup*& g = g_groups[group_id];
        if (!g) { g = new LocalGroup(); g->n = nranks; }
        if (g->n != nranks || g->members >= nranks) { msdp_set_error("comm_init_local: group %d has %d of %d members", group_id, g->members, g->n); return MSDP_EINVAL; }
        ++g->members;
        h->lgroup = g;
    }
    return comm_partition(h, nranks, rank);
}

// Members in different processes (one per GPU of a node, or several on one GPU): `name` identifies the group (a POSIX shared-memory
// name, e.g. "/msdp_<pid of the launcher>_<counter>"; every member passes the same one).  Rank 0 allocates the arena and exports it,
// the others map it; with ranks on different devices the mapping goes over peer access (hipIpcMemLazyEnablePeerAccess).
static int comm_init_ipc_attach(msdp_handle h, int32_t nranks, int32_t rank, unsigned long long my_ino);
extern "C" int msdp_comm_init_ipc(msdp_handle h, int32_t nranks, int32_t rank, const char* name) {
    MSDP_CHECK_H(h);
    if (nranks < 1 || nranks > LOCAL_MAX_RANKS || rank < 0 || rank >= nranks || !name || name[0] != '/') { msdp_set_error("comm_init_ipc: bad arguments (the name starts with '/')"); return MSDP_EINVAL; }
    if (h->d.costkind == COST_HERM) { msdp_set_error("comm_init_ipc: a Hermitian handle joins no communicator (row-sharded complex factors are not implemented)"); return MSDP_EUNSUPPORTED; }
    if (h->d.costkind == COST_BLOCK) { msdp_set_error("comm_init_ipc: a %s handle joins no communicator (row-sharded block rows are not implemented)", msdp_block_kind_name(h->d.efree)); return MSDP_EUNSUPPORTED; }
    if (h->d.costkind == COST_SPLR) { msdp_set_error("comm_init_ipc: a sparse-plus-low-rank handle joins no communicator (row-sharded low-rank terms are not implemented)"); return MSDP_EUNSUPPORTED; }
    if (h->have_point || h->use_comm) { msdp_set_error("comm_init_ipc must precede set_point / comm_init"); return MSDP_ESTATE; }
    if (h->presharded && (nranks != h->nranks || rank != h->rank)) { msdp_set_error("comm_init_ipc: shard was created as rank %d of %d", h->rank, h->nranks); return MSDP_EINVAL; }
    if (h->kind == MSDP_KIND_MULTIBLOCK || msdp_dual_kind(h)) { msdp_set_error("row sharding is not implemented for the multiblock and dual kinds"); return MSDP_EUNSUPPORTED; }
    // The host segment: rank 0 removes whatever a crashed run left under this name, creates the segment anew (O_EXCL),
    // clears it and writes the magic word LAST; the others open it without O_CREAT, wait for the magic word and check that the name
    // still leads to the segment they mapped (a stale one that rank 0 has replaced meanwhile does not).
    void* mp = MAP_FAILED;
    unsigned long long my_ino = 0;
    if (rank == 0) {
        (void)shm_unlink(name);
        const int fd = shm_open(name, O_CREAT | O_EXCL | O_RDWR, 0600);
        if (fd < 0) { msdp_set_error("comm_init_ipc: shm_open(%s, O_EXCL) failed", name); return MSDP_ECOMM; }
        if (ftruncate(fd, (off_t)sizeof(IpcShared)) != 0) { (void)close(fd); (void)shm_unlink(name); msdp_set_error("comm_init_ipc: ftruncate failed"); return MSDP_ECOMM; }
        mp = mmap(nullptr, sizeof(IpcShared), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        (void)close(fd);
        if (mp == MAP_FAILED) { (void)shm_unlink(name); msdp_set_error("comm_init_ipc: mmap failed"); return MSDP_ECOMM; }
        memset(mp, 0, sizeof(IpcShared));
        ((IpcShared*)mp)->magic.store(IPC_MAGIC);
    } else {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const bool late = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > local_barrier_timeout();
            const int fd = shm_open(name, O_RDWR, 0600);
            struct stat st;
            if (fd >= 0 && fstat(fd, &st) == 0 && (size_t)st.st_size >= sizeof(IpcShared)) {
                void* q = mmap(nullptr, sizeof(IpcShared), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
                (void)close(fd);
                if (q != MAP_FAILED) {
                    if (((IpcShared*)q)->magic.load() == IPC_MAGIC) {
                        // the name still leads here?  (rank 0 unlinks a stale segment before it creates the group's)
                        const int fd2 = shm_open(name, O_RDWR, 0600);
                        struct stat st2;
                        const bool same = fd2 >= 0 && fstat(fd2, &st2) == 0 && st2.st_ino == st.st_ino;
                        if (fd2 >= 0) (void)close(fd2);
                        if (same) { mp = q; my_ino = (unsigned long long)st.st_ino; break; }
                    }
                    (void)munmap(q, sizeof(IpcShared));
                }
            } else if (fd >= 0) (void)close(fd);
            if (late) { msdp_set_error("comm_init_ipc: rank 0 did not create the segment %s", name); return MSDP_ECOMM; }
            std::this_thread::sleep_for(std::chrono::microseconds(500));
        }
    }
    LocalGroup* g = new LocalGroup();
    g->ipc = true; g->n = nranks; g->members = 1; g->my_rank = rank; g->shm = (IpcShared*)mp; g->shm_name = name;
    h->lgroup = g;
    int rc = comm_init_ipc_attach(h, nranks, rank, my_ino);
    if (rc) {
        // (a member that fails here tells the others, and leaves nothing behind: mapping, group record and -- rank 0 -- the name)
        local_break(g);
        msdp_local_leave(h);
    }
    return rc;
}
static int comm_init_ipc_attach(msdp_handle h, int32_t nranks, int32_t rank, unsigned long long my_ino) {
    LocalGroup* g = h->lgroup;
    const char* name = g->shm_name.c_str();
    int rc = comm_partition(h, nranks, rank);
    if (rc) return rc;
    IpcShared* sh = g->shm;
    const size_t slot_bytes = msdp_xpersist_slot_bytes() + 256;
    const size_t ldx = (size_t)std::max(h->ldcap, 64);
    // every member's own exchange buffer: its rows + a slot for every foreign row it references (the largest halo of the group: the
    // members vote below, through the segment)
    sh->vote[rank] = h->xr_halo_rows;
    const size_t stage = std::max<size_t>(((size_t)msdp_rows_capacity(h) * ldx * sizeof(double) + 255) / 256 * 256, (size_t)1 << 16);
    const size_t total = slot_bytes + (size_t)nranks * stage;
    if (rank == 0) {
        void* p = nullptr;
        if (hipExtMallocWithFlags(&p, total, hipDeviceMallocFinegrained) != hipSuccess) { (void)hipGetLastError(); msdp_set_error("comm_init_ipc: arena allocation of %zu bytes failed", total); local_break(g); return MSDP_ENOMEM; }
        HIPCHK(hipMemset(p, 0, total));
        HIPCHK(hipDeviceSynchronize());
        hipIpcMemHandle_t hd;
        if (hipIpcGetMemHandle(&hd, p) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(p); msdp_set_error("comm_init_ipc: hipIpcGetMemHandle failed"); local_break(g); return MSDP_ECOMM; }
        g->arena = (char*)p;
        sh->arena = hd; sh->arena_bytes = total; sh->stage_bytes = stage; sh->slot_bytes = slot_bytes;
        sh->arena_ready.store(1);
    } else {
        const auto t0 = std::chrono::steady_clock::now();
        while (!sh->arena_ready.load()) {
            if (sh->broken.load() || std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > local_barrier_timeout()) { msdp_set_error("comm_init_ipc: rank 0 did not publish the arena"); return MSDP_ECOMM; }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
        if (sh->arena_bytes != total || sh->stage_bytes != stage) { msdp_set_error("comm_init_ipc: the members disagree about the problem size"); local_break(g); return MSDP_EINVAL; }
        void* p = nullptr;
        hipIpcMemHandle_t hd = sh->arena;
        if (hipIpcOpenMemHandle(&p, hd, hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); msdp_set_error("comm_init_ipc: hipIpcOpenMemHandle failed"); local_break(g); return MSDP_ECOMM; }
        g->arena = (char*)p;
    }
    g->xr_slots = (unsigned long long*)g->arena;
    g->xr_err = (int*)(g->arena + msdp_xpersist_slot_bytes());
    g->stage = g->arena + slot_bytes;
    g->stage_bytes = stage;
    sh->attached.fetch_add(1);
    LOCAL_BARRIER(g);                                        // everybody has mapped the arena; the halo sizes are in the segment
    if (rank != 0) {
        // (once more behind the first barrier: a segment of an earlier run that passed every wait above on stale values)
        const int fd2 = shm_open(name, O_RDWR, 0600);
        struct stat st2;
        const bool same = fd2 >= 0 && fstat(fd2, &st2) == 0 && (unsigned long long)st2.st_ino == my_ino;
        if (fd2 >= 0) (void)close(fd2);
        if (!same) { msdp_set_error("comm_init_ipc: attached to a stale segment %s", name); return MSDP_ECOMM; }
    }
    size_t hmax = 0;
    for (int q = 0; q < nranks; ++q) hmax = std::max<size_t>(hmax, (size_t)sh->vote[q]);
    // (four regions of rows + halo slots each: the one-reduction trip of msdp_pipe.h publishes H md alternately in two and its refresh
    // rows in two more; the two-reduction trip and the TR tail use the first)
    const size_t rows_doubles = 4 * ((size_t)msdp_rows_capacity(h) + hmax) * ldx;
    g->xr_halo_max = (int)hmax;
    // the exchange buffer of MY rows (+ my halo slots): my own allocation (on my device), exported; then the others', mapped
    {
        void* p = nullptr;
        if (hipExtMallocWithFlags(&p, rows_doubles * sizeof(double), hipDeviceMallocFinegrained) != hipSuccess) { (void)hipGetLastError(); msdp_set_error("comm_init_ipc: exchange buffer allocation failed"); local_break(g); return MSDP_ENOMEM; }
        HIPCHK(hipMemset(p, 0, rows_doubles * sizeof(double)));
        HIPCHK(hipDeviceSynchronize());
        hipIpcMemHandle_t hd;
        if (hipIpcGetMemHandle(&hd, p) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(p); msdp_set_error("comm_init_ipc: hipIpcGetMemHandle (exchange buffer) failed"); local_break(g); return MSDP_ECOMM; }
        g->xr_rows[rank] = (double*)p;
        sh->rows_handle[rank] = hd;
    }
    LOCAL_BARRIER(g);                                        // everybody has exported its buffer
    for (int q = 0; q < nranks; ++q) {
        if (q == rank) continue;
        void* p = nullptr;
        hipIpcMemHandle_t hd = sh->rows_handle[q];
        if (hipIpcOpenMemHandle(&p, hd, hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); msdp_set_error("comm_init_ipc: hipIpcOpenMemHandle (exchange buffer of rank %d) failed", q); local_break(g); return MSDP_ECOMM; }
        g->xr_rows[q] = (double*)p;
    }
    g->xr_rows_doubles = rows_doubles;
    // Round 6, the two-level reductions of msdp_psync.h (psync2): every member's own block -- its local slot regions, the member lines the
    // others' leaders push into, its error word -- fine-grained memory of ITS device, exported like the exchange buffer; and where the
    // members sit: the PCI bus ids tell how many share a device (their workgroups must be resident together) and whether any two own
    // different ones (then the reductions are two-level and the pushed rows cross devices)
    {
        void* p = nullptr;
        const size_t bb = msdp_xr2_block_bytes();
        if (hipExtMallocWithFlags(&p, bb, hipDeviceMallocFinegrained) != hipSuccess) { (void)hipGetLastError(); msdp_set_error("comm_init_ipc: synchronisation block allocation failed"); return MSDP_ENOMEM; }
        g->xr2_blk[rank] = (unsigned long long*)p;
        int rc2 = msdp_xr2_reset(h->stream, g->xr2_blk[rank]);
        if (rc2) return rc2;
        HIPCHK(hipStreamSynchronize(h->stream));
        hipIpcMemHandle_t hd;
        if (hipIpcGetMemHandle(&hd, p) != hipSuccess) { (void)hipGetLastError(); msdp_set_error("comm_init_ipc: hipIpcGetMemHandle (synchronisation block) failed"); return MSDP_ECOMM; }
        sh->blk_handle[rank] = hd;
        int dev = 0;
        char bus[32] = {0};
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetPCIBusId(bus, (int)sizeof(bus), dev) != hipSuccess) { (void)hipGetLastError(); snprintf(bus, sizeof(bus), "device-%d", dev); }
        memcpy(sh->devid[rank], bus, sizeof(bus));
    }
    LOCAL_BARRIER(g);                                        // every block is exported, every device id is in the segment
    for (int q = 0; q < nranks; ++q) {
        if (q == rank) continue;
        void* p = nullptr;
        hipIpcMemHandle_t hd = sh->blk_handle[q];
        if (hipIpcOpenMemHandle(&p, hd, hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); msdp_set_error("comm_init_ipc: hipIpcOpenMemHandle (synchronisation block of rank %d) failed", q); return MSDP_ECOMM; }
        g->xr2_blk[q] = (unsigned long long*)p;
    }
    {
        if (hipMalloc((void**)&g->xr2_table, LOCAL_MAX_RANKS * sizeof(unsigned long long*)) != hipSuccess) { (void)hipGetLastError(); msdp_set_error("comm_init_ipc: out of device memory"); return MSDP_ENOMEM; }
        unsigned long long* tab[LOCAL_MAX_RANKS];
        for (int q = 0; q < LOCAL_MAX_RANKS; ++q) tab[q] = g->xr2_blk[q < nranks ? q : rank];
        HIPCHK(msdp_memcpy(g->xr2_table, tab, sizeof(tab), hipMemcpyHostToDevice));
        int share = 1;
        bool multi = false;
        for (int q = 0; q < nranks; ++q) {
            int cnt = 0;
            for (int t = 0; t < nranks; ++t) cnt += strncmp(sh->devid[q], sh->devid[t], sizeof(sh->devid[q])) == 0 ? 1 : 0;
            share = std::max(share, cnt);
            if (strncmp(sh->devid[q], sh->devid[rank], sizeof(sh->devid[q])) != 0) multi = true;
        }
        // (`multi` as every member sees it: true on all of them as soon as two devices are involved)
        bool any_multi = false;
        for (int q = 0; q < nranks; ++q) for (int t = 0; t < nranks; ++t) if (strncmp(sh->devid[q], sh->devid[t], sizeof(sh->devid[q])) != 0) any_multi = true;
        (void)multi;
        h->xr2_blk = g->xr2_blk[rank]; h->xr2_peers = g->xr2_table; h->xr2_share = share; h->xr2_multi = any_multi; h->lgroup_is_ipc = true;
    }
    LOCAL_BARRIER(g);
    return 0;
}

extern "C" int msdp_comm_init(msdp_handle h, int32_t nranks, int32_t rank, const void* id128) {
    MSDP_CHECK_H(h);
    if (nranks < 1 || rank < 0 || rank >= nranks || !id128) { msdp_set_error("bad comm arguments"); return MSDP_EINVAL; }
    if (h->d.costkind == COST_HERM) { msdp_set_error("comm_init: a Hermitian handle joins no communicator (row-sharded complex factors are not implemented)"); return MSDP_EUNSUPPORTED; }
    if (h->d.costkind == COST_BLOCK) { msdp_set_error("comm_init: a %s handle joins no communicator (row-sharded block rows are not implemented)", msdp_block_kind_name(h->d.efree)); return MSDP_EUNSUPPORTED; }
    if (h->d.costkind == COST_SPLR) { msdp_set_error("comm_init: a sparse-plus-low-rank handle joins no communicator (row-sharded low-rank terms are not implemented)"); return MSDP_EUNSUPPORTED; }
    if (h->have_point) { msdp_set_error("comm_init must precede set_point"); return MSDP_ESTATE; }
    if (h->presharded && (nranks != h->nranks || rank != h->rank)) { msdp_set_error("comm_init: shard was created as rank %d of %d", h->rank, h->nranks); return MSDP_EINVAL; }
    if (h->kind == MSDP_KIND_MULTIBLOCK || msdp_dual_kind(h)) {
        msdp_set_error("row sharding is not implemented for the multiblock and dual kinds");
        return MSDP_EUNSUPPORTED;
    }
    ncclUniqueId id;
    memcpy(&id, id128, 128);
    ncclComm_t comm;
    ncclResult_t r = ncclCommInitRank(&comm, nranks, id, rank);
    if (r != ncclSuccess) { msdp_set_error("ncclCommInitRank failed: %s", ncclGetErrorString(r)); return MSDP_ECOMM; }
    h->comm = comm;
    return comm_partition(h, nranks, rank);
}

// The row partition of a communicator of `nranks` members (RCCL or the in-process stand-in)
static int comm_partition(msdp_handle h, int32_t nranks, int32_t rank) {
    h->nranks = nranks;
    h->rank = rank;
    h->use_comm = true;      // also with nranks == 1: a size-1 communicator exercises the same RCCL calls
    const int cap = msdp_rows_capacity(h);
    h->d.row0 = rank * cap;
    int r1 = h->d.row0 + cap;
    if (r1 > h->d.n) r1 = h->d.n;
    h->d.n_loc = r1 > h->d.row0 ? r1 - h->d.row0 : 0;
    int rc = msdp_alloc_common(h);
    if (rc) return rc;
    if (h->d.costkind == COST_SPARSE && (rc = msdp_upload_sparse_rows(h))) return rc;
    if (h->d.costkind == COST_DENSE && !h->presharded) {
        msdp_set_error("dense C must be created per shard (msdp_create_onlyunitdiag_dense_synthetic)");
        return MSDP_EUNSUPPORTED;
    }
    if ((rc = msdp_alloc_vectors(h, h->pcap))) return rc;
    return halo_setup(h);
}

extern "C" int msdp_debug_shard(msdp_handle h, int32_t nranks, int32_t rank) {
    MSDP_CHECK_H(h);
    if (nranks < 1 || rank < 0 || rank >= nranks) { msdp_set_error("bad shard (%d of %d)", rank, nranks); return MSDP_EINVAL; }
    if (h->have_point || h->use_comm) { msdp_set_error("debug_shard must precede set_point / comm_init"); return MSDP_ESTATE; }
    if (h->d.costkind == COST_BLOCK) { msdp_set_error("debug_shard: a %s handle is not row-sharded", msdp_block_kind_name(h->d.efree)); return MSDP_EUNSUPPORTED; }
    if (h->d.costkind == COST_DENSE || h->d.costkind == COST_SPLR || h->d.costkind == COST_HERM || h->kind == MSDP_KIND_MULTIBLOCK || msdp_dual_kind(h)) {
        msdp_set_error("debug_shard: sparse-C and affine (unitdiag / unittrace / generic) handles only");
        return MSDP_EUNSUPPORTED;
    }
    h->nranks = nranks;
    h->rank = rank;
    h->presharded = true;                  // lets msdp_debug_set_full_rows stand in for the all-gather
    const int cap = msdp_rows_capacity(h);
    h->d.row0 = rank * cap;
    int r1 = h->d.row0 + cap;
    if (r1 > h->d.n) r1 = h->d.n;
    h->d.n_loc = r1 > h->d.row0 ? r1 - h->d.row0 : 0;
    int rc = msdp_alloc_common(h);
    if (rc) return rc;
    if (h->d.costkind == COST_SPARSE && (rc = msdp_upload_sparse_rows(h))) return rc;
    return msdp_alloc_vectors(h, h->pcap);
}

extern "C" int msdp_local_rows(msdp_handle h, int64_t* row0, int64_t* row1) {
    MSDP_CHECK_H(h);
    if (row0) *row0 = h->d.row0;
    if (row1) *row1 = h->d.row0 + h->d.n_loc;
    return 0;
}

// Test / measurement only: average time of one collective call of the given kind on the handle's stream (reps back to back).
//   0 exchange of the direction rows, 1 all-reduce of one partial-sum array, 2 exchange + sums (msdp_trip1.hip), 3 all-reduce of
//   three arrays, 4 rows then sums as two ungrouped all-gathers
extern "C" int msdp_debug_time_collective(msdp_handle h, int32_t which, int32_t reps, double* avg_us) {
    MSDP_CHECK_H(h);
    if (!avg_us || reps < 1 || which < 0 || which > 4) return MSDP_EINVAL;
    if (!h->use_comm) { msdp_set_error("debug_time_collective: no communicator"); return MSDP_ESTATE; }
    int rc = 0;
    auto one = [&]() -> int {
        switch (which) {
            case 0: return msdp_exchange_rows(h, h->d.md);
            case 1: return msdp_allreduce_partials(h, P_DHD, 1);
            case 2: return msdp_exchange_rows_sums(h, h->d.md);
            case 3: return msdp_allreduce_partials(h, P_S1, 3);
            default: { int r = msdp_exchange_rows(h, h->d.md); return r ? r : msdp_allgather_vec(h, h->d.xs, h->d.xs_all, 4); }
        }
    };
    const long long keep = h->coll_calls;
    for (int i = 0; i < 3 && !rc; ++i) rc = one();
    if (rc) return rc;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    for (int i = 0; i < reps && !rc; ++i) rc = one();
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    h->coll_calls = keep;
    if (rc) return rc;
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *avg_us = 1e3 * (double)ms / reps;
    return 0;
}

extern "C" int msdp_debug_collective_calls(msdp_handle h, int64_t* calls) {
    MSDP_CHECK_H(h);
    if (!calls) return MSDP_EINVAL;
    *calls = h->coll_calls;
    return 0;
}
