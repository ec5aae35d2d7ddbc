// msdp_bench.hip -- measurement and trace entry points (msdp_bench_*, msdp_debug_persist_trace).
#include "msdp_common.h"

// ------------------------------------------------------------------ measurement
static void algo_cost(msdp_handle h, double* bytes, double* flops) {
    const Dev& d = h->d;
    const double n = d.n_loc, p = d.p;
    if (d.costkind == COST_SPARSE) {
        // nnz*(8+4) + (n+1)*4 + 3*8*n*p + 8*n ; 2*nnz*p + 5*n*p
        *bytes = (double)d.nnz * 12.0 + (n + 1) * 4.0 + 24.0 * n * p + 8.0 * n;
        *flops = 2.0 * (double)d.nnz * p + 5.0 * n * p;
    } else if (d.costkind == COST_SPLR) {
        // the sparse launch plus the low-rank term: the gather source read once more by the projection (8 n p), V read by
        // the projection and by the row launch (2 * 8 n q), T written and read (q p, negligible); 2 n q p flops each
        const double q = d.lrq;
        *bytes = (double)d.nnz * 12.0 + (n + 1) * 4.0 + 24.0 * n * p + 8.0 * n + 8.0 * n * p + 16.0 * n * q + 16.0 * q * p;
        *flops = 2.0 * (double)d.nnz * p + 5.0 * n * p + 4.0 * n * q * p;
    } else if (d.costkind == COST_HERM) {
        // p = the real width: complex values of 16 bytes, a complex multiply-add (4 fma) per entry and double2
        *bytes = (double)d.nnz * 20.0 + (n + 1) * 4.0 + 24.0 * n * p + 8.0 * n;
        *flops = 4.0 * (double)d.nnz * p + 5.0 * n * p;
    } else if (d.costkind == COST_BLOCK) {
        // d.nnz = stored values (d^2 per block entry, 8 bytes each), one 4-byte column index per d^2 of them; the multiplier
        // blocks (d values per row) in place of eG; 2 d n p flops more for Lambda U and as many for sym(W Y') and its product
        const double dd = (double)d.blk * d.blk;
        *bytes = (double)d.nnz * (8.0 + 4.0 / dd) + (d.nb + 1) * 4.0 + 24.0 * n * p + 8.0 * n * d.blk;
        *flops = 2.0 * (double)d.nnz * p + (1.0 + 6.0 * d.blk) * n * p;
        if (d.efree) {
            // the pose-graph kind: nb free rows carry no multiplier and no projection -- Lambda is nb d^2 values with
            // d = blk - 1, and the 6 d p flops per row of Lambda U, sym(W Y') and its product fall on the nb d rotation rows
            const double dr = d.blk - 1.0;
            *bytes = (double)d.nnz * (8.0 + 4.0 / dd) + (d.nb + 1) * 4.0 + 24.0 * n * p - 8.0 * d.nb * p + 8.0 * d.nb * dr * dr;
            *flops = 2.0 * (double)d.nnz * p + 1.0 * n * p + 6.0 * dr * (d.nb * dr) * p;
        }
    } else if (d.costkind == COST_DENSE) {
        *bytes = 8.0 * n * (double)d.n + 24.0 * n * p;
        *flops = 2.0 * n * (double)d.n * p;
    } else {
        msdp_affine_algo_cost(h, bytes, flops);
    }
}

extern "C" int msdp_bench_hessvec(msdp_handle h, int32_t reps, double* avg_ms, double* algo_bytes, double* algo_flops) {
    MSDP_CHECK_H(h);
    if (reps < 1 || !avg_ms) return MSDP_EINVAL;
    int rc = msdp_ensure_state(h);
    if (rc) return rc;
    // direction: the Riemannian gradient at the resident point
    HIPCHK(msdp_memcpy_async(h->d.md, h->d.Gr[msdp_host_cur(h)], (size_t)msdp_rows_capacity(h) * h->d.ld * sizeof(double),
                          hipMemcpyDeviceToDevice, h->stream));
    if ((rc = msdp_k_set_active(h, 1))) return rc;
    for (int i = 0; i < 3; ++i) if ((rc = msdp_launch_hess(h))) return rc;
    // replay a graph of 50 back-to-back launches so the host launch path is not what is timed
    const int per = 50;
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    const bool graph = msdp_use_graphs(h);
    if (graph) {
        HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        for (int i = 0; i < per && !rc; ++i) rc = msdp_launch_hess(h);
        hipError_t e = hipStreamEndCapture(h->stream, &g);
        if (rc) return rc;
        if (e != hipSuccess) { msdp_set_error("graph capture failed: %s", hipGetErrorString(e)); return MSDP_EHIP; }
        HIPCHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        HIPCHK(hipGraphLaunch(ge, h->stream));
    }
    const int nrep = (reps + per - 1) / per;
    reps = nrep * per;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    for (int i = 0; i < nrep; ++i) {
        if (graph) { HIPCHK(hipGraphLaunch(ge, h->stream)); }
        else for (int t = 0; t < per; ++t) if ((rc = msdp_launch_hess(h))) return rc;
    }
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    if (ge) (void)hipGraphExecDestroy(ge);
    if (g) (void)hipGraphDestroy(g);
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *avg_ms = (double)ms / reps;
    if ((rc = msdp_k_set_active(h, 0))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    double b, f;
    algo_cost(h, &b, &f);
    if (algo_bytes) *algo_bytes = b;
    if (algo_flops) *algo_flops = f;
    return 0;
}

// Time ONE kernel of the tCG trip in isolation (graph of 50 back-to-back launches):
// which = 0 hess, 1 upd1, 2 upd2.  Exits are disabled (bench mode).
extern "C" int msdp_bench_kernel(msdp_handle h, int32_t which, int32_t reps, double* avg_ms) {
    MSDP_CHECK_H(h);
    if (reps < 1 || !avg_ms || which < 0 || which > 2) return MSDP_EINVAL;
    int rc = msdp_ensure_state(h);
    if (rc) return rc;
    msdp_rtr_opts o;
    msdp_rtr_default_opts(&o);
    o.maxinner = 0x7ffffff0; o.maxiter = 1;
    msdp_fill_ctl(h, &o);
    h->h_ctl->bench_mode = 1;
    if ((rc = msdp_push_ctl(h))) return rc;
    if ((rc = msdp_launch_costgrad(h, msdp_host_cur(h)))) return rc;
    if ((rc = msdp_launch_rtr_begin(h))) return rc;
    if ((rc = msdp_launch_tcg_init(h))) return rc;
    for (int i = 0; i < 2; ++i)
        if ((rc = msdp_launch_hess(h)) || (rc = msdp_launch_upd1(h)) || (rc = msdp_launch_upd2(h))) return rc;
    if ((rc = msdp_launch_hess(h))) return rc;
    if (which == 2 && (rc = msdp_launch_upd1(h))) return rc;      // upd2 reads frame 1
    const int per = 50;
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < per && !rc; ++i)
        rc = which == 0 ? msdp_launch_hess(h) : (which == 1 ? msdp_launch_upd1(h) : msdp_launch_upd2(h));
    hipError_t e = hipStreamEndCapture(h->stream, &g);
    if (rc) return rc;
    if (e != hipSuccess) { msdp_set_error("graph capture failed: %s", hipGetErrorString(e)); return MSDP_EHIP; }
    HIPCHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    HIPCHK(hipGraphLaunch(ge, h->stream));
    const int nrep = (reps + per - 1) / per;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    for (int i = 0; i < nrep; ++i) HIPCHK(hipGraphLaunch(ge, h->stream));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    (void)hipGraphExecDestroy(ge);
    (void)hipGraphDestroy(g);
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *avg_ms = (double)ms / (nrep * per);
    h->h_ctl->bench_mode = 0;
    h->h_ctl->done = 0;
    if ((rc = msdp_push_ctl(h))) return rc;
    if ((rc = msdp_k_set_active(h, 0))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->state_valid = false;
    return 0;
}

// Measurement only: where the time of a persistent tCG trip goes.  Runs msdp_bench_tcg_trip(reps) on the traced instance of the
// persistent kernel and returns thread 0's s_memtime stamps of 7 phase boundaries (see msdp_persist.hip, TSTAMP) for every
// workgroup and the trips j0 .. j0 + nj - 1: out[((g * nj + t) * 8 + phase)], cap >= G * nj * 8 entries; dims = {G, nj, j0}.
extern "C" int msdp_bench_tcg_trip(msdp_handle h, int32_t reps, double* avg_ms);
extern "C" int msdp_debug_persist_trace(msdp_handle h, int32_t reps, uint64_t* out, int64_t cap, int32_t* dims, double* avg_ms) {
    MSDP_CHECK_H(h);
    if (!out || !dims || !avg_ms) return MSDP_EINVAL;
    if (!msdp_persist_eligible(h)) { msdp_set_error("persist_trace: the persistent kernel does not apply to this handle"); return MSDP_EUNSUPPORTED; }
    int G = 0, nj = 0, j0 = 0;
    msdp_persist_trace_dims(h, &G, &nj, &j0);
    dims[0] = G; dims[1] = nj; dims[2] = j0;
    const bool fused = reps <= 0;                                  // the TR iterations of one trustregions() call in the fused launch
    if (fused) { G = msdp_fused_grid(h); dims[0] = G; }            // (the fused launch plans its own grid)
    const size_t cnt = (size_t)G * nj * 8 * (fused ? 2 : 1);       // (fused: + the trips of one TR iteration, msdp_pipe.h MSDP_TRACE_KSEL)
    if (fused) { j0 = 0; dims[2] = 0; }
    if (cap < (int64_t)cnt || (!fused && reps < j0 + nj)) { msdp_set_error("persist_trace: cap >= %zu entries and reps >= %d needed", cnt, j0 + nj); return MSDP_EINVAL; }
    if (!h->trace_buf) {
        void* p = nullptr;
        int rc = msdp_dev_alloc_bytes(h, &p, (size_t)2 * MSDP_MAX_GRID * nj * 8 * sizeof(unsigned long long));
        if (rc) return rc;
        h->trace_buf = (unsigned long long*)p;
    }
    HIPCHK(hipMemset(h->trace_buf, 0, cnt * sizeof(unsigned long long)));
    h->d.trace = h->trace_buf;
    int rc;
    if (fused) {
        // one call with the options of the handle's last msdp_rtr (the reference's inner-solver defaults before any): avg_ms = its time
        msdp_rtr_opts o = h->last_opts;
        if (o.maxinner < 1) { msdp_rtr_default_opts(&o); o.maxiter = 40; o.maxinner = 100; }
        if (!msdp_persist_fused_ok(h)) { h->d.trace = nullptr; msdp_set_error("persist_trace: the fused launch does not apply to this handle"); return MSDP_EUNSUPPORTED; }
        msdp_rtr_stats st;
        rc = msdp_rtr(h, &o, &st);
        *avg_ms = st.seconds * 1e3;
    } else rc = msdp_bench_tcg_trip(h, reps, avg_ms);
    h->d.trace = nullptr;
    if (rc) return rc;
    HIPCHK(msdp_memcpy(out, h->trace_buf, cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int msdp_bench_tcg_trip(msdp_handle h, int32_t reps, double* avg_ms) {
    MSDP_CHECK_H(h);
    if (reps < 1 || !avg_ms) return MSDP_EINVAL;
    int rc = msdp_ensure_state(h);
    if (rc) return rc;
    msdp_rtr_opts o;
    msdp_rtr_default_opts(&o);
    o.maxinner = 0x7ffffff0; o.maxiter = 1;
    msdp_fill_ctl(h, &o);
    h->h_ctl->bench_mode = 1;
    if (msdp_persist_eligible(h)) {
        // persistent kernel: `reps` trips with the exits disabled in one launch (run twice, time the second)
        h->h_ctl->maxinner = reps;
        if ((rc = msdp_push_ctl(h))) return rc;
        if ((rc = msdp_launch_costgrad(h, msdp_host_cur(h)))) return rc;
        if ((rc = msdp_launch_rtr_begin(h))) return rc;
        h->d.status = nullptr;
        rc = msdp_launch_tcg_persist(h);
        if (!rc) {
            hipError_t e1 = hipEventRecord(h->ev0, h->stream);
            rc = msdp_launch_tcg_persist(h);
            hipError_t e2 = hipEventRecord(h->ev1, h->stream);
            hipError_t e3 = hipEventSynchronize(h->ev1);
            float ms = 0.f;
            hipError_t e4 = hipEventElapsedTime(&ms, h->ev0, h->ev1);
            if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess) { msdp_set_error("bench events failed"); rc = MSDP_EHIP; }
            *avg_ms = (double)ms / reps;
        }
        {
            void* dp = nullptr;
            if (hipHostGetDevicePointer(&dp, (void*)h->h_status, 0) == hipSuccess) h->d.status = (unsigned long long*)dp;
        }
        h->h_ctl->bench_mode = 0;
        h->h_ctl->done = 0;
        int rc2 = msdp_push_ctl(h);
        HIPCHK(hipStreamSynchronize(h->stream));
        h->state_valid = false;
        int perr = 0;
        HIPCHK(msdp_memcpy(&perr, h->psync_err, sizeof(int), hipMemcpyDeviceToHost));
        if (perr) { msdp_set_error("persistent tCG: grid synchronisation timed out"); return MSDP_EHIP; }
        return rc ? rc : rc2;
    }
    if (msdp_blockpersist_eligible(h)) {
        // block kinds, option "block_persist": the same measurement of msdp_blockpersist.hip (run twice, time the second)
        h->h_ctl->maxinner = reps;
        if ((rc = msdp_push_ctl(h))) return rc;
        if ((rc = msdp_launch_costgrad(h, msdp_host_cur(h)))) return rc;
        if ((rc = msdp_launch_rtr_begin(h))) return rc;
        rc = msdp_launch_tcg_blockpersist(h, 1);
        if (!rc) {
            hipError_t e1 = hipEventRecord(h->ev0, h->stream);
            rc = msdp_launch_tcg_blockpersist(h, 0);
            hipError_t e2 = hipEventRecord(h->ev1, h->stream);
            hipError_t e3 = hipEventSynchronize(h->ev1);
            float ms = 0.f;
            hipError_t e4 = hipEventElapsedTime(&ms, h->ev0, h->ev1);
            if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess) { msdp_set_error("bench events failed"); rc = MSDP_EHIP; }
            *avg_ms = (double)ms / reps;
        }
        h->h_ctl->bench_mode = 0;
        h->h_ctl->done = 0;
        int rc2 = msdp_push_ctl(h);
        HIPCHK(hipStreamSynchronize(h->stream));
        h->state_valid = false;
        int perr = 0;
        HIPCHK(msdp_memcpy(&perr, h->psync_err, sizeof(int), hipMemcpyDeviceToHost));
        if (perr) {
            HIPCHK(hipMemset(h->psync_err, 0, sizeof(int)));
            msdp_set_error("persistent tCG (%s kind): grid synchronisation timed out", msdp_block_kind_name(h->d.efree));
            return MSDP_EHIP;
        }
        return rc ? rc : rc2;
    }
    if (h->use_comm && h->lgroup && h->nranks > 1 && h->d.costkind == COST_SPARSE) {
        // in-process ranks: the cross-rank persistent tCG when every member can run it (`reps` trips, exits disabled, one launch per
        // member; run twice, time the second) -- every member calls this function together
        int agreed = 0;
        if ((rc = msdp_local_vote_min(h, msdp_xpersist_eligible(h, h->nranks), &agreed))) return rc;
        bool xuse = false;
        if (agreed && (rc = msdp_xr_begin(h, &xuse))) return rc;
        if (xuse) {
            h->h_ctl->maxinner = reps;
            if ((rc = msdp_push_ctl(h))) return rc;
            if ((rc = msdp_launch_costgrad(h, msdp_host_cur(h)))) return rc;
            if ((rc = msdp_launch_rtr_begin(h))) return rc;
            h->d.status = nullptr;
            float ms = 0.f;
            for (int pass = 0; pass < 2 && !rc; ++pass) {
                if (pass && (rc = msdp_xr_begin(h, &xuse))) break;
                HIPCHK(hipEventRecord(h->ev0, h->stream));
                rc = msdp_xr_launch(h);
                HIPCHK(hipEventRecord(h->ev1, h->stream));
                HIPCHK(hipEventSynchronize(h->ev1));
                HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
                if (!rc) rc = msdp_xr_check(h);
                { int rcb = msdp_local_barrier(h); if (rcb) return rcb; }
            }
            *avg_ms = (double)ms / reps;
            msdp_restore_status_ptr(h);
            h->h_ctl->bench_mode = 0;
            h->h_ctl->done = 0;
            int rc2 = msdp_push_ctl(h);
            HIPCHK(hipStreamSynchronize(h->stream));
            h->state_valid = false;
            h->xpersist_last = true;
            return rc ? rc : rc2;
        }
    }
    if ((rc = msdp_push_ctl(h))) return rc;
    if ((rc = msdp_launch_costgrad(h, msdp_host_cur(h)))) return rc;
    if ((rc = msdp_launch_rtr_begin(h))) return rc;
    h->h_ctl->done = 0;
    if ((rc = msdp_tcg_begin(h))) return rc;
    if ((rc = msdp_enqueue_trips(h, 2))) return rc;
    const int CH = MSDP_TCG_CHUNK;
    const bool graph = msdp_use_graphs(h);
    if (graph && (rc = msdp_ensure_chunk_graph(h, CH))) return rc;
    const int nchunks = (reps + CH - 1) / CH;
    reps = nchunks * CH;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    for (int i = 0; i < nchunks; ++i) if ((rc = msdp_launch_chunk(h, CH, graph))) return rc;
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *avg_ms = (double)ms / reps;
    h->h_ctl->bench_mode = 0;
    h->h_ctl->done = 0;
    if ((rc = msdp_push_ctl(h))) return rc;
    if ((rc = msdp_k_set_active(h, 0))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->state_valid = false;
    return 0;
}
