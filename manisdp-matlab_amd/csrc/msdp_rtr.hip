// msdp_rtr.hip -- host side of the device-resident RTR / tCG driver (msdp_rtr): which path a call takes (fused launch,
// persistent tCG, chunk graphs, lock-step chunks, cross-rank persistent tCG) and the host loop around each.
#include "msdp_common.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>

extern "C" int msdp_debug_last_rtr_device_ms(msdp_handle h, double* ms) {
    MSDP_CHECK_H(h);
    if (!ms) return MSDP_EINVAL;
    *ms = h->last_rtr_device_ms;
    return 0;
}

extern "C" int msdp_tcg_path(msdp_handle h, int32_t* path) {
    MSDP_CHECK_H(h);
    if (!path) return MSDP_EINVAL;
    if (!h->have_point) { msdp_set_error("tcg_path: no resident point"); return MSDP_ESTATE; }
    *path = (msdp_persist_eligible(h) || msdp_blockpersist_eligible(h)) ? 1 : ((h->use_comm && h->lgroup && h->xpersist_last) ? 2 : 0);   // 2: the last call ran the cross-rank persistent tCG
    return 0;
}

// Which of the chunked trips msdp_tcg_begin / msdp_enqueue_trips take for the resident point, in their order of tests: 1 the
// linear-product trip (msdp_trip1.hip), 2 the two-launch trip (msdp_trip2.hip), 3 three launches per trip; 0: a persistent path
extern "C" int msdp_debug_trip_form(msdp_handle h, int32_t* form) {
    MSDP_CHECK_H(h);
    if (!form) return MSDP_EINVAL;
    int32_t path = 0;
    const int rc = msdp_tcg_path(h, &path);
    if (rc) return rc;
    *form = path ? 0 : (msdp_trip1_ok(h) ? 1 : (msdp_trip2_ok(h) ? 2 : 3));
    return 0;
}

// ------------------------------------------------------------------ RTR driver
int msdp_push_ctl(msdp_handle h) {
    HIPCHK(msdp_memcpy_async(h->d.ctl, h->h_ctl, sizeof(Ctl), hipMemcpyHostToDevice, h->stream));
    return 0;
}
static int pull_ctl(msdp_handle h) {
    HIPCHK(msdp_memcpy_async(h->h_ctl, h->d.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

void msdp_fill_ctl(msdp_handle h, const msdp_rtr_opts* o) {
    Ctl* c = h->h_ctl;
    const int cur = c->cur;
    const double sigma = c->sigma;
    const double z0 = c->z_sphere[0], z1 = c->z_sphere[1];
    memset(c, 0, sizeof(Ctl));
    c->cur = cur; c->sigma = sigma; c->z_sphere[0] = z0; c->z_sphere[1] = z1;
    c->maxiter = o->maxiter; c->maxinner = o->maxinner; c->mininner = o->mininner;
    c->tolgradnorm = o->tolgradnorm; c->kappa = o->kappa; c->theta = o->theta;
    c->rho_prime = o->rho_prime; c->rho_reg = o->rho_regularization;
    c->persist_refresh = h->tune.persist_refresh;
    c->persist_early = h->tune.persist_early;
    c->pipe_refresh = h->tune.pipe_refresh == 1 ? 2 : h->tune.pipe_refresh;   // never 1 (see msdp_set_option)
    c->pipe_local = h->tune.pipe_local;
    c->persist_goff = h->tune.persist_goff;
    c->psync_backoff = h->tune.psync_backoff;
    c->psync8_backoff = h->tune.psync8_backoff;
    // trustregions.m:363-372; typicaldist: pi*sqrt(n) (ManiSDP_onlyunitdiag.m:137) or pi (spherefactory.m:111)
    // ... or sqrt(n*p) (euclideanfactory.m:57) or sqrt(dim) = sqrt(nb (p d - d (d + 1) / 2)) (stiefelstackedfactory.m:43,53);
    // with efree free rows per block d = blk - efree and the product's sqrt(nb (p d - d (d + 1) / 2) + nb efree p)
    // (productmanifold.m:160-166 over the two)
    const double stf_d = (double)(h->d.blk - h->d.efree);
    const double stf_dim = (double)h->d.nb * ((double)h->d.p * stf_d - 0.5 * stf_d * (stf_d + 1.0) + (double)h->d.efree * h->d.p);
    const double typical = (h->d.manifold == MANI_OBLIQUE) ? M_PI * sqrt((double)h->d.n)
                           : (h->d.manifold == MANI_EUCLID ? sqrt((double)h->d.n * (double)h->d.p)
                           : (h->d.manifold == MANI_STIEFEL ? sqrt(std::max(stf_dim, 1.0)) : M_PI));
    c->Delta_bar = (o->Delta_bar > 0) ? o->Delta_bar : typical;
    c->Delta0 = (o->Delta0 > 0) ? o->Delta0 : c->Delta_bar / 8.0;
}

bool msdp_use_graphs(msdp_handle h) { return h->tune.graph && !h->use_comm; }

// Start of a tCG (tCG.m:102-157).  Two-launch trips (msdp_trip2.hip): the Hess-vec of trip j+1 rides in the launch that closes
// trip j, so the first one is issued here, behind the initialisation.
int msdp_tcg_begin(msdp_handle h) {
    if (msdp_trip1_ok(h)) {
        // sharded trip with one all-reduce (msdp_trip1.hip): the first product is a direct one on the gradient rows
        int rc;
        h->d.xn = h->nranks;
        if (!h->use_comm) h->d.xs_all = h->d.xs;
        h->trip1_count = 0;
        if ((rc = msdp_launch_trip1_init(h))) return rc;
        if ((rc = msdp_exchange_rows(h, h->d.md))) return rc;
        if ((rc = msdp_launch_trip1_head(h, true))) return rc;
        return msdp_allreduce_partials(h, P_DHD, 1);
    }
    if (msdp_trip2_ok(h)) {
        int rc = msdp_launch_trip2_init(h);
        return rc ? rc : msdp_launch_trip2_head(h);
    }
    return h->d.pcM ? msdp_pose_precon_init(h) : msdp_launch_tcg_init(h);   // (option "precon" of the pose-graph kind: msdp_pose_precon.hip)
}
int msdp_enqueue_trips(msdp_handle h, int cnt) {
    int rc;
    if (msdp_trip1_ok(h)) {
        const int refresh = h->tune.persist_refresh;
        for (int t = 0; t < cnt; ++t) {
            if ((rc = msdp_launch_trip1_upd(h))) return rc;                         // tCG.m:166-241
            // eta and r ping-pong: trip t (counted from 0) of a running tCG writes r' into r2 when t is even (after the end of
            // a tCG the launches are no-ops and the buffer does not matter)
            const double* rnew = (h->trip1_count & 1) ? h->d.r : h->d.r2;
            if ((rc = msdp_exchange_rows_sums(h, rnew))) return rc;                 // rows of r' + every rank's three sums
            if ((rc = msdp_launch_trip1_head(h, false))) return rc;                 // tCG.m:227-287, tCG.m:163 by linearity
            ++h->trip1_count;
            // every refresh-th trip multiplies directly once more (inside a graph capture the count is not the replay's: there
            // msdp_launch_chunk appends the refresh behind the graph -- one rank, no collective in between)
            if (!h->trip1_capture && refresh > 0 && (h->trip1_count % refresh) == 0) {
                if ((rc = msdp_exchange_rows(h, h->d.md))) return rc;
                if ((rc = msdp_launch_trip1_head(h, true))) return rc;
            }
            if ((rc = msdp_allreduce_partials(h, P_DHD, 1))) return rc;             // <mdelta, H mdelta> over all ranks (tCG.m:166)
        }
        return 0;
    }
    if (msdp_trip2_ok(h)) {
        for (int t = 0; t < cnt; ++t) {
            if ((rc = msdp_launch_trip2_upd(h))) return rc;    // tCG.m:166-241
            if ((rc = msdp_launch_trip2_head(h))) return rc;   // tCG.m:227-287, then tCG.m:163 of the next trip
        }
        return 0;
    }
    const bool pc = h->d.pcM != nullptr;                  // pose-graph kind, option "precon": the preconditioned updates (msdp_pose_precon.hip)
    for (int t = 0; t < cnt; ++t) {
        if ((rc = msdp_launch_hess(h))) return rc;        // tCG.m:163
        if ((rc = pc ? msdp_pose_precon_upd1(h) : msdp_launch_upd1(h))) return rc;        // tCG.m:166-241
        if ((rc = pc ? msdp_pose_precon_upd2(h) : msdp_launch_upd2(h))) return rc;        // tCG.m:249-287
    }
    return 0;
}

// One hipGraph of CH tCG trips (3*CH kernel nodes).  All kernel arguments are the Dev
// struct by value and all run-time state lives in device memory, so the same executable
// graph is replayed for every chunk until the Dev struct changes (new p / reallocation).
// Kernels of a finished tCG exit at their first instruction, so replaying a whole chunk
// past the end of the solve is safe.
int msdp_ensure_chunk_graph(msdp_handle h, int CH) {
    h->d.full = h->d.md;
    // The affine kinds bake the current slot's pointers (eS[cur], Y[cur]) into the launches on the host, so
    // they keep one executable graph per slot; the other kinds read `cur` on the device.
    const int slot = (h->d.costkind == COST_AFFINE) ? h->h_ctl->cur : 0;
    if (h->chunk_len != CH || memcmp(&h->chunk_sig, &h->d, sizeof(Dev)) != 0) {
        for (int s = 0; s < 2; ++s)
            if (h->chunk_execs[s]) { (void)hipGraphExecDestroy(h->chunk_execs[s]); h->chunk_execs[s] = nullptr; }
        h->chunk_sig = h->d;
        h->chunk_len = CH;
    }
    if (!h->chunk_execs[slot]) {
        hipGraph_t g = nullptr;
        HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        const int count_keep = h->trip1_count;
        h->trip1_capture = true;
        int rc = msdp_enqueue_trips(h, CH);
        h->trip1_capture = false;
        h->trip1_count = count_keep;
        hipError_t e = hipStreamEndCapture(h->stream, &g);
        if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
        if (e != hipSuccess) { msdp_set_error("graph capture failed: %s", hipGetErrorString(e)); return MSDP_EHIP; }
        e = hipGraphInstantiate(&h->chunk_execs[slot], g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) { msdp_set_error("graph instantiate failed: %s", hipGetErrorString(e)); h->chunk_execs[slot] = nullptr; return MSDP_EHIP; }
    }
    h->chunk_exec = h->chunk_execs[slot];
    return 0;
}

int msdp_launch_chunk(msdp_handle h, int CH, bool graph) {
    if (graph) {
        HIPCHK(hipGraphLaunch(h->chunk_exec, h->stream));
        if (msdp_trip1_ok(h)) {
            // msdp_trip1.hip on one rank: the refresh schedule of the linear products, behind every (refresh / CH)-th replay
            const int refresh = h->tune.persist_refresh, before = h->trip1_count;
            h->trip1_count += CH;
            if (refresh > 0 && h->trip1_count / refresh != before / refresh) {
                int rc = msdp_exchange_rows(h, h->d.md);
                if (!rc) rc = msdp_launch_trip1_head(h, true);
                if (rc) return rc;
            }
        }
        return 0;
    }
    return msdp_enqueue_trips(h, CH);
}

// tCG of the current TR iteration when the rows are sharded over a communicator.  Every rank must issue the SAME
// sequence of collectives, so how many chunks are enqueued may depend only on device state that is identical on all
// ranks: the `tcg_running` flag, which every rank computes from the same all-reduced sums.  The flag after each chunk
// is copied to a pinned word behind the chunk (an event marks the copy); the host stays ONE chunk ahead of the device
// -- chunk i+1 is already enqueued when the flag of chunk i is read -- so the stream never drains while the host
// decides, and at most one chunk of no-op trips (whose collectives still run) follows the end of a tCG.
static int run_tcg_lockstep(msdp_handle h, int maxinner) {
    const int CH = MSDP_TCG_CHUNK;
    const int nchunks = (maxinner + CH - 1) / CH;
    int rc;
    h->d.status = nullptr;                                         // no host-mapped progress word on this path
    if ((rc = msdp_tcg_begin(h))) return rc;                            // trustregions.m:484-496
    int enq = 0;
    auto push_chunk = [&]() -> int {
        int r2 = msdp_enqueue_trips(h, CH);
        if (r2) return r2;
        HIPCHK(msdp_memcpy_async((void*)&h->h_flags[enq & 1], &h->d.ctl->tcg_running, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipEventRecord(h->ev_flag[enq & 1], h->stream));
        ++enq;
        return 0;
    };
    if ((rc = push_chunk())) return rc;
    if (nchunks > 1 && (rc = push_chunk())) return rc;
    for (int i = 0; i < enq; ++i) {
        HIPCHK(hipEventSynchronize(h->ev_flag[i & 1]));
        if (!h->h_flags[i & 1]) break;                             // finished inside chunk i; what follows is a no-op
        if (enq < nchunks && (rc = push_chunk())) return rc;       // slot (i & 1) is free again: chunk i + 2 takes it
    }
    return 0;
}

// Run the tCG inner loop of the current TR iteration: chunks of CH trips are enqueued one
// ahead of the device (so the graph-launch latency is hidden) while the host polls the
// host-mapped progress word the lead thread of k_tcg_upd2 publishes every trip.
static int run_tcg(msdp_handle h, int maxinner, int k, bool* done_out = nullptr) {
    const int CH = MSDP_TCG_CHUNK;
    const bool graph = msdp_use_graphs(h);
    int rc;
    if (graph && (rc = msdp_ensure_chunk_graph(h, CH))) return rc;
    if ((rc = msdp_tcg_begin(h))) return rc;                           // trustregions.m:484-496
    int enq = 0;
    if ((rc = msdp_launch_chunk(h, CH, graph))) return rc;
    enq = 1;
    if (enq * CH < maxinner) { if ((rc = msdp_launch_chunk(h, CH, graph))) return rc; enq = 2; }
    const unsigned long long want = (unsigned long long)(unsigned)(k + 1);
    const auto t0 = std::chrono::steady_clock::now();
    auto last_query = t0;
    long spins = 0;
    for (;;) {
        const unsigned long long s = *h->h_status;
        if ((s >> 32) == want) {
            const int active = (int)(s & 1ULL);
            const int jraw = (int)((s & 0xffffffffULL) >> 1);
            if (done_out && (jraw & 0x40000000)) *done_out = true;
            const int j = jraw & 0x3fffffff;
            if (!active) break;
            if (enq * CH < maxinner && j >= (enq - 1) * CH) {
                if ((rc = msdp_launch_chunk(h, CH, graph))) return rc;
                ++enq;
                continue;
            }
        }
        std::this_thread::sleep_for(std::chrono::microseconds(10));     // polite polling (a chunk of 8 trips lasts ~0.2 ms)
        if ((++spins & 0xff) == 0 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - last_query).count() > 1.0) {
            last_query = std::chrono::steady_clock::now();      // hipStreamQuery is not a cheap poll (can block for tens of ms): safety net only
            if (hipStreamQuery(h->stream) == hipSuccess) {
                // everything enqueued has run: the final status must be visible now
                const unsigned long long s2 = *h->h_status;
                if ((s2 >> 32) == want && !(s2 & 1ULL)) {
                    if (done_out && (((s2 & 0xffffffffULL) >> 1) & 0x40000000)) *done_out = true;
                    break;
                }
                if (enq * CH >= maxinner || (s2 >> 32) != want) {
                    msdp_set_error("tCG progress word inconsistent (status %llx, TR iteration %d)", s2, k);
                    return MSDP_EHIP;
                }
            }
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 120.0) {
                msdp_set_error("tCG made no progress for 120 s");
                return MSDP_EHIP;
            }
        }
    }
    return 0;
}

void msdp_restore_status_ptr(msdp_handle h) {
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, (void*)h->h_status, 0) == hipSuccess) h->d.status = (unsigned long long*)dp;
}

// Did a persistent launch give up on a grid synchronisation?  (Its bounded spins turn a would-be hang -- the
// workgroups of the launch not all resident because something else occupies CUs -- into this flag.)
static int persist_timed_out(msdp_handle h, bool* out) {
    int perr = 0;
    HIPCHK(msdp_memcpy(&perr, h->psync_err, sizeof(int), hipMemcpyDeviceToHost));
    *out = perr != 0;
    return 0;
}

// ctl and the persistent kernels' error word with ONE host synchronisation (the word lands in a pinned slot of h_flags)
static int pull_ctl_and_err(msdp_handle h, bool* timed_out) {
    HIPCHK(msdp_memcpy_async((void*)&h->h_flags[8], h->psync_err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    int rc = pull_ctl(h);
    if (rc) return rc;
    *timed_out = h->h_flags[8] != 0;
    return 0;
}

// The body of msdp_rtr.  *timed_out: a persistent launch reported a grid-synchronisation time-out (the resident
// point is then in an undefined state; the caller restores the start point and calls again, which takes the
// chunked path because h->persist_failed is set).
static int rtr_core(msdp_handle h, const msdp_rtr_opts* opts, bool* timed_out) {
    int rc;
    *timed_out = false;
    msdp_fill_ctl(h, opts);
    *h->h_status = 0;
    if ((rc = msdp_push_ctl(h))) return rc;
    int cur = h->h_ctl->cur;
    if ((rc = msdp_launch_costgrad(h, cur))) return rc;          // trustregions.m:405
    if ((rc = msdp_launch_rtr_begin(h))) return rc;
    const bool timing = h->tune.timing != 0;
    double t_tcg = 0.0, t_rest = 0.0, t_enq_sum = 0.0, t_enq_max = 0.0;
    const bool async_tr = h->d.costkind == COST_SPARSE && !h->use_comm;
    const bool persist = async_tr && msdp_persist_eligible(h);
    const bool fused = persist && !h->tune.fail_persist && msdp_persist_fused_ok(h);
    // the fused launch reads ctl on the device (a solve that is already done is a no-op there): the host needs the state of
    // the start point only on the other paths -- one host round trip less per call (20-100 us, host to host)
    if (!fused && (rc = pull_ctl(h))) return rc;
    if (!fused) HIPCHK(hipEventRecord(h->ev0, h->stream));       // (msdp_debug_last_rtr_device_ms: closed in msdp_rtr)
    h->last_rtr_fused = fused;
    if (persist && h->tune.fail_persist) {                       // test hook: behave as if the launch had timed out
        h->tune.fail_persist = 0;
        *timed_out = true;
        return 0;
    }
    if (fused) {
        // Fused path: the whole trustregions() loop (every tCG, retraction, cost/gradient at the proposal and the
        // accept/reject logic) runs in ONE launch; the host only waits for it (msdp_persist.hip, FUSE = true).
        const auto ta = std::chrono::steady_clock::now();
        h->d.status = nullptr;                                            // no progress word needed
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        rc = msdp_launch_rtr_fused(h);
        msdp_restore_status_ptr(h);
        if (rc) return rc;
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        if ((rc = pull_ctl_and_err(h, timed_out))) return rc;
        {   // (the stream is idle: the events are complete)
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_rtr_device_ms = (double)ms; else (void)hipGetLastError();
        }
        if (*timed_out) return 0;
        t_tcg = std::chrono::duration<double>(std::chrono::steady_clock::now() - ta).count();
    } else if (persist) {
        // Persistent path: one launch runs the whole tCG of a TR iteration with the working set on chip
        // (msdp_persist.hip), a second one the rest of the iteration (msdp_trtail.hip: retraction, cost and gradient at
        // the proposal, accept/reject; each clears the other's synchronisation slots).  The host stays one TR iteration
        // ahead of the device: iteration i+1 is enqueued as soon as the kernel of iteration i publishes that it has
        // started; a finished solve (ctl->done) turns everything still enqueued into no-ops and is reported through
        // the same progress word.
        bool first_iter = true;
        auto enqueue_iter = [&]() -> int {
            int r2;
            if ((r2 = msdp_launch_tcg_persist(h, first_iter ? 1 : 0))) return r2;   // trustregions.m:484-496 + tCG.m
            first_iter = false;
            return msdp_launch_tr_tail(h);                                // :540-729
        };
        // (round 5: up to AHEAD iterations beyond the last one known to have started -- with ONE the device waited for the host
        // whenever an iteration was shorter than the host's polling sleep + two launches: 78 us per TR iteration whatever its tCG
        // (tools/fused_overhead_probe.py).  What is enqueued behind a finished solve returns at once: at most AHEAD - 1 pairs of
        // empty launches per call.)
        const int AHEAD = 3;
        int enq = 0, started = 0;
        bool done = false;
        const auto ta = std::chrono::steady_clock::now();
        auto last_query = ta;
        while (!done) {
            while (enq < opts->maxiter && enq < started + AHEAD) {
                const auto te = std::chrono::steady_clock::now();
                if ((rc = enqueue_iter())) return rc;
                if (timing) {
                    const double de = std::chrono::duration<double>(std::chrono::steady_clock::now() - te).count();
                    t_enq_sum += de; if (de > t_enq_max) t_enq_max = de;
                }
                ++enq;
                last_query = std::chrono::steady_clock::now();
            }
            if (started >= enq) break;                           // every iteration of the budget has started (or maxiter = 0)
            long spins = 0;
            for (;;) {
                const unsigned long long s = *h->h_status;
                const int it = (int)(s >> 32);
                if (it > started && it <= enq) {
                    started = it;
                    if (((s & 0xffffffffULL) >> 1) & 0x40000000) done = true;
                    break;
                }
                // a TR iteration lasts 0.02-2 ms: poll politely (a hard spin burns a full core; under a container CPU quota that
                // got this thread throttled for tens of ms at a time, seen as 60 ms holes in the kernel trace of the G81 solve)
                std::this_thread::sleep_for(std::chrono::microseconds(20));
                if ((++spins & 0xff) == 0) {
                    // hipStreamQuery is NOT a cheap poll (every call makes the runtime touch the queue; called every
                    // few microseconds it stalled the stream for tens of ms, seen as gaps in the kernel trace): it is
                    // only the safety net against a lost progress word; on a stream that is running a long kernel one call was
                    // measured to block for ~40 ms, so ask only after 2 s without any progress
                    const auto now = std::chrono::steady_clock::now();
                    if (std::chrono::duration<double>(now - last_query).count() > 2.0) {
                        last_query = now;
                        if (hipStreamQuery(h->stream) == hipSuccess) {
                            const unsigned long long s2 = *h->h_status;
                            const int it2 = (int)(s2 >> 32);
                            if (it2 > started && it2 <= enq) { started = it2; if (((s2 & 0xffffffffULL) >> 1) & 0x40000000) done = true; break; }
                            // everything enqueued has run and the word never arrived: a launch that gave up on a grid
                            // synchronisation exits without publishing
                            if ((rc = persist_timed_out(h, timed_out))) return rc;
                            if (*timed_out) return 0;
                            msdp_set_error("persistent tCG: progress word inconsistent (status %llx, expected iteration %d..%d)", s2, started + 1, enq);
                            return MSDP_EHIP;
                        }
                    }
                    if (std::chrono::duration<double>(now - ta).count() > 300.0) {
                        msdp_set_error("persistent tCG made no progress for 300 s");
                        return MSDP_EHIP;
                    }
                }
            }
        }
        if ((rc = pull_ctl(h))) return rc;
        if ((rc = persist_timed_out(h, timed_out))) return rc;
        if (*timed_out) return 0;
        t_tcg = std::chrono::duration<double>(std::chrono::steady_clock::now() - ta).count();
    } else if (async_tr) {
        // No host sync between TR iterations: the proposal slot is resolved on the device, the next
        // iteration's tcg_init + first chunks are enqueued right behind k_rtr_decide, and k_tcg_init
        // publishes `done` through the progress word (a finished solve turns everything enqueued into no-ops).
        int k = 0;
        bool done = false;
        while (k < opts->maxiter) {
            const auto ta = std::chrono::steady_clock::now();
            if ((rc = run_tcg(h, opts->maxinner, k, &done))) return rc;
            const auto tb = std::chrono::steady_clock::now();
            t_tcg += std::chrono::duration<double>(tb - ta).count();
            if (done) break;
            if ((rc = msdp_launch_retract(h))) return rc;             // :540
            if ((rc = msdp_launch_costgrad(h, 3))) return rc;         // :544 (proposal slot, device-resolved)
            if ((rc = msdp_launch_rtr_decide(h))) return rc;          // :548-729
            ++k;
        }
        if ((rc = pull_ctl(h))) return rc;
    } else {
        // One host synchronisation per TR iteration (dense / affine kinds bake the slot into their launches; with a
        // communicator the tCG runs in lock-step, see run_tcg_lockstep)
        // in-process ranks, sparse C: ONE persistent tCG spans the ranks' launches (msdp_persist.hip XR) -- no collective per trip;
        // every member must be able to (a vote), otherwise all of them take the lock-step chunks
        bool xp = false;
        if (h->use_comm && h->lgroup && h->nranks > 1 && h->d.costkind == COST_SPARSE) {
            int agreed = 0;
            if ((rc = msdp_local_vote_min(h, msdp_xpersist_eligible(h, h->nranks), &agreed))) return rc;
            xp = agreed != 0;
            if (xp && (rc = msdp_xr_begin(h, &xp))) return rc;
        }
        h->xpersist_last = xp;
        // block kinds with the option "block_persist": the tCG of an iteration is ONE launch (msdp_blockpersist.hip) in place of the
        // chunked trips; retraction, cost / gradient, decision and the host synchronisation stay as they are
        const bool bp = msdp_blockpersist_eligible(h) != 0;
        if (bp && h->tune.fail_persist) {                            // test hook: behave as if the launch had timed out
            h->tune.fail_persist = 0;
            *timed_out = true;
            return 0;
        }
        bool bp_first = true;
        while (!h->h_ctl->done) {                                     // trustregions.m:441
            cur = h->h_ctl->cur;
            const auto ta = std::chrono::steady_clock::now();
            if (xp) {
                h->d.status = nullptr;
                rc = msdp_xr_launch(h);
                msdp_restore_status_ptr(h);
            }
            else if (bp) { rc = msdp_launch_tcg_blockpersist(h, bp_first ? 1 : 0); bp_first = false; }
            else if (h->use_comm) rc = run_tcg_lockstep(h, opts->maxinner);
            else rc = run_tcg(h, opts->maxinner, h->h_ctl->k);        // :495
            if (rc) return rc;
            const auto tb = std::chrono::steady_clock::now();
            if (xp && h->lgroup_is_ipc && h->tune.xtail) {
                // members in different processes: the rest of the iteration is ONE launch per member too (k_tr_tail_obl<.., XR>) -- the
                // proposal rows through the group's exchange buffer, barrier and reduction over its slots, no collective
                if ((rc = msdp_xr_tail(h))) return rc;
                // ... and the decision stays on the device: three more iterations are enqueued before the host looks (both kernels
                // return at once when the solve is done, on every member alike), one host synchronisation per FOUR iterations
                for (int ahead = 0; ahead < 3 && !rc; ++ahead) {
                    h->d.status = nullptr;
                    rc = msdp_xr_launch(h);
                    msdp_restore_status_ptr(h);
                    if (!rc) rc = msdp_xr_tail(h);
                }
                if (rc) return rc;
            } else {
                if ((rc = msdp_launch_retract(h))) return rc;             // :540
                if ((rc = msdp_launch_costgrad(h, cur ^ 1))) return rc;   // :544
                if ((rc = msdp_launch_rtr_decide(h))) return rc;          // :548-729
            }
            if (bp) {
                if ((rc = pull_ctl_and_err(h, timed_out))) return rc;
                if (*timed_out) return 0;
            } else if ((rc = pull_ctl(h))) return rc;
            if (xp && (rc = msdp_xr_check(h))) return rc;
            const auto tc = std::chrono::steady_clock::now();
            t_tcg += std::chrono::duration<double>(tb - ta).count();
            t_rest += std::chrono::duration<double>(tc - tb).count();
        }
    }
    if (timing) {
        fprintf(stderr, "[msdp_rtr] enqueue total %.3f ms, slowest %.3f ms\n", t_enq_sum * 1e3, t_enq_max * 1e3);
        fprintf(stderr, "[msdp_rtr] p=%d ld=%d G=%d path=%d k=%d hessvecs=%d acc=%d rej=%d  tCG phase %.3f ms  (retract+cost+decide+sync) %.3f ms\n",
                h->d.p, h->d.ld, h->d.G, (persist || msdp_blockpersist_eligible(h)) ? 1 : 0, h->h_ctl->k, h->h_ctl->hessvecs,
                h->h_ctl->accepted, h->h_ctl->rejected, t_tcg * 1e3, t_rest * 1e3);
    }
    return 0;
}

extern "C" int msdp_rtr(msdp_handle h, const msdp_rtr_opts* opts, msdp_rtr_stats* stats) {
    MSDP_CHECK_H(h);
    if (!opts) { msdp_set_error("rtr: null options"); return MSDP_EINVAL; }
    if (!h->have_point) { msdp_set_error("rtr: no resident point (call msdp_set_point)"); return MSDP_ESTATE; }
    if (opts->rho_prime >= 0.25) { msdp_set_error("options.rho_prime must be strictly smaller than 1/4"); return MSDP_EINVAL; }
    if (opts->maxinner < 1 || opts->maxiter < 0) { msdp_set_error("rtr: maxinner >= 1 and maxiter >= 0 required"); return MSDP_EINVAL; }
    const auto t0 = std::chrono::steady_clock::now();
    h->last_opts = *opts;
    (void)msdp_window_eligible(h);                                 // (builds the patch plan of the LDS-staged S*U outside any graph capture)
    // The persistent kernels assume that all their workgroups are resident together.  When the GPU is shared (a
    // second handle solving on another stream, another process) that can fail; the launch then gives up after a
    // bounded spin.  Keep a copy of the start point so that the call can be repeated on the chunked path.
    const int cur0 = h->h_ctl->cur;
    const size_t cnt = (size_t)msdp_rows_capacity(h) * h->ldcap;
    const bool guard = (h->d.costkind == COST_SPARSE && !h->use_comm && msdp_persist_eligible(h)) || msdp_blockpersist_eligible(h);
    if (guard) {
        if (h->rtr_start_cap < cnt) {
            if (h->rtr_start) msdp_dev_free(h, h->rtr_start);
            h->rtr_start = nullptr; h->rtr_start_cap = 0;
            int rc0 = msdp_dev_alloc<double>(h, &h->rtr_start, cnt);
            if (rc0) return rc0;
            h->rtr_start_cap = cnt;
        }
        HIPCHK(msdp_memcpy_async(h->rtr_start, h->d.Y[cur0], cnt * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
    bool timed_out = false;
    int rc = rtr_core(h, opts, &timed_out);
    if (rc) return rc;
    if (timed_out) {
        if (!guard) { msdp_set_error("persistent tCG: grid synchronisation timed out"); return MSDP_EHIP; }
        fprintf(stderr, "libmanisdp_hip: a persistent tCG launch could not synchronise its workgroups (GPU shared with another "
                        "launch?); this handle continues on the chunked path\n");
        h->persist_failed = true;
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemset(h->psync_err, 0, sizeof(int)));
        h->h_ctl->cur = cur0;
        HIPCHK(msdp_memcpy_async(h->d.Y[cur0], h->rtr_start, cnt * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        msdp_restore_status_ptr(h);
        h->chunk_len = 0;                                          // re-capture the chunk graph against the current Dev
        rc = rtr_core(h, opts, &timed_out);
        if (rc) return rc;
        if (timed_out) { msdp_set_error("persistent tCG: time-out on the chunked path (internal error)"); return MSDP_EHIP; }
    }
    h->state_valid = true;
    h->gradnorm_valid = true;
    if (!h->last_rtr_fused) {
        // (the other paths: the stream time of everything the call enqueued behind the evaluation of its start point, host gaps included)
        float ms = 0.f;
        if (hipEventRecord(h->ev1, h->stream) == hipSuccess && hipEventSynchronize(h->ev1) == hipSuccess &&
            hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_rtr_device_ms = (double)ms; else (void)hipGetLastError();
    }
    if (stats) {
        const Ctl* c = h->h_ctl;
        memset(stats, 0, sizeof(*stats));
        stats->cost = c->fx; stats->gradnorm = c->norm_grad; stats->Delta = c->Delta;
        stats->iters = c->k; stats->hessvecs = c->hessvecs; stats->accepted = c->accepted;
        stats->rejected = c->rejected; stats->cost_evals = c->cost_evals;
        stats->last_stop_inner = c->last_stop_inner;
        stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return 0;
}

extern "C" int msdp_rtr_host(msdp_handle h, int32_t p, double* Y, const msdp_rtr_opts* opts, msdp_rtr_stats* stats) {
    int rc = msdp_set_point(h, p, Y);
    if (rc) return rc;
    if ((rc = msdp_rtr(h, opts, stats))) return rc;
    return msdp_get_point(h, Y);
}
