// msdp_api.hip -- C ABI of libmanisdp_hip.so (include/manisdp_hip.h): the error string, handle life cycle,
// resident-point I/O, factor operations, options and the fine-grained parity entry points.  Device memory: msdp_mem.hip;
// sharding: msdp_comm.hip; the RTR driver: msdp_rtr.hip; measurement: msdp_bench.hip.
#include "msdp_common.h"
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static thread_local char g_err[1024] = "";
void msdp_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* msdp_last_error(void) { return g_err; }
extern "C" const char* msdp_version(void) { return "manisdp_hip 0.1.0 (gfx950)"; }

static bool boundary_colmajor(msdp_handle h) { return h->kind == MSDP_KIND_UNITTRACE || h->kind == MSDP_KIND_GENERIC || h->kind == MSDP_KIND_DUAL; }

static void choose_grid(msdp_handle h) {
    Dev& d = h->d;
    int half = d.ld / 2, lpr = 1;
    while (lpr < half && lpr < 64) lpr <<= 1;
    const int rows_per_step = MSDP_WAVES * (64 / lpr);
    int want = (msdp_rows_capacity(h) + rows_per_step - 1) / rows_per_step;
    // At most one workgroup per CU: beyond 256 some CUs get a second 1024-thread workgroup and the launch waits for it
    // (measured on G81 p=32: G=320 -> 27.4 us per tCG trip, G=256 -> 24.1 us).  Round 3 (tools/archive/grid_probe.py, option grid):
    // 512 workgroups -- two full rounds -- lose as well, at every size: n = 40 000, p = 40: 50.6 us per trip against 43.1 with
    // 256; n = 80 000, p = 40: 79.0 / 71.3; n = 250 000, p = 64: 390 / 378; n = 10^6, p = 32: 770 / 766 (the stand-alone S*U
    // kernel alone gains 8 % from 512 at n = 10^6 and loses 8 % at n = 40 000).
    const int gmax = MSDP_MAX_GRID;
    int G = ((want + 7) / 8) * 8;
    if (G < 8) G = 8;
    if (G > 256) G = 256;
    if (h->tune.grid > 0) G = std::min((gmax / 8) * 8, std::max(8, ((h->tune.grid + 7) / 8) * 8));    // A/B switch
    d.G = G;
    d.sweep = (h->tune.sweep >= 2 || (h->tune.sweep == 1 && (int64_t)msdp_rows_capacity(h) * d.ld >= ((int64_t)1 << 21))) ? 1 : 0;
    // bit 1: streaming (nt) accesses for the operands a gather launch touches once -- from 3 * 2^22 vector entries on (96 MB:
    // n = 250 000 at p = 32 loses 14 % with them, p = 64 and n = 10^6 at p = 16 gain 17 %), or with sweep = 3; bits 4-7: 64-row
    // steps per workgroup and window of the stand-alone Hess-vec, minus one
    if (d.sweep && (h->tune.sweep == 3 || (h->tune.sweep == 1 && (int64_t)msdp_rows_capacity(h) * d.ld >= ((int64_t)3 << 22)))) d.sweep |= 2;
    if (d.sweep && h->tune.sweep_k > 1) d.sweep |= (std::min(h->tune.sweep_k, 16) - 1) << 4;
}

// (Re)allocate every n_loc x ld vector for factor widths up to pcap.
int msdp_alloc_vectors(msdp_handle h, int pcap) {
    Dev& d = h->d;
    const int ldcap = ((pcap + 1) / 2) * 2;
    const size_t rows = (size_t)msdp_rows_capacity(h);
    const size_t cnt = rows * (size_t)ldcap;
    double** vecs[] = {&d.Y[0], &d.Y[1], &d.Gr[0], &d.Gr[1], &d.eta[0], &d.eta[1], &d.Heta[0], &d.Heta[1],
                       &d.r, &d.r2, &d.md, &d.md2, &d.Hmd, &d.W0, &d.W1};
    if (h->full_buf) msdp_dev_free(h, h->full_buf);
    h->full_buf = nullptr;
    d.full = nullptr;
    {
        // ONE allocation for the fifteen factor-sized vectors (15 hipMalloc calls were 15 of the 19 ms the first set_point of
        // a G81 solve took -- 7 % of the 0.22-s solve, tools/archive/g81_host_profile.py); each vector starts on a 256-byte boundary
        const size_t nvec = sizeof(vecs) / sizeof(vecs[0]);
        const size_t stride = (cnt + 31) / 32 * 32;
        if (h->vec_pool) msdp_dev_free(h, h->vec_pool);
        h->vec_pool = nullptr;
        for (double** v : vecs) *v = nullptr;
        int rc = msdp_dev_alloc<double>(h, &h->vec_pool, stride * nvec);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(h->vec_pool, 0, stride * nvec * sizeof(double), h->stream));
        size_t i = 0;
        for (double** v : vecs) *v = h->vec_pool + stride * (i++);
    }
    if (d.mdx) msdp_dev_free(h, d.mdx);
    d.mdx = nullptr;
    {
        // regions of one vector each: the EARLY trips of the persistent tCG alternate between the first two (msdp_persist.hip), the
        // one-reduction trips too and use the next two for their direct exchanges; the fused launch of msdp_pipe.h exchanges the
        // proposal's rows and the gradient rows of the two point slots through three more (round 6) -- where the persistent kernels can
        // apply at all (rows per rank within their reach)
        const size_t xcnt = (msdp_rows_capacity(h) <= 65536 ? 7 : 4) * cnt;
        int rc = msdp_dev_alloc_uncached<double>(h, &d.mdx, xcnt);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(d.mdx, 0, xcnt * sizeof(double), h->stream));
    }
    if (h->use_comm || h->nranks > 1) {
        int rc = msdp_dev_alloc<double>(h, &h->full_buf, cnt * (size_t)h->nranks);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(h->full_buf, 0, cnt * h->nranks * sizeof(double), h->stream));
        d.full = h->full_buf;
        for (int s2 = 0; s2 < 2; ++s2) {
            if (h->yfull[s2]) { msdp_dev_free(h, h->yfull[s2]); h->yfull[s2] = nullptr; }
            if (d.costkind != COST_AFFINE) continue;
            int rc2 = msdp_dev_alloc<double>(h, &h->yfull[s2], cnt * (size_t)h->nranks);
            if (rc2) return rc2;
            HIPCHK(hipMemsetAsync(h->yfull[s2], 0, cnt * h->nranks * sizeof(double), h->stream));
        }
    }
    h->pcap = pcap;
    h->ldcap = ldcap;
    if (h->pc_z) return msdp_pose_precon_vectors(h);               // option "precon" (msdp_pose_precon.hip): its vector follows the capacity
    return 0;
}

int msdp_alloc_common(msdp_handle h) {
    Dev& d = h->d;
    int rc;
    // msdp_comm_init / msdp_debug_shard call this a second time (the row split changed): release the first set
    if (d.ctl) { msdp_dev_free(h, d.ctl); d.ctl = nullptr; }
    if (d.F) { msdp_dev_free(h, d.F); d.F = nullptr; }
    if (d.P) { msdp_dev_free(h, d.P); d.P = nullptr; }
    if (h->psync_slots) { msdp_dev_free(h, h->psync_slots); h->psync_slots = nullptr; }
    if (h->psync_err) { msdp_dev_free(h, h->psync_err); h->psync_err = nullptr; }
    if ((rc = msdp_dev_alloc<Ctl>(h, &d.ctl, 1))) return rc;
    if ((rc = msdp_dev_alloc<Frame>(h, &d.F, 2))) return rc;
    // behind the partial-sum arrays: the sums of the sharded one-all-reduce trip (msdp_trip1.hip) and its arrival counter
    const size_t p_doubles = (size_t)MSDP_NPART * MSDP_MAX_GRID + 4 + 4 * MSDP_XS_MAX_RANKS + 2;
    if ((rc = msdp_dev_alloc<double>(h, &d.P, p_doubles))) return rc;
    HIPCHK(hipMemset(d.ctl, 0, sizeof(Ctl)));
    HIPCHK(hipMemset(d.F, 0, 2 * sizeof(Frame)));
    HIPCHK(hipMemset(d.P, 0, p_doubles * sizeof(double)));
    d.xs = d.P + (size_t)MSDP_NPART * MSDP_MAX_GRID;
    d.xs_all = d.xs + 4;
    d.xcount = reinterpret_cast<unsigned*>(d.xs_all + 4 * MSDP_XS_MAX_RANKS);
    d.xn = h->nranks;
    {
        char* ps = nullptr;
        if ((rc = msdp_dev_alloc_uncached<char>(h, &ps, msdp_psync_bytes()))) return rc;
        h->psync_slots = (unsigned long long*)ps;
        if ((rc = msdp_dev_alloc<int>(h, &h->psync_err, 1))) return rc;
        HIPCHK(hipMemset(h->psync_err, 0, sizeof(int)));
    }
    const size_t rows = (size_t)msdp_rows_capacity(h);
    for (int s = 0; s < 2; ++s) {
        if (d.eG[s]) { msdp_dev_free(h, d.eG[s]); d.eG[s] = nullptr; }
        if ((rc = msdp_dev_alloc<double>(h, &d.eG[s], rows))) return rc;
        HIPCHK(hipMemset(d.eG[s], 0, rows * sizeof(double)));
    }
    return 0;
}

static int new_handle(int kind, int64_t n, msdp_handle* out) {
    if (!out) { msdp_set_error("out handle pointer is null"); return MSDP_EINVAL; }
    if (n <= 0 || n > 0x7fffffff) { msdp_set_error("matrix order n = %lld out of range", (long long)n); return MSDP_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        msdp_set_error("no HIP device visible: libmanisdp_hip has no CPU fallback");
        return MSDP_EHIP;
    }
    msdp_handle h = new msdp_handle_s();
    h->kind = kind;
    h->d.n = (int)n;
    h->d.n_loc = (int)n;
    h->d.row0 = 0;
    h->d.manifold = (kind == MSDP_KIND_UNITTRACE) ? MANI_SPHERE : (kind == MSDP_KIND_GENERIC ? MANI_EUCLID : MANI_OBLIQUE);
    {
        // the documented environment switches, read once per handle (msdp_set_option changes them afterwards)
        auto on = [](const char* name) { const char* e = getenv(name); return e && atoi(e) != 0; };
        if (on("MSDP_NO_PERSIST")) h->tune.persist = 0;
        if (on("MSDP_NO_FUSED_RTR")) h->tune.fused_rtr = 0;
        if (on("MSDP_NO_PERSIST_PIPE")) h->tune.persist_pipe = 0;
        if (on("MSDP_NO_GRAPH")) h->tune.graph = 0;
        if (on("MSDP_TIMING")) h->tune.timing = 1;
        if (on("MSDP_ESC_DEBUG")) h->tune.esc_debug = 1;
        h->d.persist_ep = h->tune.persist_ep;
        if (const char* e = getenv("MSDP_AFFINE_ROUTE")) h->tune.affine_route = !strcmp(e, "gram") ? 2 : (!strcmp(e, "sddmm") ? 1 : 0);
    }
    hipError_t e = hipSuccess;
    if (!msdp_host_kit_take(h)) {
        e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_ctl, sizeof(Ctl), hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_frame, 2 * sizeof(Frame), hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_flags, 64, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_status, 64, hipHostMallocMapped);
    }
    if (e == hipSuccess) e = hipEventCreate(&h->ev0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev1);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_flag[0], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_flag[1], hipEventDisableTiming);
    if (e == hipSuccess) {
        *h->h_status = 0;
        void* dp = nullptr;
        e = hipHostGetDevicePointer(&dp, (void*)h->h_status, 0);
        h->d.status = (unsigned long long*)dp;
    }
    if (e != hipSuccess) {
        msdp_set_error("stream/event/pinned setup failed: %s", hipGetErrorString(e));
        delete h;
        return MSDP_EHIP;
    }
    *out = h;
    return 0;
}

// Upload the CSR rows [row0, row0+n_loc) of the host copy.
int msdp_upload_sparse_rows(msdp_handle h) {
    Dev& d = h->d;
    const int r0 = d.row0, r1 = d.row0 + d.n_loc;
    const int base = h->h_rowptr[r0];
    const int64_t nnz = h->h_rowptr[r1] - base;
    std::vector<int> rp((size_t)msdp_rows_capacity(h) + 1);
    for (int i = 0; i <= d.n_loc; ++i) rp[i] = h->h_rowptr[r0 + i] - base;
    for (size_t i = d.n_loc + 1; i < rp.size(); ++i) rp[i] = rp[d.n_loc];
    if (h->d_rowptr) msdp_dev_free(h, h->d_rowptr);
    if (h->d_colind) msdp_dev_free(h, h->d_colind);
    if (h->d_cval) msdp_dev_free(h, h->d_cval);
    int rc;
    if ((rc = msdp_dev_alloc<int>(h, &h->d_rowptr, rp.size()))) return rc;
    if ((rc = msdp_dev_alloc<int>(h, &h->d_colind, (size_t)nnz))) return rc;
    if ((rc = msdp_dev_alloc<double>(h, &h->d_cval, (size_t)nnz))) return rc;
    HIPCHK(msdp_memcpy(h->d_rowptr, rp.data(), rp.size() * sizeof(int), hipMemcpyHostToDevice));
    if (nnz) {
        HIPCHK(msdp_memcpy(h->d_colind, h->h_colind.data() + base, nnz * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(msdp_memcpy(h->d_cval, h->h_cval.data() + base, nnz * sizeof(double), hipMemcpyHostToDevice));
    }
    d.rowptr = h->d_rowptr; d.colind = h->d_colind; d.cval = h->d_cval; d.nnz = nnz;
    // ELL copy when every row is short (fixed-degree graphs such as G81: W = 5)
    int W = 0;
    for (int i = 0; i < d.n_loc; ++i) W = std::max(W, rp[i + 1] - rp[i]);
    d.ellW = 0; d.ellc = nullptr; d.ellv = nullptr;
    h->ell_own_col = false;
    if (W >= 1 && W <= 8) {
        // stored width 5 or 8 (the persistent tCG kernel is instantiated for these and loads every slice
        // without a branch); the padding entries are (own row, 0.0)
        W = W <= 5 ? 5 : 8;
        const size_t cap = (size_t)msdp_rows_capacity(h);
        std::vector<int> ec((size_t)W * cap);
        std::vector<double> ev((size_t)W * cap, 0.0);
        for (int w = 0; w < W; ++w)
            for (size_t i = 0; i < cap; ++i) ec[(size_t)w * cap + i] = (int)std::min<size_t>(i, d.n_loc ? d.n_loc - 1 : 0) + d.row0;
        for (int i = 0; i < d.n_loc; ++i)
            for (int t = rp[i]; t < rp[i + 1]; ++t) {
                const int w = t - rp[i];
                ec[(size_t)w * cap + i] = h->h_colind[base + t];
                ev[(size_t)w * cap + i] = h->h_cval[base + t];
            }
        if (h->d_ellc) msdp_dev_free(h, h->d_ellc);
        if (h->d_ellv) msdp_dev_free(h, h->d_ellv);
        if ((rc = msdp_dev_alloc<int>(h, &h->d_ellc, ec.size()))) return rc;
        if ((rc = msdp_dev_alloc<double>(h, &h->d_ellv, ev.size()))) return rc;
        HIPCHK(msdp_memcpy(h->d_ellc, ec.data(), ec.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(msdp_memcpy(h->d_ellv, ev.data(), ev.size() * sizeof(double), hipMemcpyHostToDevice));
        d.ellW = W; d.ell_stride = (int64_t)cap; d.ellc = h->d_ellc; d.ellv = h->d_ellv;
        // every stored row references itself -- through its diagonal entry or, with fewer than W entries, through a padding slot: what
        // the own-column form of the fused tCG needs (msdp_pipe.h, OWNC)
        bool own = true;
        for (int i = 0; i < d.n_loc && own; ++i) {
            bool has = rp[i + 1] - rp[i] < W;
            for (int t = rp[i]; t < rp[i + 1] && !has; ++t) has = h->h_colind[base + t] == i + d.row0;
            own = has;
        }
        h->ell_own_col = own;
    }
    return 0;
}

extern "C" int msdp_set_device(int32_t device) {
    HIPCHK(hipSetDevice(device));
    return 0;
}
extern "C" int msdp_device_count(int32_t* count) {
    if (!count) return MSDP_EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return 0;
}

extern "C" void msdp_rtr_default_opts(msdp_rtr_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->maxiter = 1000; o->maxinner = 100; o->mininner = 1;
    o->tolgradnorm = 1e-6; o->kappa = 0.1; o->theta = 1.0; o->rho_prime = 0.1;
    o->rho_regularization = 1e3; o->Delta_bar = -1.0; o->Delta0 = -1.0;
}

extern "C" int msdp_create_onlyunitdiag_csc(int64_t n, const int64_t* jc, const int64_t* ir,
                                            const double* pr, int32_t pcap, msdp_handle* out) {
    if (!jc || (!ir && jc[n] > 0) || (!pr && jc[n] > 0)) { msdp_set_error("null sparse arrays"); return MSDP_EINVAL; }
    msdp_handle h = nullptr;
    int rc = new_handle(MSDP_KIND_ONLYUNITDIAG, n, &h);
    if (rc) return rc;
    const int64_t nnz = jc[n];
    if (nnz > 0x7fffffff) { msdp_set_error("nnz(C) too large"); msdp_destroy(h); return MSDP_EINVAL; }
    h->h_rowptr.resize(n + 1);
    h->h_colind.resize(nnz);
    h->h_cval.assign(pr, pr + nnz);
    for (int64_t i = 0; i <= n; ++i) h->h_rowptr[i] = (int)jc[i];
    for (int64_t k = 0; k < nnz; ++k) {
        if (ir[k] < 0 || ir[k] >= n) { msdp_set_error("row index out of range"); msdp_destroy(h); return MSDP_EINVAL; }
        h->h_colind[k] = (int)ir[k];
    }
    h->d.costkind = COST_SPARSE;
    if ((rc = msdp_alloc_common(h)) || (rc = msdp_upload_sparse_rows(h)) || (rc = msdp_alloc_vectors(h, pcap > 0 ? pcap : 32))) {
        msdp_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

// C = Cs + V diag(s) V' (ManiSDP_onlyunitdiag.m:6 with C held implicitly): the sparse handle plus the low-rank fields
extern "C" int msdp_create_onlyunitdiag_csc_lowrank(int64_t n, const int64_t* jc, const int64_t* ir, const double* pr, int32_t q,
                                                    const double* V, const double* s, int32_t pcap, msdp_handle* out) {
    if (q < 1 || q > MSDP_LOWRANK_MAX) { msdp_set_error("low-rank term: q = %d outside 1 .. %d", q, MSDP_LOWRANK_MAX); return MSDP_EINVAL; }
    if (!V || !s) { msdp_set_error("low-rank term: null V or s"); return MSDP_EINVAL; }
    if (!out) { msdp_set_error("out handle pointer is null"); return MSDP_EINVAL; }
    if (n <= 0 || n > 0x7fffffff) { msdp_set_error("matrix order n = %lld out of range", (long long)n); return MSDP_EINVAL; }
    msdp_handle h = nullptr;
    int rc = msdp_create_onlyunitdiag_csc(n, jc, ir, pr, pcap, &h);
    if (rc) return rc;
    if ((rc = msdp_lowrank_setup(h, q, V, s))) { msdp_destroy(h); return rc; }
    h->d.costkind = COST_SPLR;
    *out = h;
    return 0;
}

// C = A + iB Hermitian (msdp_hermitian.hip): the pattern as above, val = nnz (re, im) pairs; pcap counts complex columns
extern "C" int msdp_create_onlyunitdiag_csc_hermitian(int64_t n, const int64_t* jc, const int64_t* ir, const double* val, int32_t pcap,
                                                      msdp_handle* out) {
    if (!out) { msdp_set_error("out handle pointer is null"); return MSDP_EINVAL; }
    if (n <= 0 || n > 0x7fffffff) { msdp_set_error("matrix order n = %lld out of range", (long long)n); return MSDP_EINVAL; }
    if (!jc || (!ir && jc[n] > 0) || (!val && jc[n] > 0)) { msdp_set_error("null sparse arrays"); return MSDP_EINVAL; }
    const int64_t nnz = jc[n];
    if (nnz < 0 || nnz > 0x7fffffff) { msdp_set_error("nnz(C) too large"); return MSDP_EINVAL; }
    if (pcap > 512) { msdp_set_error("Hermitian cost: pcap = %d complex columns exceeds 512 (real width 1024)", pcap); return MSDP_EUNSUPPORTED; }
    for (int64_t j = 0; j < n; ++j) {
        if (jc[j] > jc[j + 1] || jc[j] < 0 || jc[j + 1] > nnz) { msdp_set_error("column pointers not monotone"); return MSDP_EINVAL; }
        for (int64_t k = jc[j]; k < jc[j + 1]; ++k) {
            if (ir[k] < 0 || ir[k] >= n) { msdp_set_error("row index out of range"); return MSDP_EINVAL; }
            if (ir[k] == j && val[2 * k + 1] != 0.0) {
                msdp_set_error("Hermitian cost: diagonal entry %lld has the imaginary part %g (a Hermitian matrix has a real diagonal)", (long long)j, val[2 * k + 1]);
                return MSDP_EINVAL;
            }
        }
    }
    msdp_handle h = nullptr;
    int rc = new_handle(MSDP_KIND_ONLYUNITDIAG, n, &h);
    if (rc) return rc;
    h->h_rowptr.resize(n + 1);
    h->h_colind.resize(nnz);
    for (int64_t i = 0; i <= n; ++i) h->h_rowptr[i] = (int)jc[i];
    for (int64_t k = 0; k < nnz; ++k) h->h_colind[k] = (int)ir[k];
    h->d.costkind = COST_HERM;
    if ((rc = msdp_alloc_common(h)) || (rc = msdp_hermitian_setup(h, val)) || (rc = msdp_alloc_vectors(h, 2 * (pcap > 0 ? pcap : 32)))) {
        msdp_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

// X_[ii] = I_d on the stacked Stiefel manifold (msdp_stiefel.hip): C of order N = n d in block CSR of block order d
extern "C" int msdp_create_onlyunitblockdiag_csc(int64_t N, int32_t d, const int64_t* jc, const int64_t* ir, const double* val,
                                                 int32_t pcap, msdp_handle* out) {
    if (!out) { msdp_set_error("out handle pointer is null"); return MSDP_EINVAL; }
    if (N <= 0 || N > 0x7fffffff) { msdp_set_error("matrix order N = %lld out of range", (long long)N); return MSDP_EINVAL; }
    if (d != 2 && d != 3) { msdp_set_error("unit-block-diagonal handle: block order d = %d (2 or 3)", d); return MSDP_EINVAL; }
    if (N % d != 0) { msdp_set_error("unit-block-diagonal handle: N = %lld is no multiple of the block order d = %d", (long long)N, d); return MSDP_EINVAL; }
    if (!jc || (!ir && jc[N] > 0) || (!val && jc[N] > 0)) { msdp_set_error("null sparse arrays"); return MSDP_EINVAL; }
    const int64_t nnz = jc[N];
    if (nnz < 0 || nnz > 0x7fffffff) { msdp_set_error("nnz(C) too large"); return MSDP_EINVAL; }
    if (pcap > 256) { msdp_set_error("unit-block-diagonal handle: pcap = %d exceeds the supported width of 256", pcap); return MSDP_EUNSUPPORTED; }
    for (int64_t j = 0; j < N; ++j) {
        if (jc[j] > jc[j + 1] || jc[j] < 0 || jc[j + 1] > nnz) { msdp_set_error("column pointers not monotone"); return MSDP_EINVAL; }
        for (int64_t k = jc[j]; k < jc[j + 1]; ++k)
            if (ir[k] < 0 || ir[k] >= N) { msdp_set_error("row index out of range"); return MSDP_EINVAL; }
    }
    msdp_handle h = nullptr;
    int rc = new_handle(MSDP_KIND_ONLYUNITDIAG, N, &h);
    if (rc) return rc;
    h->d.manifold = MANI_STIEFEL;
    h->d.costkind = COST_BLOCK;
    if ((rc = msdp_alloc_common(h)) || (rc = msdp_stiefel_setup(h, d, 0, jc, ir, val)) || (rc = msdp_alloc_vectors(h, pcap > 0 ? std::max(pcap, d) : 32))) {
        msdp_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

// The pose-graph problem, (X_[ii])_{1..d,1..d} = I_d with one free row per block (msdp_stiefel.hip, d.efree = 1): C of order N = n (d + 1) in
// block CSR of block order d + 1; the manifold is productmanifold.m:160-166 over stiefelstackedfactory.m:53 and euclideanfactory.m:57
extern "C" int msdp_create_posegraph_csc(int64_t N, int32_t d, const int64_t* jc, const int64_t* ir, const double* val,
                                         int32_t pcap, msdp_handle* out) {
    if (!out) { msdp_set_error("out handle pointer is null"); return MSDP_EINVAL; }
    if (N <= 0 || N > 0x7fffffff) { msdp_set_error("matrix order N = %lld out of range", (long long)N); return MSDP_EINVAL; }
    if (d != 2 && d != 3) { msdp_set_error("pose-graph handle: dimension d = %d (2 or 3)", d); return MSDP_EINVAL; }
    if (N % (d + 1) != 0) { msdp_set_error("pose-graph handle: N = %lld is no multiple of the block order d + 1 = %d", (long long)N, d + 1); return MSDP_EINVAL; }
    if (!jc || (!ir && jc[N] > 0) || (!val && jc[N] > 0)) { msdp_set_error("null sparse arrays"); return MSDP_EINVAL; }
    const int64_t nnz = jc[N];
    if (nnz < 0 || nnz > 0x7fffffff) { msdp_set_error("nnz(C) too large"); return MSDP_EINVAL; }
    if (pcap > MSDP_BLOCK_PMAX) { msdp_set_error("pose-graph handle: pcap = %d exceeds the supported width of %d", pcap, MSDP_BLOCK_PMAX); return MSDP_EUNSUPPORTED; }
    for (int64_t j = 0; j < N; ++j) {
        if (jc[j] > jc[j + 1] || jc[j] < 0 || jc[j + 1] > nnz) { msdp_set_error("column pointers not monotone"); return MSDP_EINVAL; }
        for (int64_t k = jc[j]; k < jc[j + 1]; ++k)
            if (ir[k] < 0 || ir[k] >= N) { msdp_set_error("row index out of range"); return MSDP_EINVAL; }
    }
    msdp_handle h = nullptr;
    int rc = new_handle(MSDP_KIND_ONLYUNITDIAG, N, &h);
    if (rc) return rc;
    h->d.manifold = MANI_STIEFEL;
    h->d.costkind = COST_BLOCK;
    if ((rc = msdp_alloc_common(h)) || (rc = msdp_stiefel_setup(h, d + 1, 1, jc, ir, val)) || (rc = msdp_alloc_vectors(h, pcap > 0 ? std::max(pcap, d) : 32))) {
        msdp_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" int msdp_create_onlyunitdiag_dense(int64_t n, const double* C, int32_t pcap, msdp_handle* out) {
    if (!C) { msdp_set_error("null C"); return MSDP_EINVAL; }
    msdp_handle h = nullptr;
    int rc = new_handle(MSDP_KIND_ONLYUNITDIAG, n, &h);
    if (rc) return rc;
    h->d.costkind = COST_DENSE;
    if ((rc = msdp_alloc_common(h)) || (rc = msdp_dense_setup(h, C)) || (rc = msdp_alloc_vectors(h, pcap > 0 ? pcap : 32))) {
        msdp_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" int msdp_create_onlyunitdiag_dense_synthetic(int64_t n, uint64_t seed, int32_t nranks, int32_t rank,
                                                       int32_t pcap, msdp_handle* out) {
    if (nranks < 1 || rank < 0 || rank >= nranks) { msdp_set_error("bad shard (%d of %d)", rank, nranks); return MSDP_EINVAL; }
    msdp_handle h = nullptr;
    int rc = new_handle(MSDP_KIND_ONLYUNITDIAG, n, &h);
    if (rc) return rc;
    h->d.costkind = COST_DENSE;
    h->nranks = nranks;
    h->rank = rank;
    h->presharded = true;
    const int cap = msdp_rows_capacity(h);
    h->d.row0 = std::min<int64_t>(n, (int64_t)rank * cap);
    h->d.n_loc = (int)std::min<int64_t>(cap, n - h->d.row0);
    if ((rc = msdp_alloc_common(h)) || (rc = msdp_dense_setup_synthetic(h, seed)) ||
        (rc = msdp_alloc_vectors(h, pcap > 0 ? pcap : 32))) {
        msdp_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

// Test-only: fill the gather buffer of a pre-sharded handle that has NO communicator (a single process
// standing in for rank r of N) with all n rows of a host matrix, so that the non-square shard kernels can be
// checked against a full-size reference on one GPU.  With a communicator the all-gather does this.
extern "C" int msdp_debug_set_full_rows(msdp_handle h, const double* rows_host) {
    MSDP_CHECK_H(h);
    if (!h->presharded || h->use_comm || !h->d.p) { msdp_set_error("debug_set_full_rows: pre-sharded, communicator-free handle with a point"); return MSDP_ESTATE; }
    Dev& d = h->d;
    const size_t cnt = (size_t)d.n * d.p;
    double* stage = nullptr;
    if (hipMalloc((void**)&stage, cnt * sizeof(double)) != hipSuccess) { msdp_set_error("staging alloc failed"); return MSDP_ENOMEM; }
    hipError_t e = msdp_memcpy_async(stage, rows_host, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream);
    int rc = 0;
    if (e != hipSuccess) { msdp_set_error("H2D failed"); rc = MSDP_EHIP; }
    if (!rc) rc = msdp_k_pack(h, stage, h->full_buf, d.n, d.p, d.ld, false);
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(stage);
    return rc;
}

extern "C" int msdp_create_affine(int32_t kind, int64_t n, int64_t m, const int64_t* at_jc, const int64_t* at_ir,
                                  const double* at_pr, const double* b, const double* c, int32_t pcap,
                                  msdp_handle* out) {
    if (kind != MSDP_KIND_UNITDIAG && kind != MSDP_KIND_UNITTRACE && kind != MSDP_KIND_GENERIC) { msdp_set_error("bad kind %d", kind); return MSDP_EINVAL; }
    if (!at_jc || !b || !c || m <= 0) { msdp_set_error("null/empty affine data"); return MSDP_EINVAL; }
    msdp_handle h = nullptr;
    int rc = new_handle(kind, n, &h);
    if (rc) return rc;
    h->d.costkind = COST_AFFINE;
    h->d.m = m;
    if ((rc = msdp_alloc_common(h)) || (rc = msdp_affine_setup(h, at_jc, at_ir, at_pr, b, c)) ||
        (rc = msdp_alloc_vectors(h, pcap > 0 ? pcap : 32))) {
        msdp_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" int msdp_create_multiblock(int32_t nb, const int64_t* block_n, int32_t nob, int64_t m, const int64_t* at_jc,
                                      const int64_t* at_ir, const double* at_pr, const double* b, const double* c,
                                      int32_t pcap, msdp_handle* out) {
    if (nb < 1 || !block_n || nob < 0 || nob > nb) { msdp_set_error("multiblock: bad block description"); return MSDP_EINVAL; }
    if (!at_jc || !b || !c || m <= 0) { msdp_set_error("null/empty affine data"); return MSDP_EINVAL; }
    // offsets of the blocks inside the direct sum (rows) and inside the concatenated vec (entries)
    std::vector<int64_t> r0((size_t)nb + 1, 0), e0((size_t)nb + 1, 0);
    for (int i = 0; i < nb; ++i) {
        if (block_n[i] < 1) { msdp_set_error("multiblock: block %d has order %lld", i, (long long)block_n[i]); return MSDP_EINVAL; }
        r0[i + 1] = r0[i] + block_n[i];
        e0[i + 1] = e0[i] + block_n[i] * block_n[i];
    }
    const int64_t N = r0[nb], E = e0[nb], nnz = at_jc[m];
    // Per-block storage (round 4): every dense operand is the concatenation of its diagonal blocks, memory and work ~ sum n_i^2.
    // Default from 16 blocks or N >= 4096 on; MSDP_MULTIBLOCK_BLOCKED = 0 / 1 forces the embedded N x N form / this one (tests).
    bool blocked = nb >= 16 || N >= 4096;
    if (const char* e = getenv("MSDP_MULTIBLOCK_BLOCKED")) { if (*e == '0') blocked = false; else if (*e == '1') blocked = true; }
    if (blocked) {
        if (N > 0x3fffffff) { msdp_set_error("multiblock: total order too large"); return MSDP_EUNSUPPORTED; }
        msdp_handle hb = nullptr;
        int rcb = new_handle(MSDP_KIND_UNITDIAG, N, &hb);
        if (rcb) return rcb;
        hb->d.costkind = COST_AFFINE;
        hb->d.m = m;
        if ((rcb = msdp_alloc_common(hb)) || (rcb = msdp_affine_setup_blocked(hb, nb, block_n, at_jc, at_ir, at_pr, b, c)) ||
            (rcb = msdp_alloc_vectors(hb, pcap > 0 ? pcap : 32))) { msdp_destroy(hb); return rcb; }
        hb->kind = MSDP_KIND_MULTIBLOCK;
        hb->mb_n.assign(block_n, block_n + nb); hb->mb_nob = nob;
        std::vector<unsigned char> rfb((size_t)N, 0);
        bool anyb = false;
        for (int i = nob; i < nb; ++i)
            for (int64_t a = r0[i]; a < r0[i + 1]; ++a) { rfb[(size_t)a] = 1; anyb = true; }
        if (anyb) {
            unsigned char* drf = nullptr;
            if ((rcb = msdp_dev_alloc<unsigned char>(hb, &drf, (size_t)N))) { msdp_destroy(hb); return rcb; }
            if (msdp_memcpy(drf, rfb.data(), (size_t)N, hipMemcpyHostToDevice) != hipSuccess) { msdp_set_error("multiblock: upload failed"); msdp_destroy(hb); return MSDP_EHIP; }
            hb->d.rowfree = drf;
        }
        *out = hb;
        return 0;
    }
    if (N > 46000) { msdp_set_error("multiblock: total order %lld too large for the embedded dense representation", (long long)N); return MSDP_EUNSUPPORTED; }
    // embed: entry (a, b) of block i -> entry (r0_i + a, r0_i + b) of the N x N direct sum (column-major vec index)
    auto embed = [&](int64_t e, int64_t* g) -> bool {
        if (e < 0 || e >= E) return false;
        const int i = (int)(std::upper_bound(e0.begin(), e0.end(), e) - e0.begin()) - 1;
        const int64_t l = e - e0[i], a = l % block_n[i], bb = l / block_n[i];
        *g = (r0[i] + a) + (r0[i] + bb) * N;
        return true;
    };
    std::vector<int64_t> ir((size_t)nnz);
    for (int64_t t = 0; t < nnz; ++t)
        if (!embed(at_ir[t], &ir[(size_t)t])) { msdp_set_error("multiblock: At row index out of range"); return MSDP_EINVAL; }
    std::vector<double> cN((size_t)N * N, 0.0);
    for (int i = 0; i < nb; ++i)
        for (int64_t bb = 0; bb < block_n[i]; ++bb)
            for (int64_t a = 0; a < block_n[i]; ++a)
                cN[(size_t)((r0[i] + a) + (r0[i] + bb) * N)] = c[e0[i] + a + bb * block_n[i]];
    msdp_handle h = nullptr;
    int rc = msdp_create_affine(MSDP_KIND_UNITDIAG, N, m, at_jc, ir.data(), at_pr, b, cN.data(), pcap, &h);
    if (rc) return rc;
    h->kind = MSDP_KIND_MULTIBLOCK;
    h->mb_n.assign(block_n, block_n + nb); h->mb_nob = nob;
    std::vector<unsigned char> rf((size_t)N, 0);
    bool any = false;
    for (int i = nob; i < nb; ++i)
        for (int64_t a = r0[i]; a < r0[i + 1]; ++a) { rf[(size_t)a] = 1; any = true; }
    if (any) {
        unsigned char* drf = nullptr;
        if ((rc = msdp_dev_alloc<unsigned char>(h, &drf, (size_t)N))) { msdp_destroy(h); return rc; }
        if (msdp_memcpy(drf, rf.data(), (size_t)N, hipMemcpyHostToDevice) != hipSuccess) { msdp_set_error("multiblock: upload failed"); msdp_destroy(h); return MSDP_EHIP; }
        h->d.rowfree = drf;
    }
    if (nb > 1) {                                          // block ranges per row: the dense contraction skips the zero off-diagonal blocks
        std::vector<int> lo((size_t)N), hi((size_t)N);
        for (int i = 0; i < nb; ++i)
            for (int64_t a = r0[i]; a < r0[i + 1]; ++a) { lo[(size_t)a] = (int)r0[i]; hi[(size_t)a] = (int)r0[i + 1]; }
        int *dlo = nullptr, *dhi = nullptr;
        if ((rc = msdp_dev_alloc<int>(h, &dlo, (size_t)N)) || (rc = msdp_dev_alloc<int>(h, &dhi, (size_t)N))) { msdp_destroy(h); return rc; }
        if (msdp_memcpy(dlo, lo.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
            msdp_memcpy(dhi, hi.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) { msdp_set_error("multiblock: upload failed"); msdp_destroy(h); return MSDP_EHIP; }
        h->d.blk_lo = dlo; h->d.blk_hi = dhi;
    }
    *out = h;
    return 0;
}


extern "C" int msdp_create_dual_unitdiag(int64_t n, int64_t m, const int64_t* at_jc, const int64_t* at_ir, const double* at_pr,
                                         const double* dAAt, const double* b, const double* c, int32_t nf, const int64_t* b_jc,
                                         const int64_t* b_ir, const double* b_pr, const double* cf, int32_t pcap, msdp_handle* out) {
    if (!at_jc || !at_ir || !at_pr || !dAAt || !b || !c || m <= 0) { msdp_set_error("dual_unitdiag: null/empty data"); return MSDP_EINVAL; }
    if (nf < 0 || (nf > 0 && (!b_jc || !b_ir || !b_pr || !cf))) { msdp_set_error("dual_unitdiag: bad free part"); return MSDP_EINVAL; }
    msdp_handle h = nullptr;
    int rc = msdp_create_affine(MSDP_KIND_UNITDIAG, n, m, at_jc, at_ir, at_pr, b, c, pcap, &h);
    if (rc) return rc;
    h->kind = MSDP_KIND_DUAL_UNITDIAG;
    if ((rc = msdp_dual_setup(h, at_jc, at_ir, at_pr, b, c, dAAt, nf, b_jc, b_ir, b_pr, cf, false))) { msdp_destroy(h); return rc; }
    *out = h;
    return 0;
}

// src/dual/ManiDSDP.m: the same data on the Euclidean factor (the affine generic kind's manifold and boundary)
extern "C" int msdp_create_dual(int64_t n, int64_t m, const int64_t* at_jc, const int64_t* at_ir, const double* at_pr,
                                const double* dAAt, const double* b, const double* c, int32_t nf, const int64_t* b_jc,
                                const int64_t* b_ir, const double* b_pr, const double* cf, int32_t pcap, msdp_handle* out) {
    if (!at_jc || !at_ir || !at_pr || !dAAt || !b || !c || m <= 0) { msdp_set_error("dual: null/empty data"); return MSDP_EINVAL; }
    if (nf < 0 || (nf > 0 && (!b_jc || !b_ir || !b_pr || !cf))) { msdp_set_error("dual: bad free part"); return MSDP_EINVAL; }
    msdp_handle h = nullptr;
    int rc = msdp_create_affine(MSDP_KIND_GENERIC, n, m, at_jc, at_ir, at_pr, b, c, pcap, &h);
    if (rc) return rc;
    h->kind = MSDP_KIND_DUAL;
    if ((rc = msdp_dual_setup(h, at_jc, at_ir, at_pr, b, c, dAAt, nf, b_jc, b_ir, b_pr, cf, true))) { msdp_destroy(h); return rc; }
    *out = h;
    return 0;
}

// src/dual/ManiDSDP_multiblock.m: the blocks of msdp_create_multiblock (per-block storage only, the first nob blocks unit-diagonal:
// oblique rows, the others Euclidean through the rowfree flag) with the dual data of msdp_create_dual
extern "C" int msdp_create_dual_multiblock(int32_t nb, const int64_t* block_n, int32_t nob, int64_t m, const int64_t* at_jc,
                                           const int64_t* at_ir, const double* at_pr, const double* dAAt, const double* b,
                                           const double* c, int32_t nf, const int64_t* b_jc, const int64_t* b_ir, const double* b_pr,
                                           const double* cf, int32_t pcap, msdp_handle* out) {
    if (nb < 1 || !block_n || nob < 0 || nob > nb) { msdp_set_error("dual_multiblock: bad block description"); return MSDP_EINVAL; }
    if (!at_jc || !at_ir || !at_pr || !dAAt || !b || !c || m <= 0 || !out) { msdp_set_error("dual_multiblock: null/empty data"); return MSDP_EINVAL; }
    if (nf < 0 || (nf > 0 && (!b_jc || !b_ir || !b_pr || !cf))) { msdp_set_error("dual_multiblock: bad free part"); return MSDP_EINVAL; }
    std::vector<int64_t> r0((size_t)nb + 1, 0);
    for (int i = 0; i < nb; ++i) {
        if (block_n[i] < 1) { msdp_set_error("dual_multiblock: block %d has order %lld", i, (long long)block_n[i]); return MSDP_EINVAL; }
        r0[(size_t)i + 1] = r0[(size_t)i] + block_n[i];
    }
    const int64_t N = r0[(size_t)nb];
    if (N > 0x3fffffff) { msdp_set_error("dual_multiblock: total order too large"); return MSDP_EUNSUPPORTED; }
    msdp_handle h = nullptr;
    int rc = new_handle(MSDP_KIND_UNITDIAG, N, &h);
    if (rc) return rc;
    h->d.costkind = COST_AFFINE;
    h->d.m = m;
    if ((rc = msdp_alloc_common(h)) || (rc = msdp_affine_setup_blocked(h, nb, block_n, at_jc, at_ir, at_pr, b, c)) ||
        (rc = msdp_alloc_vectors(h, pcap > 0 ? pcap : 32))) { msdp_destroy(h); return rc; }
    h->kind = MSDP_KIND_DUAL_MULTIBLOCK;
    h->mb_n.assign(block_n, block_n + nb); h->mb_nob = nob;
    if (nob < nb) {
        std::vector<unsigned char> rf((size_t)N, 0);
        for (int64_t a = r0[(size_t)nob]; a < N; ++a) rf[(size_t)a] = 1;
        unsigned char* drf = nullptr;
        if ((rc = msdp_dev_alloc<unsigned char>(h, &drf, (size_t)N))) { msdp_destroy(h); return rc; }
        if (msdp_memcpy(drf, rf.data(), (size_t)N, hipMemcpyHostToDevice) != hipSuccess) { msdp_set_error("dual_multiblock: upload failed"); msdp_destroy(h); return MSDP_EHIP; }
        h->d.rowfree = drf;
    }
    // nob == nb: the unit-diagonal dual kind's closures (tt = bA - sigma*As), otherwise the generic kind's
    if ((rc = msdp_dual_setup(h, at_jc, at_ir, at_pr, b, c, dAAt, nf, b_jc, b_ir, b_pr, cf, nob < nb)) ||
        (rc = msdp_dual_set_zrows(h, r0[(size_t)nob]))) { msdp_destroy(h); return rc; }
    *out = h;
    return 0;
}

extern "C" int msdp_dual_info(msdp_handle h, int32_t* g_identity) {
    MSDP_CHECK_H(h);
    if (!msdp_dual_kind(h) || !g_identity) { msdp_set_error("dual_info: not a dual handle / null out"); return MSDP_ESTATE; }
    *g_identity = msdp_dual_g_identity(h);
    return 0;
}

extern "C" int msdp_dual_set_penalty(msdp_handle h, double sigma, const double* w) {
    MSDP_CHECK_H(h);
    if (!msdp_dual_kind(h)) { msdp_set_error("dual_set_penalty: not a dual handle"); return MSDP_ESTATE; }
    h->state_valid = false;
    h->gradnorm_valid = false;
    h->chunk_len = 0;      // sigma is baked into the captured Hess-vec launches (both dual kinds): force a re-capture
    return msdp_dual_set_penalty_impl(h, sigma, w);
}

extern "C" int msdp_dual_outer_step(msdp_handle h, double* scal, double* Af, double* z) {
    MSDP_CHECK_H(h);
    if (!msdp_dual_kind(h)) { msdp_set_error("dual_outer_step: not a dual handle"); return MSDP_ESTATE; }
    if (!scal || (!z && h->kind == MSDP_KIND_DUAL_UNITDIAG)) { msdp_set_error("dual_outer_step: null argument"); return MSDP_EINVAL; }
    if (!h->have_point) { msdp_set_error("no resident point"); return MSDP_ESTATE; }
    h->state_valid = false;
    int rc = msdp_dual_outer_step_impl(h, scal, Af, z);
    h->dual_valid = (rc == 0);
    return rc;
}

extern "C" int msdp_dual_get_y(msdp_handle h, double* y) {
    MSDP_CHECK_H(h);
    if (!msdp_dual_kind(h) || !h->dual_valid || !y) { msdp_set_error("dual_get_y: call msdp_dual_outer_step first"); return MSDP_ESTATE; }
    return msdp_dual_get_y_impl(h, y);
}

extern "C" int msdp_destroy(msdp_handle h) {
    if (!h) return 0;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    msdp_comm_release(h);
    for (void* p : h->allocs) if (!msdp_uc_free(p)) (void)hipFree(p);
    for (int s2 = 0; s2 < 2; ++s2) if (h->ev_flag[s2]) (void)hipEventDestroy(h->ev_flag[s2]);
    for (int s2 = 0; s2 < 2; ++s2) if (h->chunk_execs[s2]) (void)hipGraphExecDestroy(h->chunk_execs[s2]);
    msdp_affine_release(h);
    msdp_densesym_release(h);
    msdp_window_release(h);
    msdp_block_eigs_release(h);
    msdp_halo_release(h);
    if (h->xr_paddr) (void)hipFree(h->xr_paddr);
    msdp_local_leave(h);
    if (h->lc_tmp) (void)hipFree(h->lc_tmp);
    if (h->esc_rp) (void)hipFree(h->esc_rp);
    if (h->esc_ci) (void)hipFree(h->esc_ci);
    if (h->esc_cv) (void)hipFree(h->esc_cv);
    if (h->esc_z) (void)hipFree(h->esc_z);
    msdp_escape_workspace_park(h->esc_mem, h->esc_cap);      // esc_prev lives inside it; kept for the next handle of the process
    if (h->lz_slots && !msdp_uc_free(h->lz_slots)) (void)hipFree(h->lz_slots);
    msdp_blockeig_release(h);
    if (h->esc_top) (void)hipFree(h->esc_top);
    if (h->xr_ev) (void)hipEventDestroy(h->xr_ev);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    msdp_host_kit_give(h);                                         // the stream and the pinned control blocks: to the next handle of the process
    delete h;
    return 0;
}

extern "C" int msdp_set_multipliers(msdp_handle h, const double* y, double sigma) {
    MSDP_CHECK_H(h);
    if (h->d.costkind != COST_AFFINE) { msdp_set_error("set_multipliers: handle has no affine constraints"); return MSDP_ESTATE; }
    if (msdp_dual_kind(h)) { msdp_set_error("set_multipliers: dual handles take msdp_dual_set_penalty"); return MSDP_ESTATE; }
    h->state_valid = false;
    h->chunk_len = 0;      // sigma is baked into the captured launches: force a re-capture
    return msdp_affine_set_multipliers(h, y, sigma);
}

// ------------------------------------------------------------------ point I/O

// Stage a boundary-layout host matrix (local rows) into a device vector.
static int upload_rows(msdp_handle h, const double* host, double* dst) {
    Dev& d = h->d;
    const size_t cnt = (size_t)d.n_loc * d.p;
    double* stage = nullptr;
    hipError_t e = hipMalloc((void**)&stage, (cnt ? cnt : 1) * sizeof(double));
    if (e != hipSuccess) { msdp_set_error("staging alloc failed"); return MSDP_ENOMEM; }
    int rc = 0;
    if (boundary_colmajor(h)) {
        // n x p column-major; each rank reads its row block of every column
        if (h->nranks == 1) {
            e = msdp_memcpy_async(stage, host, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream);
        } else {
            e = msdp_memcpy2d_async(stage, (size_t)d.n_loc * sizeof(double), host + d.row0, (size_t)d.n * sizeof(double),
                                 (size_t)d.n_loc * sizeof(double), d.p, hipMemcpyHostToDevice, h->stream);
        }
    } else {
        e = msdp_memcpy_async(stage, host + (size_t)d.row0 * d.p, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream);
    }
    if (e != hipSuccess) { msdp_set_error("H2D copy failed: %s", hipGetErrorString(e)); rc = MSDP_EHIP; }
    if (!rc) rc = msdp_k_pack(h, stage, dst, d.n_loc, d.p, d.ld, boundary_colmajor(h));
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(stage);
    return rc;
}

static int download_rows(msdp_handle h, const double* src, double* host) {
    Dev& d = h->d;
    const size_t cnt = (size_t)d.n_loc * d.p;
    double* stage = nullptr;
    hipError_t e = hipMalloc((void**)&stage, (cnt ? cnt : 1) * sizeof(double));
    if (e != hipSuccess) { msdp_set_error("staging alloc failed"); return MSDP_ENOMEM; }
    int rc = msdp_k_unpack(h, src, stage, d.n_loc, d.p, d.ld, boundary_colmajor(h));
    if (!rc) {
        if (boundary_colmajor(h) && h->nranks > 1)
            e = msdp_memcpy2d_async(host + d.row0, (size_t)d.n * sizeof(double), stage, (size_t)d.n_loc * sizeof(double),
                                 (size_t)d.n_loc * sizeof(double), d.p, hipMemcpyDeviceToHost, h->stream);
        else
            e = msdp_memcpy_async(host + (boundary_colmajor(h) ? 0 : (size_t)d.row0 * d.p), stage, cnt * sizeof(double),
                               hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess) { msdp_set_error("D2H copy failed: %s", hipGetErrorString(e)); rc = MSDP_EHIP; }
    }
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(stage);
    return rc;
}

extern "C" int msdp_set_point(msdp_handle h, int32_t p, const double* Y) {
    MSDP_CHECK_H(h);
    if (p < 1 || !Y) { msdp_set_error("set_point: p = %d, Y = %p", p, (const void*)Y); return MSDP_EINVAL; }
    if (p > 1024) { msdp_set_error("factor width p = %d exceeds the supported maximum of 1024", p); return MSDP_EUNSUPPORTED; }
    Dev& d = h->d;
    if (d.manifold == MANI_STIEFEL && p > MSDP_BLOCK_PMAX) { msdp_set_error("set_point: a %s handle holds factor widths up to %d (p = %d)", msdp_block_kind_name(d.efree), MSDP_BLOCK_PMAX, p); return MSDP_EUNSUPPORTED; }
    if (d.costkind == COST_HERM && (p & 1)) { msdp_set_error("set_point: a Hermitian handle takes the real view of a complex factor, an even width (p = %d)", p); return MSDP_EINVAL; }
    if (p > h->pcap) {
        int rc = msdp_alloc_vectors(h, p + 16);
        if (rc) return rc;
    }
    d.p = p;
    d.ld = ((p + 1) / 2) * 2;
    if (!h->use_comm && h->nranks == 1) d.full = d.md;   // overwritten per launch by allgather_rows
    choose_grid(h);
    if (!msdp_cost_sparse_rows(d.costkind)) {
        int rc = msdp_dense_reserve(h, d.costkind == COST_AFFINE ? 2 : 1);
        if (rc) return rc;
    }
    h->h_ctl->cur = 0;
    // zero the slot so pad columns and pad rows are exactly zero
    HIPCHK(hipMemsetAsync(d.Y[0], 0, (size_t)msdp_rows_capacity(h) * h->ldcap * sizeof(double), h->stream));
    HIPCHK(hipMemsetAsync(d.Y[1], 0, (size_t)msdp_rows_capacity(h) * h->ldcap * sizeof(double), h->stream));
    int rc = upload_rows(h, Y, d.Y[0]);
    if (rc) return rc;
    h->have_point = true;
    h->state_valid = false;
    h->gradnorm_valid = false;
    return 0;
}


// The resident point has been rewritten into slot `slot` with width p: make it the current one
static int adopt_point(msdp_handle h, int slot, int p) {
    Dev& d = h->d;
    d.p = p;
    d.ld = ((p + 1) / 2) * 2;
    if (!h->use_comm && h->nranks == 1) d.full = d.md;
    choose_grid(h);
    if (!msdp_cost_sparse_rows(d.costkind)) {
        int rc = msdp_dense_reserve(h, d.costkind == COST_AFFINE ? 2 : 1);
        if (rc) return rc;
    }
    h->h_ctl->cur = slot;
    h->state_valid = false;
    h->gradnorm_valid = false;
    return 0;
}
// (for the re-shaping calls of the block kinds, msdp_blockfactor.hip)
int msdp_adopt_point(msdp_handle h, int slot, int p) { return adopt_point(h, slot, p); }

extern "C" int msdp_factor_gram(msdp_handle h, double* G) {
    MSDP_CHECK_H(h);
    if (h->d.costkind == COST_HERM) { msdp_set_error("factor_gram: not for a Hermitian handle (the rank cut of a complex factor stays on the host)"); return MSDP_EUNSUPPORTED; }
    if (h->d.manifold == MANI_STIEFEL) { msdp_set_error("factor_gram: not for a %s handle (the rank cut and the re-orthonormalisation of the blocks stay on the host)", msdp_block_kind_name(h->d.efree)); return MSDP_EUNSUPPORTED; }
    if (!h->have_point || !G) { msdp_set_error("factor_gram: no resident point / null out"); return MSDP_ESTATE; }
    Dev& d = h->d;
    const int ld = d.ld, p = d.p;
    int nblk = (int)std::min<int64_t>(64, std::max<int64_t>(1, (int64_t)(1 << 22) / ((int64_t)ld * ld)));
    double* buf = nullptr;
    if (hipMalloc((void**)&buf, ((size_t)nblk + 1) * ld * ld * sizeof(double)) != hipSuccess) { msdp_set_error("factor_gram: scratch alloc failed"); return MSDP_ENOMEM; }
    double* out = buf + (size_t)nblk * ld * ld;
    int rc = msdp_k_fgram(h, d.Y[msdp_host_cur(h)], buf, nblk, out);
    if (!rc && h->use_comm) rc = msdp_allreduce_array(h, out, (size_t)ld * ld);
    if (!rc && msdp_memcpy2d_async(G, (size_t)p * sizeof(double), out, (size_t)ld * sizeof(double), (size_t)p * sizeof(double), p,
                                hipMemcpyDeviceToHost, h->stream) != hipSuccess) { msdp_set_error("factor_gram: D2H failed"); rc = MSDP_EHIP; }
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(buf);
    return rc;
}

extern "C" int msdp_factor_rotate(msdp_handle h, int32_t r, const double* Q) {
    MSDP_CHECK_H(h);
    if (h->d.costkind == COST_HERM) { msdp_set_error("factor_rotate: not for a Hermitian handle (the rank cut of a complex factor stays on the host)"); return MSDP_EUNSUPPORTED; }
    if (h->d.manifold == MANI_STIEFEL) { msdp_set_error("factor_rotate: not for a %s handle (the rank cut and the re-orthonormalisation of the blocks stay on the host)", msdp_block_kind_name(h->d.efree)); return MSDP_EUNSUPPORTED; }
    if (!h->have_point || !Q) { msdp_set_error("factor_rotate: no resident point / null Q"); return MSDP_ESTATE; }
    Dev& d = h->d;
    if (r < 1 || r > d.p) { msdp_set_error("factor_rotate: r = %d outside 1..p = %d", r, d.p); return MSDP_EINVAL; }
    const int cur = msdp_host_cur(h), ldn = ((r + 1) / 2) * 2;
    double* qd = nullptr;
    if (hipMalloc((void**)&qd, (size_t)d.p * r * sizeof(double)) != hipSuccess) { msdp_set_error("factor_rotate: scratch alloc failed"); return MSDP_ENOMEM; }
    int rc = 0;
    if (msdp_memcpy_async(qd, Q, (size_t)d.p * r * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess) { msdp_set_error("factor_rotate: H2D failed"); rc = MSDP_EHIP; }
    if (!rc) rc = msdp_k_frotate(h, msdp_rows_capacity(h), r, ldn, d.Y[cur], qd, d.Y[cur ^ 1]);
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(qd);
    if (rc) return rc;
    return adopt_point(h, cur ^ 1, r);
}

extern "C" int msdp_factor_append(msdp_handle h, int32_t k, const double* V, double alpha, int32_t normalize) {
    MSDP_CHECK_H(h);
    if (h->d.costkind == COST_HERM) { msdp_set_error("factor_append: not for a Hermitian handle (the rank cut of a complex factor stays on the host)"); return MSDP_EUNSUPPORTED; }
    if (h->d.manifold == MANI_STIEFEL) { msdp_set_error("factor_append: not for a %s handle (the rank cut and the re-orthonormalisation of the blocks stay on the host)", msdp_block_kind_name(h->d.efree)); return MSDP_EUNSUPPORTED; }
    if (!h->have_point || !V) { msdp_set_error("factor_append: no resident point / null V"); return MSDP_ESTATE; }
    Dev& d = h->d;
    if (k < 1) { msdp_set_error("factor_append: k = %d", k); return MSDP_EINVAL; }
    if (d.p + k > h->pcap) { msdp_set_error("factor_append: width %d exceeds the allocated capacity %d (use msdp_set_point)", d.p + k, h->pcap); return MSDP_EUNSUPPORTED; }
    if (d.manifold != MANI_OBLIQUE && normalize) { msdp_set_error("factor_append: row normalisation is the oblique kinds'"); return MSDP_EUNSUPPORTED; }
    const int cur = msdp_host_cur(h), pn = d.p + k, ldn = ((pn + 1) / 2) * 2;
    double* vd = nullptr;
    if (hipMalloc((void**)&vd, (size_t)std::max(d.n_loc, 1) * k * sizeof(double)) != hipSuccess) { msdp_set_error("factor_append: scratch alloc failed"); return MSDP_ENOMEM; }
    int rc = 0;
    // my rows of every column of the n x k column-major V
    if (msdp_memcpy2d_async(vd, (size_t)d.n_loc * sizeof(double), V + d.row0, (size_t)d.n * sizeof(double), (size_t)d.n_loc * sizeof(double), k,
                         hipMemcpyHostToDevice, h->stream) != hipSuccess) { msdp_set_error("factor_append: H2D failed"); rc = MSDP_EHIP; }
    if (!rc) rc = msdp_k_fappend(h, msdp_rows_capacity(h), k, ldn, d.Y[cur], vd, alpha, normalize, d.Y[cur ^ 1]);
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(vd);
    if (rc) return rc;
    return adopt_point(h, cur ^ 1, pn);
}

// Rank cut and escape widening of all blocks of a multiblock factor (msdp_blockreshape.hip); every check before any launch.
extern "C" int msdp_block_reshape(msdp_handle h, int32_t nb, const int64_t* row0, const int64_t* nblk, const int32_t* p_in,
                                  const double* w, const double* V, int32_t k, double theta, int32_t strict, int32_t delta,
                                  double alpha, int32_t min_facsize, int32_t mode,
                                  int32_t* p_out, int32_t* r_out, int32_t* nne_out, double* U) {
    MSDP_CHECK_H(h);
    if (nb < 1 || !row0 || !nblk || !p_in || !w || k < 0 || k > 64 || (k > 0 && !V) || delta < 0 || delta > k || (mode != 0 && mode != 1) ||
        (mode == 1 && !U) || !p_out || !r_out || !nne_out) { msdp_set_error("block_reshape: bad argument"); return MSDP_EINVAL; }
    if (h->kind != MSDP_KIND_MULTIBLOCK && h->kind != MSDP_KIND_DUAL_MULTIBLOCK) { msdp_set_error("block_reshape: the multiblock kinds only"); return MSDP_EUNSUPPORTED; }
    if (h->nranks > 1 || h->use_comm) { msdp_set_error("block_reshape: not on a row-sharded handle"); return MSDP_EUNSUPPORTED; }
    if ((size_t)nb != h->mb_n.size()) { msdp_set_error("block_reshape: %d blocks given, the handle has %zu (all blocks, in order)", nb, h->mb_n.size()); return MSDP_EINVAL; }
    int64_t at = 0;
    for (int b = 0; b < nb; ++b) {
        if (row0[b] != at || nblk[b] != h->mb_n[(size_t)b]) { msdp_set_error("block_reshape: block %d is not block %d of the handle (all blocks, in order)", b, b); return MSDP_EINVAL; }
        at += nblk[b];
    }
    if (!h->have_point) { msdp_set_error("block_reshape: no resident point"); return MSDP_ESTATE; }
    Dev& d = h->d;
    const int maxp = msdp_block_reshape_maxp();
    for (int b = 0; b < nb; ++b) {
        if (p_in[b] < 1 || p_in[b] > d.p) { msdp_set_error("block_reshape: width %d of block %d outside 1..p = %d", p_in[b], b, d.p); return MSDP_EINVAL; }
        if (nblk[b] >= min_facsize && p_in[b] > maxp) { msdp_set_error("block_reshape: block widths up to %d (block %d has %d)", maxp, b, p_in[b]); return MSDP_EUNSUPPORTED; }
    }
    const int cur = msdp_host_cur(h);
    int pn = 0;
    int rc = msdp_block_reshape_run(h, cur, nb, nblk, p_in, w, V, k, theta, strict, delta, alpha, min_facsize, mode, h->mb_nob, p_out, r_out, nne_out, &pn);
    if (rc) return rc;
    if (mode == 1) {                                       // U_i = [0, V_i(:, 1:nne_i)] in the boundary layout of the new point (:137-141)
        std::fill(U, U + (size_t)d.n * pn, 0.0);
        int64_t r = 0;
        for (int b = 0; b < nb; ++b) {
            const int c0 = p_out[b] - nne_out[b];
            for (int64_t i = 0; i < nblk[b]; ++i)
                for (int c = 0; c < nne_out[b]; ++c) U[(size_t)(r + i) * pn + c0 + c] = V[(size_t)(r + i) * k + c];
            r += nblk[b];
        }
    }
    return adopt_point(h, cur ^ 1, pn);
}

// Device-side copy of the resident point and back: lets a caller restart from the same point without another PCIe
// upload (bench.py: the start point of every timed step is already in HBM).
extern "C" int msdp_point_snapshot(msdp_handle h) {
    MSDP_CHECK_H(h);
    if (!h->have_point) { msdp_set_error("no resident point"); return MSDP_ESTATE; }
    const size_t cnt = (size_t)msdp_rows_capacity(h) * h->ldcap;
    if (h->snap_cap < cnt) {
        if (h->snap) msdp_dev_free(h, h->snap);
        h->snap = nullptr; h->snap_cap = 0;
        int rc = msdp_dev_alloc<double>(h, &h->snap, cnt);
        if (rc) return rc;
        h->snap_cap = cnt;
    }
    HIPCHK(msdp_memcpy_async(h->snap, h->d.Y[msdp_host_cur(h)], cnt * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->snap_p = h->d.p;
    return 0;
}
extern "C" int msdp_point_restore(msdp_handle h) {
    MSDP_CHECK_H(h);
    if (!h->snap || h->snap_p != h->d.p || !h->have_point) { msdp_set_error("point_restore: no snapshot of the current width"); return MSDP_ESTATE; }
    const size_t cnt = (size_t)msdp_rows_capacity(h) * h->ldcap;
    h->h_ctl->cur = 0;
    HIPCHK(msdp_memcpy_async(h->d.Y[0], h->snap, cnt * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    h->state_valid = false;
    h->gradnorm_valid = false;
    return 0;
}

extern "C" int msdp_get_point(msdp_handle h, double* Y) {
    MSDP_CHECK_H(h);
    if (!h->have_point) { msdp_set_error("no resident point"); return MSDP_ESTATE; }
    return download_rows(h, h->d.Y[msdp_host_cur(h)], Y);
}

// Test-only: eta and Heta as the LAST tCG solve of msdp_rtr left them (tCG.m:95: [eta, Heta, ...] = tCG(...)); meaningful after
// a call with maxiter = 1 on the paths that hand the step over through global memory (chunked path, persistent kernel with the
// option fused_rtr = 0).  tCG keeps Heta = Hess(eta) by linearity (tCG.m:192-220); tests/test_gpu_onlyunitdiag.py bounds the
// deviation of the persistent kernel, whose Hess-vecs are assembled as C*r_new + beta*C*mdelta_old (msdp_persist.hip, TWOSYNC).
extern "C" int msdp_debug_get_tcg_step(msdp_handle h, double* eta, double* Heta) {
    MSDP_CHECK_H(h);
    if (!h->have_point || !eta || !Heta) { msdp_set_error("debug_get_tcg_step: no resident point / null out"); return MSDP_ESTATE; }
    Frame f;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(msdp_memcpy(&f, &h->d.F[0], sizeof(Frame), hipMemcpyDeviceToHost));
    const int ix = f.eta_idx ? 1 : 0;
    int rc = download_rows(h, h->d.eta[ix], eta);
    if (!rc) rc = download_rows(h, h->d.Heta[ix], Heta);
    return rc;
}

// Every row of the resident point on every rank (one all-gather, then the download): the host loops of the row-sharded
// affine kinds run replicated on all ranks and need identical inputs for their rank / escape decisions.
extern "C" int msdp_get_point_all(msdp_handle h, double* Y) {
    MSDP_CHECK_H(h);
    if (!h->have_point || !Y) { msdp_set_error("get_point_all: no resident point / null out"); return MSDP_ESTATE; }
    if (h->nranks == 1 && !h->use_comm) return download_rows(h, h->d.Y[msdp_host_cur(h)], Y);
    if (!h->use_comm) { msdp_set_error("get_point_all: needs a communicator"); return MSDP_ESTATE; }
    Dev& d = h->d;
    int rc = msdp_allgather_rows(h, d.Y[msdp_host_cur(h)]);
    if (rc) return rc;
    const size_t cnt = (size_t)d.n * d.p;
    double* stage = nullptr;
    if (hipMalloc((void**)&stage, (cnt ? cnt : 1) * sizeof(double)) != hipSuccess) { msdp_set_error("staging alloc failed"); return MSDP_ENOMEM; }
    rc = msdp_k_unpack(h, h->full_buf, stage, d.n, d.p, d.ld, boundary_colmajor(h));
    if (!rc && msdp_memcpy_async(Y, stage, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess) { msdp_set_error("D2H copy failed"); rc = MSDP_EHIP; }
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(stage);
    return rc;
}

extern "C" int msdp_get_p(msdp_handle h, int32_t* p) {
    MSDP_CHECK_H(h);
    if (!p) return MSDP_EINVAL;
    *p = h->d.p;
    return 0;
}

// The plans of the symmetric contraction follow the dense_sym* options: reserve again where a dense operand is resident
static int dense_rereserve(msdp_handle h) {
    return (h->have_point && !msdp_cost_sparse_rows(h->d.costkind) && !h->blocked) ? msdp_dense_reserve(h, h->d.costkind == COST_AFFINE ? 2 : 1) : 0;
}

extern "C" int msdp_set_option(msdp_handle h, const char* name, int32_t value) {
    MSDP_CHECK_H(h);
    if (!name) { msdp_set_error("set_option: null name"); return MSDP_EINVAL; }
    Tuning& t = h->tune;
    if (!strcmp(name, "persist")) t.persist = value != 0;
    else if (!strcmp(name, "fused_rtr")) t.fused_rtr = value != 0;
    else if (!strcmp(name, "graph")) { t.graph = value != 0; h->chunk_len = 0; }
    else if (!strcmp(name, "affine_route")) { if (value < 0 || value > 2) { msdp_set_error("affine_route: 0 auto, 1 sddmm, 2 gram"); return MSDP_EINVAL; } t.affine_route = value; h->chunk_len = 0; h->state_valid = false; }
    else if (!strcmp(name, "timing")) t.timing = value != 0;
    else if (!strcmp(name, "esc_debug")) t.esc_debug = value != 0;
    else if (!strcmp(name, "escape_deflate")) t.escape_deflate = value != 0;
    else if (!strcmp(name, "escape_warm")) t.escape_warm = value != 0;
    else if (!strcmp(name, "escape_start_y")) t.escape_start_y = value != 0;
    else if (!strcmp(name, "xpersist")) t.xpersist = value != 0;
    else if (!strcmp(name, "persist_refresh")) t.persist_refresh = value > 0 ? value : 0;
    else if (!strcmp(name, "xtail")) t.xtail = value ? 1 : 0;
    else if (!strcmp(name, "xr_twolevel")) t.xr_twolevel = value ? 1 : 0;
    else if (!strcmp(name, "window")) { t.window = value < 0 ? 0 : (value > 3 ? 3 : value); h->chunk_len = 0; }
    else if (!strcmp(name, "window_lds")) { t.window_lds = value < 16 ? 16 : (value > 144 ? 144 : value); h->chunk_len = 0; msdp_window_release(h); }
    else if (!strcmp(name, "persist_early")) t.persist_early = value > 0 ? value : 0;
    else if (!strcmp(name, "persist_pipe")) t.persist_pipe = value > 0 ? 1 : 0;
    else if (!strcmp(name, "pipe_refresh")) t.pipe_refresh = value > 0 ? (value < 2 ? 2 : value) : 0;   // (1 would store the refresh rows of trip j + 1 into the regions a slower workgroup still gathers those of trip j from: msdp_pipe.h)
    else if (!strcmp(name, "pipe_local")) t.pipe_local = value > 0 ? 1 : 0;
    else if (!strcmp(name, "pipe_own")) t.pipe_own = value > 0 ? 1 : 0;
    else if (!strcmp(name, "pipe_wide")) t.pipe_wide = value > 0 ? 1 : 0;
    else if (!strcmp(name, "persist_goff")) t.persist_goff = value ? 1 : 0;
    else if (!strcmp(name, "persist_ep")) { t.persist_ep = value ? 1 : 0; h->d.persist_ep = t.persist_ep; h->persist_sig_fn = nullptr; }
    else if (!strcmp(name, "persist_slots")) { t.persist_slots = (value == 3 || value == 4) ? value : 0; h->d.persist_slots = t.persist_slots; }
    else if (!strcmp(name, "psync_backoff")) t.psync_backoff = value > 0 ? value : 0;
    else if (!strcmp(name, "psync8_backoff")) t.psync8_backoff = value > 0 ? (value > 255 ? 255 : value) : 0;
    else if (!strcmp(name, "affine_overlap")) { t.affine_overlap = value != 0; h->chunk_len = 0; }
    else if (!strcmp(name, "trip1")) { t.trip1 = value < 0 ? 0 : (value > 2 ? 2 : value); h->chunk_len = 0; }
    else if (!strcmp(name, "dense_sk")) t.dense_sk = value < 0 ? 0 : value;
    else if (!strcmp(name, "sweep_k")) { t.sweep_k = value < 1 ? 1 : value; choose_grid(h); h->chunk_len = 0; }
    else if (!strcmp(name, "sweep")) { t.sweep = value < 0 ? 0 : (value > 3 ? 3 : value); choose_grid(h); h->chunk_len = 0; }
    else if (!strcmp(name, "trip2")) { t.trip2 = value < 0 ? 0 : (value > 2 ? 2 : value); h->chunk_len = 0; }
    else if (!strcmp(name, "escape_method")) { if (value < 0 || value > 2) { msdp_set_error("escape_method: 0 auto, 1 lanczos, 2 block"); return MSDP_EINVAL; } t.escape_method = value; }
    else if (!strcmp(name, "escape_rr")) { if (value != 0 && value != 1) { msdp_set_error("escape_rr: 0 host, 1 device"); return MSDP_EINVAL; } t.escape_rr = value; }
    else if (!strcmp(name, "be_width")) { if (value != 0 && value != 32 && value != 64 && value != 128) { msdp_set_error("be_width: 0, 32, 64 or 128"); return MSDP_EINVAL; } t.be_width = value; }
    else if (!strcmp(name, "be_degree")) t.be_degree = value > 0 ? value : 0;
    else if (!strcmp(name, "be_grid")) t.be_grid = value > 0 ? (value > MSDP_MAX_GRID ? MSDP_MAX_GRID : value) : 0;
    else if (!strcmp(name, "be_lpr")) { if (value != 0 && value != 8 && value != 16 && value != 32 && value != 64) { msdp_set_error("be_lpr: 0, 8, 16, 32 or 64"); return MSDP_EINVAL; } t.be_lpr = value; }
    else if (!strcmp(name, "lanczos_onesync")) t.lanczos_onesync = value != 0;
    else if (!strcmp(name, "lanczos_qglobal")) t.lanczos_qglobal = value != 0;
    else if (!strcmp(name, "block_skip")) t.block_skip = value != 0;
    else if (!strcmp(name, "halo_exchange")) { t.halo_exchange = value != 0; h->state_valid = false; }
    else if (!strcmp(name, "dense_pack")) { t.dense_pack = value != 0; h->chunk_len = 0; }
    else if (!strcmp(name, "affine_fuse")) { t.affine_fuse = value != 0; h->chunk_len = 0; h->state_valid = false; }
    else if (!strcmp(name, "affine_side")) { t.affine_side = value != 0; h->chunk_len = 0; }
    else if (!strcmp(name, "affine_broute")) { t.affine_broute = value != 0; h->chunk_len = 0; }
    else if (!strcmp(name, "dense_sym")) { t.dense_sym = value < 0 ? 0 : (value > 2 ? 2 : value); h->chunk_len = 0; return dense_rereserve(h); }
    else if (!strcmp(name, "dense_sym_min")) { t.dense_sym_min = value > 0 ? value : 0; h->chunk_len = 0; return dense_rereserve(h); }
    else if (!strcmp(name, "dense_sym_res")) { t.dense_sym_res = value > 0 ? value : 0; h->chunk_len = 0; return dense_rereserve(h); }
    else if (!strcmp(name, "dense_sym_rt")) { t.dense_sym_rt = (value >= 1 && value <= 4) ? value : 0; h->chunk_len = 0; return dense_rereserve(h); }
    else if (!strcmp(name, "dense_sym_db")) { t.dense_sym_db = (value >= 0 && value <= 2) ? value : 0; h->chunk_len = 0; }
    else if (!strcmp(name, "dense_sym_len")) { t.dense_sym_len = value > 0 ? value : 0; h->chunk_len = 0; return dense_rereserve(h); }
    else if (!strcmp(name, "blk_groups")) t.blk_groups = value > 0 ? (value > 16 ? 16 : value) : 0;
    else if (!strcmp(name, "debug_fail_persist")) t.fail_persist = value != 0;
    else if (!strcmp(name, "block_persist")) { if (value < 0 || value > 1) { msdp_set_error("block_persist: 0 or 1"); return MSDP_EINVAL; } t.block_persist = value; }
    else if (!strcmp(name, "block_persist_grid")) t.block_persist_grid = value > 0 ? value : 0;
    else if (!strcmp(name, "block_persist_wide")) t.block_persist_wide = value != 0;
    else if (!strcmp(name, "precon")) {
        if (value < 0 || value > 1) { msdp_set_error("precon: 0 or 1"); return MSDP_EINVAL; }
        return msdp_pose_precon_set(h, value);             // (d.pcM is part of the chunk graph's signature: the graph is captured again)
    }
    else if (!strcmp(name, "round_order")) {
        if (value != 0 && value != 1) { msdp_set_error("round_order: 0 index order, 1 colour order"); return MSDP_EINVAL; }
        int rc = value ? msdp_round_color_check(h, "round_order") : 0;
        if (rc) return rc;
        t.round_order = value;
    }
    else if (!strcmp(name, "debug_xr_skip")) t.fail_xr = value != 0;
    else if (!strcmp(name, "debug_fail_block")) t.fail_block = value != 0;
    else if (!strcmp(name, "grid")) { t.grid = value > 0 ? value : 0; choose_grid(h); h->chunk_len = 0; }
    else { msdp_set_error("set_option: unknown option '%s'", name); return MSDP_EINVAL; }
    return 0;
}

extern "C" int msdp_get_kind(msdp_handle h, int32_t* kind) {
    MSDP_CHECK_H(h);
    if (!kind) return MSDP_EINVAL;
    *kind = h->kind;
    return 0;
}

// ------------------------------------------------------------------ fine-grained ops
int msdp_ensure_state(msdp_handle h) {
    if (!h->have_point) { msdp_set_error("no resident point"); return MSDP_ESTATE; }
    (void)msdp_window_eligible(h);                                 // (patch plan of the LDS-staged S*U: built here, outside any graph capture)
    if (h->state_valid) return 0;
    h->h_ctl->done = 0;
    h->h_ctl->bench_mode = 0;
    int rc = msdp_push_ctl(h);
    if (rc) return rc;
    if ((rc = msdp_launch_costgrad(h, msdp_host_cur(h)))) return rc;
    h->state_valid = true;
    return 0;
}

extern "C" int msdp_cost(msdp_handle h, double* f) {
    MSDP_CHECK_H(h);
    if (!f) return MSDP_EINVAL;
    int rc = msdp_ensure_state(h);
    if (rc) return rc;
    // re-run the reduction of the stored partials only if they are still those of the
    // resident point; simplest is to recompute the cost
    h->h_ctl->done = 0;
    if ((rc = msdp_push_ctl(h))) return rc;
    if ((rc = msdp_launch_costgrad(h, msdp_host_cur(h)))) return rc;
    if ((rc = msdp_k_sum_to(h, P_F, &h->d.ctl->fx))) return rc;
    double v = 0.0;
    HIPCHK(msdp_memcpy_async(&v, &h->d.ctl->fx, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *f = v;
    return 0;
}

extern "C" int msdp_rgrad(msdp_handle h, double* G) {
    MSDP_CHECK_H(h);
    int rc = msdp_ensure_state(h);
    if (rc) return rc;
    return download_rows(h, h->d.Gr[msdp_host_cur(h)], G);
}

extern "C" int msdp_hessvec(msdp_handle h, const double* U, double* H) {
    MSDP_CHECK_H(h);
    int rc = msdp_ensure_state(h);
    if (rc) return rc;
    if ((rc = upload_rows(h, U, h->d.md))) return rc;
    if ((rc = msdp_k_set_active(h, 1))) return rc;
    if ((rc = msdp_launch_hess(h))) return rc;
    if ((rc = msdp_k_set_active(h, 0))) return rc;
    return download_rows(h, h->d.Hmd, H);
}

extern "C" int msdp_proj(msdp_handle h, const double* U, double* V) {
    MSDP_CHECK_H(h);
    if (!h->have_point) { msdp_set_error("no resident point"); return MSDP_ESTATE; }
    int rc = upload_rows(h, U, h->d.W0);
    if (rc) return rc;
    if (h->d.manifold == MANI_OBLIQUE) rc = msdp_k_proj_obl(h, h->d.Y[msdp_host_cur(h)], h->d.W0, h->d.W1);
    else if (h->d.manifold == MANI_STIEFEL) rc = msdp_stiefel_proj(h, h->d.Y[msdp_host_cur(h)], h->d.W0, h->d.W1);
    else rc = msdp_sphere_proj(h, h->d.Y[msdp_host_cur(h)], h->d.W0, h->d.W1);
    if (rc) return rc;
    return download_rows(h, h->d.W1, V);
}

// Z = tangent_Y(blockdiag(M_i^-1) R) at the resident point of a pose-graph handle with the option "precon" set
extern "C" int msdp_precon_apply(msdp_handle h, const double* R, double* Z) {
    MSDP_CHECK_H(h);
    if (!R || !Z) { msdp_set_error("precon_apply: null array"); return MSDP_EINVAL; }
    if (!h->d.pcM) { msdp_set_error("precon_apply: the option \"precon\" is not set on this handle"); return MSDP_ESTATE; }
    if (!h->have_point) { msdp_set_error("no resident point"); return MSDP_ESTATE; }
    int rc = upload_rows(h, R, h->d.W0);
    if (rc) return rc;
    if ((rc = msdp_pose_precon_apply(h, h->d.Y[msdp_host_cur(h)], h->d.W0, h->d.W1))) return rc;
    return download_rows(h, h->d.W1, Z);
}

extern "C" int msdp_retr(msdp_handle h, const double* U, double* Z) {
    MSDP_CHECK_H(h);
    if (!h->have_point) { msdp_set_error("no resident point"); return MSDP_ESTATE; }
    int rc = upload_rows(h, U, h->d.W0);
    if (rc) return rc;
    if (h->d.manifold == MANI_OBLIQUE) rc = msdp_k_retr_obl(h, h->d.Y[msdp_host_cur(h)], h->d.W0, h->d.W1, 1.0);
    else if (h->d.manifold == MANI_STIEFEL) rc = msdp_stiefel_retr(h, h->d.Y[msdp_host_cur(h)], h->d.W0, h->d.W1, 1.0);
    else rc = msdp_sphere_retr(h, h->d.Y[msdp_host_cur(h)], h->d.W0, h->d.W1, 1.0);
    if (rc) return rc;
    return download_rows(h, h->d.W1, Z);
}

extern "C" int msdp_get_z(msdp_handle h, double* z) {
    MSDP_CHECK_H(h);
    if (h->kind != MSDP_KIND_ONLYUNITDIAG) { msdp_set_error("get_z: only for onlyunitdiag handles"); return MSDP_EUNSUPPORTED; }
    int rc = msdp_ensure_state(h);
    if (rc) return rc;
    HIPCHK(msdp_memcpy_async(z + h->d.row0, h->d.eG[msdp_host_cur(h)], (size_t)h->d.n_loc * sizeof(double),
                          hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// The multiplier blocks Lambda_i = sym((C Y)_i Y_i') of a unit-block-diagonal handle at the resident point (a pose-graph handle:
// of its rotation rows, d x d with d = blk - efree)
extern "C" int msdp_get_blockmult(msdp_handle h, double* Lam) {
    MSDP_CHECK_H(h);
    if (h->d.manifold != MANI_STIEFEL) { msdp_set_error("get_blockmult: only for unit-block-diagonal and pose-graph handles"); return MSDP_EUNSUPPORTED; }
    if (!Lam) { msdp_set_error("get_blockmult: null out"); return MSDP_EINVAL; }
    int rc = msdp_ensure_state(h);
    if (rc) return rc;
    const size_t lord = (size_t)(h->d.blk - h->d.efree);
    HIPCHK(msdp_memcpy_async(Lam, h->d.Lam[msdp_host_cur(h)], (size_t)h->d.nb * lord * lord * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// z of ALL rows on every rank of a row-sharded handle (one all-gather): input of the replicated host loop
extern "C" int msdp_get_z_all(msdp_handle h, double* z) {
    MSDP_CHECK_H(h);
    if (h->kind != MSDP_KIND_ONLYUNITDIAG || !z) { msdp_set_error("get_z_all: onlyunitdiag handles / null out"); return MSDP_EUNSUPPORTED; }
    if (!h->use_comm || h->nranks == 1) return msdp_get_z(h, z);
    int rc = msdp_ensure_state(h);
    if (rc) return rc;
    const size_t cap = (size_t)msdp_rows_capacity(h);
    if ((rc = msdp_allgather_vec(h, h->d.eG[msdp_host_cur(h)], h->full_buf, cap))) return rc;     // the gather buffer is free here
    HIPCHK(msdp_memcpy_async(z, h->full_buf, (size_t)h->d.n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// co() of the line search at retr(Y + alpha*U): for onlyunitdiag co = sum((Y*C).*Y) = 2 f.
extern "C" int msdp_linesearch_cost(msdp_handle h, const double* U, double alpha, double* val) {
    MSDP_CHECK_H(h);
    if (h->d.manifold == MANI_STIEFEL) { msdp_set_error("linesearch_cost: not for a %s handle (its solver takes the widening step without a line search)", msdp_block_kind_name(h->d.efree)); return MSDP_EUNSUPPORTED; }
    if (!h->have_point || !val) { msdp_set_error("linesearch_cost: no point / null out"); return MSDP_ESTATE; }
    int rc;
    const int cur = msdp_host_cur(h);
    Dev& d = h->d;
    if (U && alpha != 0.0) {
        if ((rc = upload_rows(h, U, d.W0))) return rc;
        if (d.manifold == MANI_OBLIQUE) rc = msdp_k_retr_obl(h, d.Y[cur], d.W0, d.Y[cur ^ 1], alpha);
        else rc = msdp_sphere_retr(h, d.Y[cur], d.W0, d.Y[cur ^ 1], alpha);
        if (rc) return rc;
    } else {
        HIPCHK(msdp_memcpy_async(d.Y[cur ^ 1], d.Y[cur], (size_t)msdp_rows_capacity(h) * d.ld * sizeof(double),
                              hipMemcpyDeviceToDevice, h->stream));
    }
    if (d.costkind == COST_AFFINE) return msdp_affine_linesearch_cost(h, d.Y[cur ^ 1], val);
    h->h_ctl->done = 0;
    if ((rc = msdp_push_ctl(h))) return rc;
    if ((rc = msdp_launch_costgrad(h, cur ^ 1))) return rc;
    if ((rc = msdp_k_sum_to(h, P_F, &d.ctl->fx_prop))) return rc;
    double v = 0.0;
    HIPCHK(msdp_memcpy_async(&v, &d.ctl->fx_prop, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *val = 2.0 * v;
    return 0;
}

// Adopt the retraction of Y + alpha*U as the new resident point (result of line_search).
extern "C" int msdp_linesearch_accept(msdp_handle h) {
    MSDP_CHECK_H(h);
    if (h->d.manifold == MANI_STIEFEL) { msdp_set_error("linesearch_accept: not for a %s handle (its solver takes the widening step without a line search)", msdp_block_kind_name(h->d.efree)); return MSDP_EUNSUPPORTED; }
    h->h_ctl->cur ^= 1;
    h->state_valid = false;
    h->gradnorm_valid = false;
    return 0;
}

extern "C" int msdp_escape_eigs(msdp_handle h, int32_t k, double tol, int32_t maxit, double* lam_min, double* V,
                                double* lam_max, int32_t* iters) {
    MSDP_CHECK_H(h);
    int rc = msdp_ensure_state(h);
    if (rc) return rc;
    if (!h->gradnorm_valid) {
        // |S*Y|_F and f at the resident point (decides whether span(Y) may be deflated)
        h->h_ctl->done = 0;
        if ((rc = msdp_push_ctl(h))) return rc;
        if ((rc = msdp_launch_costgrad(h, msdp_host_cur(h)))) return rc;
        if ((rc = msdp_k_sum_to(h, P_GG, &h->d.ctl->gg_prop))) return rc;
        if ((rc = msdp_k_sum_to(h, P_F, &h->d.ctl->fx_prop))) return rc;
        double v[2] = {0.0, 0.0};
        HIPCHK(msdp_memcpy_async(&v[0], &h->d.ctl->gg_prop, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(msdp_memcpy_async(&v[1], &h->d.ctl->fx_prop, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->h_ctl->norm_grad = sqrt(v[0] > 0 ? v[0] : 0.0);
        h->h_ctl->fx = v[1];
        h->gradnorm_valid = true;
    }
    return msdp_escape_impl(h, k, tol, maxit, lam_min, V, lam_max, iters, nullptr);
}

// Same for an explicit dense symmetric S handed over by the AL loop of the affine kinds (S = C - A'y - diag(z) or
// - z*I is formed on the host exactly as in ManiSDP_unitdiag.m:65-67 / ManiSDP_unittrace.m:65-67): replaces the
// O(n^3) eig(S) of :68 by Lanczos runs whose S*v is a device GEMV.  span(Y) is deflated when the last RTR call
// ended with a small gradient (grad = 2*S*Y for these problems).
extern "C" int msdp_escape_eigs_matrix(msdp_handle h, const double* S, int32_t k, double tol, int32_t maxit,
                                       double* lam_min, double* V, double* lam_max, int32_t* iters) {
    MSDP_CHECK_H(h);
    if (!S || !lam_min || !V) { msdp_set_error("escape_eigs_matrix: null argument"); return MSDP_EINVAL; }
    if (!h->have_point) { msdp_set_error("no resident point"); return MSDP_ESTATE; }
    const int n = h->d.n, nS = msdp_dense_nS(n);
    double* M = nullptr;
    if (hipMalloc((void**)&M, (size_t)n * nS * sizeof(double)) != hipSuccess) { msdp_set_error("escape_eigs_matrix: allocation failed"); return MSDP_ENOMEM; }
    hipError_t e = hipMemsetAsync(M, 0, (size_t)n * nS * sizeof(double), h->stream);
    if (e == hipSuccess)
        e = msdp_memcpy2d_async(M, (size_t)nS * sizeof(double), S, (size_t)n * sizeof(double), (size_t)n * sizeof(double), n,
                             hipMemcpyHostToDevice, h->stream);
    int rc = 0;
    if (e != hipSuccess) { msdp_set_error("escape_eigs_matrix: upload failed: %s", hipGetErrorString(e)); rc = MSDP_EHIP; }
    if (!rc) rc = msdp_escape_impl(h, k, tol, maxit, lam_min, V, lam_max, iters, M);
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(M);
    return rc;
}

extern "C" int msdp_al_primal(msdp_handle h, double* obj, double* Ax) {
    MSDP_CHECK_H(h);
    if (!obj || !Ax) { msdp_set_error("al_primal: null argument"); return MSDP_EINVAL; }
    if (h->d.costkind != COST_AFFINE) { msdp_set_error("al_primal: affine handles only"); return MSDP_EUNSUPPORTED; }
    if (!h->have_point) { msdp_set_error("no resident point"); return MSDP_ESTATE; }
    h->state_valid = false;                    // the scratch vectors / partial sums of the resident state are reused
    return msdp_affine_al_primal(h, obj, Ax);
}

extern "C" int msdp_al_dual(msdp_handle h, const double* y, double* z) {
    MSDP_CHECK_H(h);
    if (!y || (!z && h->kind != MSDP_KIND_GENERIC)) { msdp_set_error("al_dual: null argument"); return MSDP_EINVAL; }
    if (h->d.costkind != COST_AFFINE) { msdp_set_error("al_dual: affine handles only"); return MSDP_EUNSUPPORTED; }
    if (!h->have_point) { msdp_set_error("no resident point"); return MSDP_ESTATE; }
    h->state_valid = false;
    int rc = msdp_affine_al_dual(h, y, z);
    h->dual_valid = (rc == 0);
    return rc;
}

extern "C" int msdp_escape_eigs_dual(msdp_handle h, int32_t k, double tol, int32_t maxit, double* lam_min, double* V,
                                     double* lam_max, int32_t* iters) {
    MSDP_CHECK_H(h);
    if (!lam_min || !V) { msdp_set_error("escape_eigs_dual: null argument"); return MSDP_EINVAL; }
    if (h->d.costkind != COST_AFFINE || !h->dual_valid) { msdp_set_error("escape_eigs_dual: call msdp_al_dual first"); return MSDP_ESTATE; }
    // per-block storage: d.Sdual holds sum n_i * nS_i doubles, not an n x nS matrix -- the eigen-pairs come block by block
    if (h->blocked) { msdp_set_error("escape_eigs_dual: this multiblock handle stores its blocks only (msdp_block_eigs)"); return MSDP_EUNSUPPORTED; }
    int rc = msdp_escape_impl(h, k, tol, maxit, lam_min, V, lam_max, iters, h->d.Sdual);
    (void)hipStreamSynchronize(h->stream);
    return rc;
}

extern "C" int msdp_escape_info(msdp_handle h, int32_t* nvalid, int32_t* converged, double* residual) {
    MSDP_CHECK_H(h);
    if (nvalid) *nvalid = h->esc_nvalid;
    if (converged) *converged = h->esc_converged;
    if (residual) *residual = h->esc_maxres;
    return 0;
}

extern "C" int msdp_escape_method(msdp_handle h, int32_t* method) {
    MSDP_CHECK_H(h);
    if (!method) return MSDP_EINVAL;
    *method = h->esc_method_last;
    return 0;
}

extern "C" int msdp_escape_lower_bound(msdp_handle h, double* lam_lower) {
    MSDP_CHECK_H(h);
    if (!lam_lower) return MSDP_EINVAL;
    *lam_lower = h->esc_lower;
    return 0;
}

extern "C" int msdp_get_dual_slack(msdp_handle h, double* S) {
    MSDP_CHECK_H(h);
    if (!S) { msdp_set_error("get_dual_slack: null argument"); return MSDP_EINVAL; }
    if (h->d.costkind != COST_AFFINE || !h->dual_valid) { msdp_set_error("get_dual_slack: call msdp_al_dual first"); return MSDP_ESTATE; }
    if (h->blocked) { msdp_set_error("get_dual_slack: this multiblock handle stores its blocks only (msdp_get_dual_slack_block)"); return MSDP_EUNSUPPORTED; }
    const int n = h->d.n, nS = msdp_dense_nS(n);
    HIPCHK(msdp_memcpy2d_async(S, (size_t)n * sizeof(double), h->d.Sdual, (size_t)nS * sizeof(double), (size_t)n * sizeof(double), n,
                            hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int msdp_get_dual_slack_block(msdp_handle h, int64_t row0, int64_t nb, double* S) {
    MSDP_CHECK_H(h);
    if (!S) { msdp_set_error("get_dual_slack_block: null argument"); return MSDP_EINVAL; }
    if (h->d.costkind != COST_AFFINE || !h->dual_valid) { msdp_set_error("get_dual_slack_block: call msdp_al_dual first"); return MSDP_ESTATE; }
    const int n = h->d.n, nS = msdp_dense_nS(n);
    if (row0 < 0 || nb < 1 || row0 + nb > n) { msdp_set_error("get_dual_slack_block: rows %lld..%lld outside 0..%d", (long long)row0, (long long)(row0 + nb), n); return MSDP_EINVAL; }
    if (h->blocked) return msdp_affine_get_block(h, row0, nb, S);
    HIPCHK(msdp_memcpy2d_async(S, (size_t)nb * sizeof(double), h->d.Sdual + (size_t)row0 * nS + row0, (size_t)nS * sizeof(double),
                            (size_t)nb * sizeof(double), (size_t)nb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
