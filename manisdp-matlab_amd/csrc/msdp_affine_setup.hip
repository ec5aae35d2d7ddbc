// msdp_affine_setup.hip -- set-up and release of the per-handle state of the affine kinds (AffineState, msdp_affine_dev.h), host
// code only: no kernel is defined or launched here.  A set-up validates its input, builds the host plans (msdp_affine_plan.h:
// pure index arithmetic, tested on the CPU by tools/affine_plan_selftest.cpp), uploads them and allocates the operands.  The
// state hangs off the handle from its first allocation on, so a set-up that fails half-way leaves a handle msdp_destroy frees
// completely (the device arrays belong to the handle's allocation list).
#include "msdp_device.h"
#include "msdp_affine_dev.h"
#include <algorithm>

void msdp_affine_release(msdp_handle h) {
    if (!h->affine) return;
    msdp_dual_release(h->affine->dual);
    delete h->affine;
    h->affine = nullptr;
}

static int upload_sddmm(msdp_handle h, const SddmmPlan& s, AffineDev& a) {
    int rc;
    if ((rc = msdp_upload(h, s.it0, &a.it0)) || (rc = msdp_upload(h, s.it1, &a.it1)) || (rc = msdp_upload(h, s.kit, &a.kit)) ||
        (rc = msdp_upload(h, s.longk, &a.longk)) || (rc = msdp_upload(h, s.sk, &a.sk)) || (rc = msdp_upload(h, s.lit0, &a.lit0)) ||
        (rc = msdp_upload(h, s.lit1, &a.lit1)) || (rc = msdp_upload(h, s.lkit, &a.lkit)) || (rc = msdp_upload(h, s.us0, &a.us0)) ||
        (rc = msdp_upload(h, s.us1, &a.us1)) || (rc = msdp_upload(h, s.uk, &a.uk))) return rc;
    a.nitems = s.nitems; a.nlong = s.nlong; a.nshort = s.nshort; a.nlit = s.nlit;
    return 0;
}
// what both set-ups allocate per item and per constraint: ival, the arrival counter, b, the multipliers y (zero), w, Axb per slot
static int alloc_constraint_vectors(msdp_handle h, AffineState* st, const double* b) {
    AffineDev& a = st->a;
    const size_t m = (size_t)a.m;
    int rc;
    if ((rc = msdp_dev_alloc(h, &a.ival, (size_t)a.nitems)) || (rc = msdp_dev_alloc(h, &a.cnt, 16))) return rc;
    HIPCHK(hipMemset(a.cnt, 0, 64));
    if ((rc = msdp_upload(h, std::vector<double>(b, b + m), &a.b))) return rc;
    void* p = nullptr;
    if ((rc = msdp_dev_alloc_bytes(h, &p, m * sizeof(double)))) return rc;
    st->d_y = (double*)p; a.y = st->d_y;
    HIPCHK(hipMemset(st->d_y, 0, m * sizeof(double)));
    if ((rc = msdp_dev_alloc_bytes(h, &p, m * sizeof(double)))) return rc;
    a.w = (double*)p;
    for (int s = 0; s < 2; ++s) {
        if ((rc = msdp_dev_alloc_bytes(h, &p, m * sizeof(double)))) return rc;
        a.Axb[s] = (double*)p;
    }
    return 0;
}

int msdp_affine_setup(msdp_handle h, const int64_t* jc, const int64_t* ir, const double* pr, const double* b,
                      const double* c) {
    Dev& d = h->d;
    const int n = d.n, nS = msdp_dense_nS(n);
    const int64_t m = d.m;
    const int64_t nnz = jc[m];
    // ---- validate
    if (nnz > 0x7fffffff) { msdp_set_error("nnz(At) too large"); return MSDP_EINVAL; }
    if ((int64_t)n * nS > 0x7fffffffLL) { msdp_set_error("n too large for the affine kinds"); return MSDP_EUNSUPPORTED; }
    // ---- build the plans
    const AffinePlans pl = plan_affine(n, nS, m, jc, ir, pr, c);
    if (pl.ent.bad >= 0) { msdp_set_error("At row index out of range"); return MSDP_EINVAL; }
    const EntryPlan& ent = pl.ent;
    const SddmmPlan& sd = pl.sd;
    const UpperPlan& upv = pl.upv;            // symmetric data only (Gram route on Wsym), with the tiled adjoint and the B route
    const TiledPlan& til = pl.til;
    const BRoutePlan& br = pl.br;
    const SupportPlan& sp = pl.sp;
    const bool sym = pl.sym, tiled = til.ntp > 0;
    // ---- upload
    AffineState* st = new AffineState();
    h->affine = st;
    AffineDev& a = st->a;
    a.n = n; a.nS = nS; a.m = m;
    st->nnz = nnz;
    int rc;
    if ((rc = upload_sddmm(h, sd, a))) return rc;
    if ((rc = msdp_upload(h, ent.cjc, &a.cjc)) || (rc = msdp_upload(h, ent.ci, &a.ci)) || (rc = msdp_upload(h, ent.cj, &a.cj)) ||
        (rc = msdp_upload(h, ent.cv, &a.cv)) || (rc = msdp_upload(h, ent.rp, &a.rp)) || (rc = msdp_upload(h, ent.rk, &a.rk)) ||
        (rc = msdp_upload(h, ent.rv, &a.rv)) || (rc = msdp_upload(h, ent.cidx, &a.cidx))) return rc;
    if (sym) {
        if ((rc = msdp_upload(h, upv.ucidx, &a.ucidx)) || (rc = msdp_upload(h, upv.ucv, &a.ucv)) || (rc = msdp_upload(h, upv.uit0, &a.uit0)) ||
            (rc = msdp_upload(h, upv.uit1, &a.uit1)) || (rc = msdp_upload(h, upv.ukit, &a.ukit)) || (rc = msdp_upload(h, upv.ulongk, &a.ulongk)) ||
            (rc = msdp_upload(h, upv.ucjc, &a.ucjc))) return rc;
        a.unitems = upv.unitems; a.unlong = upv.unlong;
        a.usym = 1;
        h->dense_symmetric = true;                       // c and every A_k are symmetric: so are eS and A'(w) (msdp_densesym.hip)
    }
    if (tiled) {
        if ((rc = msdp_upload(h, til.trp, &a.trp)) || (rc = msdp_upload(h, til.trk, &a.trk)) || (rc = msdp_upload(h, til.trv, &a.trv)) ||
            (rc = msdp_upload(h, til.tpi, &a.tp_i)) || (rc = msdp_upload(h, til.tpj, &a.tp_j)) || (rc = msdp_upload(h, til.lpos, &a.lpos)) ||
            (rc = msdp_upload(h, til.lmir, &a.lmir)) || (rc = msdp_upload(h, til.ls0, &a.ls0)) || (rc = msdp_upload(h, til.ls1, &a.ls1))) return rc;
        a.ntp = til.ntp; a.nlong_e = til.nlong_e;
    }
    if (br.bW > 0) {
        if (br.packed && ((rc = msdp_upload(h, br.bpk, &a.bpk)) || (rc = msdp_upload(h, br.bdict, &a.bdict)))) return rc;
        if ((rc = msdp_upload(h, br.bidx, &a.bidx)) || (rc = msdp_upload(h, br.bval, &a.bval)) || (rc = msdp_upload(h, br.blong, &a.blong)) ||
            (rc = msdp_upload(h, br.blpos, &a.blpos)) || (rc = msdp_upload(h, br.blmir, &a.blmir)) || (rc = msdp_upload(h, br.bls0, &a.bls0)) ||
            (rc = msdp_upload(h, br.bls1, &a.bls1)) || (rc = msdp_upload(h, br.blk, &a.blk)) || (rc = msdp_upload(h, br.blv, &a.blv))) return rc;
        a.bnlong = br.bnlong;
        a.bW = br.bW;
    }
    if (sp.nsup > 0) {
        if ((rc = msdp_upload(h, sp.sup, &a.sup)) || (rc = msdp_upload(h, sp.suprow, &a.suprow)) || (rc = msdp_upload(h, sp.sqj, &a.sqj)) ||
            (rc = msdp_upload(h, sp.sqk, &a.sqk)) || (rc = msdp_upload(h, sp.sqv, &a.sqv)) || (rc = msdp_upload(h, sp.sqmore, &a.sqmore)) ||
            (rc = msdp_upload(h, sp.rkx, &a.rkx))) return rc;
        a.nsup = sp.nsup;
    }
    // ---- allocate the operands
    if ((rc = alloc_constraint_vectors(h, st, b))) return rc;
    void* p = nullptr;
    // dense C (n x nS) from the column-major vector c (symmetric)
    const size_t msz = (size_t)n * a.nS * sizeof(double);
    if ((rc = msdp_dev_alloc_bytes(h, &p, msz))) return rc;
    st->Cdense = (double*)p; d.Cd = st->Cdense;
    HIPCHK(hipMemset(st->Cdense, 0, msz));
    HIPCHK(msdp_memcpy2d(st->Cdense, (size_t)a.nS * sizeof(double), c, (size_t)n * sizeof(double), (size_t)n * sizeof(double), n,
                       hipMemcpyHostToDevice));
    for (int s = 0; s < 2; ++s) {
        if ((rc = msdp_dev_alloc_bytes(h, &p, msz))) return rc;
        d.eS[s] = (double*)p;
        // restricted adjoint: eS = C outside the entries At touches, from the start
        if (a.nsup > 0) HIPCHK(msdp_memcpy(d.eS[s], st->Cdense, msz, hipMemcpyDeviceToDevice));
        else HIPCHK(hipMemset(d.eS[s], 0, msz));
    }
    if ((rc = msdp_dev_alloc_bytes(h, &p, msz))) return rc;
    d.AyU = (double*)p;
    HIPCHK(hipMemset(d.AyU, 0, msz));
    // the Gram scratch may share AyU: W is consumed (k_gram_apply) before the adjoint rewrites AyU, and the cost /
    // line-search calls never touch AyU.  With the restricted adjoint AyU must stay zero outside the entries At
    // touches, so the Gram scratch and the dual slack of msdp_al_dual get buffers of their own.
    a.W = d.AyU;
    d.Sdual = d.AyU;
    if (a.bW > 0) {
        if ((rc = msdp_dev_alloc_bytes(h, &p, msz))) return rc;
        a.Wg = (double*)p;
        HIPCHK(hipMemset(a.Wg, 0, msz));
    }
    if (a.nsup > 0) {
        if ((rc = msdp_dev_alloc_bytes(h, &p, msz))) return rc;
        a.W = (double*)p;
        if ((rc = msdp_dev_alloc_bytes(h, &p, msz))) return rc;
        d.Sdual = (double*)p;
        HIPCHK(hipMemset(d.Sdual, 0, msz));
    }
    h->h_ctl->sigma = 1.0;
    return 0;
}

// Set-up of the multiblock kind with per-block storage.  jc / ir / pr: At over the CONCATENATED vecs of the blocks (ir = e0_i + a +
// b*n_i, column-major inside block i); c likewise.  Nothing of size N^2 is built, on the host or on the device.
int msdp_affine_setup_blocked(msdp_handle h, int nb, const int64_t* block_n, const int64_t* jc, const int64_t* ir, const double* pr,
                              const double* b, const double* c) {
    Dev& d = h->d;
    const int N = d.n;
    const int64_t m = d.m, nnz = jc[m];
    // ---- validate, build the plans
    if (nnz > 0x7fffffff) { msdp_set_error("nnz(At) too large"); return MSDP_EINVAL; }
    std::vector<int> bns(nb);
    for (int i = 0; i < nb; ++i) bns[i] = msdp_dense_nS((int)block_n[i]);
    const BlockedPlan bp = plan_blocked(nb, block_n, bns.data(), m, jc, ir, pr);
    if (bp.status == 1) { msdp_set_error("multiblock: sum n_i^2 too large"); return MSDP_EUNSUPPORTED; }
    if (bp.status == 2) { msdp_set_error("multiblock: At row index out of range"); return MSDP_EINVAL; }
    const SddmmPlan sd = plan_sddmm(m, bp.cjc.data());
    const int64_t etot = bp.etot;
    // ---- upload
    AffineState* st = new AffineState();
    h->affine = st;
    AffineDev& a = st->a;
    a.n = N; a.nS = msdp_dense_nS(N); a.m = m;
    st->nnz = nnz;
    st->blk = new BlockedDev();
    BlockedDev& bd = *st->blk;
    st->blk_r0 = bp.r0; st->blk_off = bp.off; st->blk_n = bp.bn; st->blk_ns = bp.bns;
    int rc;
    if ((rc = upload_sddmm(h, sd, a))) return rc;
    if ((rc = msdp_upload(h, bp.cjc, &a.cjc)) || (rc = msdp_upload(h, bp.ci, &a.ci)) || (rc = msdp_upload(h, bp.cj, &a.cj)) ||
        (rc = msdp_upload(h, bp.cv, &a.cv)) || (rc = msdp_upload(h, bp.rbase, &bd.rbase)) || (rc = msdp_upload(h, bp.rlo, &bd.rlo)) ||
        (rc = msdp_upload(h, bp.rhi, &bd.rhi)) || (rc = msdp_upload(h, bp.rns, &bd.rns)) || (rc = msdp_upload(h, bp.prp, &bd.prp)) ||
        (rc = msdp_upload(h, bp.prk, &bd.prk)) || (rc = msdp_upload(h, bp.prv, &bd.prv)) ||
        (rc = msdp_upload(h, bp.tile_row0, &bd.tile_row0)) || (rc = msdp_upload(h, bp.longq, &bd.longq)))
        return rc;
    bd.nb = nb; bd.N = N; bd.ntile = (int)bp.tile_row0.size(); bd.etot = etot; bd.nlongq = bp.nlongq;
    // Gram route on the blocks (k_block_gram + k_gram_apply): the stored position of every nonzero, and room for W = Ya Yb' block by block
    if ((rc = msdp_upload(h, bp.pos, &a.cidx)) || (rc = msdp_dev_alloc(h, &a.W, (size_t)etot))) return rc;
    // ---- allocate the operands
    if ((rc = alloc_constraint_vectors(h, st, b))) return rc;
    void* p = nullptr;
    // c, block by block, into the padded storage; eS, AyU start as zeros
    const size_t msz = (size_t)etot * sizeof(double);
    {
        std::vector<double> cb((size_t)etot, 0.0);
        for (int i = 0; i < nb; ++i)
            for (int bb = 0; bb < bp.bn[i]; ++bb)
                for (int aa = 0; aa < bp.bn[i]; ++aa)
                    cb[(size_t)(bp.off[i] + (int64_t)aa * bp.bns[i] + bb)] = c[bp.e0[i] + aa + (int64_t)bb * bp.bn[i]];
        if ((rc = msdp_dev_alloc_bytes(h, &p, msz))) return rc;
        st->Cdense = (double*)p; d.Cd = st->Cdense;
        HIPCHK(msdp_memcpy(st->Cdense, cb.data(), msz, hipMemcpyHostToDevice));
    }
    for (int s2 = 0; s2 < 2; ++s2) {
        if ((rc = msdp_dev_alloc_bytes(h, &p, msz))) return rc;
        d.eS[s2] = (double*)p;
        HIPCHK(hipMemset(d.eS[s2], 0, msz));
    }
    if ((rc = msdp_dev_alloc_bytes(h, &p, msz))) return rc;
    d.AyU = (double*)p;
    HIPCHK(hipMemset(d.AyU, 0, msz));
    d.Sdual = d.AyU;
    h->blocked = true;
    h->dense_symmetric = false;
    // (a.W: the blocks' own Gram storage, allocated above -- msdp_affine_launch_A takes the Gram route on it once the panel is wide
    //  enough; the N x N routes of use_gram_route / the B route never apply to this storage)
    h->h_ctl->sigma = 1.0;
    return 0;
}
// One diagonal block of the dual slack (per-block storage): rows row0 .. row0 + nbk - 1 must be exactly one block
int msdp_affine_get_block(msdp_handle h, int64_t row0, int64_t nbk, double* S) {
    AffineState* st = h->affine;
    if (!st || !st->blk) { msdp_set_error("get_block: not a handle with per-block storage"); return MSDP_ESTATE; }
    for (size_t i = 0; i + 1 < st->blk_r0.size(); ++i)
        if (st->blk_r0[i] == row0 && st->blk_n[i] == nbk) {
            HIPCHK(msdp_memcpy2d_async(S, (size_t)nbk * sizeof(double), h->d.Sdual + st->blk_off[i], (size_t)st->blk_ns[i] * sizeof(double),
                                    (size_t)nbk * sizeof(double), (size_t)nbk, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            return 0;
        }
    msdp_set_error("get_dual_slack_block: rows %lld..%lld are not one block of this handle", (long long)row0, (long long)(row0 + nbk));
    return MSDP_EINVAL;
}

// Where block (row0, n) of the per-block storage lives in d.Sdual (msdp_blockjacobi.hip)
int msdp_affine_block_source(msdp_handle h, int64_t row0, int64_t n, int64_t* off, int64_t* ld) {
    AffineState* st = h->affine;
    if (!st || !st->blk) { msdp_set_error("block_source: not a handle with per-block storage"); return MSDP_ESTATE; }
    for (size_t i = 0; i + 1 < st->blk_r0.size(); ++i)
        if (st->blk_r0[i] == row0 && st->blk_n[i] == n) { *off = st->blk_off[i]; *ld = st->blk_ns[i]; return 0; }
    msdp_set_error("block_eigs: rows %lld..%lld are not one block of this handle", (long long)row0, (long long)(row0 + n));
    return MSDP_EINVAL;
}

int msdp_affine_set_multipliers(msdp_handle h, const double* y, double sigma) {
    AffineState* st = h->affine;
    if (!st) { msdp_set_error("affine state missing"); return MSDP_ESTATE; }
    if (!(sigma > 0)) { msdp_set_error("sigma must be positive"); return MSDP_EINVAL; }
    HIPCHK(msdp_memcpy_async(st->d_y, y, st->a.m * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    st->sigma = sigma;
    h->h_ctl->sigma = sigma;
    return 0;
}

// (test / diagnostic) What the set-up planned and which branch the last Hess-vec and the last A(.) took: 16 ints, the unused ones
// zero (include/manisdp_hip.h lists the fields).  Host only: nothing is launched and the handle is not modified.
extern "C" int msdp_debug_affine_plan(msdp_handle h, int32_t* out) {
    if (!h || !out) { msdp_set_error("affine_plan: null argument"); return MSDP_EINVAL; }
    const AffineState* st = h->affine;
    if (!st || st->dual || st->blk) { msdp_set_error("affine_plan: not a primal affine handle with N x N storage"); return MSDP_ESTATE; }
    const AffineDev& a = st->a;
    const int32_t v[16] = {a.usym, a.ntp, a.nlong_e, a.bW, a.bpk != nullptr, a.bnlong, a.nsup, a.nlong, a.nshort, a.nlit, a.n, a.nS,
                           st->last_hess_path, st->last_A_route, 0, 0};
    for (int i = 0; i < 16; ++i) out[i] = v[i];
    return 0;
}
