// msdp_blockpersist.hip -- the whole truncated-CG solve of one trust-region iteration in ONE launch for the block kinds
// (MANI_STIEFEL / COST_BLOCK, msdp_stiefel.hip: the unit-block-diagonal kind and, with d.efree = 1, the pose-graph kind):
// tCG.m:95-292 with the working set on chip, the counterpart of msdp_persist.hip for blocks of B = D + EF rows
// of which the first D are Stiefel rows and the last EF (0 or 1) is free.  Option "block_persist" (default off).
//
// The generic path runs a trip as three launches (k_stf_hess, k_tcg_upd1, k_stf_upd2) inside
// hipGraph chunks with the host polling a progress word.  Here a lane group of LPR lanes owns one block per row slot (R slots),
// one double2 per lane and row: the B rows of eta, Heta, r, mdelta and Hmdelta of its blocks stay in registers for the whole
// launch (blocks of four rows in two slots keep Heta as r - grad: HDER below); the D rotation rows of Y, the B rows of the gradient and the D x D multiplier block Lambda_i of the current point are
// read once and kept in LDS (msdp_blockpersist_plan.h has the sizes).  Workgroups of 512 threads, at most one per CU; chunks
// over blocks (msdp_chunk_rows), so that a block never straddles two workgroups.
// The block-CSR entries of C (d.brp / bci / bval) are NOT staged: they are static during the launch and re-read from L2 with
// plain loads every trip (a block row of a degree-8 pose graph has some 17 entries of B * B values: staging them beside Y and
// the gradient would halve the row slots that fit the LDS).  Up to four entries of a block row are gathered together
// (bp_batch: what the registers of an instance leave).
//
// A trip (the two-reduction form; no assembled products, every Hess-vec is a direct gather):
//   1  the rows of the direction go to the exchange buffer d.mdx with agent-coherent stores (st2_sc1)
//   2  value-less grid barrier (pbarrier)
//   3  gather C * mdelta over the block row with agent-coherent loads (ld2_sc1, spmm_block_via of msdp_device.h)
//   4  W = C mdelta - (Lambda (+) 0) mdelta; rotation rows W_i - sym(W_i Y_i') Y_i, the free row as it is
//   5  grid reduction 1: <mdelta, Hmdelta>
//   6  the decisions of k_tcg_upd1 (tCG.m:166-241)                7  eta, Heta, r
//   8  grid reduction 2: <eta', grad>, <eta', Heta'>, <r', r'>
//   9  the decisions of msdp_tcg_upd2_scalars (tCG.m:227-287)    10  mdelta = tangent(r + beta mdelta), block by block
// Every workgroup has gathered the rows of trip j before it posts reduction 1 of that trip, and nobody stores the rows of trip
// j + 1 before reduction 2 has returned: one exchange buffer is enough.  The sums are formed in one fixed order in every
// workgroup (msdp_psync.h), so all of them take the same decisions.  Every wait is a bounded spin of msdp_psync.h that raises
// the handle's error word; the host then repeats the call on the chunked path (msdp_rtr.hip).
// Two slot regions alternate from launch to launch (the host passes which); a launch clears the other one at its start, so
// that a region is clean when its turn comes -- the role the TR-tail kernel plays for msdp_persist.hip.
//
// Contraction is pinned to the source as in msdp_persist.hip: an `a * b + c` inside one expression is an fma, nothing else is.
#pragma clang fp contract(on)
#include "msdp_device.h"
#include <math.h>

#include "msdp_psync.h"
#include "msdp_blockpersist_plan.h"

static_assert(PB == MSDP_BP_THREADS && PWAVES == MSDP_BP_WAVES, "the plan and msdp_psync.h agree on the workgroup");

// the two slot regions at their start state and the error word cleared (first TR iteration of a call)
__global__ void k_psync_reset_blk(unsigned long long* slots, int* err) {
    const int tot = (int)PSYNC_CNT_OFF;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += gridDim.x * blockDim.x) { slots[i] = PSYNC_SENT; slots[PSYNC_REGION + i] = PSYNC_SENT; }
    if (blockIdx.x == 0 && threadIdx.x < 64) { slots[PSYNC_CNT_OFF + threadIdx.x] = 0ULL; slots[PSYNC_REGION + PSYNC_CNT_OFF + threadIdx.x] = 0ULL; }
    if (blockIdx.x == 0 && threadIdx.x == 0) *err = 0;
}

// st2_sc1 of msdp_psync.h with the row's share of the byte offset in a scalar register: a lane keeps ONE offset per block, not one
// per row of it
__device__ __forceinline__ void bp_st2_sc1(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff, double2 d2) {
    const long long a = __double_as_longlong(d2.x), b = __double_as_longlong(d2.y);
    v4u v;
    v.x = (unsigned)(a & 0xffffffffLL); v.y = (unsigned)((unsigned long long)a >> 32);
    v.z = (unsigned)(b & 0xffffffffLL); v.w = (unsigned)((unsigned long long)b >> 32);
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, voff, soff, MSDP_CPOL_SC1);
}

// T = sym(A(1:D, :) Bm(1:D, :)') of two blocks a lane group holds, one double2 per lane and row: the sums of
// msdp_block_symdot at NCH = 1, in its order
template <int D, int LPR, int RA, int RB>
__device__ __forceinline__ void bp_symdot(const double2 (&A)[RA], const double2 (&Bm)[RB], double (&T)[D][D]) {
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = a; b < D; ++b) {
            double s = 0.0;
            s += A[a].x * Bm[b].x + A[a].y * Bm[b].y;
            if (b != a) s += A[b].x * Bm[a].x + A[b].y * Bm[a].y;
            s = msdp_group_sum<LPR>(s);
            T[a][b] = T[b][a] = (b != a) ? 0.5 * s : s;
        }
}

// entries of a block row gathered together, by block order and row slots
constexpr int bp_batch(int B, int R) { return R == 1 ? 4 : (B == 2 ? 4 : (B == 3 ? 2 : 1)); }

template <int D, int EF, int LPR, int R, int BPCB = bp_batch(D + EF, R)>
__global__ __launch_bounds__(PB) void k_tcg_persist_blk(Dev d, unsigned long long* slots, int* err, int region) {
    constexpr int B = D + EF, DD = D * D;
    constexpr int BPW = 64 / LPR;                 // blocks per wave and slot
    constexpr int RSTEP = PWAVES * BPW;           // blocks per slot of the workgroup
    constexpr int CB = BPCB;                      // block entries of a gather in flight together (what the registers leave)
    extern __shared__ double lds[];
    __shared__ double sh[3 * PWAVES];
    __shared__ double shb[8];
    double2* Ys = reinterpret_cast<double2*>(lds);        // [R][D][PB]
    double2* Gs = Ys + R * D * PB;                        // [R][B][PB]
    double* Ls = reinterpret_cast<double*>(Gs + R * B * PB);   // [R * RSTEP][D * D]

    const Ctl* c = d.ctl;
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    const double gg = c->gg;
    if (c->done) {                                        // k_tcg_init on a finished solve: the same frame, nothing else
        if (lead) {
            frame_store(&d.F[0], gg, gg, 0.0, 0.0, 0.0, sqrt(gg), 0.0, 0.0, 0, 0, 5, 0, 0, 1);
            frame_store(&d.F[1], gg, gg, 0.0, 0.0, 0.0, sqrt(gg), 0.0, 0.0, 0, 0, 5, 0, 0, 1);
            d.ctl->tcg_running = 0;
        }
        return;
    }
    const int G = d.G;
    psync_reset_other(slots + (size_t)(region ^ 1) * PSYNC_REGION);
    slots += (size_t)region * PSYNC_REGION;

    int lo, hi;
    msdp_chunk_rows(d.nb, G, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    const unsigned uld = (unsigned)d.ld;
    const bool colok = 2 * sub < d.ld;
    const unsigned colb = colok ? 16u * (unsigned)sub : 0u;      // byte offset of the lane's columns in a row
    const int cur = c->cur;
    const bool bench = c->bench_mode != 0;
    const double Delta = c->Delta, kappa = c->kappa, theta = c->theta;
    const int mininner = c->mininner, maxinner = c->maxinner;
    const int backoff = c->psync_backoff;
    const double* __restrict__ Yl = cur ? d.Y[1] : d.Y[0];
    const double* __restrict__ gl = cur ? d.Gr[1] : d.Gr[0];
    const double* __restrict__ Lam = cur ? d.Lam[1] : d.Lam[0];
    const int slot0 = wave * BPW + rsub;
#define BP_SLOT(r) ((r) * RSTEP + slot0)
#define BP_BLK(r) (lo + BP_SLOT(r))
#define BP_OK(r) (BP_BLK(r) < hi)

    const double2 zz = make_double2(0.0, 0.0);
    // HDER (blocks of four rows in two slots): five resident vectors are 160 registers and the trip spilled; there Heta is not
    // kept but follows from r = grad + Heta (tCG.m:198, :220, :238 update both by the same vector), as in msdp_persist.hip
    constexpr bool HDER = (B == 4 && R == 2);
    double2 eta[R][B], he[HDER ? 1 : R][B], rr[R][B], md[R][B], hm[R][B];
#define BP_HE(r, a) he[HDER ? 0 : (r)][a]
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const bool ok = BP_OK(r);
        const int bc = ok ? BP_BLK(r) : 0;                // (block 0 exists: loads from a clamped block, then masked)
#pragma unroll
        for (int a = 0; a < B; ++a) {
            const int64_t o = ((int64_t)bc * B + a) * d.ld + (colok ? 2 * sub : 0);
            double2 g = ld2(gl + o);
            if (!(ok && colok)) g = zz;
            Gs[(r * B + a) * PB + threadIdx.x] = g;
            eta[r][a] = zz; BP_HE(r, a) = zz; rr[r][a] = g; md[r][a] = g; hm[r][a] = zz;      // tCG.m:102-157
            if (a < D) {
                double2 y = ld2(Yl + o);
                if (!(ok && colok)) y = zz;
                Ys[(r * D + a) * PB + threadIdx.x] = y;
            }
        }
        if (sub == 0) {
#pragma unroll
            for (int i = 0; i < DD; ++i) Ls[BP_SLOT(r) * DD + i] = ok ? Lam[(int64_t)bc * DD + i] : 0.0;
        }
    }
    // the clearing stores of the other region are performed before this workgroup's first post (the launch that uses that
    // region starts behind the end of this one)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const unsigned vec_bytes = (unsigned)((size_t)d.nb * B * d.ld * sizeof(double));
    __amdgpu_buffer_rsrc_t rs_md = __builtin_amdgcn_make_buffer_rsrc(d.mdx, 0, vec_bytes, 0x00020000);
    auto ldx = [&](unsigned off) -> double2 { return ld2_sc1(rs_md, off); };

    unsigned gen = 0, nbar = 0;
    double z_r = gg, d_Pd = gg, e_Pd = 0.0, e_Pe = 0.0, model_value = 0.0, alpha = 0.0, beta = 0.0;
    const double norm_r0 = sqrt(gg);
    const double nr0t = tcg_nr0t(norm_r0, theta);                          // the same in every trip
    int j = 0, stop = 5;
    bool failed = false;
    for (;;) {
        // ---- 1, 2: the direction rows to the neighbours
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int a = 0; a < B; ++a)
                if (BP_OK(r) && colok) bp_st2_sc1(rs_md, (unsigned)BP_BLK(r) * (unsigned)B * uld * 8u + colb, (unsigned)a * uld * 8u, md[r][a]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // my rows are performed before my workgroup arrives
        if (!pbarrier(slots, nbar++, G, shb, err)) { failed = true; break; }
        // ---- 3, 4: Hmdelta (tCG.m:163; stiefelstackedfactory.m:93-101, the free row by euclideanfactory.m)
        double pd = 0.0, u1 = 0.0, u2 = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool ok = BP_OK(r);
            const int k0 = ok ? d.brp[BP_BLK(r)] : 0, k1 = ok ? d.brp[BP_BLK(r) + 1] : 0;
            double2 w[B];
#pragma unroll
            for (int a = 0; a < B; ++a) w[a] = zz;
            spmm_block_via<B, CB>(d, k0, k1, colb, uld, ldx, w);
            if (!colok) {
#pragma unroll
                for (int a = 0; a < B; ++a) w[a] = zz;
            }
            double2 y[D];
#pragma unroll
            for (int a = 0; a < D; ++a) y[a] = Ys[(r * D + a) * PB + threadIdx.x];
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b < D; ++b) {
                    const double l = Ls[BP_SLOT(r) * DD + a * D + b];
                    w[a].x -= l * md[r][b].x; w[a].y -= l * md[r][b].y;
                }
            double T[D][D];
            bp_symdot<D, LPR>(w, y, T);
#pragma unroll
            for (int a = 0; a < B; ++a) {
                double2 h = w[a];
                if (a < D) {
#pragma unroll
                    for (int b = 0; b < D; ++b) { h.x -= T[a][b] * y[b].x; h.y -= T[a][b] * y[b].y; }
                }
                hm[r][a] = h;
                pd += md[r][a].x * h.x + md[r][a].y * h.y;
            }
        }
        // ---- 5, 6
        if (!psync(slots, gen++, G, 1, pd, u1, u2, sh, shb, err, -1, backoff, false)) { failed = true; break; }
        const double d_Hd = pd;                                                        // :166
        alpha = z_r / d_Hd;                                                            // :170
        const double e_Pe_new = tcg_e_Pe_new(e_Pe, alpha, e_Pd, d_Pd);
        if (!bench && !tcg_step_inside(d_Hd, e_Pe_new, Delta)) {
            const double tau = tcg_tau(e_Pd, d_Pd, e_Pe, Delta);
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int a = 0; a < B; ++a) {
                    eta[r][a] = make_double2(eta[r][a].x - tau * md[r][a].x, eta[r][a].y - tau * md[r][a].y);   // :192
                    if (HDER) rr[r][a] = make_double2(rr[r][a].x - tau * hm[r][a].x, rr[r][a].y - tau * hm[r][a].y);
                    else BP_HE(r, a) = make_double2(BP_HE(r, a).x - tau * hm[r][a].x, BP_HE(r, a).y - tau * hm[r][a].y);   // :198
                }
            stop = tcg_boundary_stop(d_Hd);
            ++j;
            break;
        }
        // ---- 7, 8: the trial step and its three inner products (tCG.m:215-241)
        double s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int a = 0; a < B; ++a) {
                const double2 g = Gs[(r * B + a) * PB + threadIdx.x];
                const double2 ne = make_double2(eta[r][a].x - alpha * md[r][a].x, eta[r][a].y - alpha * md[r][a].y);   // :215
                const double2 nr = make_double2(rr[r][a].x - alpha * hm[r][a].x, rr[r][a].y - alpha * hm[r][a].y);     // :238
                const double2 nh = HDER ? make_double2(nr.x - g.x, nr.y - g.y)
                                        : make_double2(BP_HE(r, a).x - alpha * hm[r][a].x, BP_HE(r, a).y - alpha * hm[r][a].y);   // :220
                s1 += ne.x * g.x + ne.y * g.y;
                s2 += ne.x * nh.x + ne.y * nh.y;
                s3 += nr.x * nr.x + nr.y * nr.y;
            }
        if (!psync(slots, gen++, G, 3, s1, s2, s3, sh, shb, err, -1, backoff, false)) { failed = true; break; }
        // ---- 9
        e_Pe = e_Pe_new;
        const double new_model = s1 + 0.5 * s2;                                        // :227
        const double r_r = s3;
        if (!bench && !tcg_model_decreased(new_model, model_value)) { stop = 6; ++j; break; }   // (eta, Heta stay)
#pragma unroll
        for (int r = 0; r < R; ++r)                                                    // :233-238 commit (the trial's expressions)
#pragma unroll
            for (int a = 0; a < B; ++a) {
                eta[r][a] = make_double2(eta[r][a].x - alpha * md[r][a].x, eta[r][a].y - alpha * md[r][a].y);
                if (!HDER) BP_HE(r, a) = make_double2(BP_HE(r, a).x - alpha * hm[r][a].x, BP_HE(r, a).y - alpha * hm[r][a].y);
                rr[r][a] = make_double2(rr[r][a].x - alpha * hm[r][a].x, rr[r][a].y - alpha * hm[r][a].y);
            }
        model_value = new_model;
        ++j;
        const double norm_r = sqrt(r_r);
        if (!bench && !tcg_unconverged(j, mininner, norm_r, norm_r0, nr0t, kappa)) {
            stop = tcg_converged_stop(kappa, nr0t);
            break;
        }
        if (j >= maxinner) break;                                                      // :160 (stop stays 5)
        beta = tcg_recurrences(r_r, alpha, z_r, e_Pd, d_Pd);
        // ---- 10: mdelta = tangent(r + beta mdelta) (:273, :283); the free row of the projection is the row itself
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double2 v[B], y[D];
#pragma unroll
            for (int a = 0; a < B; ++a) v[a] = make_double2(rr[r][a].x + beta * md[r][a].x, rr[r][a].y + beta * md[r][a].y);
#pragma unroll
            for (int a = 0; a < D; ++a) y[a] = Ys[(r * D + a) * PB + threadIdx.x];
            double T[D][D];
            bp_symdot<D, LPR>(v, y, T);
#pragma unroll
            for (int a = 0; a < B; ++a) {
                double2 t = v[a];
                if (a < D) {
#pragma unroll
                    for (int b = 0; b < D; ++b) { t.x -= T[a][b] * y[b].x; t.y -= T[a][b] * y[b].y; }
                }
                md[r][a] = t;
            }
        }
    }
    if (failed) return;
    // ---- what the generic path leaves: eta, Heta and the closing frame (trustregions.m:540-550 read them)
    __amdgpu_buffer_rsrc_t rs_eta = __builtin_amdgcn_make_buffer_rsrc(d.eta[0], 0, vec_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t rs_heta = __builtin_amdgcn_make_buffer_rsrc(d.Heta[0], 0, vec_bytes, 0x00020000);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int a = 0; a < B; ++a)
            if (BP_OK(r) && colok) {
                // (through descriptors, at the byte offsets of the row stores of a trip: no 64-bit address lives across the loop)
                const unsigned o = (unsigned)BP_BLK(r) * (unsigned)B * uld * 8u + colb, so = (unsigned)a * uld * 8u;
                bp_st2_sc1(rs_eta, o, so, eta[r][a]);
                const double2 g = Gs[(r * B + a) * PB + threadIdx.x];
                bp_st2_sc1(rs_heta, o, so, HDER ? make_double2(rr[r][a].x - g.x, rr[r][a].y - g.y) : BP_HE(r, a));
            }
    if (lead) {
        frame_store(&d.F[0], z_r, d_Pd, e_Pd, e_Pe, model_value, norm_r0, alpha, beta, 0, j, stop, 0, 0, 0);
        frame_store(&d.F[1], z_r, d_Pd, e_Pd, e_Pe, model_value, norm_r0, alpha, beta, 0, j, stop, 0, 0, 0);
        d.ctl->tcg_running = 0;
    }
#undef BP_SLOT
#undef BP_BLK
#undef BP_OK
#undef BP_HE
}

// ------------------------------------------------------------------ host
typedef void (*blkpersist_fn)(Dev, unsigned long long*, int*, int);

template <int D, int EF>
static blkpersist_fn blk_kernel_de(int lpr, int R) {
#define BPK(L) if (lpr == L) return R == 1 ? k_tcg_persist_blk<D, EF, L, 1> : k_tcg_persist_blk<D, EF, L, 2>;
    BPK(1) BPK(2) BPK(4) BPK(8) BPK(16)
#undef BPK
    return nullptr;
}
static blkpersist_fn blk_kernel(const Dev& d, const BlockPersistPlan& pl) {
    if (pl.R < 1 || pl.R > 2) return nullptr;
    const int D = d.blk - d.efree;
    if (D == 2 && d.efree == 0) return blk_kernel_de<2, 0>(pl.lpr, pl.R);
    if (D == 3 && d.efree == 0) return blk_kernel_de<3, 0>(pl.lpr, pl.R);
    if (D == 2 && d.efree == 1) return blk_kernel_de<2, 1>(pl.lpr, pl.R);
    if (D == 3 && d.efree == 1) return blk_kernel_de<3, 1>(pl.lpr, pl.R);
    return nullptr;
}

static int blk_cus() {
    static int cus = -1;
    if (cus < 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) cus = v;
        else cus = 0;
        (void)hipGetLastError();
    }
    return cus;
}

// the plan of this handle at its current width (the lanes follow the row stride ld, like the row kernels of the kinds)
static BlockPersistPlan blk_plan(msdp_handle h) {
    const Dev& d = h->d;
    BlockPersistPlan none = {0, 0, 0, 0, 0, 0};
    if (d.manifold != MANI_STIEFEL || d.costkind != COST_BLOCK || !d.brp || d.nb < 1) return none;
    if ((size_t)d.nb * d.blk * d.ld * sizeof(double) >= ((size_t)1 << 31)) return none;      // 32-bit byte offsets into the exchange buffer
    return msdp_blockpersist_plan(d.nb, d.blk, d.efree, d.ld, blk_cus(), h->tune.block_persist_grid, h->tune.block_persist_wide);
}

int msdp_blockpersist_plan_of(msdp_handle h, int* lpr, int* G, int* R, size_t* lds) {
    const BlockPersistPlan pl = blk_plan(h);
    if (lpr) *lpr = pl.lpr;
    if (G) *G = pl.G;
    if (R) *R = pl.R;
    if (lds) *lds = pl.lds;
    return pl.ok;
}

// 1: the persistent kernel above runs this handle's tCG (option on, a plan exists, all its workgroups are co-resident)
int msdp_blockpersist_eligible(msdp_handle h) {
    const Dev& d = h->d;
    if (!h->tune.block_persist || !h->tune.persist || h->persist_failed || h->use_comm || h->nranks != 1) return 0;
    if (d.manifold != MANI_STIEFEL || d.costkind != COST_BLOCK) return 0;
    if (d.pcM) return 0;                                  // option "precon": the kernel above has no preconditioner, the generic trips run
    if (!h->psync_slots || !h->psync_err || !d.mdx) return 0;
    const BlockPersistPlan pl = blk_plan(h);
    if (!pl.ok) return 0;
    blkpersist_fn fn = blk_kernel(d, pl);
    if (!fn) return 0;
    if (h->blkpersist_sig_fn == (const void*)fn && h->blkpersist_sig_G == pl.G && h->blkpersist_sig_lds == pl.lds) return h->blkpersist_sig_ok;
    int ok = 0, dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)fn, PB, pl.lds) == hipSuccess)
        ok = (per_cu >= 1 && cus >= pl.G) ? 1 : 0;        // one workgroup per CU: never rely on two sharing a CU
    (void)hipGetLastError();
    h->blkpersist_sig_fn = (const void*)fn; h->blkpersist_sig_G = pl.G; h->blkpersist_sig_lds = pl.lds; h->blkpersist_sig_ok = ok;
    return ok;
}

// The whole tCG of the current TR iteration, one launch.  reset_slots: first launch of a call (both slot regions and the error
// word start clean); the launches of a call alternate between the two regions.
int msdp_launch_tcg_blockpersist(msdp_handle h, int reset_slots) {
    const BlockPersistPlan pl = blk_plan(h);
    blkpersist_fn fn = pl.ok ? blk_kernel(h->d, pl) : nullptr;
    if (!fn) { msdp_set_error("persistent tCG (%s kind): not eligible", msdp_block_kind_name(h->d.efree)); return MSDP_ESTATE; }
    Dev dp = h->d;
    dp.G = pl.G;
    dp.status = nullptr;                                  // the host does not poll: one synchronisation per TR iteration
    if (reset_slots) {
        hipLaunchKernelGGL(k_psync_reset_blk, dim3(8), dim3(256), 0, h->stream, h->psync_slots, h->psync_err);
        HIPCHK(hipGetLastError());
        h->blkpersist_region = 0;
    }
    HIPCHK(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
    hipLaunchKernelGGL(fn, dim3(pl.G), dim3(PB), pl.lds, h->stream, dp, h->psync_slots, h->psync_err, h->blkpersist_region);
    HIPCHK(hipGetLastError());
    h->blkpersist_region ^= 1;
    return 0;
}

// msdp_debug_persist_form for the block kinds: 0 (two reductions per trip) where the kernel above applies, else -1
extern "C" int msdp_debug_block_persist_form(msdp_handle h, int32_t* form) {
    if (!h || !form) return MSDP_EINVAL;
    *form = msdp_blockpersist_eligible(h) ? 0 : -1;
    return 0;
}

// The plan of the handle at its resident width: out = {eligible, lanes per block, workgroups, row slots, LDS bytes} (tests)
extern "C" int msdp_debug_block_persist_plan(msdp_handle h, int32_t* out) {
    if (!h || !out) return MSDP_EINVAL;
    int lpr = 0, G = 0, R = 0;
    size_t lds = 0;
    const int ok = msdp_blockpersist_plan_of(h, &lpr, &G, &R, &lds);
    out[0] = ok && msdp_blockpersist_eligible(h) ? 1 : 0; out[1] = lpr; out[2] = G; out[3] = R; out[4] = (int32_t)lds;
    return 0;
}
