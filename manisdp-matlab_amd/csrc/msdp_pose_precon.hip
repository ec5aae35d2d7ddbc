// msdp_pose_precon.hip -- block-Jacobi preconditioned truncated CG for the pose-graph kind (msdp_stiefel.hip at EF = 1; option "precon" of
// msdp_set_option, default off).  The device follows the preconditioned branch of Manopt's tCG (tCG.m:117-125, :260-287) where
// the generic trips follow the identity branch:
//   M_i = sym(C_[ii])     the diagonal block of order B = d + 1 of pose i -- fixed for the life of the handle, unscaled,
//                         independent of the point and of Lambda; inverted once on the host (fp64 Cholesky), nb * B * B doubles
//   precon(x, r) = tangent_x(blockdiag(M_i^-1) r): Stiefel projection on the rotation rows, identity on the free row --
//                         symmetric positive definite on the tangent space
// The trust region is measured in the M-norm (e_Pe, e_Pd, d_Pd of the frame are M-inner products, as in Manopt); Delta_bar and
// Delta0 keep their values.  The stop test (:249) stays on norm_r = sqrt(<r, r>) and norm_r0 = sqrt(gg).
//
// A trip stays three launches: k_stf_hess as it is, then
//   k_pose_pc_upd1   tCG.m:166-241, the decisions of k_tcg_upd1 block by block; with the rows of the new r of a block in registers
//                    also z = tangent(M_i^-1 r) -> d.pcz and a fourth partial sum <z, r>
//   k_pose_pc_upd2   tCG.m:227-287 with beta = <z, r> / <z_old, r_old> and mdelta = tangent(z + beta mdelta)
// and k_pose_pc_init in place of k_tcg_init (tCG.m:102-157: r = grad, z = precon(r), mdelta = z, eta = Heta = 0).  <z, r> of the
// start is a grid sum of its own: the init launch leaves its partials in P_ZR0, and the first upd1 of a tCG (frame `fresh`) sums
// them where later ones read z_r and d_Pd from the frame -- no host synchronisation.  upd1 writes its <z, r_new> partials to
// another array, P_ZRN, since the workgroups of that first launch still read P_ZR0.  Neither array is used by the kind otherwise.
//
// Lane layout and instances are those of msdp_stiefel.hip: LPR lanes own a block, NCH double2 per row and lane, widths up to 256
// (the ladder and the workgroup sizes BlockRows / BlockRows3 of msdp_device.h; the first update holds four rows of the new r and
// of z, three of y and the 4 x 4 values of M_i^-1 beside the six streamed operands at d = 3: the three-vector size).  Only r_new,
// z and the D rotation rows of Y are resident per block; eta, Heta, mdelta, H mdelta and the
// gradient stream through.  No instance uses scratch (DESIGN.md lists the registers per instance).
// The kernels of msdp_stiefel.hip and msdp_kernels.hip are not touched (msdp_tcg_upd2_scalars serves both, by a compile-time switch): what selects these launchers is
// d.pcM != nullptr, a field of Dev, so the chunk graph (whose signature is the Dev) is captured again when the option flips.
#include "msdp_device.h"
#include <math.h>
#include <cmath>
#include <vector>

// z = tangent_y(Minv r) for one block held by a lane group: z[a] = sum_b Minv[a][b] r[b] (b ascending), then the rotation rows
// minus sym(z y') y; the free row stays.  mi: the B * B values of the block, row-major (the same addresses in every lane)
template <int D, int LPR, int NCH>
__device__ __forceinline__ void pc_apply_block(const double* __restrict__ mi, const double2 (&r)[D + 1][NCH], const double2 (&y)[D][NCH],
                                               double2 (&z)[D + 1][NCH]) {
    constexpr int B = D + 1;
#pragma unroll
    for (int a = 0; a < B; ++a) {
        double m[B];
#pragma unroll
        for (int b = 0; b < B; ++b) m[b] = mi[a * B + b];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            double2 s = make_double2(m[0] * r[0][ch].x, m[0] * r[0][ch].y);
#pragma unroll
            for (int b = 1; b < B; ++b) { s.x = fma(m[b], r[b][ch].x, s.x); s.y = fma(m[b], r[b][ch].y, s.y); }
            z[a][ch] = s;
        }
    }
    double T[D][D];
    msdp_block_symdot<D, LPR, NCH>(z, y, T);
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b)
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) { z[a][ch].x -= T[a][b] * y[b][ch].x; z[a][ch].y -= T[a][b] * y[b][ch].y; }
}

// the D rotation rows of block blk of Y (zero beyond the row stride)
template <int D, int LPR, int NCH>
__device__ __forceinline__ void pc_load_rot(const Dev& d, const double* __restrict__ Yl, int blk, int sub, double2 (&y)[D][NCH]) {
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const int col = 2 * sub + ch * 2 * LPR;
            y[a][ch] = (col < d.ld) ? ld2(Yl + ((int64_t)blk * (D + 1) + a) * d.ld + col) : make_double2(0.0, 0.0);
        }
}

// Z = tangent_Y(blockdiag(M_i^-1) R) for vectors in the handle's layout (msdp_precon_apply)
template <int D, int LPR, int NCH>
__global__ __launch_bounds__((BlockRows<D + 1, NCH>::threads)) void k_pose_pc_apply(Dev d, const double* __restrict__ Yl,
                                                                               const double* __restrict__ R, double* __restrict__ Z) {
    constexpr int B = D + 1, WAVES = BlockRows<D + 1, NCH>::threads / 64, BPW = 64 / LPR;
    int lo, hi;
    msdp_chunk_rows(d.nb, d.G, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    for (int b0 = lo + wave * BPW; b0 < hi; b0 += WAVES * BPW) {
        const int blk = b0 + rsub;
        if (blk < hi) {
            double2 r[B][NCH], y[D][NCH], z[B][NCH];
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    r[a][ch] = (col < d.ld) ? ld2(R + ((int64_t)blk * B + a) * d.ld + col) : make_double2(0.0, 0.0);
                }
            pc_load_rot<D, LPR, NCH>(d, Yl, blk, sub, y);
            pc_apply_block<D, LPR, NCH>(d.pcM + (int64_t)blk * (B * B), r, y, z);
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    if (col < d.ld) st2(Z + ((int64_t)blk * B + a) * d.ld + col, z[a][ch]);
                }
        }
    }
}

// tCG.m:102-157: eta = 0, Heta = 0, r = grad, z = precon(r), mdelta = z; the partials of <z, r> -> P_ZR0.  The frame carries
// gg in z_r and d_Pd until the first upd1 replaces them by that sum (`fresh`); norm_r0 = sqrt(gg)
template <int D, int LPR, int NCH>
__global__ __launch_bounds__((BlockRows<D + 1, NCH>::threads)) void k_pose_pc_init(Dev d) {
    __shared__ double sh[3 * MSDP_WAVES];
    const Ctl* c = d.ctl;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int act = c->done ? 0 : 1;
        frame_store(&d.F[0], c->gg, c->gg, 0.0, 0.0, 0.0, sqrt(c->gg), 0.0, 0.0, act, 0, 5, 0, 0, 1);
        frame_store(&d.F[1], c->gg, c->gg, 0.0, 0.0, 0.0, sqrt(c->gg), 0.0, 0.0, act, 0, 5, 0, 0, 1);
        d.ctl->tcg_running = act;
        msdp_publish(d, c->k, 0, act);
    }
    if (c->done) return;
    constexpr int B = D + 1, WAVES = BlockRows<D + 1, NCH>::threads / 64, BPW = 64 / LPR;
    int lo, hi;
    msdp_chunk_rows(d.nb, d.G, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    const double* __restrict__ Yl = c->cur ? d.Y[1] : d.Y[0];
    const double* __restrict__ g = c->cur ? d.Gr[1] : d.Gr[0];
    const double2 zero = make_double2(0.0, 0.0);
    double pzr = 0.0;
    for (int b0 = lo + wave * BPW; b0 < hi; b0 += WAVES * BPW) {
        const int blk = b0 + rsub;
        if (blk < hi) {
            double2 r[B][NCH], y[D][NCH], z[B][NCH];
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    r[a][ch] = (col < d.ld) ? ld2(g + ((int64_t)blk * B + a) * d.ld + col) : zero;
                }
            pc_load_rot<D, LPR, NCH>(d, Yl, blk, sub, y);
            pc_apply_block<D, LPR, NCH>(d.pcM + (int64_t)blk * (B * B), r, y, z);
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    if (col < d.ld) {
                        const int64_t o = ((int64_t)blk * B + a) * d.ld + col;
                        st2(d.r + o, r[a][ch]);
                        st2(d.md + o, z[a][ch]);
                        st2(d.eta[0] + o, zero);
                        st2(d.Heta[0] + o, zero);
                        pzr += z[a][ch].x * r[a][ch].x + z[a][ch].y * r[a][ch].y;
                    }
                }
        }
    }
    msdp_put_partial(d.P, P_ZR0, pzr, sh);
}

// tCG.m:166-241, block-shaped: the decisions of k_tcg_upd1 (negative curvature or boundary exit with tau; else new_eta,
// new_Heta, the new r and the sums s1, s2, r_r), and with the rows of the new r of a block in registers z = tangent(M_i^-1 r)
// -> d.pcz and the fourth sum <z, r>
template <int D, int LPR, int NCH>
__global__ __launch_bounds__((BlockRows3<D + 1, NCH>::threads)) void k_pose_pc_upd1(Dev d) {
    __shared__ double sh[3 * MSDP_WAVES];
    __shared__ double sh4[3 * MSDP_WAVES];
    __shared__ double shb[2];
    const Frame* fi = &d.F[0];
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    const int active = fi->active, fresh = fi->fresh;
    double z_r = fi->z_r, d_Pd = fi->d_Pd;
    const double e_Pd = fi->e_Pd, e_Pe = fi->e_Pe;
    const double model_value = fi->model_value, norm_r0 = fi->norm_r0, beta0 = fi->beta, alpha0 = fi->alpha;
    const int j = fi->j, stop0 = fi->stop, ix = fi->eta_idx, mi = fi->md_idx;
    if (!active) {
        if (lead) frame_store(&d.F[1], z_r, d_Pd, e_Pd, e_Pe, model_value, norm_r0, alpha0, beta0, 0, j, stop0, ix, mi, 0);
        return;
    }
    const Ctl* c = d.ctl;
    const bool bench = c->bench_mode != 0;
    const double Delta = c->Delta;
    constexpr int B = D + 1, WAVES = BlockRows3<D + 1, NCH>::threads / 64, BPW = 64 / LPR;
    int lo, hi;
    msdp_chunk_rows(d.nb, d.G, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    const double* __restrict__ eta = ix ? d.eta[1] : d.eta[0];
    const double* __restrict__ Heta = ix ? d.Heta[1] : d.Heta[0];
    double* __restrict__ neta = ix ? d.eta[0] : d.eta[1];
    double* __restrict__ nHeta = ix ? d.Heta[0] : d.Heta[1];
    const double* __restrict__ g = c->cur ? d.Gr[1] : d.Gr[0];
    const double* __restrict__ Yl = c->cur ? d.Y[1] : d.Y[0];
    const double* __restrict__ mdp = d.md;
    // <mdelta, H mdelta> (:166) and, on the first trip of a tCG, z_r(0) = d_Pd(0) = <z, r> of the init launch
    if (threadIdx.x < 64) {
        const double a = msdp_sum_partials(d.P, P_DHD, d.G);
        const double b = fresh ? msdp_sum_partials(d.P, P_ZR0, d.G) : 0.0;
        if (threadIdx.x == 0) { shb[0] = a; shb[1] = b; }
    }
    __syncthreads();
    const double d_Hd = shb[0];
    if (fresh) { z_r = shb[1]; d_Pd = z_r; }
    const double alpha = z_r / d_Hd;                                           // :170
    const double e_Pe_new = tcg_e_Pe_new(e_Pe, alpha, e_Pd, d_Pd);
    if (!bench && !tcg_step_inside(d_Hd, e_Pe_new, Delta)) {
        const double tau = tcg_tau(e_Pd, d_Pd, e_Pe, Delta);
        for (int b0 = lo + wave * BPW; b0 < hi; b0 += WAVES * BPW) {
            const int blk = b0 + rsub;
            if (blk < hi) {
#pragma unroll
                for (int a = 0; a < B; ++a)
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) {
                        const int col = 2 * sub + ch * 2 * LPR;
                        if (col < d.ld) {
                            const int64_t o = ((int64_t)blk * B + a) * d.ld + col;
                            const double2 e = ld2(eta + o), he = ld2(Heta + o), m = ld2(mdp + o), hm = ld2(d.Hmd + o);
                            st2(neta + o, make_double2(e.x - tau * m.x, e.y - tau * m.y));          // :192
                            st2(nHeta + o, make_double2(he.x - tau * hm.x, he.y - tau * hm.y));    // :198
                        }
                    }
            }
        }
        if (lead) frame_store(&d.F[1], z_r, d_Pd, e_Pd, e_Pe, model_value, norm_r0, alpha0, beta0, 0, j + 1, tcg_boundary_stop(d_Hd), ix ^ 1, mi, 0);
        return;
    }
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    for (int b0 = lo + wave * BPW; b0 < hi; b0 += WAVES * BPW) {
        const int blk = b0 + rsub;
        if (blk < hi) {
            double2 nr[B][NCH], y[D][NCH], z[B][NCH];
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    nr[a][ch] = make_double2(0.0, 0.0);
                    if (col < d.ld) {
                        const int64_t o = ((int64_t)blk * B + a) * d.ld + col;
                        const double2 e = ld2(eta + o), he = ld2(Heta + o), m = ld2(mdp + o), hm = ld2(d.Hmd + o);
                        const double2 rr = ld2(d.r + o), gv = ld2(g + o);
                        const double2 ne = make_double2(e.x - alpha * m.x, e.y - alpha * m.y);         // :215
                        const double2 nh = make_double2(he.x - alpha * hm.x, he.y - alpha * hm.y);     // :220
                        const double2 rn = make_double2(rr.x - alpha * hm.x, rr.y - alpha * hm.y);     // :238
                        st2(neta + o, ne);
                        st2(nHeta + o, nh);
                        st2(d.r + o, rn);
                        nr[a][ch] = rn;
                        s1 += ne.x * gv.x + ne.y * gv.y;      // <new_eta, grad>     :227
                        s2 += ne.x * nh.x + ne.y * nh.y;      // <new_eta, new_Heta>
                        s3 += rn.x * rn.x + rn.y * rn.y;      // r_r                 :241
                    }
                }
            pc_load_rot<D, LPR, NCH>(d, Yl, blk, sub, y);
            pc_apply_block<D, LPR, NCH>(d.pcM + (int64_t)blk * (B * B), nr, y, z);                      // :265
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    if (col < d.ld) {
                        st2(d.pcz + ((int64_t)blk * B + a) * d.ld + col, z[a][ch]);
                        s4 += z[a][ch].x * nr[a][ch].x + z[a][ch].y * nr[a][ch].y;                    // <z, r>  :270
                    }
                }
        }
    }
    msdp_put_partials3(d.P, P_S1, s1, P_S2, s2, P_S3, s3, sh);
    msdp_put_partial(d.P, P_ZRN, s4, sh4);
    if (lead)   // :214
        frame_store(&d.F[1], z_r, d_Pd, e_Pd, e_Pe_new, model_value, norm_r0, alpha, beta0, 1, j, stop0, ix, mi, 0);
}

// tCG.m:227-287: the scalar decisions (msdp_tcg_upd2_scalars in its preconditioned form: beta = z_r_new / z_r with z_r_new = <z, r>
// of the upd1 launch, P_ZRN), then mdelta = tangent(z + beta mdelta) block by block (:273, :283)
template <int D, int LPR, int NCH>
__global__ __launch_bounds__((BlockRows<D + 1, NCH>::threads)) void k_pose_pc_upd2(Dev d) {
    __shared__ double shb[4];
    double beta;
    if (!msdp_tcg_upd2_scalars<true>(d, shb, beta)) return;
    constexpr int B = D + 1, WAVES = BlockRows<D + 1, NCH>::threads / 64, BPW = 64 / LPR;
    int lo, hi;
    msdp_chunk_rows(d.nb, d.G, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    const double* __restrict__ Yl = d.ctl->cur ? d.Y[1] : d.Y[0];
    for (int b0 = lo + wave * BPW; b0 < hi; b0 += WAVES * BPW) {
        const int blk = b0 + rsub;
        if (blk < hi) {
            double2 v[B][NCH], y[D][NCH];
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    v[a][ch] = make_double2(0.0, 0.0);
                    if (col < d.ld) {
                        const int64_t o = ((int64_t)blk * B + a) * d.ld + col;
                        const double2 zz = ld2(d.pcz + o), m = ld2(d.md + o);
                        v[a][ch] = make_double2(zz.x + beta * m.x, zz.y + beta * m.y);
                    }
                }
            pc_load_rot<D, LPR, NCH>(d, Yl, blk, sub, y);
            double T[D][D];
            msdp_block_symdot<D, LPR, NCH>(v, y, T);
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    if (col < d.ld) {
                        double2 t = v[a][ch];
                        if (a < D) {
#pragma unroll
                            for (int b = 0; b < D; ++b) { t.x -= T[a][b] * y[b][ch].x; t.y -= T[a][b] * y[b][ch].y; }
                        }
                        st2(d.md + ((int64_t)blk * B + a) * d.ld + col, t);
                    }
                }
        }
    }
}

// C_[ii] of every block row (zeros where the pattern has no diagonal entry): one thread per block, set-up only
template <int D>
__global__ void k_pose_pc_diag(int nb, const int* __restrict__ brp, const int* __restrict__ bci, const double* __restrict__ bval,
                               double* __restrict__ out) {
    constexpr int BB = (D + 1) * (D + 1);
    for (int blk = blockIdx.x * blockDim.x + threadIdx.x; blk < nb; blk += gridDim.x * blockDim.x) {
        int kd = -1;
        for (int k = brp[blk]; k < brp[blk + 1]; ++k) if (bci[k] == blk) kd = k;
        for (int q = 0; q < BB; ++q) out[(int64_t)blk * BB + q] = kd >= 0 ? bval[(int64_t)kd * BB + q] : 0.0;
    }
}

// ------------------------------------------------------------------ launchers
// one instance per lanes-per-block count (MSDP_BLOCK_WIDTH_LADDER, widths up to 256) and d
#define PC_LAUNCH_D(BLOCK, KERNEL, DD, h, ...)                                                              \
    MSDP_BLOCK_WIDTH_LADDER((h)->d.ld, hipLaunchKernelGGL((KERNEL<DD, LPR_, NCH_>), dim3((h)->d.G), dim3(BLOCK<DD + 1, NCH_>::threads), \
                                                          0, (h)->stream, __VA_ARGS__)) {                  \
        msdp_set_error("pose-graph handle: factor width p = %d exceeds the supported maximum of 256", (h)->d.p); \
        return MSDP_EUNSUPPORTED;                                                                           \
    }
#define PC_DISPATCH(BLOCK, KERNEL, h, ...)                                                                  \
    do {                                                                                                    \
        if ((h)->d.manifold != MANI_STIEFEL || !(h)->d.efree || !(h)->d.brp || !(h)->d.pcM || !(h)->d.pcz) { \
            msdp_set_error("preconditioned tCG: not a pose-graph handle with the option \"precon\" set");   \
            return MSDP_ESTATE;                                                                             \
        }                                                                                                   \
        if ((h)->d.blk == 3) { PC_LAUNCH_D(BLOCK, KERNEL, 2, h, __VA_ARGS__) }                              \
        else { PC_LAUNCH_D(BLOCK, KERNEL, 3, h, __VA_ARGS__) }                                              \
        HIPCHK(hipGetLastError());                                                                          \
    } while (0)

int msdp_pose_precon_init(msdp_handle h) {
    PC_DISPATCH(BlockRows, k_pose_pc_init, h, h->d);
    return 0;
}
int msdp_pose_precon_upd1(msdp_handle h) {
    PC_DISPATCH(BlockRows3, k_pose_pc_upd1, h, h->d);
    return 0;
}
int msdp_pose_precon_upd2(msdp_handle h) {
    PC_DISPATCH(BlockRows, k_pose_pc_upd2, h, h->d);
    return 0;
}
int msdp_pose_precon_apply(msdp_handle h, const double* Y, const double* R, double* Z) {
    PC_DISPATCH(BlockRows, k_pose_pc_apply, h, h->d, Y, R, Z);
    return 0;
}

// the vector z of the preconditioned trips, for the handle's current row capacity (msdp_alloc_vectors calls this again when the
// capacity grows)
int msdp_pose_precon_vectors(msdp_handle h) {
    const size_t cnt = (size_t)msdp_rows_capacity(h) * h->ldcap;
    if (h->pc_z_cap < cnt) {
        if (h->pc_z) msdp_dev_free(h, h->pc_z);
        h->pc_z = nullptr; h->pc_z_cap = 0;
        int rc = msdp_dev_alloc<double>(h, &h->pc_z, cnt);
        if (rc) return rc;
        h->pc_z_cap = cnt;
        HIPCHK(hipMemsetAsync(h->pc_z, 0, cnt * sizeof(double), h->stream));
    }
    if (h->d.pcM) h->d.pcz = h->pc_z;
    return 0;
}

static const char* pc_kind_name(msdp_handle h) {
    if (h->d.manifold == MANI_STIEFEL) return msdp_block_kind_name(h->d.efree);
    switch (h->kind) {
        case MSDP_KIND_ONLYUNITDIAG: return "onlyunitdiag";
        case MSDP_KIND_UNITDIAG: return "unitdiag";
        case MSDP_KIND_UNITTRACE: return "unittrace";
        case MSDP_KIND_GENERIC: return "generic";
        case MSDP_KIND_MULTIBLOCK: return "multiblock";
        case MSDP_KIND_DUAL_UNITDIAG: return "dual unitdiag";
        case MSDP_KIND_DUAL: return "dual";
        case MSDP_KIND_DUAL_MULTIBLOCK: return "dual multiblock";
    }
    return "unknown";
}

// Option "precon" (msdp_set_option).  on = 1: M_i^-1 of every block on the first call (the diagonal blocks are gathered on the
// device, symmetrised, factored and inverted on the host in fp64, uploaded once), the vector z; a block with a non-positive or
// non-finite pivot refuses the option and leaves the handle as it was.  on = 0: the generic trips again (the buffers are kept).
int msdp_pose_precon_set(msdp_handle h, int on) {
    Dev& d = h->d;
    if (d.manifold == MANI_STIEFEL && d.costkind == COST_BLOCK && !d.efree) {
        msdp_set_error("precon: not for a unit-block-diagonal handle (the diagonal blocks of its cost matrix are zero: there is nothing to invert)");
        return MSDP_EUNSUPPORTED;
    }
    if (d.manifold != MANI_STIEFEL || d.costkind != COST_BLOCK || !d.brp) {
        msdp_set_error("precon: the block-Jacobi preconditioner is the pose-graph kind's, this is a handle of the %s kind", pc_kind_name(h));
        return MSDP_EUNSUPPORTED;
    }
    if (!on) { d.pcM = nullptr; d.pcz = nullptr; return 0; }
    const int B = d.blk, BB = B * B;
    if (!h->pc_minv) {
        double* buf = nullptr;
        int rc = msdp_dev_alloc<double>(h, &buf, (size_t)d.nb * BB);
        if (rc) return rc;
        const dim3 gr((d.nb + 255) / 256), bl(256);
        if (B == 3) hipLaunchKernelGGL(k_pose_pc_diag<2>, gr, bl, 0, h->stream, d.nb, d.brp, d.bci, d.bval, buf);
        else hipLaunchKernelGGL(k_pose_pc_diag<3>, gr, bl, 0, h->stream, d.nb, d.brp, d.bci, d.bval, buf);
        std::vector<double> M((size_t)d.nb * BB);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = msdp_memcpy_async(M.data(), buf, M.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) { msdp_dev_free(h, buf); msdp_set_error("precon: reading the diagonal blocks failed: %s", hipGetErrorString(e)); return MSDP_EHIP; }
        for (int i = 0; i < d.nb; ++i) {
            double* m = M.data() + (size_t)i * BB;
            double A[4][4], L[4][4] = {}, Li[4][4] = {};
            for (int a = 0; a < B; ++a)
                for (int b = 0; b < B; ++b) A[a][b] = 0.5 * (m[a * B + b] + m[b * B + a]);
            for (int a = 0; a < B; ++a) {                                  // Cholesky A = L L'
                for (int b = 0; b <= a; ++b) {
                    double s = A[a][b];
                    for (int k = 0; k < b; ++k) s -= L[a][k] * L[b][k];
                    if (a == b) {
                        if (!(s > 0.0) || !std::isfinite(s)) {
                            msdp_dev_free(h, buf);
                            msdp_set_error("precon: diagonal block %d of the pose-graph cost matrix is not positive definite (pivot %d = %g)", i, a, s);
                            return MSDP_EUNSUPPORTED;
                        }
                        L[a][a] = std::sqrt(s);
                    } else L[a][b] = s / L[b][b];
                }
            }
            for (int c = 0; c < B; ++c)                                    // Li = L^-1 by forward substitution
                for (int a = c; a < B; ++a) {
                    double s = (a == c) ? 1.0 : 0.0;
                    for (int k = c; k < a; ++k) s -= L[a][k] * Li[k][c];
                    Li[a][c] = s / L[a][a];
                }
            for (int a = 0; a < B; ++a)                                    // A^-1 = Li' Li
                for (int b = 0; b < B; ++b) {
                    double s = 0.0;
                    for (int k = (a > b ? a : b); k < B; ++k) s += Li[k][a] * Li[k][b];
                    m[a * B + b] = s;
                    if (!std::isfinite(s)) {
                        msdp_dev_free(h, buf);
                        msdp_set_error("precon: the inverse of diagonal block %d of the pose-graph cost matrix is not finite", i);
                        return MSDP_EUNSUPPORTED;
                    }
                }
        }
        e = msdp_memcpy(buf, M.data(), M.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) { msdp_dev_free(h, buf); msdp_set_error("precon: uploading the inverse blocks failed: %s", hipGetErrorString(e)); return MSDP_EHIP; }
        h->pc_minv = buf;
    }
    d.pcM = h->pc_minv;
    int rc = msdp_pose_precon_vectors(h);
    if (rc) { d.pcM = nullptr; d.pcz = nullptr; }
    return rc;
}
