// msdp_blockfactor.hip -- what runs BETWEEN two trustregions() calls of the block kinds (MANI_STIEFEL: the unit-block-diagonal
// kind, efree = 0, and the pose-graph kind, efree = 1; d in {2, 3}) without the factor leaving the device, and the rounding after
// the solve:
//   msdp_blockfactor_gram     G = Y'Y (p x p) for the rank decision (the kernels of msdp_factor_gram)
//   msdp_blockfactor_rotate   Y <- polar_blocks(Y Q), new width r                 (the rank cut)
//   msdp_blockfactor_append   Y <- polar_blocks([Y, alpha V]), new width p + k    (the escape widening)
//   msdp_blockfactor_round    R_i = the nearest rotation to Y_i W (and t_i = tau_i W), the determinant sign by majority
// polar_blocks replaces the d rotation rows of every block by their polar factor (A A')^(-1/2) A; a free row (pose-graph kind) is
// the plain product / concatenation.  The oblique calls msdp_factor_* stay refused for these handles (msdp_api.hip).
//
// Rotate and append are two launches: the plain product / concatenation into the OTHER point slot at its new row stride (the
// kernels of msdp_factor_rotate / _append, which also zero the pad columns), then k_blk_polar in place over that slot -- a lane
// group of LPR lanes owns one block, its d rows of NCH double2 each in registers as in k_stf_retract, so no block is read after
// another has been written.  The calls are launch-bound (n = 10 000, p = 8: 80 000 x 8 doubles).
//
// Unlike the retraction (G = I + eta eta' >= I) the Gram matrix G = A A' of a block met here can be as ill-conditioned as the
// rank cut makes it.  One application of G^(-1/2) from a Jacobi eigen-decomposition leaves |A A' - I| ~ 4 eps cond(G); the
// kernel therefore applies it TWICE -- the second pass starts from cond ~ 1 and ends at rounding.  A block whose first-pass
// eigenvalues satisfy lambda_min <= 1e-12 lambda_max (an eigenvalue carries an absolute error of a few eps lambda_max: at this
// ratio it still has about three digits, enough for the second pass to be well-posed; an exactly singular G and a zero block
// are included) is DEGENERATE: the kernel leaves it as it is and counts it.  With a non-zero count the call returns 0 with
// *ndeg set and does NOT adopt the new point: the resident point, its width and the handle's state are as before, and the caller
// takes that re-shape on the host (whose SVD picks an arbitrary factor there).
// No floating-point atomics (the counters are integers), no inline assembly.
#include "msdp_device.h"
#include <algorithm>

#define BF_THREADS 256          // 4 waves a workgroup: the kernels below hold a block in at most 2 * 3 * 2 double2 per lane

// first-pass eigenvalues -> the block has a usable polar factor (false on a NaN as well)
template <int D>
__device__ __forceinline__ bool bf_well_posed(const double (&lam)[D]) {
    double lmin = lam[0], lmax = lam[0];
#pragma unroll
    for (int k = 1; k < D; ++k) { lmin = fmin(lmin, lam[k]); lmax = fmax(lmax, lam[k]); }
    return lmin > 1e-12 * lmax;
}

// The d rotation rows of every block of Y (nb blocks of D + EF rows, row stride ld) <- their polar factor, in place, two passes
template <int D, int EF, int LPR, int NCH>
__global__ __launch_bounds__(BF_THREADS) void k_blk_polar(double* __restrict__ Y, int nb, int ld, int* __restrict__ ndeg) {
    constexpr int B = D + EF, BPW = 64 / LPR, WAVES = BF_THREADS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    for (int b0 = (blockIdx.x * WAVES + wave) * BPW; b0 < nb; b0 += gridDim.x * WAVES * BPW) {
        const int blk = b0 + rsub;
        if (blk < nb) {
            double2 x[D][NCH];
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    x[a][ch] = (col < ld) ? ld2(Y + ((int64_t)blk * B + a) * ld + col) : make_double2(0.0, 0.0);
                }
            bool ok = true;
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                double Gm[D][D], R[D][D], lam[D];
                msdp_block_symdot<D, LPR, NCH>(x, x, Gm);       // A A': the same bits in every lane of the group
                msdp_sym_invsqrt_eig<D>(Gm, R, lam, false);
                if (pass == 0) ok = bf_well_posed<D>(lam);
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    double2 t[D];
#pragma unroll
                    for (int a = 0; a < D; ++a) {
                        t[a] = make_double2(0.0, 0.0);
#pragma unroll
                        for (int b = 0; b < D; ++b) { t[a].x += R[a][b] * x[b][ch].x; t[a].y += R[a][b] * x[b][ch].y; }
                    }
#pragma unroll
                    for (int a = 0; a < D; ++a) x[a][ch] = t[a];
                }
            }
            if (ok) {
#pragma unroll
                for (int a = 0; a < D; ++a)
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) {
                        const int col = 2 * sub + ch * 2 * LPR;
                        if (col < ld) st2(Y + ((int64_t)blk * B + a) * ld + col, x[a][ch]);
                    }
            } else if (sub == 0) {
                atomicAdd(ndeg, 1);
            }
        }
    }
}

// Rounding, first launch: Zt_i = [Y_i; tau_i] W (D + EF rows of D entries, W p x D row-major) and the count of det Z_i < 0
template <int D, int EF, int LPR, int NCH>
__global__ __launch_bounds__(BF_THREADS) void k_blk_round_z(const double* __restrict__ Y, int nb, int ld, int p, const double* __restrict__ W,
                                                            double* __restrict__ Zt, int* __restrict__ nneg) {
    constexpr int B = D + EF, BPW = 64 / LPR, WAVES = BF_THREADS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    double w[NCH][2][D];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int col = 2 * sub + ch * 2 * LPR + e;
#pragma unroll
            for (int c = 0; c < D; ++c) w[ch][e][c] = (col < p) ? W[(int64_t)col * D + c] : 0.0;
        }
    for (int b0 = (blockIdx.x * WAVES + wave) * BPW; b0 < nb; b0 += gridDim.x * WAVES * BPW) {
        const int blk = b0 + rsub;
        if (blk < nb) {
            double Z[B][D];
#pragma unroll
            for (int a = 0; a < B; ++a) {
                double2 y[NCH];
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    y[ch] = (col < ld) ? ld2(Y + ((int64_t)blk * B + a) * ld + col) : make_double2(0.0, 0.0);
                }
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    double s = 0.0;
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) s += y[ch].x * w[ch][0][c] + y[ch].y * w[ch][1][c];
                    Z[a][c] = msdp_group_sum<LPR>(s);
                }
            }
            if (sub == 0) {
                double det;
                if (D == 2) det = Z[0][0] * Z[1][1] - Z[0][1] * Z[1][0];
                else det = Z[0][0] * (Z[1][1] * Z[D - 1][D - 1] - Z[1][D - 1] * Z[D - 1][1])
                         - Z[0][1] * (Z[1][0] * Z[D - 1][D - 1] - Z[1][D - 1] * Z[D - 1][0])
                         + Z[0][D - 1] * (Z[1][0] * Z[D - 1][1] - Z[1][1] * Z[D - 1][0]);
#pragma unroll
                for (int a = 0; a < B; ++a)
#pragma unroll
                    for (int c = 0; c < D; ++c) Zt[((int64_t)blk * B + a) * D + c] = Z[a][c];
                if (det < 0.0) atomicAdd(nneg, 1);
            }
        }
    }
}

// Rounding, second launch, one thread per block: the global reflection where the majority of the determinants is negative (last
// column of Z_i, last entry of t_i), then R_i = the nearest rotation to Z_i = V diag(lambda^(-1/2) s) V' Z_i from Z_i Z_i' =
// V diag(lambda) V', s = -1 on the smallest eigenvalue where det Z_i < 0; a second plain pass as in k_blk_polar
template <int D, int EF>
__global__ __launch_bounds__(BF_THREADS) void k_blk_round_rot(const double* __restrict__ Zt, int nb, const int* __restrict__ nneg,
                                                              double* __restrict__ Rout, double* __restrict__ tout, int* __restrict__ ndeg) {
    constexpr int B = D + EF;
    const bool flip = 2 * (int64_t)(*nneg) > nb;
    for (int blk = blockIdx.x * blockDim.x + threadIdx.x; blk < nb; blk += gridDim.x * blockDim.x) {
        double Z[D][D];
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int c = 0; c < D; ++c) {
                const double v = Zt[((int64_t)blk * B + a) * D + c];
                Z[a][c] = (flip && c == D - 1) ? -v : v;
            }
        if (EF) {
#pragma unroll
            for (int c = 0; c < D; ++c) {
                const double v = Zt[((int64_t)blk * B + D) * D + c];
                tout[(int64_t)blk * D + c] = (flip && c == D - 1) ? -v : v;
            }
        }
        double det;
        if (D == 2) det = Z[0][0] * Z[1][1] - Z[0][1] * Z[1][0];
        else det = Z[0][0] * (Z[1][1] * Z[D - 1][D - 1] - Z[1][D - 1] * Z[D - 1][1])
                 - Z[0][1] * (Z[1][0] * Z[D - 1][D - 1] - Z[1][D - 1] * Z[D - 1][0])
                 + Z[0][D - 1] * (Z[1][0] * Z[D - 1][1] - Z[1][1] * Z[D - 1][0]);
        bool ok = true;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            double Gm[D][D], R[D][D], lam[D], T[D][D];
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = a; b < D; ++b) {
                    double s = 0.0;
#pragma unroll
                    for (int c = 0; c < D; ++c) s += Z[a][c] * Z[b][c];
                    Gm[a][b] = Gm[b][a] = s;
                }
            msdp_sym_invsqrt_eig<D>(Gm, R, lam, pass == 0 && det < 0.0);
            if (pass == 0) ok = bf_well_posed<D>(lam);
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    double s = 0.0;
#pragma unroll
                    for (int b = 0; b < D; ++b) s += R[a][b] * Z[b][c];
                    T[a][c] = s;
                }
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int c = 0; c < D; ++c) Z[a][c] = T[a][c];
        }
        if (ok) {
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int c = 0; c < D; ++c) Rout[(int64_t)blk * (D * D) + a * D + c] = Z[a][c];
        } else {
            atomicAdd(ndeg, 1);
        }
    }
}

// ------------------------------------------------------------------ launchers
// One instance per lanes-per-block count of the row stride `ld_` (the new one of a rotate / append): MSDP_BLOCK_WIDTH_LADDER
static int bf_grid(int nb, int lpr) {
    const int per_wg = (BF_THREADS / 64) * (64 / lpr);
    return std::max(1, std::min(1024, (nb + per_wg - 1) / per_wg));
}
#define BF_DISPATCH_L(KERNEL, DD, EE, h, nb_, ld_, ...)                                              \
    do {                                                                                             \
        MSDP_BLOCK_WIDTH_LADDER(ld_, hipLaunchKernelGGL((KERNEL<DD, EE, LPR_, NCH_>), dim3(bf_grid(nb_, LPR_)), dim3(BF_THREADS), 0, \
                                                        (h)->stream, __VA_ARGS__))                  \
        { msdp_set_error("block factor: row stride %d exceeds the supported maximum of 256", (int)(ld_)); return MSDP_EUNSUPPORTED; } \
    } while (0)
#define BF_DISPATCH(KERNEL, h, nb_, ld_, ...)                                                        \
    do {                                                                                             \
        const int dd_ = (h)->d.blk - (h)->d.efree;                                                   \
        if (dd_ == 2 && !(h)->d.efree) BF_DISPATCH_L(KERNEL, 2, 0, h, nb_, ld_, __VA_ARGS__);        \
        else if (dd_ == 3 && !(h)->d.efree) BF_DISPATCH_L(KERNEL, 3, 0, h, nb_, ld_, __VA_ARGS__);   \
        else if (dd_ == 2) BF_DISPATCH_L(KERNEL, 2, 1, h, nb_, ld_, __VA_ARGS__);                    \
        else BF_DISPATCH_L(KERNEL, 3, 1, h, nb_, ld_, __VA_ARGS__);                                  \
        HIPCHK(hipGetLastError());                                                                   \
    } while (0)

// The handle is one of the two block kinds (d in {2, 3}, efree in {0, 1}); otherwise the error names the call
static int bf_check_kind(msdp_handle h, const char* call) {
    const Dev& d = h->d;
    const int dd = d.blk - d.efree;
    if (d.manifold != MANI_STIEFEL || d.costkind != COST_BLOCK || !d.brp || (d.efree != 0 && d.efree != 1) || (dd != 2 && dd != 3) ||
        h->nranks != 1 || h->use_comm) {
        msdp_set_error("%s: for unit-block-diagonal and pose-graph handles only (the other kinds take msdp_factor_gram / _rotate / _append)", call);
        return MSDP_EUNSUPPORTED;
    }
    return 0;
}

// one device allocation for a call: `doubles` doubles, then `ints` zeroed ints
static int bf_scratch(msdp_handle h, const char* call, size_t doubles, size_t ints, double** dbl, int** cnt) {
    void* buf = nullptr;
    if (hipMalloc(&buf, (doubles ? doubles : 1) * sizeof(double) + (ints ? ints : 1) * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        msdp_set_error("%s: scratch alloc failed", call);
        return MSDP_ENOMEM;
    }
    *dbl = (double*)buf;
    *cnt = (int*)(*dbl + (doubles ? doubles : 1));
    if (hipMemsetAsync(*cnt, 0, (ints ? ints : 1) * sizeof(int), h->stream) != hipSuccess) {
        (void)hipFree(buf);
        msdp_set_error("%s: scratch memset failed", call);
        return MSDP_EHIP;
    }
    return 0;
}

extern "C" int msdp_blockfactor_gram(msdp_handle h, double* G) {
    MSDP_CHECK_H(h);
    int rc = bf_check_kind(h, "blockfactor_gram");
    if (rc) return rc;
    if (!h->have_point || !G) { msdp_set_error("blockfactor_gram: no resident point / null out"); return MSDP_ESTATE; }
    Dev& d = h->d;
    const int ld = d.ld, p = d.p;
    const int nblk = (int)std::min<int64_t>(64, std::max<int64_t>(1, (int64_t)(1 << 22) / ((int64_t)ld * ld)));
    double* buf = nullptr; int* cnt = nullptr;
    if ((rc = bf_scratch(h, "blockfactor_gram", ((size_t)nblk + 1) * ld * ld, 1, &buf, &cnt))) return rc;
    double* out = buf + (size_t)nblk * ld * ld;
    rc = msdp_k_fgram(h, d.Y[msdp_host_cur(h)], buf, nblk, out);
    if (!rc && msdp_memcpy2d_async(G, (size_t)p * sizeof(double), out, (size_t)ld * sizeof(double), (size_t)p * sizeof(double), p,
                                   hipMemcpyDeviceToHost, h->stream) != hipSuccess) { msdp_set_error("blockfactor_gram: D2H failed"); rc = MSDP_EHIP; }
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(buf);
    return rc;
}

// After the plain product / concatenation stands in slot `to` at row stride ldn: the polar pass, the count, then adopt or undo
static int bf_polar_and_adopt(msdp_handle h, const char* call, int to, int pn, int ldn, int* cnt, int32_t* ndeg) {
    Dev& d = h->d;
    BF_DISPATCH(k_blk_polar, h, d.nb, ldn, d.Y[to], d.nb, ldn, cnt);
    int bad = 0;
    if (msdp_memcpy_async(&bad, cnt, sizeof(int), hipMemcpyDeviceToHost, h->stream) != hipSuccess) { msdp_set_error("%s: D2H failed", call); return MSDP_EHIP; }
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t slot_bytes = (size_t)msdp_rows_capacity(h) * h->ldcap * sizeof(double);
    *ndeg = bad;
    if (bad) {                                             // not adopted: the other slot as msdp_set_point left it
        HIPCHK(hipMemsetAsync(d.Y[to], 0, slot_bytes, h->stream));
        return 0;
    }
    int rc = msdp_adopt_point(h, to, pn);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(d.Y[to ^ 1], 0, slot_bytes, h->stream));     // the old point at the old stride: nothing of it stays behind
    return 0;
}

extern "C" int msdp_blockfactor_rotate(msdp_handle h, int32_t r, const double* Q, int32_t* ndeg) {
    MSDP_CHECK_H(h);
    int rc = bf_check_kind(h, "blockfactor_rotate");
    if (rc) return rc;
    if (!h->have_point) { msdp_set_error("blockfactor_rotate: no resident point"); return MSDP_ESTATE; }
    if (!Q || !ndeg) { msdp_set_error("blockfactor_rotate: null argument"); return MSDP_EINVAL; }
    Dev& d = h->d;
    const int dd = d.blk - d.efree;
    if (r < dd || r > d.p) { msdp_set_error("blockfactor_rotate: r = %d outside d = %d .. p = %d (d orthonormal rows need d columns)", r, dd, d.p); return MSDP_EINVAL; }
    const int cur = msdp_host_cur(h), ldn = ((r + 1) / 2) * 2;
    double* qd = nullptr; int* cnt = nullptr;
    if ((rc = bf_scratch(h, "blockfactor_rotate", (size_t)d.p * r, 1, &qd, &cnt))) return rc;
    if (msdp_memcpy_async(qd, Q, (size_t)d.p * r * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess) { msdp_set_error("blockfactor_rotate: H2D failed"); rc = MSDP_EHIP; }
    if (!rc) rc = msdp_k_frotate(h, msdp_rows_capacity(h), r, ldn, d.Y[cur], qd, d.Y[cur ^ 1]);
    if (!rc) rc = bf_polar_and_adopt(h, "blockfactor_rotate", cur ^ 1, r, ldn, cnt, ndeg);
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(qd);
    return rc;
}

extern "C" int msdp_blockfactor_append(msdp_handle h, int32_t k, const double* V, double alpha, int32_t* ndeg) {
    MSDP_CHECK_H(h);
    int rc = bf_check_kind(h, "blockfactor_append");
    if (rc) return rc;
    if (!h->have_point) { msdp_set_error("blockfactor_append: no resident point"); return MSDP_ESTATE; }
    if (!V || !ndeg || k < 1) { msdp_set_error("blockfactor_append: k = %d / null argument", k); return MSDP_EINVAL; }
    Dev& d = h->d;
    if (d.p + k > h->pcap || d.p + k > MSDP_BLOCK_PMAX) { msdp_set_error("blockfactor_append: width %d exceeds the allocated capacity %d (use msdp_set_point)", d.p + k, std::min(h->pcap, MSDP_BLOCK_PMAX)); return MSDP_EUNSUPPORTED; }
    const int cur = msdp_host_cur(h), pn = d.p + k, ldn = ((pn + 1) / 2) * 2;
    double* vd = nullptr; int* cnt = nullptr;
    if ((rc = bf_scratch(h, "blockfactor_append", (size_t)d.n * k, 1, &vd, &cnt))) return rc;
    if (msdp_memcpy_async(vd, V, (size_t)d.n * k * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess) { msdp_set_error("blockfactor_append: H2D failed"); rc = MSDP_EHIP; }
    if (!rc) rc = msdp_k_fappend(h, msdp_rows_capacity(h), k, ldn, d.Y[cur], vd, alpha, 0, d.Y[cur ^ 1]);
    if (!rc) rc = bf_polar_and_adopt(h, "blockfactor_append", cur ^ 1, pn, ldn, cnt, ndeg);
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(vd);
    return rc;
}

static int bf_round_launch(msdp_handle h, const double* Y, const double* Wd, double* Zt, double* Rd, double* td, int* cnt) {
    Dev& d = h->d;
    BF_DISPATCH(k_blk_round_z, h, d.nb, d.ld, Y, d.nb, d.ld, d.p, Wd, Zt, cnt);
    const dim3 gr((d.nb + BF_THREADS - 1) / BF_THREADS), bl(BF_THREADS);
    const int dd = d.blk - d.efree;
    if (dd == 2 && !d.efree) hipLaunchKernelGGL((k_blk_round_rot<2, 0>), gr, bl, 0, h->stream, (const double*)Zt, d.nb, (const int*)cnt, Rd, td, cnt + 1);
    else if (dd == 3 && !d.efree) hipLaunchKernelGGL((k_blk_round_rot<3, 0>), gr, bl, 0, h->stream, (const double*)Zt, d.nb, (const int*)cnt, Rd, td, cnt + 1);
    else if (dd == 2) hipLaunchKernelGGL((k_blk_round_rot<2, 1>), gr, bl, 0, h->stream, (const double*)Zt, d.nb, (const int*)cnt, Rd, td, cnt + 1);
    else hipLaunchKernelGGL((k_blk_round_rot<3, 1>), gr, bl, 0, h->stream, (const double*)Zt, d.nb, (const int*)cnt, Rd, td, cnt + 1);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int msdp_blockfactor_round(msdp_handle h, const double* W, double* R, double* t, int32_t* flipped, int32_t* ndeg) {
    MSDP_CHECK_H(h);
    int rc = bf_check_kind(h, "blockfactor_round");
    if (rc) return rc;
    Dev& d = h->d;
    if (!W || !R || !flipped || !ndeg) { msdp_set_error("blockfactor_round: null argument"); return MSDP_EINVAL; }
    if ((d.efree != 0) != (t != nullptr)) { msdp_set_error("blockfactor_round: t must be NULL for a unit-block-diagonal handle and non-NULL for a pose-graph handle"); return MSDP_EINVAL; }
    if (!h->have_point) { msdp_set_error("blockfactor_round: no resident point"); return MSDP_ESTATE; }
    const int dd = d.blk - d.efree;
    const size_t nW = (size_t)d.p * dd, nZ = (size_t)d.nb * d.blk * dd, nR = (size_t)d.nb * dd * dd, nT = (size_t)d.nb * dd;
    double* buf = nullptr; int* cnt = nullptr;
    if ((rc = bf_scratch(h, "blockfactor_round", nW + nZ + nR + nT, 2, &buf, &cnt))) return rc;
    double* Wd = buf; double* Zt = Wd + nW; double* Rd = Zt + nZ; double* td = Rd + nR;
    if (hipMemsetAsync(Rd, 0, (nR + nT) * sizeof(double), h->stream) != hipSuccess ||
        msdp_memcpy_async(Wd, W, nW * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess) { msdp_set_error("blockfactor_round: H2D failed"); rc = MSDP_EHIP; }
    if (!rc) rc = bf_round_launch(h, d.Y[msdp_host_cur(h)], Wd, Zt, Rd, td, cnt);
    int c2[2] = {0, 0};
    if (!rc && (msdp_memcpy_async(R, Rd, nR * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                (t && msdp_memcpy_async(t, td, nT * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess) ||
                msdp_memcpy_async(c2, cnt, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream) != hipSuccess)) { msdp_set_error("blockfactor_round: D2H failed"); rc = MSDP_EHIP; }
    if (hipStreamSynchronize(h->stream) != hipSuccess && !rc) { msdp_set_error("blockfactor_round: device error"); rc = MSDP_EHIP; }
    (void)hipFree(buf);
    if (rc) return rc;
    *flipped = (2 * (int64_t)c2[0] > d.nb) ? 1 : 0;
    *ndeg = c2[1];
    return 0;
}
