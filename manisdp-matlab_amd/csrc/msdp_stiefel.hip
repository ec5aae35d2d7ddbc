// msdp_stiefel.hip -- the unit-block-diagonal problem  min <C, X>  s.t. X PSD of order N = n d, X_[ii] = I_d  (synchronisation
// over O(d) / SO(d): rotation averaging, pose graphs), d in {2, 3}, on the stacked Stiefel manifold of its Burer-Monteiro factor
// (MANI_STIEFEL / COST_BLOCK, msdp_create_onlyunitblockdiag_csc; manopt's stiefelstackedfactory(n, d, p)).
//
// The factor Y (N x p, row-major, row stride ld) is n blocks of d consecutive rows with Y_i Y_i' = I_d.  With sym(M) = (M + M')/2
// and the project's scaling f = <C, Y Y'> / 2:
//   multiplier  Lambda_i = sym((C Y)_i Y_i')            S = C - blockdiag(Lambda),  <C, X> = sum_i tr Lambda_i
//   gradient    grad_i = (C Y)_i - Lambda_i Y_i                                    stiefelstackedfactory.m:81-87 (egrad2rgrad)
//   Hess-vec    W = C U - blockdiag(Lambda) U,  hess_i = W_i - sym(W_i Y_i') Y_i   :93-101 (W is projected, not C U alone:
//               Lambda_i U_i Y_i' is symmetric times skew and its symmetric part does not vanish for d >= 2)
//   tangent     Z_i - sym(Z_i Y_i') Y_i                                            :81-89
//   retraction  polar: A_i = Y_i + eta_i -> (A_i A_i')^(-1/2) A_i                  :103-117 (u v' of the thin SVD)
// At d = 1 these are the expressions of the oblique kernels (msdp_kernels.hip) with Lambda = eG.
//
// Storage: block CSR of block order d, built at set-up from the caller's CSC arrays -- one column index per d x d block, d^2
// values, zero-filled where the caller's pattern is partial.  A lane group of LPR lanes owns one BLOCK, its d rows of NCH double2
// each in registers: per block entry the d rows of the neighbour block are gathered once and used d times, the index traffic is
// 1 / d^2 of plain CSR.  Workgroup chunks are over blocks, so a block never straddles two workgroups.  Lambda lives per point
// slot (d.Lam[slot], the slot scheme of eG), its diagonal in eG[slot] so that msdp_get_z serves the kind unchanged.
// The kind runs the generic per-iteration path of msdp_rtr.hip (no persistent or fused trip, no row sharding).
// SIBLINGS: msdp_pose.hip holds a copy of every kernel below for blocks of d + 1 rows whose last row is free (the pose-graph
// kind, d.efree = 1; the launchers at the end of this file hand such a handle on).  The copies differ in B = D + 1, the a < D
// guards and msdp_block_symdot_lead only: a fix to a kernel here belongs there too.
#include "msdp_device.h"
#include <algorithm>
#include <math.h>
#include <vector>

// workgroup size of the row kernels: 16 waves hide the gather latency where a block fits 128 registers per lane (NCH = 1,
// widths up to 128); two chunks per lane (widths up to 256) take 8 waves and twice the registers
template <int NCH> struct StfBlock { static constexpr int threads = NCH == 1 ? 1024 : 512; };

// cost + Riemannian gradient + Lambda at Y[slot] (gather source: d.full holds all rows of Y[slot])
template <int D, int LPR, int NCH>
__global__ __launch_bounds__(StfBlock<NCH>::threads) void k_stf_costgrad(Dev d, int slot) {
    __shared__ double sh[3 * MSDP_WAVES];
    if (d.ctl->done) return;
    constexpr int WAVES = StfBlock<NCH>::threads / 64, BPW = 64 / LPR;
    int lo, hi;
    msdp_chunk_rows(d.nb, d.G, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    const double* __restrict__ Yl = slot ? d.Y[1] : d.Y[0];
    const double* __restrict__ Xf = d.full;
    double* __restrict__ Gr = slot ? d.Gr[1] : d.Gr[0];
    double* __restrict__ eG = slot ? d.eG[1] : d.eG[0];
    double* __restrict__ Lam = slot ? d.Lam[1] : d.Lam[0];
    double pf = 0.0, pgg = 0.0;
    for (int b0 = lo + wave * BPW; b0 < hi; b0 += WAVES * BPW) {
        const int blk = b0 + rsub;
        if (blk < hi) {
            double2 acc[D][NCH], y[D][NCH];
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    acc[a][ch] = make_double2(0.0, 0.0);
                    const int col = 2 * sub + ch * 2 * LPR;
                    y[a][ch] = (col < d.ld) ? ld2(Yl + ((int64_t)blk * D + a) * d.ld + col) : make_double2(0.0, 0.0);
                }
            spmm_block<D, LPR, NCH>(d, blk, sub, Xf, acc);
            double L[D][D];
            msdp_block_symdot<D, LPR, NCH>(acc, y, L);      // Lambda = sym((C Y)_i Y_i')
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    if (col < d.ld) {
                        double2 g = acc[a][ch];
#pragma unroll
                        for (int b = 0; b < D; ++b) { g.x -= L[a][b] * y[b][ch].x; g.y -= L[a][b] * y[b][ch].y; }   // G = C Y - Lambda Y
                        st2(Gr + ((int64_t)blk * D + a) * d.ld + col, g);
                        pgg += g.x * g.x + g.y * g.y;
                    }
                }
            if (sub == 0) {
#pragma unroll
                for (int a = 0; a < D; ++a) {
#pragma unroll
                    for (int b = 0; b < D; ++b) Lam[(int64_t)blk * (D * D) + a * D + b] = L[a][b];
                    eG[blk * D + a] = L[a][a];
                    pf += 0.5 * L[a][a];
                }
            }
        }
    }
    msdp_put_partials3(d.P, P_F, pf, P_GG, pgg, -1, 0.0, sh);
}

// Hess-vec: W = C md - blockdiag(Lambda) md, Hmd_i = W_i - sym(W_i Y_i') Y_i, partial <md, Hmd>
template <int D, int LPR, int NCH>
__global__ __launch_bounds__(StfBlock<NCH>::threads) void k_stf_hess(Dev d) {
    __shared__ double sh[3 * MSDP_WAVES];
    if (!d.F[0].active) return;
    constexpr int WAVES = StfBlock<NCH>::threads / 64, BPW = 64 / LPR;
    int lo, hi;
    msdp_chunk_rows(d.nb, d.G, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    const int cur = d.ctl->cur;
    const double* __restrict__ Yl = cur ? d.Y[1] : d.Y[0];
    const double* __restrict__ Lam = cur ? d.Lam[1] : d.Lam[0];
    const double* __restrict__ Uf = d.full;
    const double* __restrict__ Ul = d.md;
    double* __restrict__ H = d.Hmd;
    double pd = 0.0;
    // one block per trip of the loop: its d rows are d independent gathers per entry already (the two row steps of the oblique
    // Hess-vec would hold 2 d rows of three vectors: beyond the registers at NCH = 2)
    for (int b0 = lo + wave * BPW; b0 < hi; b0 += WAVES * BPW) {
        const int blk = b0 + rsub;
        if (blk < hi) {
            double2 w[D][NCH], y[D][NCH], u[D][NCH];
            double L[D][D];
#pragma unroll
            for (int a = 0; a < D; ++a) {
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    w[a][ch] = make_double2(0.0, 0.0);
                    const int col = 2 * sub + ch * 2 * LPR;
                    const bool ok = col < d.ld;
                    const int64_t o = ((int64_t)blk * D + a) * d.ld + (ok ? col : 0);
                    y[a][ch] = ld2(Yl + o);
                    u[a][ch] = ld2(Ul + o);
                    if (!ok) { y[a][ch] = make_double2(0.0, 0.0); u[a][ch] = make_double2(0.0, 0.0); }
                }
#pragma unroll
                for (int b = 0; b < D; ++b) L[a][b] = Lam[(int64_t)blk * (D * D) + a * D + b];
            }
            spmm_block<D, LPR, NCH, (D == 3 ? 1 : 2)>(d, blk, sub, Uf, w);
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b < D; ++b)
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) { w[a][ch].x -= L[a][b] * u[b][ch].x; w[a][ch].y -= L[a][b] * u[b][ch].y; }
            double T[D][D];
            msdp_block_symdot<D, LPR, NCH>(w, y, T);
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    if (col < d.ld) {
                        double2 h = w[a][ch];
#pragma unroll
                        for (int b = 0; b < D; ++b) { h.x -= T[a][b] * y[b][ch].x; h.y -= T[a][b] * y[b][ch].y; }
                        st2(H + ((int64_t)blk * D + a) * d.ld + col, h);
                        pd += u[a][ch].x * h.x + u[a][ch].y * h.y;
                    }
                }
        }
    }
    msdp_put_partial(d.P, P_DHD, pd, sh);
}

// tCG.m:227-287: the scalar decisions (msdp_tcg_upd2_scalars), then mdelta = tangent(r + beta mdelta) block by block (:273, :283)
template <int D, int LPR, int NCH>
__global__ __launch_bounds__(StfBlock<NCH>::threads) void k_stf_upd2(Dev d) {
    __shared__ double shb[4];
    double beta;
    if (!msdp_tcg_upd2_scalars(d, shb, beta)) return;
    constexpr int WAVES = StfBlock<NCH>::threads / 64, BPW = 64 / LPR;
    int lo, hi;
    msdp_chunk_rows(d.nb, d.G, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    const double* __restrict__ Yl = d.ctl->cur ? d.Y[1] : d.Y[0];
    for (int b0 = lo + wave * BPW; b0 < hi; b0 += WAVES * BPW) {
        const int blk = b0 + rsub;
        if (blk < hi) {
            double2 v[D][NCH], y[D][NCH];
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    v[a][ch] = y[a][ch] = make_double2(0.0, 0.0);
                    if (col < d.ld) {
                        const int64_t o = ((int64_t)blk * D + a) * d.ld + col;
                        const double2 rr = ld2(d.r + o), m = ld2(d.md + o);
                        y[a][ch] = ld2(Yl + o);
                        v[a][ch] = make_double2(rr.x + beta * m.x, rr.y + beta * m.y);
                    }
                }
            double T[D][D];
            msdp_block_symdot<D, LPR, NCH>(v, y, T);
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    if (col < d.ld) {
                        double2 t = v[a][ch];
#pragma unroll
                        for (int b = 0; b < D; ++b) { t.x -= T[a][b] * y[b][ch].x; t.y -= T[a][b] * y[b][ch].y; }
                        st2(d.md + ((int64_t)blk * D + a) * d.ld + col, t);
                    }
                }
        }
    }
}

// x_prop = retr(x, eta) into the other slot -- the polar factor of every block of x + eta -- and the partial of
// <eta, grad + .5 * Heta> (trustregions.m:549-550)
template <int D, int LPR, int NCH>
__global__ __launch_bounds__(StfBlock<NCH>::threads) void k_stf_retract(Dev d) {
    __shared__ double sh[3 * MSDP_WAVES];
    const Ctl* c = d.ctl;
    if (c->done) return;
    constexpr int WAVES = StfBlock<NCH>::threads / 64, BPW = 64 / LPR;
    int lo, hi;
    msdp_chunk_rows(d.nb, d.G, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    const int cur = c->cur, ix = d.F[0].eta_idx;
    const double* __restrict__ Yl = cur ? d.Y[1] : d.Y[0];
    const double* __restrict__ g = cur ? d.Gr[1] : d.Gr[0];
    const double* __restrict__ eta = ix ? d.eta[1] : d.eta[0];
    const double* __restrict__ Heta = ix ? d.Heta[1] : d.Heta[0];
    double* __restrict__ Yp = cur ? d.Y[0] : d.Y[1];
    double prd = 0.0;
    for (int b0 = lo + wave * BPW; b0 < hi; b0 += WAVES * BPW) {
        const int blk = b0 + rsub;
        if (blk < hi) {
            double2 x[D][NCH];
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    x[a][ch] = make_double2(0.0, 0.0);
                    if (col < d.ld) {
                        const int64_t o = ((int64_t)blk * D + a) * d.ld + col;
                        const double2 y = ld2(Yl + o), e = ld2(eta + o), he = ld2(Heta + o), gv = ld2(g + o);
                        x[a][ch] = make_double2(y.x + e.x, y.y + e.y);
                        prd += e.x * (gv.x + 0.5 * he.x) + e.y * (gv.y + 0.5 * he.y);
                    }
                }
            double Gm[D][D], R[D][D];
            msdp_block_symdot<D, LPR, NCH>(x, x, Gm);       // A A'
            msdp_sym_invsqrt<D>(Gm, R);
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    if (col < d.ld) {
                        double2 t = make_double2(0.0, 0.0);
#pragma unroll
                        for (int b = 0; b < D; ++b) { t.x += R[a][b] * x[b][ch].x; t.y += R[a][b] * x[b][ch].y; }
                        st2(Yp + ((int64_t)blk * D + a) * d.ld + col, t);
                    }
                }
        }
    }
    msdp_put_partial(d.P, P_RD, prd, sh);
}

// M.proj and M.retr for the fine-grained entry points: one thread per block
template <int D>
__global__ void k_stf_proj_simple(const double* __restrict__ Y, const double* __restrict__ U, double* __restrict__ V, int nb, int ld) {
    for (int blk = blockIdx.x * blockDim.x + threadIdx.x; blk < nb; blk += gridDim.x * blockDim.x) {
        const double* y = Y + (int64_t)blk * D * ld;
        const double* u = U + (int64_t)blk * D * ld;
        double* v = V + (int64_t)blk * D * ld;
        double T[D][D];
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = a; b < D; ++b) {
                double s = 0.0;
                for (int c = 0; c < ld; ++c) s += u[a * ld + c] * y[b * ld + c] + u[b * ld + c] * y[a * ld + c];
                T[a][b] = T[b][a] = 0.5 * s;
            }
        for (int c = 0; c < ld; ++c) {
#pragma unroll
            for (int a = 0; a < D; ++a) {
                double t = u[a * ld + c];
#pragma unroll
                for (int b = 0; b < D; ++b) t -= T[a][b] * y[b * ld + c];
                v[a * ld + c] = t;
            }
        }
    }
}
template <int D>
__global__ void k_stf_retr_simple(const double* __restrict__ Y, const double* __restrict__ U, double* __restrict__ Z, double alpha,
                                  int nb, int ld) {
    for (int blk = blockIdx.x * blockDim.x + threadIdx.x; blk < nb; blk += gridDim.x * blockDim.x) {
        const double* y = Y + (int64_t)blk * D * ld;
        const double* u = U + (int64_t)blk * D * ld;
        double* z = Z + (int64_t)blk * D * ld;
        double Gm[D][D], R[D][D];
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = a; b < D; ++b) {
                double s = 0.0;
                for (int c = 0; c < ld; ++c) s += (y[a * ld + c] + alpha * u[a * ld + c]) * (y[b * ld + c] + alpha * u[b * ld + c]);
                Gm[a][b] = Gm[b][a] = s;
            }
        msdp_sym_invsqrt<D>(Gm, R);
        for (int c = 0; c < ld; ++c) {
            double x[D];
#pragma unroll
            for (int a = 0; a < D; ++a) x[a] = y[a * ld + c] + alpha * u[a * ld + c];
#pragma unroll
            for (int a = 0; a < D; ++a) {
                double t = 0.0;
#pragma unroll
                for (int b = 0; b < D; ++b) t += R[a][b] * x[b];
                z[a * ld + c] = t;
            }
        }
    }
}

// w = C v - blockdiag(Lambda) v for a vector of n = nb * D entries (the escape's S * v): one thread per block row
template <int D>
__global__ void k_stf_sv(int nb, const int* __restrict__ brp, const int* __restrict__ bci, const double* __restrict__ bval,
                         const double* __restrict__ Lam, const double* __restrict__ v, double* __restrict__ w) {
    for (int blk = blockIdx.x * blockDim.x + threadIdx.x; blk < nb; blk += gridDim.x * blockDim.x) {
        double acc[D];
#pragma unroll
        for (int a = 0; a < D; ++a) acc[a] = 0.0;
        for (int k = brp[blk]; k < brp[blk + 1]; ++k) {
            const int j = bci[k];
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b < D; ++b) acc[a] = fma(bval[(int64_t)k * (D * D) + a * D + b], v[(int64_t)j * D + b], acc[a]);
        }
#pragma unroll
        for (int a = 0; a < D; ++a) {
            double t = acc[a];
#pragma unroll
            for (int b = 0; b < D; ++b) t -= Lam[(int64_t)blk * (D * D) + a * D + b] * v[(int64_t)blk * D + b];
            w[(int64_t)blk * D + a] = t;
        }
    }
}

// ------------------------------------------------------------------ launchers
// One instance per lanes-per-block count: widths up to 2 * 64 * 2 = 256
#define STF_LAUNCH(KERNEL, DD, L, N, h, ...) \
    hipLaunchKernelGGL((KERNEL<DD, L, N>), dim3((h)->d.G), dim3(StfBlock<N>::threads), 0, (h)->stream, __VA_ARGS__)
#define STF_DISPATCH_D(KERNEL, DD, h, ...)                                                           \
    do {                                                                                             \
        const int half = (h)->d.ld / 2;                                                              \
        if (half <= 1) STF_LAUNCH(KERNEL, DD, 1, 1, h, __VA_ARGS__);                                 \
        else if (half <= 2) STF_LAUNCH(KERNEL, DD, 2, 1, h, __VA_ARGS__);                            \
        else if (half <= 4) STF_LAUNCH(KERNEL, DD, 4, 1, h, __VA_ARGS__);                            \
        else if (half <= 8) STF_LAUNCH(KERNEL, DD, 8, 1, h, __VA_ARGS__);                            \
        else if (half <= 16) STF_LAUNCH(KERNEL, DD, 16, 1, h, __VA_ARGS__);                          \
        else if (half <= 32) STF_LAUNCH(KERNEL, DD, 32, 1, h, __VA_ARGS__);                          \
        else if (half <= 64) STF_LAUNCH(KERNEL, DD, 64, 1, h, __VA_ARGS__);                          \
        else if (half <= 128) STF_LAUNCH(KERNEL, DD, 64, 2, h, __VA_ARGS__);                         \
        else {                                                                                       \
            msdp_set_error("unit-block-diagonal handle: factor width p = %d exceeds the supported maximum of 256", (h)->d.p); \
            return MSDP_EUNSUPPORTED;                                                                \
        }                                                                                            \
    } while (0)
#define STF_DISPATCH(KERNEL, h, ...)                                                                 \
    do {                                                                                             \
        if ((h)->d.manifold != MANI_STIEFEL || !(h)->d.brp) { msdp_set_error("not a unit-block-diagonal handle"); return MSDP_ESTATE; } \
        if ((h)->d.blk == 2) STF_DISPATCH_D(KERNEL, 2, h, __VA_ARGS__);                              \
        else STF_DISPATCH_D(KERNEL, 3, h, __VA_ARGS__);                                              \
        HIPCHK(hipGetLastError());                                                                   \
    } while (0)

int msdp_stiefel_costgrad(msdp_handle h, int slot) {
    if (h->d.efree) return msdp_pose_costgrad(h, slot);      // blocks with a free row: msdp_pose.hip, here and below
    if (slot < 0 || slot > 1) { msdp_set_error("unit-block-diagonal handle: point slot %d", slot); return MSDP_EINVAL; }
    STF_DISPATCH(k_stf_costgrad, h, h->d, slot);
    return 0;
}
int msdp_stiefel_hess(msdp_handle h) {
    if (h->d.efree) return msdp_pose_hess(h);
    STF_DISPATCH(k_stf_hess, h, h->d);
    return 0;
}
int msdp_stiefel_upd2(msdp_handle h) {
    if (h->d.efree) return msdp_pose_upd2(h);
    STF_DISPATCH(k_stf_upd2, h, h->d);
    return 0;
}
int msdp_stiefel_retract(msdp_handle h) {
    if (h->d.efree) return msdp_pose_retract(h);
    STF_DISPATCH(k_stf_retract, h, h->d);
    return 0;
}
int msdp_stiefel_proj(msdp_handle h, const double* Y, const double* U, double* V) {
    if (h->d.efree) return msdp_pose_proj(h, Y, U, V);
    const Dev& d = h->d;
    const dim3 gr((d.nb + 255) / 256), bl(256);
    if (d.blk == 2) hipLaunchKernelGGL(k_stf_proj_simple<2>, gr, bl, 0, h->stream, Y, U, V, d.nb, d.ld);
    else hipLaunchKernelGGL(k_stf_proj_simple<3>, gr, bl, 0, h->stream, Y, U, V, d.nb, d.ld);
    HIPCHK(hipGetLastError());
    return 0;
}
int msdp_stiefel_retr(msdp_handle h, const double* Y, const double* U, double* Z, double alpha) {
    if (h->d.efree) return msdp_pose_retr(h, Y, U, Z, alpha);
    const Dev& d = h->d;
    const dim3 gr((d.nb + 255) / 256), bl(256);
    if (d.blk == 2) hipLaunchKernelGGL(k_stf_retr_simple<2>, gr, bl, 0, h->stream, Y, U, Z, alpha, d.nb, d.ld);
    else hipLaunchKernelGGL(k_stf_retr_simple<3>, gr, bl, 0, h->stream, Y, U, Z, alpha, d.nb, d.ld);
    HIPCHK(hipGetLastError());
    return 0;
}
int msdp_stiefel_sv(msdp_handle h, const double* Lam, const double* v, double* w) {
    if (h->d.efree) return msdp_pose_sv(h, Lam, v, w);
    const Dev& d = h->d;
    if (d.costkind != COST_BLOCK || !d.brp) { msdp_set_error("block product: not a unit-block-diagonal handle"); return MSDP_ESTATE; }
    const dim3 gr((d.nb + 255) / 256), bl(256);
    if (d.blk == 2) hipLaunchKernelGGL(k_stf_sv<2>, gr, bl, 0, h->stream, d.nb, d.brp, d.bci, d.bval, Lam, v, w);
    else hipLaunchKernelGGL(k_stf_sv<3>, gr, bl, 0, h->stream, d.nb, d.brp, d.bci, d.bval, Lam, v, w);
    HIPCHK(hipGetLastError());
    return 0;
}

// Block CSR from the caller's CSC arrays of the symmetric order-N matrix (column j is read as row j, as for the scalar kinds).
// Block row i collects the block columns its rows touch, ascending; a block the pattern covers only in part is zero-filled.
// blk = the block order of the storage; efree of its rows are free (the pose-graph kind, msdp_pose.hip), and the multiplier
// blocks Lam are of order blk - efree.
int msdp_stiefel_setup(msdp_handle h, int blk, int efree, const int64_t* jc, const int64_t* ir, const double* val) {
    Dev& d = h->d;
    if (h->nranks != 1 || h->use_comm || d.n_loc != d.n) { msdp_set_error("%s cost: single-rank handles only", msdp_block_kind_name(efree)); return MSDP_EUNSUPPORTED; }
    const int n = d.n, nb = n / blk, dd = blk * blk, ll = (blk - efree) * (blk - efree);
    std::vector<int> brp((size_t)nb + 1, 0), bci;
    std::vector<double> bval;
    std::vector<int> pos((size_t)nb, -1);               // block column -> entry of the running block row
    std::vector<int> cols;
    for (int i = 0; i < nb; ++i) {
        cols.clear();
        for (int a = 0; a < blk; ++a)
            for (int64_t k = jc[(int64_t)i * blk + a]; k < jc[(int64_t)i * blk + a + 1]; ++k) {
                const int j = (int)(ir[k] / blk);
                if (pos[j] < 0) { pos[j] = 0; cols.push_back(j); }
            }
        std::sort(cols.begin(), cols.end());
        const size_t base = bci.size();
        if (base + cols.size() > (size_t)0x7fffffff / dd) { msdp_set_error("%s cost: too many blocks in C", msdp_block_kind_name(efree)); return MSDP_EINVAL; }
        for (size_t t = 0; t < cols.size(); ++t) { pos[cols[t]] = (int)(base + t); bci.push_back(cols[t]); }
        bval.resize((base + cols.size()) * dd, 0.0);
        for (int a = 0; a < blk; ++a)
            for (int64_t k = jc[(int64_t)i * blk + a]; k < jc[(int64_t)i * blk + a + 1]; ++k)
                bval[(size_t)pos[ir[k] / blk] * dd + a * blk + (int)(ir[k] % blk)] += val[k];
        for (int j : cols) pos[j] = -1;
        brp[i + 1] = (int)bci.size();
    }
    if (bci.empty()) { bci.push_back(0); bval.assign((size_t)dd, 0.0); }      // C = 0: one unreferenced entry so that the arrays exist
    int rc;
    const int* dbrp = nullptr; const int* dbci = nullptr; const double* dbval = nullptr;
    if ((rc = msdp_upload<int>(h, brp, &dbrp)) || (rc = msdp_upload<int>(h, bci, &dbci)) || (rc = msdp_upload<double>(h, bval, &dbval))) return rc;
    for (int s = 0; s < 2; ++s) {
        if ((rc = msdp_dev_alloc<double>(h, &d.Lam[s], (size_t)nb * ll))) return rc;
        HIPCHK(hipMemset(d.Lam[s], 0, (size_t)nb * ll * sizeof(double)));
    }
    d.blk = blk; d.nb = nb; d.efree = efree; d.brp = dbrp; d.bci = dbci; d.bval = dbval;
    d.nnz = (int64_t)bci.size() * dd;
    d.rowptr = nullptr; d.colind = nullptr; d.cval = nullptr;
    d.ellW = 0; d.ell_stride = 0; d.ellc = nullptr; d.ellv = nullptr;
    return 0;
}
