// msdp_pose.hip -- the pose-graph problem  min <C, X>  s.t. X PSD of order N = n (d + 1), (X_[ii])_{1..d,1..d} = I_d  (SE(d)
// synchronisation, the non-marginalised form of SE-Sync / Cartan-Sync), d in {2, 3}, on the product of the stacked Stiefel
// manifold and a Euclidean space (MANI_STIEFEL / COST_BLOCK with d.efree = 1, msdp_create_posegraph_csc; manopt's
// productmanifold of stiefelstackedfactory(n, d, p) and euclideanfactory(n, p)).
//
// The factor Y (N x p, row-major, row stride ld) is n blocks of B = d + 1 consecutive rows: d rows Y_i with Y_i Y_i' = I_d and
// one free row tau_i.  With (C Y)_i = [G_i; g_i], sym(M) = (M + M')/2 and f = <C, Y Y'> / 2:
//   multiplier  Lambda_i = sym(G_i Y_i') (d x d)         S = C - blockdiag(Lambda_i (+) 0)
//   cost        2 f = sum_i tr Lambda_i + sum_i <g_i, tau_i>: the dual value sum tr Lambda is NOT <C, X> away from a critical point
//   gradient    [G_i - Lambda_i Y_i ; g_i]
//   Hess-vec    W = C U - blockdiag(Lambda (+) 0) U; rotation rows W_i - sym(W_i Y_i') Y_i, the free row of W as it is
//   tangent     Stiefel on the rotation rows (stiefelstackedfactory.m:81-89), identity on the free row
//   retraction  polar on the rotation rows (:103-117), tau_i + eta_tau on the free row (euclideanfactory.m:44)
// These are the kernels of msdp_stiefel.hip for blocks of B rows whose last is Euclidean; that file's kernels are not edited.
//
// Storage: the block CSR of msdp_stiefel.hip at block order B (one column index per B x B block, zero-filled where the pattern
// is partial, msdp_stiefel_setup); a lane group of LPR lanes owns one block with its B rows of NCH double2 each in registers.
// Lambda stays d x d per block (d.Lam[slot], nb * d * d doubles); eG[slot] carries its diagonal with 0 in the free-row entry,
// so that the sum of msdp_get_z is the dual value.  Widths up to 256; no instance uses scratch.
// The kind runs the generic per-iteration path of msdp_rtr.hip (no persistent or fused trip, no row sharding).
#include "msdp_device.h"
#include <math.h>

// workgroup sizes, per kernel: those of the Stiefel kind (16 waves at one chunk per lane, 8 at two) for all but the d = 3
// Hess-vec.  That one holds four rows of w and u, three of y and the 4 x 4 values of an entry: its one-chunk instances take
// 126-137 registers and spilled at the 128 of a 16-wave workgroup, so it runs 8 waves (up to 256 registers; <64, 2> takes 198).
// Cost/gradient (103-110), direction update (82-88) and retraction (72-78) fit 16 waves at d = 3 and keep them.
template <int D, int NCH> struct PoseBlock { static constexpr int threads = NCH == 1 ? 1024 : 512; };
template <int D, int NCH> struct PoseHessBlock { static constexpr int threads = (NCH == 1 && D == 2) ? 1024 : 512; };

// cost + Riemannian gradient + Lambda at Y[slot] (gather source: d.full holds all rows of Y[slot])
template <int D, int LPR, int NCH>
__global__ __launch_bounds__((PoseBlock<D, NCH>::threads)) void k_pose_costgrad(Dev d, int slot) {
    __shared__ double sh[3 * MSDP_WAVES];
    if (d.ctl->done) return;
    constexpr int B = D + 1, WAVES = PoseBlock<D, NCH>::threads / 64, BPW = 64 / LPR;
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
            double2 acc[B][NCH], y[B][NCH];
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    acc[a][ch] = make_double2(0.0, 0.0);
                    const int col = 2 * sub + ch * 2 * LPR;
                    y[a][ch] = (col < d.ld) ? ld2(Yl + ((int64_t)blk * B + a) * d.ld + col) : make_double2(0.0, 0.0);
                }
            spmm_block<B, LPR, NCH, (D == 3 ? 1 : 2)>(d, blk, sub, Xf, acc);
            double L[D][D];
            msdp_block_symdot_lead<D, LPR, NCH>(acc, y, L);      // Lambda = sym(G_i Y_i'), rotation rows only
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    if (col < d.ld) {
                        double2 g = acc[a][ch];
                        if (a < D) {
#pragma unroll
                            for (int b = 0; b < D; ++b) { g.x -= L[a][b] * y[b][ch].x; g.y -= L[a][b] * y[b][ch].y; }   // G - Lambda Y
                        } else {
                            pf += 0.5 * (g.x * y[a][ch].x + g.y * y[a][ch].y);      // <g_i, tau_i> / 2: the free row's share of f
                        }
                        st2(Gr + ((int64_t)blk * B + a) * d.ld + col, g);
                        pgg += g.x * g.x + g.y * g.y;
                    }
                }
            if (sub == 0) {
#pragma unroll
                for (int a = 0; a < D; ++a) {
#pragma unroll
                    for (int b = 0; b < D; ++b) Lam[(int64_t)blk * (D * D) + a * D + b] = L[a][b];
                    eG[blk * B + a] = L[a][a];
                    pf += 0.5 * L[a][a];
                }
                eG[blk * B + D] = 0.0;
            }
        }
    }
    msdp_put_partials3(d.P, P_F, pf, P_GG, pgg, -1, 0.0, sh);
}

// Hess-vec: W = C md - blockdiag(Lambda (+) 0) md; rotation rows W_i - sym(W_i Y_i') Y_i, free row of W; partial <md, Hmd>
template <int D, int LPR, int NCH>
__global__ __launch_bounds__((PoseHessBlock<D, NCH>::threads)) void k_pose_hess(Dev d) {
    __shared__ double sh[3 * MSDP_WAVES];
    if (!d.F[0].active) return;
    constexpr int B = D + 1, WAVES = PoseHessBlock<D, NCH>::threads / 64, BPW = 64 / LPR;
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
    for (int b0 = lo + wave * BPW; b0 < hi; b0 += WAVES * BPW) {
        const int blk = b0 + rsub;
        if (blk < hi) {
            // the free row of Y is not needed: y holds the D rotation rows, w and u all B rows
            double2 w[B][NCH], y[D][NCH], u[B][NCH];
            double L[D][D];
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    w[a][ch] = make_double2(0.0, 0.0);
                    const int col = 2 * sub + ch * 2 * LPR;
                    const bool ok = col < d.ld;
                    u[a][ch] = ld2(Ul + ((int64_t)blk * B + a) * d.ld + (ok ? col : 0));
                    if (!ok) u[a][ch] = make_double2(0.0, 0.0);
                }
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    const bool ok = col < d.ld;
                    y[a][ch] = ld2(Yl + ((int64_t)blk * B + a) * d.ld + (ok ? col : 0));
                    if (!ok) y[a][ch] = make_double2(0.0, 0.0);
                }
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b < D; ++b) L[a][b] = Lam[(int64_t)blk * (D * D) + a * D + b];
            spmm_block<B, LPR, NCH, 1>(d, blk, sub, Uf, w);
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b < D; ++b)
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) { w[a][ch].x -= L[a][b] * u[b][ch].x; w[a][ch].y -= L[a][b] * u[b][ch].y; }
            double T[D][D];
            msdp_block_symdot_lead<D, LPR, NCH>(w, y, T);
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    if (col < d.ld) {
                        double2 h = w[a][ch];
                        if (a < D) {
#pragma unroll
                            for (int b = 0; b < D; ++b) { h.x -= T[a][b] * y[b][ch].x; h.y -= T[a][b] * y[b][ch].y; }
                        }
                        st2(H + ((int64_t)blk * B + a) * d.ld + col, h);
                        pd += u[a][ch].x * h.x + u[a][ch].y * h.y;
                    }
                }
        }
    }
    msdp_put_partial(d.P, P_DHD, pd, sh);
}

// tCG.m:227-287: the scalar decisions (msdp_tcg_upd2_scalars), then mdelta = tangent(r + beta mdelta) block by block (:273, :283);
// the free row of the tangent projection is r + beta mdelta itself
template <int D, int LPR, int NCH>
__global__ __launch_bounds__((PoseBlock<D, NCH>::threads)) void k_pose_upd2(Dev d) {
    __shared__ double shb[4];
    double beta;
    if (!msdp_tcg_upd2_scalars(d, shb, beta)) return;
    constexpr int B = D + 1, WAVES = PoseBlock<D, NCH>::threads / 64, BPW = 64 / LPR;
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
                        const double2 rr = ld2(d.r + o), m = ld2(d.md + o);
                        v[a][ch] = make_double2(rr.x + beta * m.x, rr.y + beta * m.y);
                    }
                }
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    y[a][ch] = (col < d.ld) ? ld2(Yl + ((int64_t)blk * B + a) * d.ld + col) : make_double2(0.0, 0.0);
                }
            double T[D][D];
            msdp_block_symdot_lead<D, LPR, NCH>(v, y, T);
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

// x_prop = retr(x, eta) into the other slot -- the polar factor of the rotation rows of x + eta, the free row of x + eta as it
// is -- and the partial of <eta, grad + .5 * Heta> (trustregions.m:549-550)
template <int D, int LPR, int NCH>
__global__ __launch_bounds__((PoseBlock<D, NCH>::threads)) void k_pose_retract(Dev d) {
    __shared__ double sh[3 * MSDP_WAVES];
    const Ctl* c = d.ctl;
    if (c->done) return;
    constexpr int B = D + 1, WAVES = PoseBlock<D, NCH>::threads / 64, BPW = 64 / LPR;
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
            double2 x[B][NCH];
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    x[a][ch] = make_double2(0.0, 0.0);
                    if (col < d.ld) {
                        const int64_t o = ((int64_t)blk * B + a) * d.ld + col;
                        const double2 y = ld2(Yl + o), e = ld2(eta + o), he = ld2(Heta + o), gv = ld2(g + o);
                        x[a][ch] = make_double2(y.x + e.x, y.y + e.y);
                        prd += e.x * (gv.x + 0.5 * he.x) + e.y * (gv.y + 0.5 * he.y);
                    }
                }
            double Gm[D][D], R[D][D];
            msdp_block_symdot_lead<D, LPR, NCH>(x, x, Gm);       // A A' of the rotation rows
            msdp_sym_invsqrt<D>(Gm, R);
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    if (col < d.ld) {
                        double2 t = x[a][ch];                   // the free row: tau + eta
                        if (a < D) {
                            t = make_double2(0.0, 0.0);
#pragma unroll
                            for (int b = 0; b < D; ++b) { t.x += R[a][b] * x[b][ch].x; t.y += R[a][b] * x[b][ch].y; }
                        }
                        st2(Yp + ((int64_t)blk * B + a) * d.ld + col, t);
                    }
                }
        }
    }
    msdp_put_partial(d.P, P_RD, prd, sh);
}

// M.proj and M.retr for the fine-grained entry points: one thread per block
template <int D>
__global__ void k_pose_proj_simple(const double* __restrict__ Y, const double* __restrict__ U, double* __restrict__ V, int nb, int ld) {
    constexpr int B = D + 1;
    for (int blk = blockIdx.x * blockDim.x + threadIdx.x; blk < nb; blk += gridDim.x * blockDim.x) {
        const double* y = Y + (int64_t)blk * B * ld;
        const double* u = U + (int64_t)blk * B * ld;
        double* v = V + (int64_t)blk * B * ld;
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
            v[D * ld + c] = u[D * ld + c];
        }
    }
}
template <int D>
__global__ void k_pose_retr_simple(const double* __restrict__ Y, const double* __restrict__ U, double* __restrict__ Z, double alpha,
                                   int nb, int ld) {
    constexpr int B = D + 1;
    for (int blk = blockIdx.x * blockDim.x + threadIdx.x; blk < nb; blk += gridDim.x * blockDim.x) {
        const double* y = Y + (int64_t)blk * B * ld;
        const double* u = U + (int64_t)blk * B * ld;
        double* z = Z + (int64_t)blk * B * ld;
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
            z[D * ld + c] = y[D * ld + c] + alpha * u[D * ld + c];
        }
    }
}

// w = C v - blockdiag(Lambda (+) 0) v for a vector of n = nb * B entries (the escape's S * v): one thread per block row
template <int D>
__global__ void k_pose_sv(int nb, const int* __restrict__ brp, const int* __restrict__ bci, const double* __restrict__ bval,
                          const double* __restrict__ Lam, const double* __restrict__ v, double* __restrict__ w) {
    constexpr int B = D + 1;
    for (int blk = blockIdx.x * blockDim.x + threadIdx.x; blk < nb; blk += gridDim.x * blockDim.x) {
        double acc[B];
#pragma unroll
        for (int a = 0; a < B; ++a) acc[a] = 0.0;
        for (int k = brp[blk]; k < brp[blk + 1]; ++k) {
            const int j = bci[k];
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int b = 0; b < B; ++b) acc[a] = fma(bval[(int64_t)k * (B * B) + a * B + b], v[(int64_t)j * B + b], acc[a]);
        }
#pragma unroll
        for (int a = 0; a < B; ++a) {
            double t = acc[a];
            if (a < D) {
#pragma unroll
                for (int b = 0; b < D; ++b) t -= Lam[(int64_t)blk * (D * D) + a * D + b] * v[(int64_t)blk * B + b];
            }
            w[(int64_t)blk * B + a] = t;
        }
    }
}

// ------------------------------------------------------------------ launchers
// One instance per lanes-per-block count: widths up to 2 * 64 * 2 = 256
#define POSE_LAUNCH(BLOCK, KERNEL, DD, L, N, h, ...) \
    hipLaunchKernelGGL((KERNEL<DD, L, N>), dim3((h)->d.G), dim3(BLOCK<DD, N>::threads), 0, (h)->stream, __VA_ARGS__)
#define POSE_DISPATCH_D(BLOCK, KERNEL, DD, h, ...)                                                          \
    do {                                                                                                    \
        const int half = (h)->d.ld / 2;                                                                     \
        if (half <= 1) POSE_LAUNCH(BLOCK, KERNEL, DD, 1, 1, h, __VA_ARGS__);                                \
        else if (half <= 2) POSE_LAUNCH(BLOCK, KERNEL, DD, 2, 1, h, __VA_ARGS__);                           \
        else if (half <= 4) POSE_LAUNCH(BLOCK, KERNEL, DD, 4, 1, h, __VA_ARGS__);                           \
        else if (half <= 8) POSE_LAUNCH(BLOCK, KERNEL, DD, 8, 1, h, __VA_ARGS__);                           \
        else if (half <= 16) POSE_LAUNCH(BLOCK, KERNEL, DD, 16, 1, h, __VA_ARGS__);                         \
        else if (half <= 32) POSE_LAUNCH(BLOCK, KERNEL, DD, 32, 1, h, __VA_ARGS__);                         \
        else if (half <= 64) POSE_LAUNCH(BLOCK, KERNEL, DD, 64, 1, h, __VA_ARGS__);                         \
        else if (half <= 128) POSE_LAUNCH(BLOCK, KERNEL, DD, 64, 2, h, __VA_ARGS__);                        \
        else {                                                                                              \
            msdp_set_error("pose-graph handle: factor width p = %d exceeds the supported maximum of 256", (h)->d.p); \
            return MSDP_EUNSUPPORTED;                                                                       \
        }                                                                                                   \
    } while (0)
#define POSE_DISPATCH(BLOCK, KERNEL, h, ...)                                                                \
    do {                                                                                                    \
        if ((h)->d.manifold != MANI_STIEFEL || !(h)->d.efree || !(h)->d.brp) { msdp_set_error("not a pose-graph handle"); return MSDP_ESTATE; } \
        if ((h)->d.blk == 3) POSE_DISPATCH_D(BLOCK, KERNEL, 2, h, __VA_ARGS__);                             \
        else POSE_DISPATCH_D(BLOCK, KERNEL, 3, h, __VA_ARGS__);                                             \
        HIPCHK(hipGetLastError());                                                                          \
    } while (0)

int msdp_pose_costgrad(msdp_handle h, int slot) {
    if (slot < 0 || slot > 1) { msdp_set_error("pose-graph handle: point slot %d", slot); return MSDP_EINVAL; }
    POSE_DISPATCH(PoseBlock, k_pose_costgrad, h, h->d, slot);
    return 0;
}
int msdp_pose_hess(msdp_handle h) {
    POSE_DISPATCH(PoseHessBlock, k_pose_hess, h, h->d);
    return 0;
}
int msdp_pose_upd2(msdp_handle h) {
    POSE_DISPATCH(PoseBlock, k_pose_upd2, h, h->d);
    return 0;
}
int msdp_pose_retract(msdp_handle h) {
    POSE_DISPATCH(PoseBlock, k_pose_retract, h, h->d);
    return 0;
}
int msdp_pose_proj(msdp_handle h, const double* Y, const double* U, double* V) {
    const Dev& d = h->d;
    const dim3 gr((d.nb + 255) / 256), bl(256);
    if (d.blk == 3) hipLaunchKernelGGL(k_pose_proj_simple<2>, gr, bl, 0, h->stream, Y, U, V, d.nb, d.ld);
    else hipLaunchKernelGGL(k_pose_proj_simple<3>, gr, bl, 0, h->stream, Y, U, V, d.nb, d.ld);
    HIPCHK(hipGetLastError());
    return 0;
}
int msdp_pose_retr(msdp_handle h, const double* Y, const double* U, double* Z, double alpha) {
    const Dev& d = h->d;
    const dim3 gr((d.nb + 255) / 256), bl(256);
    if (d.blk == 3) hipLaunchKernelGGL(k_pose_retr_simple<2>, gr, bl, 0, h->stream, Y, U, Z, alpha, d.nb, d.ld);
    else hipLaunchKernelGGL(k_pose_retr_simple<3>, gr, bl, 0, h->stream, Y, U, Z, alpha, d.nb, d.ld);
    HIPCHK(hipGetLastError());
    return 0;
}
int msdp_pose_sv(msdp_handle h, const double* Lam, const double* v, double* w) {
    const Dev& d = h->d;
    if (d.costkind != COST_BLOCK || !d.efree || !d.brp) { msdp_set_error("block product: not a pose-graph handle"); return MSDP_ESTATE; }
    const dim3 gr((d.nb + 255) / 256), bl(256);
    if (d.blk == 3) hipLaunchKernelGGL(k_pose_sv<2>, gr, bl, 0, h->stream, d.nb, d.brp, d.bci, d.bval, Lam, v, w);
    else hipLaunchKernelGGL(k_pose_sv<3>, gr, bl, 0, h->stream, d.nb, d.brp, d.bci, d.bval, Lam, v, w);
    HIPCHK(hipGetLastError());
    return 0;
}
