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
// The kind runs the generic per-iteration path of msdp_rtr.hip (no fused trip, no row sharding; msdp_blockpersist.hip holds its
// persistent tCG).
//
// The same kernels serve the pose-graph problem  (X_[ii])_{1..d,1..d} = I_d  of order N = n (d + 1)  (SE(d) synchronisation, the
// non-marginalised form of SE-Sync / Cartan-Sync; d.efree = 1, msdp_create_posegraph_csc; manopt's productmanifold of
// stiefelstackedfactory(n, d, p) and euclideanfactory(n, p)): every kernel is templated on EF, the free rows per block (0 or
// 1), and a block is B = D + EF consecutive rows -- D rotation rows Y_i and, at EF = 1, one free row tau_i.  Whatever streams
// runs over the rows 0 .. B-1; y, Lambda, the sym(.) and the polar factor over the rows 0 .. D-1, and the Stiefel part of a store
// stands behind `a < D` (compile-time true at EF = 0).  With (C Y)_i = [G_i; g_i] the free row adds:
//   multiplier  Lambda_i = sym(G_i Y_i') stays d x d      S = C - blockdiag(Lambda_i (+) 0); eG carries 0 in the free-row entry
//   cost        2 f = sum_i tr Lambda_i + sum_i <g_i, tau_i>: the dual value sum tr Lambda is NOT <C, X> away from a critical point
//   gradient    [G_i - Lambda_i Y_i ; g_i]                Hess-vec: the free row of W as it is
//   tangent     identity on the free row                  retraction: tau_i + eta_tau (euclideanfactory.m:44)
// The storage is the block CSR above at block order B.  No instance uses scratch (DESIGN.md section 4 lists the registers).
#include "msdp_device.h"
#include <algorithm>
#include <math.h>
#include <vector>

// cost + Riemannian gradient + Lambda at Y[slot] (gather source: d.full holds all rows of Y[slot])
template <int D, int EF, int LPR, int NCH>
__global__ __launch_bounds__((BlockRows<D + EF, NCH>::threads)) void k_stf_costgrad(Dev d, int slot) {
    __shared__ double sh[3 * MSDP_WAVES];
    if (d.ctl->done) return;
    constexpr int B = D + EF, WAVES = BlockRows<B, NCH>::threads / 64, BPW = 64 / LPR;
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
            spmm_block<B, LPR, NCH, (B == 4 ? 1 : 2)>(d, blk, sub, Xf, acc);
            double L[D][D];
            msdp_block_symdot<D, LPR, NCH>(acc, y, L);      // Lambda = sym(G_i Y_i'), rotation rows only
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
                if constexpr (EF) eG[blk * B + D] = 0.0;
            }
        }
    }
    msdp_put_partials3(d.P, P_F, pf, P_GG, pgg, -1, 0.0, sh);
}

// Hess-vec: W = C md - blockdiag(Lambda (+) 0) md; rotation rows Hmd_i = W_i - sym(W_i Y_i') Y_i, a free row of W as it is;
// partial <md, Hmd>
template <int D, int EF, int LPR, int NCH>
__global__ __launch_bounds__((BlockRows3<D + EF, NCH>::threads)) void k_stf_hess(Dev d) {
    __shared__ double sh[3 * MSDP_WAVES];
    if (!d.F[0].active) return;
    constexpr int B = D + EF, WAVES = BlockRows3<B, NCH>::threads / 64, BPW = 64 / LPR;
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
            // a free row of Y is not needed: y holds the D rotation rows, w and u all B rows.  The ORDER of these loads is measured,
            // per kind, and the compiler's schedule follows it: without a free row y, u and the row of Lambda come row by row (u
            // for all rows first, then y, cost 4 % at d = 3, p = 8: 10.36 against 9.96 us); with one, u first and then y (row by
            // row takes 2-6 registers more).  profiles/block_rowkernels_kernel_regs.md has both.
            double2 w[B][NCH], y[D][NCH], u[B][NCH];
            double L[D][D];
            if constexpr (EF == 0) {
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
            } else {
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
            }
            spmm_block<B, LPR, NCH, (B == 2 ? 2 : 1)>(d, blk, sub, Uf, w);
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b < D; ++b)
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) { w[a][ch].x -= L[a][b] * u[b][ch].x; w[a][ch].y -= L[a][b] * u[b][ch].y; }
            double T[D][D];
            msdp_block_symdot<D, LPR, NCH>(w, y, T);
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
// on a free row the tangent projection is r + beta mdelta itself
template <int D, int EF, int LPR, int NCH>
__global__ __launch_bounds__((BlockRows<D + EF, NCH>::threads)) void k_stf_upd2(Dev d) {
    __shared__ double shb[4];
    double beta;
    if (!msdp_tcg_upd2_scalars(d, shb, beta)) return;
    constexpr int B = D + EF, WAVES = BlockRows<B, NCH>::threads / 64, BPW = 64 / LPR;
    int lo, hi;
    msdp_chunk_rows(d.nb, d.G, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    const double* __restrict__ Yl = d.ctl->cur ? d.Y[1] : d.Y[0];
    for (int b0 = lo + wave * BPW; b0 < hi; b0 += WAVES * BPW) {
        const int blk = b0 + rsub;
        if (blk < hi) {
            // v for all B rows, y for the D rotation rows; as in the Hess-vec the order of the loads is the measured one per kind:
            // y with the row of r and mdelta where there is no free row (after them: +0.6 us a trip at d = 2, p = 32), else after
            double2 v[B][NCH], y[D][NCH];
            if constexpr (EF == 0) {
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
            } else {
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
            }
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

// x_prop = retr(x, eta) into the other slot -- the polar factor of the rotation rows of every block of x + eta, a free row of
// x + eta as it is -- and the partial of <eta, grad + .5 * Heta> (trustregions.m:549-550)
template <int D, int EF, int LPR, int NCH>
__global__ __launch_bounds__((BlockRows<D + EF, NCH>::threads)) void k_stf_retract(Dev d) {
    __shared__ double sh[3 * MSDP_WAVES];
    const Ctl* c = d.ctl;
    if (c->done) return;
    constexpr int B = D + EF, WAVES = BlockRows<B, NCH>::threads / 64, BPW = 64 / LPR;
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
            msdp_block_symdot<D, LPR, NCH>(x, x, Gm);       // A A' of the rotation rows
            msdp_sym_invsqrt<D>(Gm, R);
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int col = 2 * sub + ch * 2 * LPR;
                    if (col < d.ld) {
                        double2 t = x[a][ch];                   // a free row: tau + eta
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
template <int D, int EF>
__global__ void k_stf_proj_simple(const double* __restrict__ Y, const double* __restrict__ U, double* __restrict__ V, int nb, int ld) {
    constexpr int B = D + EF;
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
            if constexpr (EF) v[D * ld + c] = u[D * ld + c];
        }
    }
}
template <int D, int EF>
__global__ void k_stf_retr_simple(const double* __restrict__ Y, const double* __restrict__ U, double* __restrict__ Z, double alpha,
                                  int nb, int ld) {
    constexpr int B = D + EF;
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
            if constexpr (EF) z[D * ld + c] = y[D * ld + c] + alpha * u[D * ld + c];
        }
    }
}

// w = C v - blockdiag(Lambda (+) 0) v for a vector of n = nb * B entries (the escape's S * v): one thread per block row
template <int D, int EF>
__global__ void k_stf_sv(int nb, const int* __restrict__ brp, const int* __restrict__ bci, const double* __restrict__ bval,
                         const double* __restrict__ Lam, const double* __restrict__ v, double* __restrict__ w) {
    constexpr int B = D + EF;
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
// One instance per lanes-per-block count (MSDP_BLOCK_WIDTH_LADDER, widths up to 256) for each of the four kinds <D, EF> =
// <d.blk - d.efree, d.efree>: the arguments of STF_KIND after the handle are a statement that names D_ and EF_
#define STF_KIND(h, ...)                                                                             \
    do {                                                                                             \
        const int dd_ = (h)->d.blk - (h)->d.efree;                                                   \
        if (dd_ == 2 && !(h)->d.efree) { constexpr int D_ = 2, EF_ = 0; __VA_ARGS__; }               \
        else if (dd_ == 3 && !(h)->d.efree) { constexpr int D_ = 3, EF_ = 0; __VA_ARGS__; }          \
        else if (dd_ == 2) { constexpr int D_ = 2, EF_ = 1; __VA_ARGS__; }                           \
        else { constexpr int D_ = 3, EF_ = 1; __VA_ARGS__; }                                         \
        HIPCHK(hipGetLastError());                                                                   \
    } while (0)
#define STF_DISPATCH(BLOCK, KERNEL, h, ...)                                                          \
    do {                                                                                             \
        if ((h)->d.manifold != MANI_STIEFEL || !(h)->d.brp) { msdp_set_error("not a %s handle", msdp_block_kind_name((h)->d.efree)); return MSDP_ESTATE; } \
        STF_KIND(h, MSDP_BLOCK_WIDTH_LADDER((h)->d.ld, hipLaunchKernelGGL((KERNEL<D_, EF_, LPR_, NCH_>), dim3((h)->d.G),          \
                                                                          dim3(BLOCK<D_ + EF_, NCH_>::threads), 0, (h)->stream, __VA_ARGS__)) { \
            msdp_set_error("%s handle: factor width p = %d exceeds the supported maximum of 256", msdp_block_kind_name((h)->d.efree), (h)->d.p); \
            return MSDP_EUNSUPPORTED;                                                                \
        });                                                                                          \
    } while (0)

int msdp_stiefel_costgrad(msdp_handle h, int slot) {
    if (slot < 0 || slot > 1) { msdp_set_error("%s handle: point slot %d", msdp_block_kind_name(h->d.efree), slot); return MSDP_EINVAL; }
    STF_DISPATCH(BlockRows, k_stf_costgrad, h, h->d, slot);
    return 0;
}
int msdp_stiefel_hess(msdp_handle h) {
    STF_DISPATCH(BlockRows3, k_stf_hess, h, h->d);
    return 0;
}
int msdp_stiefel_upd2(msdp_handle h) {
    STF_DISPATCH(BlockRows, k_stf_upd2, h, h->d);
    return 0;
}
int msdp_stiefel_retract(msdp_handle h) {
    STF_DISPATCH(BlockRows, k_stf_retract, h, h->d);
    return 0;
}
int msdp_stiefel_proj(msdp_handle h, const double* Y, const double* U, double* V) {
    const Dev& d = h->d;
    const dim3 gr((d.nb + 255) / 256), bl(256);
    STF_KIND(h, hipLaunchKernelGGL((k_stf_proj_simple<D_, EF_>), gr, bl, 0, h->stream, Y, U, V, d.nb, d.ld));
    return 0;
}
int msdp_stiefel_retr(msdp_handle h, const double* Y, const double* U, double* Z, double alpha) {
    const Dev& d = h->d;
    const dim3 gr((d.nb + 255) / 256), bl(256);
    STF_KIND(h, hipLaunchKernelGGL((k_stf_retr_simple<D_, EF_>), gr, bl, 0, h->stream, Y, U, Z, alpha, d.nb, d.ld));
    return 0;
}
int msdp_stiefel_sv(msdp_handle h, const double* Lam, const double* v, double* w) {
    const Dev& d = h->d;
    if (d.costkind != COST_BLOCK || !d.brp) { msdp_set_error("block product: not a %s handle", msdp_block_kind_name(d.efree)); return MSDP_ESTATE; }
    const dim3 gr((d.nb + 255) / 256), bl(256);
    STF_KIND(h, hipLaunchKernelGGL((k_stf_sv<D_, EF_>), gr, bl, 0, h->stream, d.nb, d.brp, d.bci, d.bval, Lam, v, w));
    return 0;
}

// Block CSR from the caller's CSC arrays of the symmetric order-N matrix (column j is read as row j, as for the scalar kinds).
// Block row i collects the block columns its rows touch, ascending; a block the pattern covers only in part is zero-filled.
// blk = the block order of the storage; efree of its rows are free (the pose-graph kind), and the multiplier
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
