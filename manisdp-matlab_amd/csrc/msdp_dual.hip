// msdp_dual.hip -- the three dual kinds (MSDP_KIND_DUAL_UNITDIAG, MSDP_KIND_DUAL, MSDP_KIND_DUAL_MULTIBLOCK): their state, kernels,
// closures and entry points.  A dual handle is an affine handle (msdp_affine_setup[_blocked] has uploaded At = A', b and C) with a
// DualState hung on its AffineState; msdp_affine_costgrad / _hess / _linesearch_cost hand over to msdp_dual_* here.  The operator is
// reached through the launchers of msdp_affine.hip only (msdp_common.h): A(.), A'(.), the dense products, the Gram matrix, the
// row dots and the gradient finish.
#include "msdp_device.h"
#include "msdp_affine_dev.h"
#include <math.h>
#include <algorithm>

// ================================================================== dual, unit diagonal
// src/dual/ManiDSDP_unitdiag.m: the variable is the dual slack S = Y'Y with diag(S) = 1 (oblique factor, as in the
// primal unit-diagonal entry point); the multipliers are the primal matrix x (n^2, dense) and the free part w.
//   cost  :174-181   S = Y'Y; sc = S(:) - c; y = iA'*sc; As = A'y - sc - x/sigma; Af = B'y - cf - w/sigma;
//                    f = b'y + sigma/2 (|As|^2 + |Af|^2)
//   grad  :183-187   X = reshape(bA - sigma*As); eG = 2*Y*X; G = eG - Y.*sum(Y.*eG)
//   hess  :189-194   yAU = reshape(A'(iA'*vec(Y'U))); eH = 2*U*X - 4*sigma*(Y*yAU) + 2*sigma*((Y*U')*Y + (Y*Y')*U)
// with iA = (diag(A*A')\A)' (:38) and bA = iA*b (:39).  The rows of A are the columns of this handle's At, so
// iA'*vec(M) is the primal kind's A(M) divided by dAAt, and A'y its adjoint: msdp_affine_launch_A / _launch_adjoint and the MFMA
// contraction are reused as they are.  With T = bA + x - sigma*C (rebuilt when the multipliers change):
//   X = T + sigma*S - sigma*A'y,      sigma*As = bA - X.
// New here: the dense Gram S = Y*Y' (k_gram_mfma, one product), the two p x p Gram matrices of the last Hessian
// term, and the element-wise kernels.
//
// ------------------------------------------------------------------ dual, generic (MSDP_KIND_DUAL)
// src/dual/ManiDSDP.m: S = Y*Y' on the Euclidean factor (n x p, :60), no diagonal constraint; G = D\A*A' (m x m).
//   cost/grad :162-171  y, Af as above; X = bA + sigma*(iAB*Af + A'(iA'*As) - As); G = 2*X*Y
//   hess      :173-177  a = iA'*vec(U*Y'); H = 2*X*U + 2*sigma*(U*(Y'Y) + Y*(U'Y)) + 4*sigma*mat(A'(D\B*B'a + G*a - 2a))*Y
// cost/grad keeps As dense:  Q = (C - x/sigma) + A'y (one adjoint; C - x/sigma is rebuilt with the multipliers, in T),
// As = Q - S, R = bA - sigma*As, v = sigma*D\(A*As + B*Af) (one row-gather SpMV of A on the dense As, B by rows), and
// X = R + A'v (the second adjoint).  So X needs no G and holds for any A and dAAt; |As|^2 comes from the same pass.
// The Hess-vec: msdp_affine_launch_A, B'a when there are free variables, one m-vector fix-up, one adjoint -- plus, unless the setup
// proved G = I (rows of A with pairwise disjoint supports and dAAt equal to their squared norms), G*a = D\A(A'a) by one
// more adjoint and the SpMV.  The outer step :65-77 is the cost state at Y followed by x = X - bA (k_dgen_outer).
struct DualState {
    int nf = 0;                     // free variables (K.f)
    const double* dinv = nullptr;   // 1 ./ dAAt                         (m)
    const double* Ac = nullptr;     // A*c                                (m)
    const int* bjc = nullptr;       // B in CSC (m x nf)
    const int* bir = nullptr;
    const double* bpr = nullptr;
    const double* cf = nullptr;     // nf
    double* wf = nullptr;           // free multipliers w                 (nf)
    double* Af = nullptr;           // Af of the last cost evaluation     (nf)
    double* x = nullptr;            // multiplier matrix x                (n x nS)
    double* bA = nullptr;           // reshape(iA*b)                      (n x nS)
    double* T = nullptr;            // bA + x - sigma*C                   (n x nS)
    double* Sg = nullptr;           // S = Y*Y'                           (n x nS)
    double* G2[2] = {nullptr, nullptr};   // Y'*Y per slot                (ld x ld)
    double* M1 = nullptr;           // U'*Y of the current Hess-vec       (ld x ld)
    double* pp_part = nullptr;      // DUAL_PP_BLOCKS x ld x ld partials
    double* scal = nullptr;         // [0] f, [1] b'y, [2] <C,eX>, [3] |As|^2
    bool T_valid = false;
    // generic kind (MSDP_KIND_DUAL) only; T then holds C - x/sigma
    bool generic = false;
    bool g_identity = false;        // G = D\A*A' is exactly I (setup check)
    const int64_t* arp = nullptr;   // A by rows: row pointers (m + 1), row-major positions i*nS + j, values
    const int64_t* apos = nullptr;
    const double* aval = nullptr;
    const int* brp = nullptr;       // B by rows (m x nf CSR)
    const int* bcol = nullptr;
    const double* bval = nullptr;
    double* R = nullptr;            // bA - sigma*As                     (n x nS)
    double* v = nullptr;            // the m-vector of the current adjoint
    double* tB = nullptr;           // B'a of the current Hess-vec        (nf)
    // multiblock kind (MSDP_KIND_DUAL_MULTIBLOCK): every n x nS operand above is the per-block storage of BlockedDev instead,
    // G2 / M1 hold one ld x ld Gram matrix per block
    bool blocked = false;
    int64_t tot = 0;                // entries of one operand: n * nS, or sum n_i * nS_i
    int nb = 1;
    const int* blk_r0 = nullptr;    // nb + 1: first row of every block
    const int* rowblk = nullptr;    // N: block of every row
    int64_t zrows = 0;              // rows of the first nob (unit-diagonal) blocks: the z of msdp_dual_outer_step
};
void msdp_dual_release(DualState* ds) { delete ds; }
#define DUAL_PP_BLOCKS 64
#define DUAL_PP_MAXLD 128

// y = (A(S) - A c) ./ dAAt in place, partial sums of b'y -> P_S1   (grid d.G)
__global__ __launch_bounds__(MSDP_BLOCK) void k_dual_y(int64_t m, double* __restrict__ w, const double* __restrict__ dinv,
                                                       const double* __restrict__ Ac, const double* __restrict__ b, double* P,
                                                       const int* skip_flag, int skip_when) {
    __shared__ double sh[3 * MSDP_WAVES];
    if (skip_flag && *skip_flag == skip_when) return;
    double pb = 0.0;
    for (int64_t k = blockIdx.x * (int64_t)MSDP_BLOCK + threadIdx.x; k < m; k += (int64_t)gridDim.x * MSDP_BLOCK) {
        const double y = (w[k] - Ac[k]) * dinv[k];
        w[k] = y;
        pb = fma(b[k], y, pb);
    }
    msdp_put_partial(P, P_S1, pb, sh);
}
// w .*= dinv (Hess-vec: iA'*vec(Y'U))
__global__ void k_dual_scale(int64_t m, double* __restrict__ w, const double* __restrict__ dinv, const int* skip_flag, int skip_when) {
    if (skip_flag && *skip_flag == skip_when) return;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < m; k += (int64_t)gridDim.x * blockDim.x) w[k] *= dinv[k];
}
// Af_j = B(:,j)'(y .* ys) - cf_j - (wf ? wf_j / sigma : 0): one workgroup per free variable (ys, cf may be null: 1, 0)
__global__ __launch_bounds__(256) void k_dual_free(const int* __restrict__ bjc, const int* __restrict__ bir, const double* __restrict__ bpr,
                                                   const double* __restrict__ y, const double* __restrict__ cf, const double* wf,
                                                   double sigma, double* __restrict__ Af, const int* skip_flag, int skip_when,
                                                   const double* __restrict__ ys = nullptr) {
    __shared__ double sh[MSDP_WAVES];
    if (skip_flag && *skip_flag == skip_when) return;
    const int j = blockIdx.x;
    double v = 0.0;
    for (int t = bjc[j] + threadIdx.x; t < bjc[j + 1]; t += blockDim.x) v = fma(bpr[t], ys ? y[bir[t]] * ys[bir[t]] : y[bir[t]], v);
    v = msdp_block_sum(v, sh);
    if (threadIdx.x == 0) Af[j] = v - (cf ? cf[j] : 0.0) - (wf ? wf[j] / sigma : 0.0);
}
// X += sigma*S, and the partial sums of |bA - X|^2 (= sigma^2 |As|^2) -> P_AXB   (MSDP_MAX_GRID workgroups)
__global__ __launch_bounds__(256) void k_dual_finish_X(int64_t tot, double* __restrict__ X, const double* __restrict__ S,
                                                       const double* __restrict__ bA, double sigma, double* P,
                                                       const int* skip_flag, int skip_when) {
    __shared__ double sh[3 * MSDP_WAVES];
    if (skip_flag && *skip_flag == skip_when) return;
    double ps = 0.0;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x) {
        const double xv = fma(sigma, S[e], X[e]);
        X[e] = xv;
        const double r = bA[e] - xv;
        ps = fma(r, r, ps);
    }
    msdp_put_partial(P, P_AXB, ps, sh);
}
// f = b'y + |bA - X|^2 / (2 sigma) + sigma/2 |Af|^2   (one workgroup)
__global__ __launch_bounds__(MSDP_BLOCK) void k_dual_cost(Dev d, double sigma, const double* __restrict__ Af, int nf, double* out,
                                                          const int* skip_flag, int skip_when) {
    __shared__ double sh[8];
    if (skip_flag && *skip_flag == skip_when) return;
    const double by = msdp_sum_partials_block(d.P, P_S1, d.G, sh);
    __syncthreads();
    const double ss = msdp_sum_partials_block(d.P, P_AXB, MSDP_MAX_GRID, sh);
    if (threadIdx.x == 0) {
        double af = 0.0;
        for (int j = 0; j < nf; ++j) af = fma(Af[j], Af[j], af);
        out[0] = by + 0.5 * ss / sigma + 0.5 * sigma * af;
        out[1] = by;
    }
}
// T = cb*bA + cx*x + cc*C: bA + x - sigma*C (unit diagonal), C - x/sigma (generic)
__global__ void k_dual_T(int64_t tot, double* __restrict__ T, const double* __restrict__ bA, const double* __restrict__ x,
                         const double* __restrict__ C, double cb, double cx, double cc) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x)
        T[e] = fma(cb, bA[e], fma(cx, x[e], cc * C[e]));
}
// generic: As = Q - S (Q = C - x/sigma + A'y in X), S <- As, R = bA - sigma*As; partial sums of (sigma*As)^2 -> P_AXB
// (MSDP_MAX_GRID workgroups: k_dual_cost divides by sigma)
__global__ __launch_bounds__(256) void k_dgen_as(int64_t tot, int n, int nS, const double* __restrict__ Q, double* __restrict__ S,
                                                 const double* __restrict__ bA, double sigma, double* __restrict__ R, double* P,
                                                 const int* skip_flag, int skip_when) {
    __shared__ double sh[3 * MSDP_WAVES];
    if (skip_flag && *skip_flag == skip_when) return;
    double ps = 0.0;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x) {
        if ((int)(e % nS) >= n) continue;                  // pad columns stay as they are (zero)
        const double as = Q[e] - S[e];
        S[e] = as;
        R[e] = fma(-sigma, as, bA[e]);
        ps = fma(sigma * as, sigma * as, ps);
    }
    msdp_put_partial(P, P_AXB, ps, sh);
}
// generic, one wave per row k of A (no atomics):
//   out_k = dinv_k * (ca * sum_t A_kt Dn[pos_t] + cb * sum_j B_kj f_j) + cw * w_k * (wd ? dinv_k : 1)
// cost/grad: Dn = As, f = Af, ca = cb = sigma, cw = 0.  Hess-vec fix-up: f = B'a, cb = 1, w = A(U Y') with wd (a = w/dAAt),
// cw = -1 when G = I; with G: Dn = A'a, ca = 1, w = a, cw = -2.  Dn / f may be null.
__global__ __launch_bounds__(256) void k_dgen_rows(int64_t m, const int64_t* __restrict__ arp, const int64_t* __restrict__ apos,
                                                   const double* __restrict__ aval, const double* __restrict__ Dn, double ca,
                                                   const int* __restrict__ brp, const int* __restrict__ bcol, const double* __restrict__ bval,
                                                   const double* __restrict__ f, double cb, const double* __restrict__ dinv,
                                                   const double* __restrict__ w, double cw, int wd, double* __restrict__ out,
                                                   const int* skip_flag, int skip_when) {
    if (skip_flag && *skip_flag == skip_when) return;
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t k = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); k < m; k += nw) {
        double sa = 0.0, sb = 0.0;
        if (Dn) for (int64_t t = arp[k] + lane; t < arp[k + 1]; t += 64) sa = fma(aval[t], Dn[apos[t]], sa);
        if (f) for (int t = brp[k] + lane; t < brp[k + 1]; t += 64) sb = fma(bval[t], f[bcol[t]], sb);
        sa = msdp_wave_sum(sa);
        sb = msdp_wave_sum(sb);
        if (lane == 0) {
            const double dk = dinv[k];
            double o = dk * fma(ca, sa, cb * sb);
            if (w) o = fma(cw * (wd ? dk : 1.0), w[k], o);
            out[k] = o;
        }
    }
}
// generic outer step :73-77 after the cost state at Y: X (Xd) = bA + sigma*(...) of :169 with the pre-update x and w,
// S holds As - x/sigma.  x <- X - bA; partial sums of <C, X> -> P_S2 and |As|^2 (As without x/sigma) -> P_S3   (grid d.G)
__global__ __launch_bounds__(MSDP_BLOCK) void k_dgen_outer(Dev d, int nS, const double* __restrict__ Xd, const double* __restrict__ S,
                                                           double* __restrict__ x, const double* __restrict__ bA,
                                                           const double* __restrict__ C, double sigma) {
    __shared__ double sh[3 * MSDP_WAVES];
    const int64_t tot = (int64_t)d.n * nS;
    double pc = 0.0, pa = 0.0;
    for (int64_t e = blockIdx.x * (int64_t)MSDP_BLOCK + threadIdx.x; e < tot; e += (int64_t)gridDim.x * MSDP_BLOCK) {
        if ((int)(e % nS) >= d.n) continue;
        const double X = Xd[e], xo = x[e];
        const double as = S[e] + xo / sigma;
        x[e] = X - bA[e];
        pc = fma(C[e], X, pc);
        pa = fma(as, as, pa);
    }
    msdp_put_partials3(d.P, P_S2, pc, P_S3, pa, -1, 0.0, sh);
}
// P = Xa' * Xb (ld x ld) from two n x ld panels: per-workgroup partials over a row range, then their sum
__global__ __launch_bounds__(256) void k_pp_gram_part(int n, int ld, const double* __restrict__ Xa, const double* __restrict__ Xb,
                                                      double* __restrict__ part, const int* skip_flag, int skip_when) {
    if (skip_flag && *skip_flag == skip_when) return;
    const int rows = (n + gridDim.x - 1) / gridDim.x;
    const int r0 = blockIdx.x * rows, r1 = min(n, r0 + rows);
    for (int e = threadIdx.x; e < ld * ld; e += blockDim.x) {
        const int a = e / ld, b = e - a * ld;
        double acc = 0.0;
        for (int k = r0; k < r1; ++k) acc = fma(Xa[(int64_t)k * ld + a], Xb[(int64_t)k * ld + b], acc);
        part[(int64_t)blockIdx.x * ld * ld + e] = acc;
    }
}
__global__ void k_pp_gram_sum(int ld, int nblk, const double* __restrict__ part, double* __restrict__ out, const int* skip_flag, int skip_when) {
    if (skip_flag && *skip_flag == skip_when) return;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < ld * ld; e += gridDim.x * blockDim.x) {
        double acc = 0.0;
        for (int q = 0; q < nblk; ++q) acc += part[(int64_t)q * ld * ld + e];
        out[e] = acc;
    }
}
// out(i,:) = coef * (Y(i,:)*M1 + U(i,:)*G2): the 2*sigma*((Y*U')*Y + (Y*Y')*U) term of :192, one more split-K slab
__global__ void k_pp_apply(int n_loc, int ld, const double* __restrict__ Y, const double* __restrict__ U, const double* __restrict__ M1,
                           const double* __restrict__ G2, double coef, double* __restrict__ out, const int* skip_flag, int skip_when) {
    if (skip_flag && *skip_flag == skip_when) return;
    const int64_t tot = (int64_t)n_loc * ld;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / ld; const int c = (int)(e - i * ld);
        double acc = 0.0;
        for (int a = 0; a < ld; ++a) acc = fma(Y[i * ld + a], M1[a * ld + c], fma(U[i * ld + a], G2[a * ld + c], acc));
        out[e] = coef * acc;
    }
}
// Outer step :73-81 on the rows of a workgroup: As = (C + A'y) - S (in Xd), x -= sigma*As, eX = x + bA,
// z_i = sum_j S_ij eX_ij, Xd = eX - diag(z); partial sums of <C, eX> -> P_S2 and |As|^2 -> P_S3   (grid d.G)
__global__ __launch_bounds__(MSDP_BLOCK) void k_dual_outer(Dev d, int nS, double* __restrict__ Xd, const double* __restrict__ S,
                                                           double* __restrict__ x, const double* __restrict__ bA,
                                                           const double* __restrict__ C, double sigma, double* __restrict__ z) {
    __shared__ double sh[3 * MSDP_WAVES];
    int lo, hi;
    msdp_chunk_rows(d.n_loc, d.G, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double pc = 0.0, pa = 0.0;
    for (int row = lo + wave; row < hi; row += MSDP_WAVES) {
        const int64_t o = (int64_t)row * nS;
        double zr = 0.0, exd = 0.0;
        for (int j = lane; j < d.n; j += 64) {
            const double as = Xd[o + j] - S[o + j];
            const double xn = x[o + j] - sigma * as;
            const double ex = xn + bA[o + j];
            x[o + j] = xn;
            Xd[o + j] = ex;
            zr = fma(S[o + j], ex, zr);
            pc = fma(C[o + j], ex, pc);
            pa = fma(as, as, pa);
            if (j == row) exd = ex;
        }
        zr = msdp_wave_sum(zr);
        if (lane == (row & 63)) { Xd[o + row] = exd - zr; z[row] = zr; }
    }
    msdp_put_partials3(d.P, P_S2, pc, P_S3, pa, -1, 0.0, sh);
}

// ------------------------------------------------------------------ dual, multiblock (MSDP_KIND_DUAL_MULTIBLOCK)
// src/dual/ManiDSDP_multiblock.m: S_i = Y_i'Y_i per block, the first nob blocks unit-diagonal (oblique rows), the others
// Euclidean (the primal multiblock kind's rowfree flag).  All operands live in the per-block storage of BlockedDev (memory and
// work ~ sum n_i^2).  nob == nb runs the unit-diagonal dual kind's closures (tt = bA - sigma*As, :257-258; tYU of :282-283),
// nob < nb the generic kind's (tt with iAB*Af and A'(iA'*As), :259-260; tYU of :284-286) -- on the blocks: S by k_block_gram,
// the dense products by k_block_contract (msdp_affine_gemm), the p_i x p_i Grams of 2*sigma*Y_i(T_i + T_i') per block in one launch
// (k_bpp_gram / k_bpp_apply).  No launch depends on nb.
// per-block Gram out_b = Xa_b' * Xb_b (ld x ld) of the rows of block b: grid (nb, chunks of the ld x ld entries)
__global__ __launch_bounds__(256) void k_bpp_gram(const int* __restrict__ blk_r0, int ld, const double* __restrict__ Xa,
                                                  const double* __restrict__ Xb, double* __restrict__ out, const int* skip_flag, int skip_when) {
    if (skip_flag && *skip_flag == skip_when) return;
    const int b = blockIdx.x;
    const int r0 = blk_r0[b], r1 = blk_r0[b + 1];
    double* __restrict__ ob = out + (int64_t)b * ld * ld;
    for (int e = blockIdx.y * blockDim.x + threadIdx.x; e < ld * ld; e += gridDim.y * blockDim.x) {
        const int a = e / ld, c = e - a * ld;
        double acc = 0.0;
        for (int k = r0; k < r1; ++k) acc = fma(Xa[(int64_t)k * ld + a], Xb[(int64_t)k * ld + c], acc);
        ob[e] = acc;
    }
}
// out(i,:) = coef * (Y(i,:)*M1_b + U(i,:)*G2_b), b = the block of row i: the 2*sigma*Y_i(T_i + T_i') term, one more slab
__global__ void k_bpp_apply(int n, int ld, const int* __restrict__ rowblk, const double* __restrict__ Y, const double* __restrict__ U,
                            const double* __restrict__ M1, const double* __restrict__ G2, double coef, double* __restrict__ out,
                            const int* skip_flag, int skip_when) {
    if (skip_flag && *skip_flag == skip_when) return;
    const int64_t tot = (int64_t)n * ld;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / ld; const int c = (int)(e - i * ld);
        const int64_t bo = (int64_t)rowblk[i] * ld * ld;
        double acc = 0.0;
        for (int a = 0; a < ld; ++a) acc = fma(Y[i * ld + a], M1[bo + a * ld + c], fma(U[i * ld + a], G2[bo + a * ld + c], acc));
        out[e] = coef * acc;
    }
}
// Outer step :86-124 after the cost state at Y, one wave per row of the direct sum.  Xd holds tt (:257-260) with the multipliers
// of the solve; Asx = As - x/sigma (generic form: in Sg; unit form: (bA - tt)/sigma); Sf = S.  x <- tt - bA (both forms of
// :102-106); rows of the unit-diagonal blocks: z_r = sum_j S_rj X_rj, X_rr -= z_r (:115-118); z = 0 on the Euclidean rows.
// Partial sums of <C, X> -> P_S2 and |As|^2 -> P_S3   (grid d.G)
__global__ __launch_bounds__(MSDP_BLOCK) void k_dmb_outer(Dev d, BlockedDev bd, double* __restrict__ Xd, const double* __restrict__ Sg,
                                                          const double* __restrict__ Sf, double* __restrict__ x, const double* __restrict__ bA,
                                                          const double* __restrict__ C, double sigma, int generic, double* __restrict__ z) {
    __shared__ double sh[3 * MSDP_WAVES];
    int lo, hi;
    msdp_chunk_rows(d.n_loc, d.G, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double pc = 0.0, pa = 0.0;
    for (int row = lo + wave; row < hi; row += MSDP_WAVES) {
        const int64_t o = bd.rbase[row];
        const int len = bd.rhi[row] - bd.rlo[row], dc = row - bd.rlo[row];
        double zr = 0.0, exd = 0.0;
        for (int j = lane; j < len; j += 64) {
            const double X = Xd[o + j], xo = x[o + j], ba = bA[o + j];
            const double asx = generic ? Sg[o + j] : (ba - X) / sigma;
            const double as = asx + xo / sigma;
            x[o + j] = X - ba;
            zr = fma(Sf[o + j], X, zr);
            pc = fma(C[o + j], X, pc);
            pa = fma(as, as, pa);
            if (j == dc) exd = X;
        }
        zr = msdp_wave_sum(zr);
        const bool ob = !(d.rowfree && d.rowfree[row]);
        if (lane == (dc & 63)) {
            if (ob) Xd[o + dc] = exd - zr;
            z[row] = ob ? zr : 0.0;
        }
    }
    msdp_put_partials3(d.P, P_S2, pc, P_S3, pa, -1, 0.0, sh);
}

static int dgen_rows_grid(int64_t m) {
    int64_t g = (m + 3) / 4;                               // four waves (rows) per workgroup
    if (g > 4096) g = 4096;
    return (int)std::max<int64_t>(g, 1);
}
static int dual_pp_gram(msdp_handle h, DualState* ds, const double* Xa, const double* Xb, double* out, const int* flag, int when) {
    const Dev& d = h->d;
    if (ds->blocked) {                                   // one ld x ld Gram per block, all blocks in one launch
        const int gy = std::max(1, std::min(64, (d.ld * d.ld + 255) / 256));
        hipLaunchKernelGGL(k_bpp_gram, dim3(ds->nb, gy), dim3(256), 0, h->stream, ds->blk_r0, d.ld, Xa, Xb, out, flag, when);
        HIPCHK(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(k_pp_gram_part, dim3(DUAL_PP_BLOCKS), dim3(256), 0, h->stream, d.n, d.ld, Xa, Xb, ds->pp_part, flag, when);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_pp_gram_sum, dim3((d.ld * d.ld + 255) / 256), dim3(256), 0, h->stream, d.ld, DUAL_PP_BLOCKS,
                       (const double*)ds->pp_part, out, flag, when);
    HIPCHK(hipGetLastError());
    return 0;
}
static int dual_check(msdp_handle h, DualState* ds) {
    if (h->d.ld > DUAL_PP_MAXLD) { msdp_set_error("dual kind: factor width p = %d exceeds the supported maximum of %d", h->d.p, DUAL_PP_MAXLD); return MSDP_EUNSUPPORTED; }
    if (!ds->T_valid) { msdp_set_error("dual kind: call msdp_dual_set_penalty after msdp_dual_outer_step"); return MSDP_ESTATE; }
    return 0;
}
// steps shared by cost/grad and the line-search cost: y, Af, S, X = T + sigma*S - sigma*A'y into Xout, f -> scal[0]
static int dual_cost_state(msdp_handle h, AffineState* st, const double* Ys, double* Xout, const int* flag, int when) {
    DualState* ds = st->dual;
    Dev& d = h->d;
    AffineDev a = st->a;
    a.p = d.p; a.ld = d.ld;
    const double sigma = st->sigma;
    int rc;
    if ((rc = msdp_affine_launch_A(h, a, st->nnz, Ys, Ys, flag, when, 0, (double*)nullptr, sigma))) return rc;
    hipLaunchKernelGGL(k_dual_y, dim3(d.G), dim3(MSDP_BLOCK), 0, h->stream, a.m, a.w, ds->dinv, ds->Ac, a.b, d.P, flag, when);
    HIPCHK(hipGetLastError());
    if (ds->nf > 0) {
        hipLaunchKernelGGL(k_dual_free, dim3(ds->nf), dim3(256), 0, h->stream, ds->bjc, ds->bir, ds->bpr, (const double*)a.w, ds->cf,
                           (const double*)ds->wf, sigma, ds->Af, flag, when);
        HIPCHK(hipGetLastError());
    }
    if ((rc = msdp_affine_gram(h, Ys, Ys, ds->Sg, flag, when))) return rc;
    if (ds->generic) {
        // Q = (C - x/sigma) + A'y; As = Q - S (into Sg), R = bA - sigma*As; v = sigma*D\(A*As + B*Af); X = R + A'v
        if ((rc = msdp_affine_launch_adjoint(h, a, (const double*)ds->T, (const double*)a.w, 1.0, Xout, flag, when, false))) return rc;
        // (per-block storage: pad columns are zero in every operand, so no column test -- n = nS = 1)
        hipLaunchKernelGGL(k_dgen_as, dim3(MSDP_MAX_GRID), dim3(256), 0, h->stream, ds->tot, ds->blocked ? 1 : a.n, ds->blocked ? 1 : a.nS, (const double*)Xout,
                           ds->Sg, (const double*)ds->bA, sigma, ds->R, d.P, flag, when);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_dgen_rows, dim3(dgen_rows_grid(a.m)), dim3(256), 0, h->stream, a.m, ds->arp, ds->apos, ds->aval,
                           (const double*)ds->Sg, sigma, ds->brp, ds->bcol, ds->bval, ds->nf > 0 ? (const double*)ds->Af : (const double*)nullptr,
                           sigma, ds->dinv, (const double*)nullptr, 0.0, 0, ds->v, flag, when);
        HIPCHK(hipGetLastError());
        if ((rc = msdp_affine_launch_adjoint(h, a, (const double*)ds->R, (const double*)ds->v, 1.0, Xout, flag, when, false))) return rc;
    } else {
        if ((rc = msdp_affine_launch_adjoint(h, a, (const double*)ds->T, (const double*)a.w, -sigma, Xout, flag, when, false))) return rc;
        hipLaunchKernelGGL(k_dual_finish_X, dim3(MSDP_MAX_GRID), dim3(256), 0, h->stream, ds->tot, Xout, (const double*)ds->Sg,
                           (const double*)ds->bA, sigma, d.P, flag, when);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_dual_cost, dim3(1), dim3(MSDP_BLOCK), 0, h->stream, d, sigma, (const double*)ds->Af, ds->nf, ds->scal, flag, when);
    HIPCHK(hipGetLastError());
    return 0;
}

int msdp_dual_costgrad(msdp_handle h, AffineState* st, int slot) {
    DualState* ds = st->dual;
    Dev& d = h->d;
    int rc;
    if ((rc = dual_check(h, ds))) return rc;
    const double* Ys = d.Y[slot];
    const int* done = &d.ctl->done;
    if ((rc = dual_cost_state(h, st, Ys, d.eS[slot], done, 1))) return rc;
    // eG = 2*X*Y -> Gr[slot], row dots YeG
    const double* slab; int64_t stride; int SK;
    const double* M[1] = {d.eS[slot]}; const double* X[1] = {Ys}; const double sc[1] = {1.0};
    if ((rc = msdp_affine_gemm(h, 1, M, X, sc, nullptr, &slab, &stride, &SK))) return rc;
    if ((rc = msdp_affine_rowdot_slabs(h, Ys, slab, stride, SK, 2.0, d.Gr[slot], d.eG[slot], P_S2))) return rc;
    // generic kind: G = 2*X*Y as is (euclideanfactory: no projection, :170); the multiblock kind projects the rows of its
    // unit-diagonal blocks only (k_obl_grad_finish with rowfree, :265-269)
    if ((rc = msdp_affine_grad_finish(h, !(ds->generic && !ds->blocked), slot, st->sigma, ds->scal))) return rc;
    return dual_pp_gram(h, ds, Ys, Ys, ds->G2[slot], done, 1);
}

int msdp_dual_hess(msdp_handle h, AffineState* st) {
    DualState* ds = st->dual;
    Dev& d = h->d;
    AffineDev a = st->a;
    a.p = d.p; a.ld = d.ld;
    const double sigma = st->sigma;
    const int cur = h->h_ctl->cur;
    const int* act = &d.F[0].active;
    int rc;
    if ((rc = dual_check(h, ds))) return rc;
    double cA = -4.0 * sigma;
    if (ds->generic) {
        // w = A(U Y') (a = w/dAAt); v = D\B*(B'a) + G*a - 2a; AyU = A'v   (:175-176)
        if ((rc = msdp_affine_launch_A(h, a, st->nnz, d.md, d.Y[cur], act, 0, 0, (double*)nullptr, sigma))) return rc;
        const bool gI = ds->g_identity;
        if (!gI) {
            int64_t g = (a.m + 255) / 256; if (g > 2048) g = 2048;
            hipLaunchKernelGGL(k_dual_scale, dim3((int)g), dim3(256), 0, h->stream, a.m, a.w, ds->dinv, act, 0);
            HIPCHK(hipGetLastError());
            if ((rc = msdp_affine_launch_adjoint(h, a, (const double*)nullptr, (const double*)a.w, 1.0, d.AyU, act, 0, false))) return rc;
        }
        if (ds->nf > 0) {
            hipLaunchKernelGGL(k_dual_free, dim3(ds->nf), dim3(256), 0, h->stream, ds->bjc, ds->bir, ds->bpr, (const double*)a.w,
                               (const double*)nullptr, (const double*)nullptr, sigma, ds->tB, act, 0, gI ? ds->dinv : (const double*)nullptr);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_dgen_rows, dim3(dgen_rows_grid(a.m)), dim3(256), 0, h->stream, a.m, ds->arp, ds->apos, ds->aval,
                           gI ? (const double*)nullptr : (const double*)d.AyU, 1.0, ds->brp, ds->bcol, ds->bval,
                           ds->nf > 0 ? (const double*)ds->tB : (const double*)nullptr, 1.0, ds->dinv, (const double*)a.w,
                           gI ? -1.0 : -2.0, gI ? 1 : 0, ds->v, act, 0);
        HIPCHK(hipGetLastError());
        if ((rc = msdp_affine_launch_adjoint(h, a, (const double*)nullptr, (const double*)ds->v, 1.0, d.AyU, act, 0, false))) return rc;
        cA = 4.0 * sigma;
    } else {
        if ((rc = msdp_affine_launch_A(h, a, st->nnz, d.Y[cur], d.md, act, 0, 0, (double*)nullptr, sigma))) return rc;
        { int64_t g = (a.m + 255) / 256; if (g > 2048) g = 2048;
          hipLaunchKernelGGL(k_dual_scale, dim3((int)g), dim3(256), 0, h->stream, a.m, a.w, ds->dinv, act, 0); }
        HIPCHK(hipGetLastError());
        if ((rc = msdp_affine_launch_adjoint(h, a, (const double*)nullptr, (const double*)a.w, 1.0, d.AyU, act, 0, false))) return rc;
    }
    const double* slab; int64_t stride; int SK;
    const double* M[2] = {d.eS[cur], d.AyU};
    const double* X[2] = {d.md, d.Y[cur]};
    const double sc[2] = {2.0, cA};
    if ((rc = msdp_affine_gemm(h, 2, M, X, sc, act, &slab, &stride, &SK))) return rc;
    if ((rc = dual_pp_gram(h, ds, d.md, d.Y[cur], ds->M1, act, 0))) return rc;
    double* extra = const_cast<double*>(slab) + (int64_t)SK * stride;
    { int64_t g = ((int64_t)d.n_loc * d.ld + 255) / 256; if (g > 4096) g = 4096;
      if (ds->blocked)
          hipLaunchKernelGGL(k_bpp_apply, dim3((int)g), dim3(256), 0, h->stream, d.n_loc, d.ld, ds->rowblk, (const double*)d.Y[cur], (const double*)d.md,
                             (const double*)ds->M1, (const double*)ds->G2[cur], 2.0 * sigma, extra, act, 0);
      else
          hipLaunchKernelGGL(k_pp_apply, dim3((int)g), dim3(256), 0, h->stream, d.n_loc, d.ld, (const double*)d.Y[cur], (const double*)d.md,
                             (const double*)ds->M1, (const double*)ds->G2[cur], 2.0 * sigma, extra, act, 0); }
    HIPCHK(hipGetLastError());
    ++SK;
    if (ds->generic && !ds->blocked) return msdp_sphere_hess_raw(h, slab, stride, SK);      // Euclidean epilogue: H as is
    return msdp_dense_hess_epilogue_obl(h, slab, stride, SK);
}

// co(Y) of :155-162 at the trial point Yt
int msdp_dual_linesearch_cost(msdp_handle h, AffineState* st, const double* Yt, double* val) {
    DualState* ds = st->dual;
    Dev& d = h->d;
    int rc;
    if ((rc = dual_check(h, ds))) return rc;
    const int other = h->h_ctl->cur ^ 1;
    if ((rc = dual_cost_state(h, st, Yt, d.eS[other], (const int*)nullptr, 0))) return rc;
    double v = 0.0;
    HIPCHK(msdp_memcpy_async(&v, ds->scal, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *val = v;
    return 0;
}

// Second half of msdp_create_dual_unitdiag / msdp_create_dual: msdp_affine_setup has uploaded At (= A'), b and C = reshape(c).
int msdp_dual_setup(msdp_handle h, const int64_t* at_jc, const int64_t* at_ir, const double* at_pr, const double* b, const double* c,
                    const double* dAAt, int32_t nf, const int64_t* b_jc, const int64_t* b_ir, const double* b_pr, const double* cf,
                    bool generic) {
    AffineState* st = h->affine;
    if (!st) { msdp_set_error("affine state missing"); return MSDP_ESTATE; }
    Dev& d = h->d;
    const int n = d.n, nS = st->a.nS;
    const int64_t m = st->a.m;
    DualState* ds = new DualState();
    st->dual = ds;
    ds->nf = nf;
    // stored position of column-major vec index r: (r % n, r / n) of the n x nS array, or of its block in the per-block storage
    ds->blocked = st->blk != nullptr;
    ds->tot = ds->blocked ? st->blk->etot : (int64_t)n * nS;
    const int nbk = ds->blocked ? (int)st->blk_n.size() : 1;
    std::vector<int64_t> e0((size_t)nbk + 1, 0);
    for (int i = 0; i < nbk; ++i) e0[(size_t)i + 1] = e0[(size_t)i] + (ds->blocked ? (int64_t)st->blk_n[(size_t)i] * st->blk_n[(size_t)i] : (int64_t)n * n);
    auto spos = [&](int64_t r) -> int64_t {
        if (!ds->blocked) return (r % n) * nS + r / n;
        const int i = (int)(std::upper_bound(e0.begin(), e0.end(), r) - e0.begin()) - 1;
        const int64_t l = r - e0[(size_t)i], bn = st->blk_n[(size_t)i];
        return st->blk_off[(size_t)i] + (l % bn) * st->blk_ns[(size_t)i] + l / bn;
    };
    std::vector<double> dinv((size_t)m), Ac((size_t)m, 0.0), bA((size_t)ds->tot, 0.0);
    for (int64_t k = 0; k < m; ++k) {
        if (!(dAAt[k] > 0.0)) { msdp_set_error("dual kind: dAAt(%lld) = %g is not positive", (long long)k, dAAt[k]); return MSDP_EINVAL; }
        dinv[(size_t)k] = 1.0 / dAAt[k];
        double acc = 0.0;
        const double bk = b[k] * dinv[(size_t)k];
        for (int64_t t = at_jc[k]; t < at_jc[k + 1]; ++t) {
            const int64_t r = at_ir[t];                    // column-major vec index i + j*n -> row-major (i, j)
            if (r < 0 || r >= e0[(size_t)nbk]) { msdp_set_error("dual kind: row index of At out of range"); return MSDP_EINVAL; }
            acc += at_pr[t] * c[r];
            bA[(size_t)spos(r)] += at_pr[t] * bk;          // bA = iA*b (:39)
        }
        Ac[(size_t)k] = acc;
    }
    int rc;
    if ((rc = msdp_upload(h, dinv, &ds->dinv)) || (rc = msdp_upload(h, Ac, &ds->Ac))) return rc;
    std::vector<int> bjc((size_t)nf + 1, 0), bir;
    std::vector<double> bpr, cfv((size_t)std::max(nf, 1), 0.0);
    for (int j = 0; j < nf; ++j) {
        for (int64_t t = b_jc[j]; t < b_jc[j + 1]; ++t) {
            if (b_ir[t] < 0 || b_ir[t] >= m) { msdp_set_error("dual kind: row index of B out of range"); return MSDP_EINVAL; }
            bir.push_back((int)b_ir[t]); bpr.push_back(b_pr[t]);
        }
        bjc[(size_t)j + 1] = (int)bir.size();
        cfv[(size_t)j] = cf[j];
    }
    if (bir.empty()) { bir.push_back(0); bpr.push_back(0.0); }
    if ((rc = msdp_upload(h, bjc, &ds->bjc)) || (rc = msdp_upload(h, bir, &ds->bir)) || (rc = msdp_upload(h, bpr, &ds->bpr)) || (rc = msdp_upload(h, cfv, &ds->cf))) return rc;
    const size_t msz = (size_t)ds->tot * sizeof(double);
    void* p = nullptr;
    double** mats[4] = {&ds->x, &ds->bA, &ds->T, &ds->Sg};
    for (int q = 0; q < 4; ++q) {
        if ((rc = msdp_dev_alloc_bytes(h, &p, msz))) return rc;
        *mats[q] = (double*)p;
        HIPCHK(hipMemset(p, 0, msz));
    }
    HIPCHK(msdp_memcpy(ds->bA, bA.data(), msz, hipMemcpyHostToDevice));
    const size_t ppsz = (size_t)DUAL_PP_MAXLD * DUAL_PP_MAXLD * sizeof(double) * nbk;      // one per block (multiblock kind)
    double** pps[3] = {&ds->G2[0], &ds->G2[1], &ds->M1};
    for (int q = 0; q < 3; ++q) {
        if ((rc = msdp_dev_alloc_bytes(h, &p, ppsz))) return rc;
        *pps[q] = (double*)p;
        HIPCHK(hipMemset(p, 0, ppsz));
    }
    if (!ds->blocked) {
        if ((rc = msdp_dev_alloc_bytes(h, &p, ppsz * DUAL_PP_BLOCKS))) return rc;
        ds->pp_part = (double*)p;
    } else {
        ds->nb = nbk;
        std::vector<int> br0((size_t)nbk + 1), rowblk((size_t)n);
        for (int i = 0; i <= nbk; ++i) br0[(size_t)i] = (int)st->blk_r0[(size_t)i];
        for (int i = 0; i < nbk; ++i) for (int r = br0[(size_t)i]; r < br0[(size_t)i + 1]; ++r) rowblk[(size_t)r] = i;
        if ((rc = msdp_upload(h, br0, &ds->blk_r0)) || (rc = msdp_upload(h, rowblk, &ds->rowblk))) return rc;
    }
    const size_t nfb = (size_t)std::max(nf, 1) * sizeof(double);
    if ((rc = msdp_dev_alloc_bytes(h, &p, nfb))) return rc;
    ds->wf = (double*)p; HIPCHK(hipMemset(p, 0, nfb));
    if ((rc = msdp_dev_alloc_bytes(h, &p, nfb))) return rc;
    ds->Af = (double*)p; HIPCHK(hipMemset(p, 0, nfb));
    if ((rc = msdp_dev_alloc_bytes(h, &p, 8 * sizeof(double)))) return rc;
    ds->scal = (double*)p; HIPCHK(hipMemset(p, 0, 8 * sizeof(double)));
    // the adjoint of the dual kind always sweeps the whole matrix (X and As are dense)
    if (!generic) return 0;
    ds->generic = true;
    // A by rows (the columns of At) with row-major positions; G = I check: disjoint supports, dAAt(k) == sum_t A_kt^2 bit for bit
    std::vector<int64_t> arp((size_t)m + 1, 0), apos;
    std::vector<double> aval;
    std::vector<unsigned char> used((size_t)e0[(size_t)nbk], 0);
    bool gI = true;
    for (int64_t k = 0; k < m; ++k) {
        double ss = 0.0;
        for (int64_t t = at_jc[k]; t < at_jc[k + 1]; ++t) {
            const int64_t r = at_ir[t];
            if (used[(size_t)r]) gI = false;
            used[(size_t)r] = 1;
            ss += at_pr[t] * at_pr[t];
            apos.push_back(spos(r));
            aval.push_back(at_pr[t]);
        }
        if (ss != dAAt[k]) gI = false;
        arp[(size_t)k + 1] = (int64_t)apos.size();
    }
    if (apos.empty()) { apos.push_back(0); aval.push_back(0.0); }
    ds->g_identity = gI;
    std::vector<int> brp((size_t)m + 1, 0), bcol(std::max<size_t>(bir.size(), 1), 0);
    std::vector<double> bval(std::max<size_t>(bir.size(), 1), 0.0);
    for (int j = 0; j < nf; ++j)
        for (int t = bjc[(size_t)j]; t < bjc[(size_t)j + 1]; ++t) ++brp[(size_t)bir[(size_t)t] + 1];
    for (int64_t k = 0; k < m; ++k) brp[(size_t)k + 1] += brp[(size_t)k];
    {
        std::vector<int> fill(brp.begin(), brp.end() - 1);
        for (int j = 0; j < nf; ++j)
            for (int t = bjc[(size_t)j]; t < bjc[(size_t)j + 1]; ++t) {
                const int q = fill[(size_t)bir[(size_t)t]]++;
                bcol[(size_t)q] = j; bval[(size_t)q] = bpr[(size_t)t];
            }
    }
    if ((rc = msdp_upload(h, arp, &ds->arp)) || (rc = msdp_upload(h, apos, &ds->apos)) || (rc = msdp_upload(h, aval, &ds->aval)) ||
        (rc = msdp_upload(h, brp, &ds->brp)) || (rc = msdp_upload(h, bcol, &ds->bcol)) || (rc = msdp_upload(h, bval, &ds->bval))) return rc;
    if ((rc = msdp_dev_alloc_bytes(h, &p, msz))) return rc;
    ds->R = (double*)p; HIPCHK(hipMemset(p, 0, msz));
    if ((rc = msdp_dev_alloc_bytes(h, &p, (size_t)m * sizeof(double)))) return rc;
    ds->v = (double*)p; HIPCHK(hipMemset(p, 0, (size_t)m * sizeof(double)));
    if ((rc = msdp_dev_alloc_bytes(h, &p, nfb))) return rc;
    ds->tB = (double*)p; HIPCHK(hipMemset(p, 0, nfb));
    return 0;
}

// the rows of the first nob blocks of a multiblock dual handle (the length of its z)
int msdp_dual_set_zrows(msdp_handle h, int64_t zrows) {
    AffineState* st = h->affine;
    if (!st || !st->dual) { msdp_set_error("dual state missing"); return MSDP_ESTATE; }
    st->dual->zrows = zrows;
    return 0;
}

int msdp_dual_g_identity(msdp_handle h) {
    AffineState* st = h->affine;
    return (st && st->dual && st->dual->g_identity) ? 1 : 0;
}

// sigma and the free multipliers w for the next trustregions() call; T = bA + x - sigma*C (generic: C - x/sigma)
int msdp_dual_set_penalty_impl(msdp_handle h, double sigma, const double* wf_host) {
    AffineState* st = h->affine;
    if (!st || !st->dual) { msdp_set_error("dual_set_penalty: not a dual handle"); return MSDP_ESTATE; }
    if (!(sigma > 0)) { msdp_set_error("sigma must be positive"); return MSDP_EINVAL; }
    DualState* ds = st->dual;
    if (ds->nf > 0) {
        if (!wf_host) { msdp_set_error("dual_set_penalty: w is null"); return MSDP_EINVAL; }
        HIPCHK(msdp_memcpy_async(ds->wf, wf_host, (size_t)ds->nf * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    st->sigma = sigma;
    h->h_ctl->sigma = sigma;
    const int64_t tot = ds->tot;
    if (ds->generic)
        hipLaunchKernelGGL(k_dual_T, dim3(2048), dim3(256), 0, h->stream, tot, ds->T, (const double*)ds->bA, (const double*)ds->x,
                           (const double*)h->d.Cd, 0.0, -1.0 / sigma, 1.0);
    else
        hipLaunchKernelGGL(k_dual_T, dim3(2048), dim3(256), 0, h->stream, tot, ds->T, (const double*)ds->bA, (const double*)ds->x,
                           (const double*)h->d.Cd, 1.0, 1.0, -sigma);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    ds->T_valid = true;
    return 0;
}

// :70-81 at the resident point: scal = {b'y, <C, eX>, |As|^2}, Af = B'y - cf (nf), z (n); x is updated on the device,
// X = eX - diag(z) is left in d.Sdual for msdp_escape_eigs_dual / msdp_get_dual_slack, y in a.w for msdp_dual_get_y.
int msdp_dual_outer_step_impl(msdp_handle h, double* scal_host, double* Af_host, double* z_host) {
    AffineState* st = h->affine;
    if (!st || !st->dual) { msdp_set_error("dual_outer_step: not a dual handle"); return MSDP_ESTATE; }
    DualState* ds = st->dual;
    Dev& d = h->d;
    AffineDev a = st->a;
    a.p = d.p; a.ld = d.ld;
    const double sigma = st->sigma;
    const double* Ys = d.Y[h->h_ctl->cur];
    int rc;
    if (ds->blocked) {
        // ManiDSDP_multiblock.m:86-124: tt of :257-260 at Y with the multipliers of the solve -> d.Sdual; x = tt - bA; z and
        // X_i - diag(z_i) on the unit-diagonal blocks (k_dmb_outer)
        if ((rc = dual_check(h, ds))) return rc;
        if ((rc = dual_cost_state(h, st, Ys, d.Sdual, (const int*)nullptr, 0))) return rc;
        if (ds->nf > 0) {                                  // Af = B'y - cf (:97)
            hipLaunchKernelGGL(k_dual_free, dim3(ds->nf), dim3(256), 0, h->stream, ds->bjc, ds->bir, ds->bpr, (const double*)a.w, ds->cf,
                               (const double*)nullptr, sigma, ds->Af, (const int*)nullptr, 0, (const double*)nullptr);
            HIPCHK(hipGetLastError());
        }
        const double* Sf = ds->Sg;
        if (ds->generic) {                                 // Sg holds As - x/sigma there: S again, into the spent R
            if ((rc = msdp_affine_gram(h, Ys, Ys, ds->R, (const int*)nullptr, 0))) return rc;
            Sf = ds->R;
        }
        hipLaunchKernelGGL(k_dmb_outer, dim3(d.G), dim3(MSDP_BLOCK), 0, h->stream, d, *st->blk, d.Sdual, (const double*)ds->Sg, Sf, ds->x,
                           (const double*)ds->bA, (const double*)d.Cd, sigma, ds->generic ? 1 : 0, d.W0);
        HIPCHK(hipGetLastError());
        if ((rc = msdp_k_sum_to(h, P_S2, ds->scal + 2)) || (rc = msdp_k_sum_to(h, P_S3, ds->scal + 3))) return rc;
        HIPCHK(msdp_memcpy_async(scal_host, ds->scal + 1, 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (ds->nf > 0) HIPCHK(msdp_memcpy_async(Af_host, ds->Af, (size_t)ds->nf * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (ds->zrows > 0 && z_host) HIPCHK(msdp_memcpy_async(z_host, d.W0, (size_t)ds->zrows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        ds->T_valid = false;
        return 0;
    }
    if (ds->generic) {
        // :66-77: X of :169 at Y with the multipliers of the solve (x, w/sigma in T and wf) -> d.Sdual; then x = X - bA
        if ((rc = dual_check(h, ds))) return rc;
        if ((rc = dual_cost_state(h, st, Ys, d.Sdual, (const int*)nullptr, 0))) return rc;
        if (ds->nf > 0) {                                  // Af = B'y - cf (:70)
            hipLaunchKernelGGL(k_dual_free, dim3(ds->nf), dim3(256), 0, h->stream, ds->bjc, ds->bir, ds->bpr, (const double*)a.w, ds->cf,
                               (const double*)nullptr, sigma, ds->Af, (const int*)nullptr, 0, (const double*)nullptr);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_dgen_outer, dim3(d.G), dim3(MSDP_BLOCK), 0, h->stream, d, a.nS, (const double*)d.Sdual, (const double*)ds->Sg,
                           ds->x, (const double*)ds->bA, (const double*)d.Cd, sigma);
        HIPCHK(hipGetLastError());
        if ((rc = msdp_k_sum_to(h, P_S2, ds->scal + 2)) || (rc = msdp_k_sum_to(h, P_S3, ds->scal + 3))) return rc;
        HIPCHK(msdp_memcpy_async(scal_host, ds->scal + 1, 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (ds->nf > 0) HIPCHK(msdp_memcpy_async(Af_host, ds->Af, (size_t)ds->nf * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        ds->T_valid = false;
        return 0;
    }
    if ((rc = msdp_affine_launch_A(h, a, st->nnz, Ys, Ys, (const int*)nullptr, 0, 0, (double*)nullptr, sigma))) return rc;
    hipLaunchKernelGGL(k_dual_y, dim3(d.G), dim3(MSDP_BLOCK), 0, h->stream, a.m, a.w, ds->dinv, ds->Ac, a.b, d.P, (const int*)nullptr, 0);
    HIPCHK(hipGetLastError());
    if ((rc = msdp_k_sum_to(h, P_S1, ds->scal + 1))) return rc;
    if (ds->nf > 0) {
        hipLaunchKernelGGL(k_dual_free, dim3(ds->nf), dim3(256), 0, h->stream, ds->bjc, ds->bir, ds->bpr, (const double*)a.w, ds->cf,
                           (const double*)nullptr, sigma, ds->Af, (const int*)nullptr, 0);
        HIPCHK(hipGetLastError());
    }
    if ((rc = msdp_affine_gram(h, Ys, Ys, ds->Sg, (const int*)nullptr, 0))) return rc;
    // (d.Sdual may alias the Gram scratch a.W: msdp_affine_launch_A has consumed it by now)
    if ((rc = msdp_affine_launch_adjoint(h, a, (const double*)d.Cd, (const double*)a.w, 1.0, d.Sdual, (const int*)nullptr, 0, false))) return rc;
    hipLaunchKernelGGL(k_dual_outer, dim3(d.G), dim3(MSDP_BLOCK), 0, h->stream, d, a.nS, d.Sdual, (const double*)ds->Sg, ds->x,
                       (const double*)ds->bA, (const double*)d.Cd, sigma, d.W0);
    HIPCHK(hipGetLastError());
    if ((rc = msdp_k_sum_to(h, P_S2, ds->scal + 2)) || (rc = msdp_k_sum_to(h, P_S3, ds->scal + 3))) return rc;
    HIPCHK(msdp_memcpy_async(scal_host, ds->scal + 1, 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (ds->nf > 0) HIPCHK(msdp_memcpy_async(Af_host, ds->Af, (size_t)ds->nf * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(msdp_memcpy_async(z_host, d.W0, (size_t)a.n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    ds->T_valid = false;
    return 0;
}

int msdp_dual_get_y_impl(msdp_handle h, double* y_host) {
    AffineState* st = h->affine;
    if (!st || !st->dual) { msdp_set_error("dual_get_y: not a dual handle"); return MSDP_ESTATE; }
    HIPCHK(msdp_memcpy_async(y_host, st->a.w, (size_t)st->a.m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
