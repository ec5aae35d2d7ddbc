/*
 * manisdp_hip.h -- C ABI of libmanisdp_hip.so, the MI355X (gfx950) hot path of
 * ManiSDP's three primal entry points.
 *
 * The reference (wangjie212/ManiSDP-matlab) has no FFI on this path: its operator
 * interface is Manopt's problem struct consumed by trustregions()
 *   problem.cost / problem.grad / problem.hess / problem.M.*
 *   (src/primal/ManiSDP_onlyunitdiag.m:28-30,39,43; ManiSDP_unitdiag.m:41-43,53,57;
 *    ManiSDP_unittrace.m:42-44,53,57).
 * This library is cut AT the trustregions() call: the factor Y stays resident in
 * HBM for the whole Riemannian trust-region solve and never crosses PCIe inside
 * tCG.  The only native-call precedent in the reference is the MEX gateway of
 * src/C-files/<fn>.cpp (plain double* via mxGetPr, errors via mexErrMsgIdAndTxt);
 * the MEX shim in manisdp-matlab_amd/matlab/manisdp_mex.cpp binds exactly the
 * entry points declared here.
 *
 * Conventions
 *  - every function returns 0 on success, a negative MSDP_E* code otherwise;
 *    msdp_last_error() returns a human-readable message (no exceptions cross the ABI);
 *  - all floating-point data is IEEE double (the reference is fp64 throughout);
 *  - sparse inputs are MATLAB-style compressed columns with 64-bit indices
 *    (mwIndex Jc/Ir, 0-based);
 *  - factor layout at the boundary is the reference's own:
 *      oblique entry points (onlyunitdiag, unitdiag): Y is p x n column-major
 *        (each point's p-vector contiguous; ManiSDP_unitdiag.m:59 X = Y'*Y);
 *      unittrace: Y is n x p column-major (ManiSDP_unittrace.m:59 X = Y*Y');
 *  - the library is single-caller per handle (MATLAB's interpreter thread).
 */
#ifndef MANISDP_HIP_H
#define MANISDP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSDP_OK              0
#define MSDP_EINVAL         -1   /* bad argument                                 */
#define MSDP_EHIP           -2   /* HIP runtime error                            */
#define MSDP_ENOMEM         -3   /* device or host allocation failed             */
#define MSDP_ESTATE         -4   /* call order violated (e.g. no point resident) */
#define MSDP_ECOMM          -5   /* RCCL error                                   */
#define MSDP_EUNSUPPORTED   -6

typedef struct msdp_handle_s* msdp_handle;

/* Problem kinds (which reference entry point the handle serves). */
#define MSDP_KIND_ONLYUNITDIAG 1   /* src/primal/ManiSDP_onlyunitdiag.m */
#define MSDP_KIND_UNITDIAG     2   /* src/primal/ManiSDP_unitdiag.m     */
#define MSDP_KIND_UNITTRACE    3   /* src/primal/ManiSDP_unittrace.m    */
#define MSDP_KIND_GENERIC      4   /* src/primal/ManiSDP.m (Euclidean manifold) */
#define MSDP_KIND_MULTIBLOCK   5   /* src/primal/ManiSDP_multiblock.m (product manifold) */
#define MSDP_KIND_DUAL_UNITDIAG 6  /* src/dual/ManiDSDP_unitdiag.m (dual approach, diag(S) = 1) */
#define MSDP_KIND_DUAL         7   /* src/dual/ManiDSDP.m (dual approach, Euclidean factor of S) */
#define MSDP_KIND_DUAL_MULTIBLOCK 8 /* src/dual/ManiDSDP_multiblock.m (dual approach, one factor per block) */

/* Options of one Riemannian trust-region solve: the fields ManiSDP sets
 * (ManiSDP_unitdiag.m:44-47) plus Manopt's defaults that are in force
 * (manopt7.0/manopt/solvers/trustregions/trustregions.m:340-351,363-372).
 * Delta_bar <= 0 / Delta0 <= 0 select the reference's defaults
 * (M.typicaldist(), Delta_bar/8). */
typedef struct {
    int32_t maxiter;          /* opts.maxiter  = options.TR_maxiter            */
    int32_t maxinner;         /* opts.maxinner = options.TR_maxinner           */
    int32_t mininner;         /* Manopt default 1                              */
    int32_t reserved0;
    double  tolgradnorm;      /* opts.tolgradnorm                              */
    double  kappa;            /* 0.1                                           */
    double  theta;            /* 1.0                                           */
    double  rho_prime;        /* 0.1                                           */
    double  rho_regularization; /* 1e3                                         */
    double  Delta_bar;        /* <=0: typicaldist                              */
    double  Delta0;           /* <=0: Delta_bar/8                              */
} msdp_rtr_opts;

/* What the AL loop reads back from trustregions(): info(end).gradnorm and the
 * cost, plus the counters the reference does not report. */
typedef struct {
    double  cost;             /* f at the returned point                       */
    double  gradnorm;         /* info(end).gradnorm                            */
    double  Delta;            /* final trust-region radius                     */
    double  seconds;          /* wall-clock of the solve (host timer)          */
    int32_t iters;            /* TR iterations performed                       */
    int32_t hessvecs;         /* sum(info.numinner)                            */
    int32_t accepted;
    int32_t rejected;
    int32_t cost_evals;
    int32_t last_stop_inner;  /* tCG stop code 1..6 of the last TR iteration   */
    int32_t reserved[2];
} msdp_rtr_stats;

void msdp_rtr_default_opts(msdp_rtr_opts* o);

/* ---------------------------------------------------------------- life cycle */

/* Select the HIP device of the calling thread (one process per GPU: LOCAL_RANK). */
int msdp_set_device(int32_t device);
int msdp_device_count(int32_t* count);

/* min <C,X>, diag X = 1 with sparse symmetric C (n x n) given as MATLAB CSC
 * (= CSR by symmetry).  Replaces the closures of ManiSDP_onlyunitdiag.m:117-130.
 * pcap: initial capacity for the factor width (grown on demand). */
int msdp_create_onlyunitdiag_csc(int64_t n, const int64_t* jc, const int64_t* ir,
                                 const double* pr, int32_t pcap, msdp_handle* out);

/* Same with a dense symmetric C (n x n, column-major == row-major). */
int msdp_create_onlyunitdiag_dense(int64_t n, const double* C, int32_t pcap,
                                   msdp_handle* out);

/* Same with C = Cs + V diag(s) V' held implicitly: Cs sparse symmetric in CSC as above (its diagonal may be present), V
 * n x q column-major, s of length q (either sign).  Stands for ManiSDP_onlyunitdiag.m:6 (the cost matrix C the closures of
 * :117-130 multiply with), without ever forming the dense n x n matrix: a product C*U is the sparse product plus the two
 * skinny ones T = diag(s) V' U (q x p, a deterministic two-stage reduction) and V T.  1 <= q <= MSDP_LOWRANK_MAX and V, s not
 * NULL, else MSDP_EINVAL.  Cost, gradient, Hess-vec, msdp_rtr (the generic per-iteration path), the Lanczos escape and
 * msdp_round_hyperplane accept the handle; joining a communicator of any form returns MSDP_EUNSUPPORTED. */
#define MSDP_LOWRANK_MAX 8
int msdp_create_onlyunitdiag_csc_lowrank(int64_t n, const int64_t* jc, const int64_t* ir, const double* pr,
                                         int32_t q, const double* V, const double* s, int32_t pcap, msdp_handle* out);

/* The complex problem  min <C, X>  s.t. X Hermitian PSD, X_ii = 1  with a sparse Hermitian C = A + iB (phase synchronisation,
 * unimodular quadratic programmes; manopt's elliptope_SDP_complex).  jc / ir as for msdp_create_onlyunitdiag_csc; val holds
 * nnz interleaved (re, im) pairs -- the bytes of a complex128 array -- in the same CSC order.  C must be Hermitian (row i is
 * read as the conjugate of column i); a diagonal entry with a non-zero imaginary part returns MSDP_EINVAL.
 * Width convention: a factor of complex width p (n x p complex numbers, row-major) crosses EVERY entry point as its real
 * view of width 2p -- msdp_set_point(h, 2p, Y) with Y the n x 2p doubles (re, im, re, im, ...) of the complex rows, and
 * msdp_get_point, msdp_hessvec, msdp_rgrad, msdp_proj, msdp_retr likewise; msdp_get_p reports 2p.  An odd width returns
 * MSDP_EINVAL.  pcap of this call counts complex columns.  msdp_cost and msdp_get_z stay real (z_i = Re conj(y_i) (C Y)_i).
 * msdp_escape_eigs returns k complex eigenvectors of S = C - diag(z): V holds k columns of n (re, im) pairs (2 n k doubles),
 * orthonormal in the complex inner product, eigenvalues ascending, none reported more often than S has it (Lanczos path on
 * the real view; span(Y) is not deflated).  msdp_rtr runs the generic per-iteration path.
 * MSDP_EUNSUPPORTED: every communicator, msdp_round_hyperplane, msdp_factor_gram / _rotate / _append -- the kind has calls
 * of its own for both: msdp_round_phases (rounding to phases) and msdp_hfactor_gram / _rotate / _append (below). */
int msdp_create_onlyunitdiag_csc_hermitian(int64_t n, const int64_t* jc, const int64_t* ir, const double* val, int32_t pcap,
                                           msdp_handle* out);

/* The unit-block-diagonal problem  min <C, X>  s.t. X PSD of order N = n d, X_[ii] = I_d (i = 1..n)  with d = 2 or 3
 * (synchronisation over O(d) / SO(d): rotation averaging, pose graphs).  jc / ir / val: the symmetric order-N cost matrix in
 * CSC as for msdp_create_onlyunitdiag_csc; it is stored in block CSR of block order d (one column index per d x d block,
 * zero-filled where the pattern covers a block in part).  d outside {2, 3} and N % d != 0 return MSDP_EINVAL; pcap > 256
 * returns MSDP_EUNSUPPORTED, as does msdp_set_point with p > 256.
 * The factor Y (N x p row-major, as for the other onlyunitdiag handles) is n blocks of d consecutive rows with
 * Y_i Y_i' = I_d: manopt's stiefelstackedfactory(n, d, p), which replaces the n d (d - 1) / 2 affine constraints and the
 * multipliers the same SDP needs through msdp_create_unitdiag.  With sym(M) = (M + M') / 2 and f = <C, Y Y'> / 2:
 *   msdp_cost      f;   Lambda_i = sym((C Y)_i Y_i'),  S = C - blockdiag(Lambda),  <C, X> = sum_i tr Lambda_i = 2 f
 *   msdp_rgrad     (C Y)_i - Lambda_i Y_i                                     (stiefelstackedfactory.m:81-87)
 *   msdp_hessvec   W_i - sym(W_i Y_i') Y_i  with  W = C U - blockdiag(Lambda) U   (:93-101)
 *   msdp_proj      Z_i - sym(Z_i Y_i') Y_i                                    (:81-89)
 *   msdp_retr      the polar factor (A_i A_i')^(-1/2) A_i of A_i = Y_i + U_i  (:103-117)
 * The trust-region radius defaults to Delta_bar = sqrt(n (p d - d (d + 1) / 2)) (:43,53), Delta0 = Delta_bar / 8.
 * msdp_set_point takes any N x p array: p < d and blocks that are not orthonormal are the caller's business.
 * msdp_get_z returns the N diagonal entries of the Lambda_i (sum = <C, X>), msdp_get_blockmult the blocks themselves.
 * msdp_rtr runs the generic per-iteration path; msdp_escape_eigs the Lanczos path on S (span(Y) deflated at near-stationary
 * points, as for the scalar kind: the columns of Y are N-vectors with S Y = 0 at a critical point).
 * MSDP_EUNSUPPORTED: every communicator, msdp_round_hyperplane, msdp_factor_gram / _rotate / _append (the rank cut and the
 * re-orthonormalisation of the blocks stay on the host), msdp_linesearch_cost / _accept. */
int msdp_create_onlyunitblockdiag_csc(int64_t N, int32_t d, const int64_t* jc, const int64_t* ir, const double* val, int32_t pcap,
                                      msdp_handle* out);
/* Lam: n d d doubles, block i = Lambda_i row-major (symmetric), at the resident point (a pose-graph handle: the d x d
 * multipliers of its rotation rows).  Other handles: MSDP_EUNSUPPORTED. */
int msdp_get_blockmult(msdp_handle h, double* Lam);

/* The pose-graph problem  min <C, X>  s.t. X PSD of order N = n (d + 1), (X_[ii])_{1..d,1..d} = I_d (i = 1..n)  with d = 2 or
 * 3 (synchronisation over SE(d), the non-marginalised form of SE-Sync / Cartan-Sync): only the leading d x d part of every
 * diagonal block is pinned, the last row and column of a block are free.  jc / ir / val: the symmetric order-N cost matrix in
 * CSC as for msdp_create_onlyunitblockdiag_csc, stored in block CSR of block order d + 1.  The caller is responsible for C
 * being bounded below on the free rows (a pose-graph C is PSD).  d outside {2, 3} and N % (d + 1) != 0 return MSDP_EINVAL;
 * pcap > 256 returns MSDP_EUNSUPPORTED, as does msdp_set_point with p > 256.
 * The factor Y (N x p row-major) is n blocks of d rows Y_i with Y_i Y_i' = I_d followed by one free row tau_i: manopt's
 * productmanifold of stiefelstackedfactory(n, d, p) and euclideanfactory(n, p), Frobenius metric.  With (C Y)_i = [G_i; g_i],
 * sym(M) = (M + M') / 2 and f = <C, Y Y'> / 2:
 *   msdp_cost      f;   Lambda_i = sym(G_i Y_i') (d x d),  S = C - blockdiag(Lambda_i (+) 0)
 *                  <C, X> = 2 f = sum_i tr Lambda_i + sum_i <g_i, tau_i>: the dual value sum_i tr Lambda_i equals <C, X> only
 *                  at a critical point (g = 0 there)
 *   msdp_rgrad     [G_i - Lambda_i Y_i ; g_i]                                  (stiefelstackedfactory.m:81-87, euclideanfactory.m:38)
 *   msdp_hessvec   W = C U - blockdiag(Lambda (+) 0) U;  rotation rows W_i - sym(W_i Y_i') Y_i, the free row of W unchanged
 *   msdp_proj      Z_i - sym(Z_i Y_i') Y_i on the rotation rows, the identity on the free row
 *   msdp_retr      the polar factor of Y_i + U_i (stiefelstackedfactory.m:103-117), tau_i + u_i on the free row (euclideanfactory.m:44)
 * The trust-region radius defaults to Delta_bar = sqrt(n (p d - d (d + 1) / 2) + n p) (productmanifold.m:160-166 over
 * stiefelstackedfactory.m:53 and euclideanfactory.m:57), Delta0 = Delta_bar / 8.
 * msdp_get_z returns N values, the diagonal of Lambda_i followed by 0 for the free row, block by block: their sum is the dual
 * value.  msdp_get_blockmult returns the n d x d blocks.  msdp_rtr runs the generic per-iteration path; msdp_escape_eigs the
 * Lanczos path on S with the zero-padded multiplier (S Y = 0 at a critical point, so span(Y) is deflated as for the other
 * kinds; for a pose-graph C the global shift 1 (x) e_{d+1} is always in the null space of S).
 * MSDP_EUNSUPPORTED, with the kind named in msdp_last_error: every communicator, msdp_debug_shard, msdp_round_hyperplane,
 * msdp_factor_gram / _rotate / _append, msdp_linesearch_cost / _accept. */
int msdp_create_posegraph_csc(int64_t N, int32_t d, const int64_t* jc, const int64_t* ir, const double* val, int32_t pcap,
                              msdp_handle* out);

/* Pre-sharded synthetic dense problem (BASELINE config 5: n = 100000, p = 64 over 8 GPUs; the full C would be
 * 80 GB): rank `rank` of `nranks` fills ITS rows of a dense symmetric C on the device from a counter-based
 * generator; msdp_synthetic_dense_entry is the same generator on the host (parity tests). */
int msdp_create_onlyunitdiag_dense_synthetic(int64_t n, uint64_t seed, int32_t nranks, int32_t rank,
                                             int32_t pcap, msdp_handle* out);
double msdp_synthetic_dense_entry(int64_t n, int64_t i, int64_t j, uint64_t seed);
/* Test-only: stand in for the all-gather on a communicator-free shard (one process = rank r of N). */
int msdp_debug_set_full_rows(msdp_handle h, const double* rows_host);
/* Test-only: the point-to-point calls of the halo exchange (one ncclGroupStart .. ncclSend + ncclRecv .. ncclGroupEnd on the
 * handle's communicator and stream) with the handle's own rank as peer: `count` doubles in -> out through two device
 * buffers.  Lets a single-GPU box run the RCCL half of the exchange; the send / receive lists are covered by the
 * in-process ranks (tests/test_gpu_local_ranks.py). */
int msdp_debug_p2p_self(msdp_handle h, int64_t count, const double* in_host, double* out_host);
/* Test-only: eta and Heta of the last tCG solve of msdp_rtr (reference layout), valid after a call with maxiter = 1 on the
 * chunked path or on the persistent path with option fused_rtr = 0.  Lets a test check tCG's invariant Heta = Hess(eta)
 * (tCG.m:192-220) on the device, i.e. bound what the persistent kernel's linearity trick for C*mdelta may drift. */
int msdp_debug_get_tcg_step(msdp_handle h, double* eta, double* Heta);
/* Test-only, host code only (no GPU touched): the dense symmetric eigen-solver (Householder + implicit QL; w ascending, row i
 * of Z = eigenvector i) and the generalised Rayleigh-Ritz problem H c = theta G c (theta ascending, +inf beyond *rank; W b x b
 * row-major, column j = coefficients of Ritz vector j, W'GW = I on the first *rank columns) of the block eigen-solver. */
int msdp_debug_sym_eig(int32_t n, const double* A, double* w, double* Z);
int msdp_debug_ritz(int32_t b, const double* G, const double* H, double* theta, double* W, int32_t* rank);
/* Test-only, host code only: the same problem for the complex panel of a Hermitian cost matrix (be_ritz_herm: complex Cholesky,
 * Householder to a real tridiagonal form, the same QL).  G, H, W: bc x bc complex, row-major, (re, im) interleaved, G and H
 * Hermitian; theta[bc] ascending, +inf beyond *rank; W^H G W = I on the first *rank columns, zero columns beyond.  Every complex
 * direction appears once. */
int msdp_debug_ritz_herm(int32_t bc, const double* G, const double* H, double* theta, double* W, int32_t* rank);
/* Test-only GPU twin of msdp_debug_ritz: uploads G and H and runs the kernel of the device Rayleigh-Ritz stage (option
 * "escape_rr" = 1; k_be_ritz, msdp_beritz.hip) alone on the current device -- no handle, no fallback to the host stage.  b = 32
 * or 64 (else MSDP_EUNSUPPORTED: the three b x b matrices of a 128-wide panel do not fit the LDS).  *status: 0 = ok (theta
 * ascending, W'GW = I, *rank = b), 1 = the kernel asks for the host stage (dependent columns: a Cholesky pivot <= 1e-11 max diag G;
 * or Jacobi not converged in 40 sweeps), 2 = breakdown (non-finite entry, max diag G <= 0); theta, W and *rank are zero then. */
int msdp_debug_ritz_device(int32_t b, const double* G, const double* H, double* theta, double* W, int32_t* rank, int32_t* status);
/* Rayleigh-Ritz stages of the block eigen-solver since the handle was created, by where their dense algebra ran: on the
 * device, on the host, and on the host after the device kernel handed the stage back (status 1 or 2 above). */
int msdp_debug_ritz_stages(msdp_handle h, int64_t* device, int64_t* host, int64_t* fallback);
/* Test-only: the (panel width, lanes per block) pairs the filter step on block storage (k_be_step_blk, msdp_blockeig.hip) is
 * instantiated for, pairs[2i], pairs[2i + 1] for the first `cap` of them; returns their number.  No GPU touched. */
int msdp_debug_be_step_blk_instances(int32_t* pairs, int32_t cap);
/* Test-only: one launch of that step on host panels at the resident point of a unit-block-diagonal or pose-graph handle.  Xin,
 * Xio: N x b row-major (N = the handle's order, b = 32 / 64 / 128 columns); Xio <- f1 * (S * Xin) - f1 * cs * Xin - f2 * Xio
 * with S = C - blockdiag(Lambda_i (+) 0) (prev = 0: without the last term).  lpr: lanes per block; a (b, lpr) pair without an
 * instance is MSDP_EUNSUPPORTED.  The route's lower limit N >= 256 does not apply. */
int msdp_debug_be_step_blk(msdp_handle h, int32_t b, int32_t lpr, const double* Xin, double* Xio, double f1, double cs, double f2,
                           int32_t prev);
/* Test-only: make a sparse-C handle rank `rank` of `nranks` WITHOUT a communicator (same row split, local CSR/ELL
 * rows with global column indices and gather buffer as msdp_comm_init sets up), so that one GPU can check every
 * shard's kernels against the unsharded result.  Call right after create, before any point is set. */
int msdp_debug_shard(msdp_handle h, int32_t nranks, int32_t rank);

/* min <C,X>, A(X) = b, diag X = 1 (kind = MSDP_KIND_UNITDIAG;
 * ManiSDP_unitdiag.m:152-171) or tr X = 1 (kind = MSDP_KIND_UNITTRACE;
 * ManiSDP_unittrace.m:156-177), or no further structure at all (kind =
 * MSDP_KIND_GENERIC; ManiSDP.m:149-164 on euclideanfactory(n, p): proj = identity,
 * retr = Y + U).  At is n^2 x m CSC (column k = vec(A_k)), b dense m, c dense n^2
 * (the shim densifies a sparse c).  Y is n x p column-major for UNITTRACE and GENERIC. */
int msdp_create_affine(int32_t kind, int64_t n, int64_t m,
                       const int64_t* at_jc, const int64_t* at_ir, const double* at_pr,
                       const double* b, const double* c, int32_t pcap, msdp_handle* out);

/* min <C,X>, A(X) = b over block-diagonal X = diag(X_1..X_nb) with diag(X_i) = 1 for the first `nob` blocks
 * (ManiSDP_multiblock.m:1-7; closures cost/grad/hess :208-249; manifold = multiblockmanifold.m:1-42 over the MEX
 * helpers src/C-files/{innerc,lincombc,projc,retrc,randc,zerovecc}.cpp: oblique factors for the first nob blocks,
 * Euclidean ones for the rest).  SeDuMi data for several SDP blocks: At is (sum n_i^2) x m CSC whose rows are the
 * concatenated column-major vecs of the blocks, c likewise, b dense m.
 * The factor crosses the boundary as ONE p x N column-major array, N = sum n_i: block i occupies columns
 * [N_i, N_i + n_i) and, when its own width p_i is smaller than p, rows p_i..p-1 of those columns are zero (zero
 * rows of a block stay zero under cost, gradient, Hess-vec, projection and retraction, so padding changes nothing).
 * Internally the problem is the unit-diagonal affine kind of order N whose constraint matrices are block diagonal,
 * with a per-row flag that switches the projection / normalisation terms off for the Euclidean blocks.
 * Storage: up to 15 blocks with N < 4096 the operands are embedded N x N arrays; beyond that every operand is the
 * concatenation of its diagonal blocks (memory and work ~ sum n_i^2; environment MSDP_MULTIBLOCK_BLOCKED = 0 / 1 forces
 * either form), msdp_get_dual_slack_block is then the way to read S and msdp_get_dual_slack returns MSDP_EUNSUPPORTED. */
int msdp_create_multiblock(int32_t nb, const int64_t* block_n, int32_t nob, int64_t m,
                           const int64_t* at_jc, const int64_t* at_ir, const double* at_pr,
                           const double* b, const double* c, int32_t pcap, msdp_handle* out);

/* Dual approach with a unit-diagonal dual slack (src/dual/ManiDSDP_unitdiag.m:8-220):
 *     sup <C,X> + <cf,w>   s.t.  A(X) + B(w) = b,  X psd,  the variable of the Riemannian subproblem is S = Y'Y with
 * diag(S) = 1 (obliquefactoryNTrans, :196-219), the multipliers are x = vec(X) and w.  Closures replaced:
 * cost :174-181, grad :183-187, hess :189-194, co/line_search :155-172; outer-step bookkeeping :70-85.
 * at_* is A' (n^2 x m CSC: column k = vec of the k-th row of the PSD part A(:, K.f+1:end)), dAAt = diag(A*A') (:37,
 * options.dAAt), c the PSD part of the cost (dense n^2), B = A(:, 1:K.f) as m x nf CSC (nf may be 0), cf its costs. */
int msdp_create_dual_unitdiag(int64_t n, int64_t m, const int64_t* at_jc, const int64_t* at_ir, const double* at_pr,
                              const double* dAAt, const double* b, const double* c, int32_t nf, const int64_t* b_jc,
                              const int64_t* b_ir, const double* b_pr, const double* cf, int32_t pcap, msdp_handle* out);
/* sigma and the free multipliers w (nf values) for the following trustregions() calls (the matrix multiplier x lives on
 * the device and starts at 0, :48).  Must be called before the first solve and after every msdp_dual_outer_step. */
int msdp_dual_set_penalty(msdp_handle h, double sigma, const double* w);
/* Outer step :70-81 at the resident point with the current sigma: y = iA'*(S(:) - c); As = A'y - sc; x -= sigma*As on the
 * device; eX = x + bA; z = sum(S.*eX); X = eX - diag(z) stays on the device for msdp_escape_eigs_dual /
 * msdp_get_dual_slack.  scal[0] = b'y, scal[1] = <C, eX>, scal[2] = |As|^2; Af[nf] = B'y - cf; z[n]. */
int msdp_dual_outer_step(msdp_handle h, double* scal, double* Af, double* z);
/* y of the last msdp_dual_outer_step (m values; data.y, :134) */
int msdp_dual_get_y(msdp_handle h, double* y);
/* Generic dual approach (src/dual/ManiDSDP.m:7-178): the arguments of msdp_create_dual_unitdiag, S = Y*Y' with Y on the
 * Euclidean manifold (euclideanfactory(n, p), :60); the factor crosses the boundary as the n x p column-major array of
 * MSDP_KIND_GENERIC.  Closures replaced: costgrad :162-171, hess :173-177, co / line_search :141-160.  The handle takes
 * msdp_dual_set_penalty, msdp_dual_get_y, msdp_rtr and the single-operator / line-search calls as the unit-diagonal kind
 * does; msdp_dual_outer_step performs :66-77 (x <- x + sigma*(iAB*(Af - w/sigma) + A'(iA'*(As - x/sigma)) - As), with
 * scal[0] = b'y, scal[1] = <C, x + bA>, scal[2] = |As|^2 and Af = B'y - cf; z is not used and may be NULL) and leaves
 * X = mat(x + bA) on the device for msdp_escape_eigs_dual / msdp_get_dual_slack.  A factor wider than 128 columns gives
 * MSDP_EUNSUPPORTED. */
int msdp_create_dual(int64_t n, int64_t m, const int64_t* at_jc, const int64_t* at_ir, const double* at_pr,
                     const double* dAAt, const double* b, const double* c, int32_t nf, const int64_t* b_jc,
                     const int64_t* b_ir, const double* b_pr, const double* cf, int32_t pcap, msdp_handle* out);
/* *g_identity = 1 when the setup proved D\A*A' = I (rows of A with pairwise disjoint supports and dAAt equal to their
 * squared norms bit for bit): the Hess-vec then skips the G*a terms of ManiDSDP.m:176.  Dual handles only. */
int msdp_dual_info(msdp_handle h, int32_t* g_identity);
/* Multiblock dual approach (src/dual/ManiDSDP_multiblock.m:8-298): nb blocks of orders block_n, S_i = Y_i'Y_i with unit diagonal
 * on the first nob blocks (oblique rows) and a Euclidean factor on the others.  at_* is the PSD part of A transposed,
 * (sum n_i^2) x m, its rows the concatenated column-major vecs of the blocks (the layout of msdp_create_multiblock); c is the
 * PSD cost in that layout; dAAt, b, nf, B (b_*), cf as for msdp_create_dual (nf = 0: no free part).  The factor crosses the
 * boundary as msdp_create_multiblock's one zero-padded array (row r of the direct sum = column r of its block's Y_i, p values).
 * The handle takes msdp_dual_set_penalty, msdp_dual_get_y, msdp_rtr, the single-operator and line-search calls,
 * msdp_get_dual_slack_block and msdp_block_eigs (they read the blocks X_i).  msdp_dual_outer_step performs :86-124: scal[0] =
 * b'y, scal[1] = <c, x + bA>, scal[2] = |As|^2, Af = B'y - cf, z = the diagonal multipliers of the first nob blocks (their rows
 * in order; may be NULL when nob = 0), X_i = mat(x + bA)_i - diag(z_i) left on the device.  msdp_get_dual_slack gives
 * MSDP_EUNSUPPORTED; a factor wider than 128 columns gives MSDP_EUNSUPPORTED. */
int msdp_create_dual_multiblock(int32_t nb, const int64_t* block_n, int32_t nob, int64_t m, const int64_t* at_jc,
                                const int64_t* at_ir, const double* at_pr, const double* dAAt, const double* b, const double* c,
                                int32_t nf, const int64_t* b_jc, const int64_t* b_ir, const double* b_pr, const double* cf,
                                int32_t pcap, msdp_handle* out);

int msdp_destroy(msdp_handle h);
/* The library keeps ONE device allocation beyond the life of the handles: the Lanczos workspace of the escape (up to 24 GB for
 * n = 20000; allocating it costs 0.05-0.5 s) is parked by msdp_destroy for the next handle of the process.  This call
 * frees it (a long-lived host such as MATLAB calls it when it unloads the binding). */
int msdp_release_cache(void);
/* The uncached device memory behind the grid synchronisations and row exchanges comes from per-process arenas with a coalescing
 * sub-allocator (msdp_mem.hip): bytes the arenas hold, bytes handed out to live handles, number of arenas.  The pool grows to
 * the high-water mark of what was live together; arenas return to the driver only while no uncached block of the process is
 * live (beyond MSDP_UC_POOL_CAP bytes -- default 1 GiB -- when the last one is freed, all of them in msdp_release_cache). */
int msdp_debug_pool_stats(int64_t* pool_bytes, int64_t* live_bytes, int64_t* arenas);
/* Free and total bytes of the current device (hipMemGetInfo), for hosts and tests that size a problem or watch for leaks
 * without a second HIP runtime in the process. */
int msdp_debug_mem_info(int64_t* free_bytes, int64_t* total_bytes);

/* AL state that changes between trustregions() calls: y and sigma
 * (ManiSDP_unitdiag.m:64,108-112).  No-op error for onlyunitdiag handles. */
int msdp_set_multipliers(msdp_handle h, const double* y, double sigma);

/* ------------------------------------------------------- resident point I/O */

/* Upload the current point in the reference layout (see header comment). */
int msdp_set_point(msdp_handle h, int32_t p, const double* Y);
int msdp_get_point(msdp_handle h, double* Y);
/* Row-sharded handles (msdp_comm_init): every row of the resident point on EVERY rank (one all-gather, then the
 * download).  The host loops of the row-sharded affine kinds run replicated on all ranks and take their rank / escape
 * decisions on identical data.  Without a communicator: the same as msdp_get_point. */
int msdp_get_point_all(msdp_handle h, double* Y);

/* The rank decision and the re-shaping of the factor between two trustregions() calls without the factor leaving the
 * device (ManiSDP_onlyunitdiag.m:52-54 svd(Y), :70-73 Y = V(:,1:r)'.*e(1:r), :78-83 Y = [Y; alpha*vS'],
 * Y = Y./sqrt(sum(Y.^2)); the same lines of ManiSDP_unitdiag.m:72-74,93-106).
 * msdp_factor_gram: G (p x p, symmetric) = Gram matrix of the p columns of the factor; its eigen-decomposition
 *   G = Q diag(e.^2) Q' gives the singular values e of Y and V(:,k)*e_k = Y*Q(:,k).
 * msdp_factor_rotate: Y <- Y*Q with Q p x r ROW-major (the rank cut; new width r).
 * msdp_factor_append: Y <- [Y, alpha*V], V n x k column-major (as msdp_escape_eigs returns it), then every row scaled to
 *   unit norm if normalize != 0 (oblique kinds).  MSDP_EUNSUPPORTED when p + k exceeds the width the handle has
 *   allocated: re-enter through msdp_set_point then. */
int msdp_factor_gram(msdp_handle h, double* G);
int msdp_factor_rotate(msdp_handle h, int32_t r, const double* Q);
int msdp_factor_append(msdp_handle h, int32_t k, const double* V, double alpha, int32_t normalize);

/* The same steps for the block kinds (msdp_create_onlyunitblockdiag_csc / msdp_create_posegraph_csc; the three calls above
 * stay refused for them), and the rounding to rotations / poses.  Any other handle: MSDP_EUNSUPPORTED, the message names the
 * call.  No resident point: MSDP_ESTATE.
 * msdp_blockfactor_gram: G (p x p) = Y'Y of the resident factor, free rows included.
 * msdp_blockfactor_rotate: Y <- polar_blocks(Y*Q), Q p x r ROW-major, d <= r <= p (else MSDP_EINVAL).
 * msdp_blockfactor_append: Y <- polar_blocks([Y, alpha*V]), V N x k column-major; MSDP_EUNSUPPORTED when p + k exceeds the
 *   allocated capacity (re-enter through msdp_set_point).
 *   polar_blocks: the d orthonormal rows of every block are replaced by their polar factor (A A')^(-1/2) A, applied twice so
 *   that ill-conditioned blocks end orthonormal to rounding; the free row of a pose-graph block is the plain product /
 *   concatenation.  A block whose Gram matrix A A' has lambda_min <= 1e-12 lambda_max is degenerate: *ndeg counts them, and
 *   with *ndeg > 0 the call returns 0 WITHOUT changing the resident point, its width or the handle's state (take that step
 *   on the host).
 * msdp_blockfactor_round: W p x d ROW-major (the caller passes the top-d eigenvectors of Y'Y).  Z_i = Y_i*W (rotation rows),
 *   t_i = tau_i*W (pose-graph handles).  Where more than half of det Z_i are negative the last column of every Z_i and the
 *   last entry of every t_i change sign (*flipped = 1).  R_i = the nearest rotation to Z_i.  R: (n, d, d) row-major; t:
 *   (n, d), NULL for a unit-block-diagonal handle and non-NULL for a pose-graph handle (else MSDP_EINVAL).  The degenerate
 *   rule applies to Z_i Z_i': with *ndeg > 0 R and t are not to be used. */
int msdp_blockfactor_gram(msdp_handle h, double* G);
int msdp_blockfactor_rotate(msdp_handle h, int32_t r, const double* Q, int32_t* ndeg);
int msdp_blockfactor_append(msdp_handle h, int32_t k, const double* V, double alpha, int32_t* ndeg);
int msdp_blockfactor_round(msdp_handle h, const double* W, double* R, double* t, int32_t* flipped, int32_t* ndeg);
/* The same steps for the Hermitian kind (msdp_create_onlyunitdiag_csc_hermitian; msdp_factor_gram / _rotate / _append stay
 * refused for it), p counting COMPLEX columns (msdp_get_p / 2).  Any other handle: MSDP_EUNSUPPORTED, the message names the
 * call.  No resident point: MSDP_ESTATE.  All three run the kernels of the real calls on the real view of the factor.
 * msdp_hfactor_gram: G = Y^H Y, p x p complex row-major, (re, im) pairs (2 p p doubles).
 * msdp_hfactor_rotate: Y <- Y*Q with Q p x r complex ROW-major, (re, im) pairs; 1 <= r <= p, else MSDP_EINVAL.
 * msdp_hfactor_append: Y <- [Y, alpha*V] with every row scaled to unit norm; V as msdp_escape_eigs returns it on such a
 *   handle: k columns of n (re, im) pairs.  MSDP_EUNSUPPORTED, with nothing modified, when p + k exceeds the complex width
 *   the handle has allocated: re-enter through msdp_set_point then.
 * After _rotate / _append the cost state is invalid, as after msdp_set_point. */
int msdp_hfactor_gram(msdp_handle h, double* G);
int msdp_hfactor_rotate(msdp_handle h, int32_t r, const double* Q);
int msdp_hfactor_append(msdp_handle h, int32_t k, const double* V, double alpha);
int msdp_get_p(msdp_handle h, int32_t* p);
/* MSDP_KIND_* of the handle: tells a binding which factor layout the handle expects at the boundary
 * (p x n for ONLYUNITDIAG / UNITDIAG, n x p for UNITTRACE / GENERIC) without guessing from array shapes. */
int msdp_get_kind(msdp_handle h, int32_t* kind);

/* ------------------------------------------------------------------ hot path */

/* Keep / bring back a device-side copy of the resident point (same width): restart a solve from the same
 * start point without another host upload (measurement; line searches that want to back-track on the device). */
int msdp_point_snapshot(msdp_handle h);
int msdp_point_restore(msdp_handle h);

/* [Y, ~, info] = trustregions(problem, Y, opts) on the resident point: the whole
 * RTR/tCG loop (trustregions.m:441-767, tCG.m:160-289) runs on the device. */
int msdp_rtr(msdp_handle h, const msdp_rtr_opts* opts, msdp_rtr_stats* stats);

/* Convenience: set_point + rtr + get_point. */
int msdp_rtr_host(msdp_handle h, int32_t p, double* Y_inout,
                  const msdp_rtr_opts* opts, msdp_rtr_stats* stats);

/* Fine-grained operators at the resident point (parity tests; reference layout).
 *   cost   : problem.cost(Y)                       -> *f
 *   rgrad  : problem.grad(Y) (after cost)          -> G
 *   hessvec: problem.hess(Y, U)                    -> H
 *   proj   : problem.M.proj(Y, U)                  -> V
 *   retr   : problem.M.retr(Y, U)                  -> Z (does not move the point) */
int msdp_cost(msdp_handle h, double* f);
int msdp_rgrad(msdp_handle h, double* G);
int msdp_hessvec(msdp_handle h, const double* U, double* H);
int msdp_proj(msdp_handle h, const double* U, double* V);
int msdp_retr(msdp_handle h, const double* U, double* Z);

/* Per-point vector the AL step needs after RTR without recomputing it on the host:
 * onlyunitdiag: z = sum((Y*C).*Y) (ManiSDP_onlyunitdiag.m:46-47), length n. */
int msdp_get_z(msdp_handle h, double* z);
/* Row-sharded handles: z of all rows on every rank (one all-gather); otherwise the same as msdp_get_z. */
int msdp_get_z_all(msdp_handle h, double* z);

/* co(Y) of the line search (ManiSDP_onlyunitdiag.m:99-101, ManiSDP_unitdiag.m:131-136,
 * ManiSDP_unittrace.m:135-140) evaluated at the retraction of Y + alpha*U, U given in
 * the reference layout; used by line_search(). alpha = 0 evaluates co(Y). */
int msdp_linesearch_cost(msdp_handle h, const double* U, double alpha, double* val);
/* Adopt the trial point of the last msdp_linesearch_cost call (nY of line_search)
 * as the resident point. */
int msdp_linesearch_accept(msdp_handle h);

/* ---------------------------------------------------------------- rounding */

/* Goemans-Williamson hyperplane rounding of the resident point of a single-rank MSDP_KIND_ONLYUNITDIAG handle to +1/-1
 * vectors, with optional 1-opt local search, on the device (not in the reference, which returns the bound and the factor).
 *   x_t = sign(Y r_t) for the `trials` rows r_t of R (trials x p row-major, p the current width; sign(0) = +1),
 *   val_t = x_t' C x_t (diagonal included), from the rows of C the handle holds.  A sparse-plus-low-rank handle
 *     (msdp_create_onlyunitdiag_csc_lowrank): val_t = x' Cs x + sum_k s_k (V_k' x)^2, the q sums V_k' x formed in the same
 *     ordered pass over the rows (per-chunk partials added in index order, then squared); in the 1-opt sweeps
 *     x_i s_i = (sparse sum over j != i) + sum_k s_k V_ik (x_i t_k - V_ik) with t_k = V_k' x held per trial, formed by
 *     one ordered pass over the rows at the start of every sweep launch (never carried between launches) and updated
 *     by t_k -= 2 V_ik x_i(old) at a flip.
 *   sweeps > 0: up to `sweeps` Gauss-Seidel sweeps of 1-opt per trial -- rows i = 0 .. n-1 in order, s_i = sum_{j != i}
 *     C_ij x_j, x_i flipped where x_i s_i > 0 (strict: a tie stays).  The 64 trials of a word sweep together; a word stops
 *     after a sweep of its own without a flip, the call when every word has stopped.  All values are then recomputed from
 *     the final vectors (never updated incrementally); the sums are deterministic (no floating-point atomics).
 *     With the option "round_order" = 1 (msdp_set_option; sparse C only) "rows i = 0 .. n-1 in order" reads "rows in (colour,
 *     index) order" of msdp_round_coloring, everything else as written here.
 * trials: a multiple of 64, at most MSDP_ROUND_MAX_TRIALS.  Sign bits are packed 64 trials per word: bit t of
 * masks[w * n + i] is set when x_i = -1 in trial 64 w + t.
 *   values0 (trials, may be NULL): the values right after the rounding;   values (trials): the final ones (== values0 when
 *   sweeps == 0);   info (2 x trials/64, may be NULL): per word the sweeps run, then per word the flips of its last sweep;
 *   masks (trials/64 x n, may be NULL): the final vectors;   *best: the trial of the smallest value (the lowest index wins a
 *   tie);   x (n entries +1 / -1, may be NULL): the vector of trial *best.
 * The point, the cost state and every other state of the handle stay as they are; the device memory of the call is
 * released before it returns.  MSDP_EINVAL: trials <= 0, not a multiple of 64 or above the cap, sweeps < 0, R / values / best
 * NULL.  MSDP_EUNSUPPORTED: any other kind, a handle that has joined a communicator.  MSDP_ESTATE: no resident point. */
#define MSDP_ROUND_MAX_TRIALS 4096
int msdp_round_hyperplane(msdp_handle h, int32_t trials, const double* R, int32_t sweeps, double* values0, double* values,
                          int32_t* info, uint64_t* masks, int32_t* best, int8_t* x);

/* Rounding of the resident point of a Hermitian handle (msdp_create_onlyunitdiag_csc_hermitian) to phases, with a
 * coordinate-minimisation local search, on the device (not in the reference).  The target is the unit circle (M = 0) or the
 * M-th roots of unity (2 <= M <= MSDP_ROUND_PHASES_MAX_M): phase synchronisation, unimodular programmes, M-PSK detection.
 *   Table: c_k = (cos, sin)(2 pi k / M), k = 0 .. M-1, built on the host in double: the angle is ((2 * pi) * k) / M with
 *     pi = 3.141592653589793, evaluated left to right, and goes to the C library's cos and sin; where 4 k is a multiple of M
 *     the entry is written as exactly (1, 0), (0, 1), (-1, 0) or (0, -1) (4 k / M = 0, 1, 2, 3), so M = 2 and M = 4 are exact.
 *   Rounding: w = sum_a Y_ia R_ta for the `trials` rows of R (trials x p complex row-major, (re, im) pairs, p = msdp_get_p / 2;
 *     complex products, no conjugate, ascending a).  M = 0: z_i = w / sqrt(w.re^2 + w.im^2), z_i = 1 where that is 0.
 *     M >= 2: z_i = c_k with the k of the largest Re(conj(c_k) w) = c.re w.re + c.im w.im, the lowest k at a tie.
 *   val_t = sum_i Re(conj(z_i) sum_j C_ij z_j), diagonal included; deterministic sums (fixed row chunks added in index
 *     order, no floating-point atomics).
 *   sweeps > 0: up to `sweeps` Gauss-Seidel sweeps per trial -- rows i = 0 .. n-1 in order, s_i = sum_{j != i} C_ij z_j in
 *     stored order.  M = 0: z_i <- -s_i / |s_i|, left as it is where |s_i|^2 == 0; exactly `sweeps` sweeps run.  M >= 2: with
 *     cur = z_i.re s.re + z_i.im s.im and cand_k the same expression for c_k, k* the minimising k (the lowest at a tie),
 *     z_i <- c_k* only where cand_k* < cur strictly.  A phase is a bit copy of its table entry, so a converged phase never
 *     counts as changed.  The 64 trials of a word sweep together; a word stops after a sweep of its own without a change, the
 *     call when every word has stopped.  All values are then recomputed from the final phases.
 *     With the option "round_order" = 1 (msdp_set_option) "rows i = 0 .. n-1 in order" reads "rows in (colour, index) order"
 *     of msdp_round_coloring, everything else as written here.
 * trials: a multiple of 64, at most MSDP_ROUND_PHASES_MAX_TRIALS.  The call holds trials * n complex numbers on the device
 * (MSDP_ENOMEM when they cannot be had) and releases every allocation before it returns.
 *   values0 (trials, may be NULL): the values right after the rounding;   values (trials): the final ones;   info
 *   (2 x trials/64, may be NULL): per word the sweeps run, then per word the changes of its last sweep (0 for M = 0);   phases
 *   (may be NULL): all final phases in the device layout [trials/64][n][64] of (re, im) pairs;   *best: the trial of the
 *   smallest value (the lowest index wins a tie);   z (n (re, im) pairs, may be NULL): the phases of trial *best;   k (n, may
 *   be NULL, must be NULL with M = 0): their table indices.
 * The point, the cost state and the options of the handle stay as they are.  MSDP_EUNSUPPORTED: any other kind of handle.
 * MSDP_EINVAL: M outside {0, 2 .. MSDP_ROUND_PHASES_MAX_M}, trials <= 0, not a multiple of 64 or above the cap, sweeps < 0,
 * R / values / best NULL, k not NULL with M = 0.  MSDP_ESTATE: no resident point. */
#define MSDP_ROUND_PHASES_MAX_TRIALS 1024
#define MSDP_ROUND_PHASES_MAX_M 64
int msdp_round_phases(msdp_handle h, int32_t M, int32_t trials, const double* R, int32_t sweeps, double* values0,
                      double* values, int32_t* info, double* phases, int32_t* best, double* z, int32_t* k);

/* The colouring behind the colour-ordered local search of the two roundings above (option "round_order" = 1 of
 * msdp_set_option), computed on the host on the first call and kept with the handle: greedy first-fit in index order,
 * color(i) = the smallest colour that no already coloured neighbour j != i of row i holds; the neighbours are the stored entries
 * of row i of C, diagonal entries left out; a row without neighbours gets colour 0.  No stored off-diagonal entry joins two
 * rows of one colour, so all rows of a colour can be updated at once, and the colours taken one after another are the serial
 * sweep over the rows sorted by (colour, index).  With "round_order" = 1 the sweeps of msdp_round_hyperplane and
 * msdp_round_phases therefore read "rows in (colour, index) order" where their descriptions say "rows i = 0 .. n-1 in order":
 * one launch per colour over the whole device; the row sums (stored order, diagonal skipped), the decision rules, the stopping
 * rule, info and every output keep their meaning, the local optimum a trial reaches is that of the other order.
 *   *ncolors: the number of colours (max color + 1);   color (n, may be NULL): the colour of every row.
 * Needs no resident point.  MSDP_EUNSUPPORTED, the kind named: every handle that refuses "round_order" = 1.  MSDP_EINVAL:
 * ncolors NULL; a pattern that is not structurally symmetric -- a stored (i, j) without a stored (j, i); the message names the
 * first such entry in row order. */
int msdp_round_coloring(msdp_handle h, int32_t* ncolors, int32_t* color);

/* ----------------------------------------------------------------- escape */

/* Few-eigenvector saddle escape (replaces eig(S) of ManiSDP_onlyunitdiag.m:50,
 * ManiSDP_unitdiag.m:68, ManiSDP_unittrace.m:68 for large n): the k smallest
 * eigenpairs and the largest eigenvalue of the dual slack S at the resident point,
 * by block Lanczos / LOBPCG on the device re-using the S*U kernel.
 * lam_min[k] ascending, V is n x k column-major, *lam_max the top eigenvalue.
 * The Lanczos path returns the negative eigenvalues it finds (at most k) and at most
 * one non-negative one, which is an upper estimate that only certifies its sign.  Further
 * copies of a multiple eigenvalue come from the deflated re-runs alone, and pairs taken
 * from one Krylov space may come before them: the k values need not be the k smallest
 * counted with multiplicity.  The sequential deflation ends when the
 * complement of what was found is non-negative or empty (n <= k, or every eigenvalue
 * negative and none left).  Values that do not exist are +inf with a zero vector, and
 * msdp_escape_info reports how many are real: never more than n.
 * Hermitian C (msdp_create_onlyunitdiag_csc_hermitian): V is k complex vectors in the real view, column-major with stride 2n
 * ((re, im) of row i of vector c at V[c*2n + 2i], V[c*2n + 2i + 1]), orthonormal in the complex inner product, every eigenvalue
 * of S reported as often as S has it.  By default the Lanczos path runs on the real view of length 2n.  With option
 * "escape_method" = 2, on a single rank and n >= 256, the block eigen-solver runs on a complex panel of 32 or 64 columns (the
 * complex columns of the factor in its start block, a complex gather per filter step, the Rayleigh-Ritz problem of order 32 /
 * 64 in complex algebra on the host); lambda_max still comes from a short Lanczos run on the real view.  At most 56 pairs per
 * call on that route (k + 8 <= 64, else MSDP_EINVAL). */
int msdp_escape_eigs(msdp_handle h, int32_t k, double tol, int32_t maxit,
                     double* lam_min, double* V, double* lam_max, int32_t* iters);

/* Same escape for an explicit dense symmetric S (n x n, column-major = row-major) formed by the AL loop of the
 * affine kinds (ManiSDP_unitdiag.m:65-68, ManiSDP_unittrace.m:65-68: S = eS - diag(z) / eS - z*I, eig(S)). */
int msdp_escape_eigs_matrix(msdp_handle h, const double* S, int32_t k, double tol, int32_t maxit,
                            double* lam_min, double* V, double* lam_max, int32_t* iters);

/* Which eigen-solver the LAST escape call on this handle ran: 1 = block Chebyshev-filtered subspace iteration
 * (msdp_blockeig.hip: sparse C; a 64- or 128-wide panel, reduction-free filter steps on the S*U kernel, Rayleigh-Ritz every
 * few hundred steps; Hermitian C with "escape_method" = 2: a complex panel of 32 or 64 columns; the block kinds with
 * "escape_method" = 2: the filter step on block storage), 0 = deflated single-vector Lanczos runs (msdp_escape.hip: dense S,
 * pre-sharded dense C, small n, Hermitian C and the block kinds unless asked). */
int msdp_escape_method(msdp_handle h, int32_t* method);

/* Collective calls this handle has issued on its communicator so far (row exchange, all-reduce, all-gather; operations grouped
 * into one RCCL launch count once).  A row-sharded tCG trip of onlyunitdiag with sparse C costs two (msdp_trip1.hip: the rows
 * of the projected residual with every rank's partial sums riding along, then the all-reduce of <mdelta, H mdelta> -- tCG.m:166),
 * three with option trip1 = 0; tests/test_gpu_local_ranks.py asserts it. */
int msdp_debug_collective_calls(msdp_handle h, int64_t* calls);
/* (new, measurement only) Device time of the LAST msdp_rtr call on this handle, by HIP events on the handle's stream around what the
 * call enqueued behind the cost / gradient evaluation of its start point (trustregions.m:441-767): on the fused path exactly the ONE launch
 * that runs every tCG trip, retraction, cost evaluation and decision of the call -- bench.py's dominant kernel, whose roofline figure is
 * algorithmic bytes of the launch / this time.  *ms < 0: no call yet. */
int msdp_debug_last_rtr_device_ms(msdp_handle h, double* ms);
/* Measurement only: average stream time (us) of one collective call: which = 0 row exchange, 1 all-reduce of one partial-sum
 * array, 2 row exchange with the sums riding along, 3 all-reduce of three arrays, 4 rows and sums as two separate all-gathers. */
int msdp_debug_time_collective(msdp_handle h, int32_t which, int32_t reps, double* avg_us);
/* Measurement only: the phases of a persistent tCG trip (tCG.m:160-289 inside k_tcg_persist_obl).  Runs `reps` trips with the
 * exits disabled on the traced instance of the kernel (17 <= p <= 32, rows of <= 5 entries: the G81 shape) and returns thread 0's
 * s_memtime stamps of every workgroup at 7 phase boundaries -- 0 top of the trip, 1 gathers + row arithmetic done, 2 first grid
 * reduction returned, 3 trial step formed and residual rows stored, 4 those stores performed, 5 second grid reduction returned,
 * 6 new direction formed -- for the trips dims[2] .. dims[2] + dims[1] - 1: out[(g * dims[1] + t) * 8 + phase], g < dims[0].
 * avg_ms = the average trip time of the same launch (HIP events).  tools/persist_timeline.py turns it into profiles/r4_persist_timeline.md.
 * reps <= 0 (round 6): the FUSED launch instead -- one trustregions() call (trustregions.m:441-767) with the options of the handle's last
 * msdp_rtr, stamps of the first dims[1] TR iterations (dims[2] = 0): 0 iteration starts, 1 first trip's products formed, 2 tCG ended
 * (bits 56..63: its trips), 3 proposal rows stored and performed, 4 barrier returned, 5 cost / gradient rows of the proposal formed,
 * 6 the iteration's reduction returned, 7 decision taken; avg_ms = the call's time.  tools/fused_timeline.py. */
int msdp_debug_persist_trace(msdp_handle h, int32_t reps, uint64_t* out, int64_t cap, int32_t* dims, double* avg_ms);

/* Outcome of the LAST msdp_escape_eigs / _matrix / _dual call on this handle.  The reference's eig(S) is exact;
 * a Lanczos run that reaches `maxit` without passing a stop test only yields an UPPER bound of lambda_min, so
 * dinf = max(0,-lambda_min)/(1+lambda_max) (ManiSDP_onlyunitdiag.m:51) would be under-estimated: the AL loop
 * must not declare optimality on it.
 *   *nvalid    : how many of the k requested pairs are real (the others are returned as lam = +inf, V = 0);
 *   *converged : 1 if every Lanczos run passed a stop test, 0 if one ended at maxit;
 *   *residual  : largest relative residual |S x - theta x| / max(|theta|, |lam_max|) among the unconverged runs. */
int msdp_escape_info(msdp_handle h, int32_t* nvalid, int32_t* converged, double* residual);
/* Lower ESTIMATE of lambda_min(S) from the LAST escape call; -inf unless that call was cold-started and undeflated
 * (options escape_deflate = 0, escape_warm = 0) and converged.  Block path: theta_0 minus its error estimate.  Lanczos path:
 * with Z = [found vectors] and S = [A E'; E B] in the basis [Z, complement],
 *   min(lambda_min(A), theta - res) - |E|_F
 * where A = Z'SZ is known exactly, |E|_F = |(I - ZZ')SZ|_F is measured and (theta, res) is the last converged,
 * non-negative Ritz pair of the complement.  NOT a certificate: a converged Ritz pair proves that SOME eigenvalue lies within
 * res of theta, not that none lies below; a warm-started or deflated run that missed the bottom of the
 * spectrum would report a bound that is too high, which is why such runs report -inf and the host loops always finish with
 * the independent, cold-started check. */
int msdp_escape_lower_bound(msdp_handle h, double* lam_lower);

/* ------------------------------------------------------------- multi-GPU */

/* Row sharding: call on every rank right after create, before any
 * point is set.  unique_id is the 128-byte RCCL id produced on rank 0 by
 * msdp_comm_unique_id and broadcast by the host launcher. */
int msdp_comm_unique_id(void* id128);
int msdp_comm_init(msdp_handle h, int32_t nranks, int32_t rank, const void* id128);
/* Test / diagnostic stand-in for the communicator: member `rank` of the in-process group `group_id` of `nranks` handles
 * (one process, ONE GPU, one host thread per handle).  Same row partition and the same code paths as msdp_comm_init --
 * row offsets, replicated operator state, lock-step tCG, order and number of collective calls -- with the three
 * collectives carried out by a host barrier and device copies / a summation kernel between the members' buffers, so a
 * single GPU executes the N-rank paths.  A member that never makes the matching call breaks the group after 120 s
 * (MSDP_ECOMM; environment variable MSDP_LOCAL_BARRIER_TIMEOUT = seconds, for legitimately slow members on a loaded GPU)
 * instead of hanging the process; a member that detects an error itself breaks the group at once. */
int msdp_comm_init_local(msdp_handle h, int32_t nranks, int32_t rank, int32_t group_id);
/* The same group with its members in DIFFERENT PROCESSES -- several ranks on one GPU, or one rank per GPU of a node with peer
 * access (replaces nothing in the reference, whose MATLAB path is one process).  `name` is a POSIX shared-memory
 * name ("/..."), the same on every member and fresh for every group.  Rank 0 allocates one fine-grained device block (the slot
 * regions of the cross-rank persistent tCG, one staging slab per rank for the collectives) and EVERY member an exchange buffer
 * for its own rows plus a slot per foreign row it references, on its own device; the blocks are exported with hipIpcGetMemHandle
 * and mapped by the others with hipIpcOpenMemHandle (peer access between devices).  With sparse C the whole
 * tCG of a trust-region iteration then runs as ONE grid-synchronised computation across the members' launches -- no collective
 * per trip; a member whose launch never arrives turns the others' bounded spins into MSDP_ECOMM.  Collectives outside the tCG
 * (cost / gradient at the proposal, AL bookkeeping) go through the staging slabs behind a barrier on the shared segment. */
int msdp_comm_init_ipc(msdp_handle h, int32_t nranks, int32_t rank, const char* name);
/* Local row range [row0, row1) of this rank. */
int msdp_local_rows(msdp_handle h, int64_t* row0, int64_t* row1);

/* ------------------------------------------- AL bookkeeping */

/* Affine handles, at the resident point (x = vec(YY')): obj = c'x and Ax = A x (m doubles;
 * the caller forms Axb = Ax - b) -- ManiSDP_unitdiag.m:59-62, ManiSDP_unittrace.m:59-62,
 * ManiSDP.m:58-63 without the n x n X on the host. */
int msdp_al_primal(msdp_handle h, double* obj, double* Ax);
/* Dual slack for the multipliers y: eS = reshape(c - At*y, n, n); unit diagonal:
 * z = sum(X.*eS) (n values), S = eS - diag(z) (ManiSDP_unitdiag.m:65-67); unit trace:
 * z = sum(eS.*X,'all') (1 value), S = eS - z*I (ManiSDP_unittrace.m:65-67); generic: S = eS
 * (ManiSDP.m:64; z untouched, may be NULL).  S stays on the device for msdp_escape_eigs_dual. */
int msdp_al_dual(msdp_handle h, const double* y, double* z);
/* lambda_min, lambda_max and <= k bottom eigenvectors of the S of the last msdp_al_dual call
 * (eig(S) of ManiSDP_unitdiag.m:68 / ManiSDP_unittrace.m:68 / ManiSDP.m:65). */
int msdp_escape_eigs_dual(msdp_handle h, int32_t k, double tol, int32_t maxit,
                          double* lam_min, double* V, double* lam_max, int32_t* iters);
/* The dense S (n x n, symmetric: column-major = row-major) of the last msdp_al_dual call: the reference's
 * data.S (ManiSDP_unitdiag.m:116, ManiSDP_unittrace.m:121) and the input of a host eig(S) for small n. */
int msdp_get_dual_slack(msdp_handle h, double* S);
/* The nb x nb diagonal block of the same matrix that starts at row / column row0 (column-major == row-major: symmetric).
 * ManiSDP_multiblock.m:78-88 takes eig(S_i) block by block: with a hundred blocks the whole N x N matrix is 100 times what
 * the host reads (N = 21 100 for example_bqp_sparse.m with t = 100: 3.5 GB per outer iteration against 35 MB). */
int msdp_get_dual_slack_block(msdp_handle h, int64_t row0, int64_t nb, double* S);
/* eig of `nb` diagonal blocks of the same matrix on the device, in one launch: what ManiSDP_multiblock.m:78-88 computes block by
 * block with eig(S{i}) -- all eigenvalues (dinf needs the extremes, the escape the count of negative ones, :129-133) and the
 * eigenvectors of the `k` smallest (:137-147 take at most options.delta of them).  Block b = rows / columns row0[b] .. row0[b] +
 * nblk[b] - 1 (a block of the handle when it stores per block); orders up to 256 (MSDP_EUNSUPPORTED beyond: the host loop over
 * msdp_get_dual_slack_block remains).  w: the eigenvalues, block after block, ascending inside a block (sum nblk values);
 * V: (sum nblk) x k row-major, row = position in the concatenation of the blocks, column c = eigenvector of the block's c-th
 * smallest eigenvalue (zero columns beyond a block's order).  One workgroup per block (msdp_blockjacobi.hip); method 0 = Householder
 * tridiagonalisation + bisection + inverse iteration when k <= 8 (the way of LAPACK's dsyevx), else 1 = cyclic Jacobi; 2 = the
 * tridiagonal method, MSDP_EUNSUPPORTED when k > 8.  Limits: 0 <= k <= 64 and method in {0, 1, 2} (MSDP_EINVAL otherwise, as for
 * nb < 1 and a block outside the matrix); k = 0 returns the eigenvalues only and V may be NULL; a block with fewer than k rows has
 * zeros in its columns beyond its order.  Vectors of eigenvalues closer than rounding resolves are an orthonormal basis of their
 * common eigenspace.  MSDP_ESTATE before msdp_al_dual (msdp_dual_outer_step on the dual multiblock kind) has built the blocks, and
 * when a Jacobi iteration has not converged in 40 sweeps.  Every check is made on the host before anything is launched, and the
 * handle stays usable after a refusal. */
int msdp_block_eigs(msdp_handle h, int32_t nb, const int64_t* row0, const int64_t* nblk, int32_t k, int32_t method, double* w, double* V);
/* The same call for blocks of order up to 1024 (MSDP_BLOCK_EIGS_LARGE_MAXN): ManiSDP_multiblock.m:78-88 again, the tridiagonal method
 * only (Householder tridiagonalisation, bisection, inverse iteration, back-transformation), a GROUP of workgroups per block of order
 * above 256 (msdp_blocktridiag.hip: the group shares the rows of the block and meets at two group barriers per Householder step;
 * blocks of order <= 256 are legal and take one workgroup).  Same outputs and layout as msdp_block_eigs.  0 <= k <= 8;
 * MSDP_EUNSUPPORTED for k > 8 and for an order above 1024 (the message names the limit and the block), MSDP_EINVAL for nb < 1, an
 * order < 1, a block outside the matrix and a range that is not one block of a handle that stores per block, MSDP_ESTATE before
 * msdp_al_dual / msdp_dual_outer_step; every check is made before anything is launched and the handle stays usable after a refusal.
 * All workgroups of a launch are resident together (the grid never exceeds what the occupancy query allows; a call with more blocks
 * runs as consecutive launches); every barrier spins a bounded number of times and a barrier that runs out makes all workgroups leave:
 * MSDP_ECOMM.  Results are bit-reproducible, and a block's results do not depend on the other blocks of the call nor on the number of
 * workgroups it was given (option "blk_groups": that number for orders above 256, 0 = by order; tests). */
#define MSDP_BLOCK_EIGS_LARGE_MAXN 1024
int msdp_block_eigs_large(msdp_handle h, int32_t nb, const int64_t* row0, const int64_t* nblk, int32_t k, double* w, double* V);
/* Diagnostic: launches and workgroups of the last msdp_block_eigs_large call on this handle (either pointer may be NULL). */
int msdp_block_eigs_large_info(msdp_handle h, int32_t* launches, int32_t* workgroups);
/* Rank cut and escape widening of ALL blocks of a multiblock factor on the device (ManiSDP_multiblock.m:109-147,
 * ManiDSDP_multiblock.m:146-181), the resident point rewritten without leaving the device.  nb / row0 / nblk: all blocks of the handle,
 * in order (MSDP_EINVAL otherwise); p_in[b]: block b's current width (its columns beyond are zero); w, V: eig(S_i) in the layout
 * msdp_block_eigs returns (sum nblk values ascending per block; (sum nblk) x k row-major).  Block i of order n_i < min_facsize is
 * left as it is (:110).  Otherwise, when p_i > 1: G = Y_i'Y_i summed over the rows in order, its eigen-decomposition (cyclic Jacobi
 * in LDS), e = sqrt(max(lambda, 0)) descending, r = #{e >= theta e_1} (strict != 0: #{e > theta e_1}, ManiDSDP_multiblock.m:146-155),
 * at least 1; r < p_i: Y_i <- Y_i Q(:, 1:r), p_i = r (:112-127).  nne = max(min(#{w_i < 0}, delta), 1 for the first nob blocks of the
 * handle, else 0), and 0 when p_i + nne > n_i (:129-136).  mode 0 (line_search = 0, :142-146): Y_i <- [Y_i, alpha V_i(:, 1:nne)], the
 * rows of the first nob blocks scaled to unit norm; mode 1 (:137-141): Y_i <- [Y_i, 0] and U_i = [0, V_i(:, 1:nne)] written to the
 * host array U in the boundary layout of the new point (N x max p_out, row-major; U may be NULL in mode 0).  Outputs per block:
 * p_out (new width), r_out (the rank found; p_in where no decomposition was made), nne_out.  Columns beyond a block's new width are
 * exact zeros; the handle's width becomes max p_out (it may shrink).  One workgroup per block in each of two launches
 * (msdp_blockreshape.hip: the decisions, then the rows -- the new row stride is known only in between); a block's result does not
 * depend on the other blocks and is bit-reproducible.  Widths: p_in <= 64 on every block the rule touches; the new width r + nne of a
 * block may exceed 64 (at most 64 + delta: an uncut block that gains escape columns) and is limited by the handle's allocated width
 * alone.  MSDP_EINVAL: nb < 1, k < 0 or > 64, delta < 0 or > k, mode not 0 / 1, a null array,
 * a width outside 1 .. p, a block list that is not the handle's; MSDP_ESTATE: no resident point; MSDP_EUNSUPPORTED: not a
 * multiblock kind, a row-sharded handle, a block of width above 64 (MSDP_BLOCK_RESHAPE_MAXP) that the rule touches, a new width above
 * the allocated one (msdp_set_point re-allocates); MSDP_ESTATE also when a Jacobi iteration has not converged in 40 sweeps.  Every refusal leaves the point and the handle as they were. */
#define MSDP_BLOCK_RESHAPE_MAXP 64
int msdp_block_reshape(msdp_handle h, int32_t nb, const int64_t* row0, const int64_t* nblk, const int32_t* p_in,
                       const double* w, const double* V, int32_t k, double theta, int32_t strict, int32_t delta,
                       double alpha, int32_t min_facsize, int32_t mode,
                       int32_t* p_out, int32_t* r_out, int32_t* nne_out, double* U);

/* Run-time switches of one handle (production = the defaults; the tests and the profiling scripts use them):
 *   "persist"      1/0  persistent single-launch tCG / Lanczos kernels where they fit (default 1; env MSDP_NO_PERSIST=1)
 *   "fused_rtr"    1/0  whole trustregions() loop in one launch for p <= 32          (default 1; env MSDP_NO_FUSED_RTR=1)
 *   "graph"        1/0  chunked tCG trips replayed as hipGraphs                      (default 1; env MSDP_NO_GRAPH=1)
 *   "affine_route" 0 = choose by bytes moved, 1 = SDDMM, 2 = Gram                    (default 0; env MSDP_AFFINE_ROUTE)
 *   "escape_deflate" 1/0 escape: deflate span(Y) at near-stationary points (default 1).  Fast, but only as accurate as
 *                       S*Y is small; a caller about to DECLARE optimality re-checks lambda_min with 0 (see solvers.py)
 *   "escape_warm"  1/0  escape: start from what the previous call found (default 1; 0 = hashed random start vector)
 *   "persist_refresh" k  persistent tCG kernel: every k-th trip exchanges the rows of the new direction itself (one extra
 *                       barrier) so that the product C*mdelta, otherwise assembled by linearity, starts afresh (default 32;
 *                       0 = never: |Heta - Hess(eta)|/|Heta| then grows to 1e-8 over 100 trips on G81)
 *   "persist_early" k  persistent tCG kernel (rows of <= 5 entries, p <= 32): k >= 1 = the neighbours' rows of tangent(r') are
 *                       gathered WHILE the second grid reduction of the trip is in flight -- the exchange buffer's halves hold a NaN
 *                       sentinel until a row is stored, so the rows are their own flags (k - 1 = units of 64 cycles a wave sleeps
 *                       between posting the reduction and its first gather); 0 = at the top of the next trip, behind that
 *                       reduction (the round-4 trip).  Same arithmetic, same decisions; measured slower (default 0)
 *   "persist_pipe" 1/0  persistent tCG kernel (rows of <= 8 entries, or CSR rows with "persist_ep"; p <= 32): ONE grid reduction per trip instead of two -- the
 *                       values of tCG.m:227-241 (model value, <r', r'>) follow from eight inner products formed BEFORE the step length
 *                       is known, the neighbours gather the rows of H*mdelta, and C*tangent(r), C*mdelta follow by linearity.
 *                       Same tests and decisions as tCG.m; <r', r'> and the model value that decide a trip carry a rounding error of
 *                       eps <r, r> / <r', r'> (the directly summed values replace them one trip later).  G81, p = 32: 6.6 -> 4.9 us
 *                       per trip (default 1; 0 = the two-reduction trip; env MSDP_NO_PERSIST_PIPE=1)
 *   "pipe_refresh" k   one-reduction trip: every k-th trip also publishes tangent(r) and mdelta, and the next one forms both
 *                       products from direct gathers (default 16: |Heta - Hess(eta)|/|Heta| <= 1.2e-11 after 100 trips on G81;
 *                       32: 6e-11, 8: 2.5e-12; the recurrences lose accuracy with the SQUARE of k)
 *   "pipe_own"     1/0  fused one-reduction launch at 17 <= p <= 32, rows of <= 5 entries: a row's entry in its own column (the
 *                       diagonal, or a padding slot of a row without one) is taken from the lane's registers, a trip gathers 12 rows
 *                       instead of 15.  Only where every row holds such an entry (msdp_debug_fused_own); bit-identical results
 *                       (default 1; 0 = every column through the exchange buffer, for A/B timing and tests)
 *   "pipe_wide"    1/0  fused own-column launch (see "pipe_own"): the wide plan -- the fewest workgroups, in multiples of 8, whose
 *                       chunks hold at most 80 rows, so that the third row slot belongs to the waves 0..3 of a workgroup alone and the
 *                       waves 4..7 run code that computes two row slots (msdp_debug_fused_plan).  Where that is another number of
 *                       workgroups than with 0 the grid reduction sums in another order: results agree to rounding, not bit for bit
 *                       (default 1; 0 = the grid and the instance of the per-iteration launches, for A/B timing and tests)
 *   "affine_overlap" 1/0  affine kinds: the 2*eS*U contraction of a Hess-vec runs on a second stream beside the A(.) / A'(.)
 *                       chain (default 0: measured slower than one stream; kept for A/B timing; results agree to rounding)
 *   "trip2"        0/1/2  chunked path, sparse C / oblique manifold / one rank: two launches per tCG trip (12 vector passes,
 *                       msdp_trip2.hip) instead of three (17 passes): 1 = where it pays, from 2^21 vector entries on (default);
 *                       2 = always (tests); 0 = never
 *   "escape_method" 0 = block eigen-solver where it applies (sparse C, n >= 512), Lanczos otherwise (default); 1 = Lanczos
 *                       always; 2 = block also for small n (tests).  Hermitian C: 0 and 1 = Lanczos on the real view; 2 = the
 *                       block eigen-solver on a complex panel (single rank, n >= 256; Lanczos below that).  Block kinds
 *                       (unit-block-diagonal, pose-graph): 0 and 1 = Lanczos over the one-thread-per-block product; 2 = the
 *                       block eigen-solver on block storage (k_be_step_blk: panels of 32 / 64 / 128 columns, a lane group per
 *                       block; order N = nb * B >= 256 and factor width p <= 112, Lanczos otherwise)
 *   "escape_rr"    0/1  block eigen-solver, dense algebra of a Rayleigh-Ritz stage (b x b problem H c = theta G c, residual
 *                       sums): 0 = on the host (default: Cholesky + tred2 / tql2 on one thread between two copies and two
 *                       synchronisations), 1 = on the device for panels of 32 / 64 columns (one workgroup, Cholesky + cyclic
 *                       Jacobi in LDS; the stage reads one record of 2b + 2 doubles behind one synchronisation).  128-wide
 *                       panels keep the host stage, and so does a stage whose kernel reports dependent columns or a breakdown
 *                       (msdp_debug_ritz_stages counts them).  The complex panel of a Hermitian C always takes the host
 *                       stage (counted as such).  Any other value: MSDP_EINVAL
 *   "be_width" 0/32/64/128, "be_degree", "be_grid", "be_lpr"  block eigen-solver: panel width, filter degree per round,
 *                       workgroups and lanes per row of the filter step (0 = automatic; measurement and tests).  "be_width"
 *                       counts REAL columns for a Hermitian C too: 32 / 64 / 128 = 16 / 32 / 64 complex columns (automatic:
 *                       32 complex columns where the factor's and the previous call's columns plus 8, and k + 8, fit; else 64)
 *   "escape_start_y" 1/0  undeflated cold-start escape runs start from a random combination of the columns of Y plus 5 %
 *                       noise instead of pure noise (default 0; the independent lambda_min check of the host loops sets it)
 *   "lanczos_onesync" 1/0  undeflated persistent Lanczos runs use one grid synchronisation per step (default 1; 0 = the
 *                       two-synchronisation kernel the deflated runs use)
 *   "halo_exchange" 1/0  row-sharded sparse C (after msdp_comm_init*): before S*U every rank receives only the rows of the
 *                       direction its rows of C reference (grouped ncclSend / ncclRecv) instead of all rows (ncclAllGather,
 *                       default 0).  Bit-identical results; msdp_get_point_all and the escape keep the all-gather
 *   "lanczos_qglobal" 1/0  deflated persistent Lanczos runs read the deflation columns in place instead of from their LDS
 *                       copy (default 0: in place only where the copy does not fit, n > ~117 000 with 40 columns; bit-identical)
 *   "block_skip"   1/0  multiblock kind: the dense contraction skips the zero off-diagonal blocks of its operands (default 1;
 *                       0 = stream the whole N x N matrices; same results, for A/B timing)
 *   "dense_pack"   1/0  dense C*U reads the MFMA-fragment-ordered copy of C (default 1; 0 = the row-major one;
 *                       bit-identical results, for A/B timing)
 *   "persist_ep"   1/0  persistent tCG kernel on CSR rows (rows of more than 8 entries): the 64 / lanes-per-row lane groups of a
 *                       wave share ONE row and split its entries where the grid leaves lanes free -- in that form the one-reduction trip
 *                       ("persist_pipe") takes CSR rows too (G1: 12.5 -> 5.5 us per trip at p <= 16; default 1; 0 = one lane group per
 *                       row, two reductions per trip).  Same row arithmetic; the row's products are summed in another order
 *   "dense_sym", "dense_sym_min", "dense_sym_rt", "dense_sym_db", "dense_sym_len", "dense_sym_res"  symmetric dense contraction
 *                       (msdp_densesym.hip): on from dense_sym_min rows (1, default) / always (2) / never (0); workgroup shape 1..4 =
 *                       8 x 16, 8 x 32, 16 x 16, 12 x 32 rows (0 = by p and n); one or two barriers per step; slice length; workgroups
 *                       assumed resident when the slices are cut (A/B timing and tests; results agree to rounding, every shape is
 *                       bit-reproducible run to run)
 *   "timing", "esc_debug"  1/0  diagnostics on stderr                                (env MSDP_TIMING, MSDP_ESC_DEBUG)
 *   "debug_fail_persist"   1    test hook: the next persistent launch reports a synchronisation time-out
 *   "block_persist"  1/0  unit-block-diagonal and pose-graph handles: the tCG of a trust-region iteration runs as ONE persistent
 *                       launch (msdp_blockpersist.hip: the vectors of a block in registers, two grid reductions and one barrier per
 *                       trip) where a plan exists -- width p <= 32, every block in one of at most two row slots of at most
 *                       min(256, CUs) workgroups -- and "persist" is on; retraction, cost / gradient, decision and one host
 *                       synchronisation per iteration as before.  Default 0: the three launches per trip of the generic path.
 *                       Same tCG.m:95-292; sums in another order (results agree to rounding).  A launch whose workgroups cannot
 *                       synchronise gives up and the call is repeated on the generic path, as for "persist"
 *   "block_persist_grid"  n  cap on the workgroups of that launch (0 = planned; tests and tuning: a small grid takes the two-slot
 *                       instances at a few hundred blocks)
 *   "block_persist_wide"  1/0  A/B switch of that launch: 1 = the largest grid the plan allows at its row slots (the blocks spread
 *                       over more compute units), 0 (default) = the fewest workgroups that need those row slots
 *   "precon"       1/0  pose-graph handles: block-Jacobi preconditioned tCG (msdp_pose_precon.hip).  M_i = sym(C_[ii]), the diagonal
 *                       block of order d + 1 of pose i (fixed, unscaled, independent of the point), is inverted once on the host in
 *                       fp64 through its Cholesky factor; precon(x, r) = tangent_x(blockdiag(M_i^-1) r).  The tCG then follows the
 *                       preconditioned branch of tCG.m: z = precon(r) at :117-125 and :260-268, z_r = <z, r> (:126, :270),
 *                       beta = z_r / zold_rold (:272), mdelta = tangent(z + beta mdelta) (:273-283), e_Pd and d_Pd by :286-287; the
 *                       stop test :249 stays on sqrt(<r, r>).  The trust region is measured in the M-norm, Delta_bar and Delta0
 *                       keep their values.  Default 0: nothing changes, no device work.  With 1 the handle runs the generic
 *                       three-launch trips also when "block_persist" is on (msdp_tcg_path reports 0).  MSDP_EUNSUPPORTED, the
 *                       handle left as it was: a block with a non-positive or non-finite pivot (the message names the first),
 *                       a unit-block-diagonal handle (its diagonal blocks are zero) and every other kind (the message names it)
 *   "round_order"  0/1  local search of msdp_round_hyperplane and msdp_round_phases: 0 = the rows in index order, one wave per word
 *                       of 64 trials walking all rows (default); 1 = the rows in (colour, index) order of msdp_round_coloring, one
 *                       launch per colour with all rows of the colour and all words side by side.  Each order is a Gauss-Seidel
 *                       sweep, bit-reproducible run to run; they end in different local optima.  1 is accepted on a single-rank
 *                       MSDP_KIND_ONLYUNITDIAG handle with a sparse real or a Hermitian cost matrix.  MSDP_EUNSUPPORTED, the kind
 *                       named: dense and sparse-plus-low-rank handles (every row is coupled to every other), the block kinds, the
 *                       affine, dual and multiblock kinds, a handle that has joined a communicator.  Any other value: MSDP_EINVAL.
 *                       A pattern that is not structurally symmetric is refused by the rounding call (see msdp_round_coloring)
 * The environment variables are read once, when the handle is created.  Unknown names -> MSDP_EINVAL. */
int msdp_set_option(msdp_handle h, const char* name, int32_t value);
/* (parity tests) Z = tangent_Y(blockdiag(M_i^-1) R) at the resident point Y of a pose-graph handle with the option "precon" set:
 * the preconditioner of its tCG applied to a host array R (N x p row-major, tangent or not).  MSDP_ESTATE without the option or
 * without a point. */
int msdp_precon_apply(msdp_handle h, const double* R, double* Z);

/* Which implementation msdp_rtr uses for the tCG inner loop at the resident point:
 * 1 = persistent single-launch kernel (working set in registers/LDS, sparse C, oblique,
 * one rank, n and p small enough to stay on chip; or a block kind with the option "block_persist"), 0 = chunked hipGraph of three kernels
 * per trip.  Both follow tCG.m:95-292; the choice is a speed matter only. */
int msdp_tcg_path(msdp_handle h, int32_t* path);
/* (test / diagnostic) The trip form of the persistent kernel at the resident point: 2 = ONE grid reduction per trip (option
 * "persist_pipe", rows of <= 8 entries or shared CSR rows, p <= 32, every vector in registers), 1 = the "persist_early" form, 0 = two reductions per
 * trip (tCG.m:166 and :227-241 separately); -1 = the tCG is not persistent.  All forms follow tCG.m:95-292. */
int msdp_debug_persist_form(msdp_handle h, int32_t* form);
/* The same for the persistent kernel of the block kinds (option "block_persist"): 0 = two reductions per trip where it applies to
 * the handle at its resident width, else -1. */
int msdp_debug_block_persist_form(msdp_handle h, int32_t* form);
/* (test / diagnostic) Its plan at the resident width: out[0] 1 = the kernel applies (option on, plan, co-residency), out[1] lanes
 * per block, out[2] workgroups, out[3] row slots per lane group, out[4] dynamic LDS bytes; out[1..4] = 0 where no plan exists. */
int msdp_debug_block_persist_plan(msdp_handle h, int32_t* out);
/* (test / diagnostic) Which trip the chunked path takes at the resident point: 1 = the linear-product trip (option "trip1"), 2 = the
 * two-launch trip (option "trip2"), 3 = three launches per trip (every other kind and storage, the option "precon" included);
 * 0 = the tCG is persistent (msdp_tcg_path reports 1 or 2).  Read-only: no launch, the handle is not modified. */
int msdp_debug_trip_form(msdp_handle h, int32_t* form);
/* (test / diagnostic) 1 = the next fused launch (option "fused_rtr") at the resident point takes the own-column instance of the
 * one-reduction trip (option "pipe_own"; every row of C holds an entry in its own column or has fewer than 5 entries); 0 = any other
 * instance, or no fused launch.  Read-only: no launch. */
int msdp_debug_fused_own(msdp_handle h, int32_t* own);
/* (test / diagnostic) The plan of the next fused launch at the resident point: *G = its workgroups (0: no fused launch applies),
 * *rw_split = the waves of a workgroup that compute all three row slots (4 in the wide plan of option "pipe_wide", where the other four
 * waves compute two; 0 = every wave computes every slot: any other instance).  Read-only: no launch. */
int msdp_debug_fused_plan(msdp_handle h, int32_t* G, int32_t* rw_split);
/* (test / diagnostic) The planning rule of the wide plan alone, host arithmetic without a handle or a launch: *G = the smallest multiple
 * of 8, at least 8 and at most min(256, cus / 8 * 8), with ceil(n_loc / G) <= 80, or 0 where there is none.  cus <= 0 asks for the
 * current device's CU count; *cus_used returns the count that was used. */
int msdp_debug_fused_wide_rule(int32_t n_loc, int32_t cus, int32_t* G, int32_t* cus_used);
/* (test / diagnostic) What the set-up of a primal affine handle (MSDP_KIND_UNITDIAG, _UNITTRACE, _GENERIC) planned from the constraint
 * data, and which branch the last calls took.  Host only: no launch, the handle is not modified.  out[0..15]:
 *    0 usym      1 = c and every A_k are symmetric entry by entry (upper view, tiled adjoint, B route possible)
 *    1 ntp       32 x 32 upper tile pairs of the tiled adjoint (0: data not symmetric, the flat adjoint kernel runs)
 *    2 nlong_e   matrix entries (i <= j) in more than 8 constraints: one wave each in the tiled adjoint
 *    3 bW        ELL width 1..4 of the B route (0: not built)
 *    4 packed    1 = the B matrix is stored as position | coefficient code (at most 256 distinct coefficients)
 *    5 bnlong    rows of B wider than bW: one wave each
 *    6 nsup      entries At touches when they are at most 1/8 of the matrix (0: restricted adjoint and sparse products not built)
 *    7 nlong     constraints of more than 128 nonzeros (summed through item values)
 *    8 nshort    the other constraints
 *    9 nlit      work items of the long constraints
 *   10 n         order of the matrix
 *   11 nS        padded row length of the dense operands
 *   12 last_hess_path   0 no Hess-vec yet, 1 two streams (option "affine_overlap"), 2 B route, 3 fused sphere / Euclidean Hess-vec
 *                       with the SDDMM as a side job of the contraction, 4 the same with the SDDMM as a launch of its own, 5 two
 *                       passes with the sparse product on the touched entries, 6 two passes with the adjoint and the two-matrix
 *                       contraction
 *   13 last_A_route     0 none yet, 1 SDDMM + finish kernel, 2 fused SDDMM, 3 Gram matrix (a side job leaves it as it was)
 *   14, 15       zero
 * MSDP_ESTATE: a dual handle, a handle with per-block storage, a kind without affine state. */
int msdp_debug_affine_plan(msdp_handle h, int32_t* out);

/* ------------------------------------------------------------ measurement */

/* Launch the Hess-vec kernel `reps` times on the library's stream between two
 * HIP events and return the average device time per launch (ms) together with
 * the algorithmic bytes/flops of one launch (SURVEY.md 8d formulas). */
int msdp_bench_hessvec(msdp_handle h, int32_t reps, double* avg_ms,
                       double* algo_bytes, double* algo_flops);
/* One kernel of the tCG trip in isolation: which = 0 Hess-vec, 1 upd1 (tCG.m:166-241),
 * 2 upd2 (tCG.m:249-287); average device time per launch in ms. */
int msdp_bench_kernel(msdp_handle h, int32_t which, int32_t reps, double* avg_ms);
/* Same for one whole tCG trip (Hess-vec + the vector updates), exits disabled. */
int msdp_bench_tcg_trip(msdp_handle h, int32_t reps, double* avg_ms);

const char* msdp_last_error(void);
const char* msdp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MANISDP_HIP_H */
