// msdp_common.h -- internal structures shared by the HIP translation units of
// libmanisdp_hip.so.  gfx950 only (wave64, 256 CUs in 8 XCDs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/manisdp_hip.h"

#define MSDP_BLOCK 1024           // threads per workgroup (16 waves: one row step per wave, latency hidden by occupancy)
#define MSDP_WAVES (MSDP_BLOCK / 64)
#define MSDP_MAX_GRID 512         // <= 512 partial sums per reduction (2 per CU)
#define MSDP_NPART 12             // number of partial-sum arrays

void msdp_set_error(const char* fmt, ...);

// Host <-> device copies (msdp_xfer.hip): signatures of hipMemcpy / hipMemcpyAsync / hipMemcpy2D / hipMemcpy2DAsync.  Unpinned caller
// memory goes through a pinned staging buffer of the process -- no msdp_*.hip file calls the hipMemcpy family itself.
hipError_t msdp_memcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
hipError_t msdp_memcpy_async(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s);
hipError_t msdp_memcpy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind);
hipError_t msdp_memcpy2d_async(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, hipStream_t s);
void msdp_xfer_release();

#define HIPCHK(expr)                                                              \
    do {                                                                          \
        hipError_t _e = (expr);                                                   \
        if (_e != hipSuccess) {                                                   \
            msdp_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                           __FILE__, __LINE__);                                   \
            return MSDP_EHIP;                                                     \
        }                                                                         \
    } while (0)

// RTR-level scalars; written only by single-workgroup kernels that run alone
// between vector kernels (no intra-launch hazards).
struct Ctl {
    double fx, fx_prop, gg, gg_prop, norm_grad, Delta, Delta_bar, Delta0;
    double tolgradnorm, kappa, theta, rho_prime, rho_reg;
    double rho, rhonum, rhoden;
    double z_sphere[2];          // unittrace: store.z per slot
    double sigma;                // AL penalty (affine kinds)
    int maxiter, maxinner, mininner;
    int k, cur, done, stop_reason;
    int hessvecs, accepted, rejected, cost_evals, last_stop_inner;
    int bench_mode;              // 1: tCG exits disabled (throughput measurement)
    int tcg_running;             // mirror of Frame.active for host polling
    int psync8_backoff;          // the eight-value reduction of the one-reduction trip (msdp_pipe.h): units before its first poll where bits 16..23 of psync_backoff are 0
    int psync_backoff;           // grid reductions of the persistent kernels: (s_sleep units of 64 cycles before the first poll) | (units after a failed poll) << 8
    int persist_goff;            // persistent tCG: gather offsets kept in registers (A/B)
    int pipe_local;              // one-reduction trip: 1 = rows of the own workgroup from LDS / registers, 0 = every row through the exchange buffer
    int pipe_refresh;            // one-reduction trip (msdp_pipe.h): every pipe_refresh-th trip the products start afresh from direct gathers
    int persist_early;           // persistent tCG: 0 = gather the neighbours' rows at the top of the trip (round 4), >= 1 = while reduction 2 is in
                                 //   flight, the rows being their own flags (msdp_persist.hip EARLY); value - 1 = s_sleep units before the first gather
    int persist_refresh;         // persistent tCG (two-synchronisation trips): every this-many trips the product C*mdelta is
                                 //   gathered directly instead of assembled by linearity (0: never); msdp_persist.hip
};

// tCG scalars (tCG.m:102-157, 286-287); two frames, each kernel reads one frame and
// writes the other so no workgroup ever reads a word another workgroup writes in
// the same launch.
struct Frame {
    double z_r, d_Pd, e_Pd, e_Pe, model_value, norm_r0, alpha, beta;
    int active, j, stop, eta_idx;
    int md_idx;       // which of md / md2 holds the current direction (fused trips ping-pong it)
    int fresh;        // 1 right after k_tcg_init: the direction is the gradient, no update step yet
};

// Partial-sum array ids
// P_AXB: |A x - b - y/sigma|^2 of the affine kinds, summed over the constraints by MSDP_MAX_GRID workgroups (every other
// array is filled by the d.G workgroups of a row-parallel launch)
enum { P_F = 0, P_GG = 1, P_DHD = 2, P_S1 = 3, P_S2 = 4, P_S3 = 5, P_RD = 6, P_AUX = 7, P_AXB = 8,
       // sphere Hess-vec, fused form (msdp_affine.hip, k_sddmm1 mode 2): <U, G>, <U, Y>, sum_k w_k (A x)_k
       P_T1 = 9, P_T2 = 10, P_T3 = 11 };
// preconditioned tCG (msdp_pose_precon.hip): <z, r> of the init launch and of an upd1 launch, in arrays its kind leaves free
enum { P_ZR0 = P_AUX, P_ZRN = P_AXB };

enum { MANI_OBLIQUE = 0, MANI_SPHERE = 1, MANI_EUCLID = 2,
       MANI_STIEFEL = 3 };   // stacked Stiefel manifold: the d rows of a block are orthonormal (msdp_stiefel.hip)
enum { COST_SPARSE = 0, COST_DENSE = 1, COST_AFFINE = 2,
       COST_SPLR = 3,     // C = Cs + V diag(s) V': the sparse rows below plus the low-rank fields lr* (msdp_lowrank.hip)
       COST_HERM = 4,     // C = A + iB Hermitian: rowptr / colind below with the complex values hzv / hzell (msdp_hermitian.hip); cval and ellv are null
       COST_BLOCK = 5 };  // C in block CSR of block order d.blk (brp / bci / bval below, msdp_stiefel.hip); rowptr, colind, cval and the ELL copy are null
// the name of a COST_BLOCK / MANI_STIEFEL kind in messages: efree = the free rows per block
static inline const char* msdp_block_kind_name(int efree) { return efree ? "pose-graph" : "unit-block-diagonal"; }
// the widest factor a COST_BLOCK handle holds
#define MSDP_BLOCK_PMAX 256
// the rows of the cost matrix are sparse rows (no dense n x n operand exists or is reserved)
static inline bool msdp_cost_sparse_rows(int costkind) { return costkind == COST_SPARSE || costkind == COST_SPLR || costkind == COST_HERM || costkind == COST_BLOCK; }

// Everything a kernel needs, passed by value.
struct Dev {
    int n;            // global number of points (matrix order)
    int n_loc;        // rows owned by this rank
    int row0;         // global index of local row 0
    int p;            // current factor width
    int ld;           // row stride in doubles (even, >= p; pad columns are zero)
    int G;            // workgroups per row-parallel launch (multiple of 8, <= MSDP_MAX_GRID)
    int manifold;     // MANI_*
    int costkind;     // COST_*
    Ctl* ctl;
    Frame* F;         // F[0], F[1]
    double* P;        // MSDP_NPART arrays of MSDP_MAX_GRID doubles
    double* Y[2];     // point per slot            (n_loc x ld)
    double* Gr[2];    // Riemannian gradient / slot (n_loc x ld)
    double* eG[2];    // per-row scalar / slot: eG (onlyunitdiag), YeG (unitdiag)  (n_loc)
    double* eta[2];
    double* Heta[2];
    double* r;
    double* r2;       // second residual buffer (two-launch trips, msdp_trip2.hip: eta and r ping-pong together)
    double* md;       // mdelta, local rows
    double* md2;      // second direction buffer (fused two-launch trips)
    double* mdx;      // persistent tCG: exchange buffer of the direction rows (uncached memory, sc1 accesses only)
    double* Hmd;
    double* full;     // gather source of n x ld (== local buffer when nranks == 1)
    double* W0;       // scratch n_loc x ld
    double* W1;
    // msdp_trip1.hip: this rank's three sums of a trip (xs[0..2]), all ranks' (xs_all[4*q + 0..2], filled by the exchange), the
    // arrival counter of the launch that forms xs, the number of ranks
    double* xs; double* xs_all; unsigned* xcount; int xn;
    int sweep;        // gather kernels walk the rows window by window (msdp_sweep_rows, msdp_device.h) instead of chunk by chunk
    // sparse C (local rows, global column indices)
    const int* rowptr;
    const int* colind;
    const double* cval;
    int64_t nnz;
    // optional ELL copy of the same rows (max row length <= 8): [w][row] slices
    int ellW;
    int64_t ell_stride;
    const int* ellc;
    const double* ellv;
    // dense C / eS (n_loc x n row-major) per slot for affine kinds
    double* Cd;       // dense cost matrix rows (COST_DENSE) or c reshaped (COST_AFFINE)
    double* Cpk;      // COST_DENSE: the same rows in MFMA-fragment order (msdp_dense.hip, k_pack_fragments)
    double* eS[2];    // affine kinds: eS per slot (n_loc x n)
    double* AyU;      // affine kinds: A'(A(.)) scratch (n_loc x n)
    double* Sdual;    // affine kinds: dual slack S of msdp_al_dual (= AyU unless the restricted adjoint is in use)
    // affine operator: At in CSC (by constraint) and CSR (by matrix entry)
    int64_t m;
    const int64_t* at_jc; const int64_t* at_ir; const double* at_pr;     // CSC n^2 x m
    const int64_t* a_rp;  const int* a_ci;  const double* a_v;           // CSR by entry (n^2 rows)
    const double* b; double* yv; double* Axb[2]; double* w;              // length m
    double* Pm;       // partial sums for m-length reductions
    unsigned long long* status;   // host-mapped progress word: (TR iteration+1) << 32 | tCG j << 1 | active
    // multiblock kind: rowfree[i] != 0 marks the rows of the blocks that carry no unit-diagonal constraint (Euclidean
    // factor of the product manifold: no projection term, no normalisation); nullptr = every row is oblique
    const unsigned char* rowfree;
    // multiblock kind: [blk_lo[i], blk_hi[i]) = the rows (= columns) of the diagonal block row i belongs to.  Every dense
    // n x n operand of that kind (cost, eS, AyU, S) is block diagonal: the contraction skips the k range outside a row
    // tile's blocks (exact zeros there).  nullptr for every other kind.
    const int* blk_lo; const int* blk_hi;
    // msdp_debug_persist_trace: s_memtime stamps of the phases of the persistent tCG trip (traced kernel instance only), else null
    unsigned long long* trace;
    // cross-rank persistent tCG (msdp_persist.hip, XR): this rank's first workgroup index among all ranks' workgroups, their total,
    // the members' exchange buffers (sc1 accesses only)
    int xr_gid0, xr_gtot;
    // round 5: every member keeps the exchanged rows of ITS rows in its OWN buffer (local HBM on its device; the others map it through
    // HIP IPC / peer access, or simply share the address space): xr_rows[q] = member q's buffer as this process sees it, xr_cap rows each
    // (the row capacity of a rank), xr_me = this member.  A gather of row c goes to member c / xr_cap -- its own for most rows of a
    // partition with locality.
    double* xr_rows[4];
    int xr_cap, xr_me, xr_halo;
    // "push" exchange (msdp_comm.hip halo_setup): a member's buffer = [its rows (xr_cap)] [one slot per foreign row its rows of C
    // reference]; buffer-local column indices of its rows (ELL copy [w][xr_cap] and CSR), and for every local row up to two
    // (member, position there) pairs it has to be stored to as well ([2][n_loc], member -1 = none)
    const int* xr_ellc; const int* xr_colind; const int* xr_pq; const int* xr_pidx;
    const unsigned long long* xr_paddr;   // [2][n_loc] address of local row i's slot in the buffer of a member that references it (0: none); built by msdp_xpersist_member
    // round 6, two-level grid reductions between members that own a device each (msdp_psync.h psync2): xr2_on, this member's block
    // (fine-grained memory of its device), the members' blocks as this process maps them (device array of xr2_n pointers), this member's
    // index among the xr2_n members; xr_sys: the pushed rows cross devices (system-scope stores)
    int xr_pipe;          // the members' launches run the one-reduction trip (msdp_pipe.h XRM) -- process ranks, rows of <= 5 entries, <16,5,3> / <8,5,2> plans
    int xr2_on, xr2_n, xr2_me, xr_sys, xr2_skip;   // (xr2_skip: test hook -- the leader waits for this many local workgroups that do not exist)
    unsigned long long* xr2_blk;
    unsigned long long* const* xr2_peers;
    int persist_slots;    // A/B: row slots of the persistent tCG plan at p = 17..32 (0: planned)
    int persist_ep;       // CSR rows: the lane groups of a wave share a row and split its entries where the grid allows (1, default) or never (0)
    // COST_SPLR (msdp_lowrank.hip): lrq = q columns of V; lrV = V row-major (n x q: a row's q values are one contiguous load);
    // lrs = s (q); lrT = T = diag(s) V' X of the gather source of the running launch (q x ld, row stride ld), written by the
    // projection launch in front of every row launch; lrTp = its per-workgroup partials (MSDP_LR_PARTS x q x ld)
    int lrq;
    const double* lrV; const double* lrs;
    double* lrT; double* lrTp;
    // COST_HERM (msdp_hermitian.hip): the complex values (re, im) of the CSR rows (beside rowptr / colind) and of the ELL slices
    // (beside ellc, padded with (row, 0 + 0i)).  A factor row of complex width p is its real view of 2p doubles: one double2 per
    // complex entry, so d.p = 2p and d.ld = 2p on such a handle
    const double2* hzv; const double2* hzell;
    // COST_BLOCK / MANI_STIEFEL (msdp_stiefel.hip): block order blk = d in {2, 3} and block count nb = n / d; the cost matrix in
    // block CSR -- block row i holds the entries brp[i] .. brp[i + 1], entry k the block column bci[k] and the d x d values
    // bval[k * d * d ..] row-major (zero where the caller's pattern is partial); Lam[slot] = the multiplier blocks
    // Lambda_i = sym((C Y)_i Y_i') of the point in that slot (nb * d * d doubles, each block row-major and symmetric); eG[slot]
    // carries their diagonals, row by row
    // The pose-graph kind is the same storage with efree = 1: blocks of blk = d + 1 rows, the last of them a free
    // (Euclidean) row; Lambda stays d x d with d = blk - efree (nb * d * d doubles per slot), eG holds 0 in the free-row entries
    int blk, nb, efree;
    // fused own-column launch in its wide plan (k_tcg_pipe_ws, msdp_pipe.h): the waves [0, rw_split) of a workgroup compute all three row
    // slots, the others two; 0 everywhere else.  (Sits in what was padding in front of the pointers: no other member moves.)
    int rw_split;
    const int* brp; const int* bci; const double* bval;
    double* Lam[2];
    // pose-graph kind, option "precon" (msdp_pose_precon.hip): pcM = the inverses M_i^-1 of the diagonal blocks sym(C_[ii]) (nb * blk * blk
    // doubles, each block row-major and symmetric), pcz = the preconditioned residual z of the running tCG (n_loc x ld).  Both null
    // while the option is off: pcM != nullptr is what selects the preconditioned launchers
    const double* pcM; double* pcz;
};
#define MSDP_LR_PARTS 128         // workgroups (= partial sums per entry of T) of the low-rank projection

// Run-time switches of a handle (msdp_set_option; the environment variables of the same meaning are read ONCE, when
// the handle is created).  Production = the defaults.
struct Tuning {
    int persist = 1;       // persistent single-launch tCG / Lanczos kernels where they fit        (MSDP_NO_PERSIST=1 -> 0)
    int fused_rtr = 1;     // whole trustregions() loop in one launch for p <= 32                  (MSDP_NO_FUSED_RTR=1 -> 0)
    int graph = 1;         // chunked tCG trips replayed as hipGraphs                              (MSDP_NO_GRAPH=1 -> 0;
                           //   rocprofv3 7.2 crashes on graph replay)
    int affine_route = 0;  // A(Ya Yb'): 0 = by bytes moved, 1 = SDDMM, 2 = Gram                   (MSDP_AFFINE_ROUTE=sddmm|gram)
    int timing = 0;        // per-call timing lines on stderr                                       (MSDP_TIMING=1)
    int esc_debug = 0;     // per-run Lanczos statistics on stderr                                  (MSDP_ESC_DEBUG=1)
    int escape_deflate = 1;  // escape: deflate span(Y) at near-stationary points (fast, approximate when S*Y != 0)
    int escape_start_y = 0;   // undeflated cold-start runs begin in span(Y) + 5 % noise (the independent lambda_min check sets it)
    int halo_exchange = 0;    // row-sharded sparse C: exchange only the referenced rows before S*U (0: the all-gather north_star prescribes)
    int block_skip = 1;       // multiblock kind: the dense contraction skips the k range outside a row tile's diagonal blocks (0: A/B, tests)
    int lanczos_qglobal = 0;  // tests: deflated persistent Lanczos reads the deflation columns in place even where they fit the LDS
    int lanczos_onesync = 1;  // undeflated persistent Lanczos runs: one grid synchronisation per step (0: two)
    int dense_pack = 1;    // dense C*U reads the fragment-ordered copy of C (0: the row-major one; same results)
    int affine_fuse = 1;   // affine kinds, SDDMM route, one rank: A(Ya Yb') and its finish in ONE launch (k_sddmm1); sphere Hess-vec: the
                           //   sparse A'(w)*Y product, the slab sum and the projection in ONE launch (k_sph_hess_fused) (0: A/B, tests)
    int affine_side = 1;   // sphere / Euclidean Hess-vec, SDDMM route, few touched entries: the SDDMM rides in the contraction launch as a side job
                           //   (msdp_dense_gemm_side) instead of a launch of its own (0: A/B, tests)
    int affine_broute = 1; // affine Hess-vec, Gram route, symmetric data with short constraints: A'(A(.)) as one sparse matrix on the Gram matrix
                           //   (k_adjoint_gram) instead of k_gram_apply + k_adjoint_tiled (0: A/B, tests)
    int dense_sym = 1;     // symmetric dense operands (p <= 32, one rank): the contraction reads the upper triangle only
                           //   (msdp_densesym.hip); 1 = from dense_sym_min rows on, 2 = always, 0 = never
    int dense_sym_min = 8192;   // see dense_sym (below, the partial slabs of the transposed products cost what the halved matrix saves: measured)
    int dense_sym_rt = 0;       // A/B: 16-row tiles per wave of k_dense_sym (0: by n; 1 or 2)
    int dense_sym_db = 0;       // A/B: double-buffered reduction, one barrier per step (0: by shape, 1: never, 2: always)
    int dense_sym_len = 0;      // A/B: slice length of a work item in 16-column steps (0: planned)
    int dense_sym_res = 0;         // workgroups of the symmetric contraction assumed resident at a time when its slices are cut (0: by shape)
    int escape_warm = 1;     // escape: start the Lanczos runs from what the previous call found (0: hashed random vector)
    int xpersist = 1;        // in-process ranks (msdp_comm_init_local), sparse C, oblique: ONE persistent tCG spanning the ranks' launches -- grid
                             //   reductions and row exchange through shared uncached memory, no collective per trip (msdp_persist.hip XR); 0: lock-step chunks
    int xtail = 1;           // process ranks (msdp_comm_init_ipc): the rest of a TR iteration behind the cross-rank tCG is one launch per member as well
                             //   (retraction, cost / gradient at the proposal, decision; msdp_trtail.hip XR); 0: sharded kernels with their collectives
    int psync8_backoff = 16;   // eight-value reduction of the one-reduction trip: units slept before the first poll (round 6: 16 against 19, 0.8 % of a G81 call)
    int psync_backoff = 19;  // grid reductions of the persistent kernels: s_sleep units (64 cycles) before the first poll | units after a
                             //   failed poll << 8.  Round 4: nothing can be visible for the first half microsecond after the posts, and
                             //   the polls of 216 workgroups are the traffic the posts compete with -- G81, p = 32: 8.03 us per trip
                             //   with 0, 7.06 (14), 6.85 (18), 6.87 (20), 7.05 (24), 7.44 (32), 7.86 (40); p = 16: 6.87 -> 5.84
                             //   (tools/psync_backoff_probe.py); sleeping between failed polls gains nothing
    int window = 1;            // stand-alone sparse S*U with the gathered rows staged once per workgroup in LDS (msdp_window.hip): 1 = for vectors
                               //   far beyond the L2s (from 3 * 2^22 entries on), 2 = always (tests), 0 = never
    int window_lds = 144;      // ... KB of LDS a window may take (A/B; one 1024-thread workgroup per CU)
    int persist_refresh = 32;  // persistent tCG: direct (three-synchronisation) trip every this-many trips, bounds the drift of C*mdelta
    int persist_slots = 0;     // A/B: row slots per lane group of the persistent tCG at p = 17..32 (0: planned; 3 or 4)
    int persist_ep = 1;        // CSR rows of the persistent tCG: entry-parallel lanes where the rows leave lanes free (A/B: 0 never)
    int persist_goff = 1;      // persistent tCG: the byte offsets of the R x EW gathers of a trip live in registers (0: recomputed per trip from the LDS copy of the column indices)
    int pipe_local = 1;        // one-reduction trip: neighbours that belong to the same workgroup are read from LDS, the diagonal from registers
    int pipe_wide = 1;         // fused own-column launch: the wide plan -- the fewest workgroups whose chunks end inside the first half of the third row slot
                               //   (<= 80 rows), waves 4..7 compute two slots (k_tcg_pipe_ws; 0: the plan of persist_grid and its instance; A/B, tests)
    int pipe_own = 1;          // fused one-reduction trip at 16 lanes per row: a row's entry in its own column from registers, 12 gathers a trip (0: all 15; A/B, tests)
    int xr_twolevel = 0;       // process ranks: 1 = two-level grid reductions (msdp_psync.h psync2) also where the flat ones would do (one device, <= 4 members); A/B, tests
    int pipe_refresh = 16;     // one-reduction trip: trips between two direct exchanges (its recurrences drift with the square of this)
    int persist_pipe = 1;      // persistent tCG: ONE grid reduction per trip (msdp_pipe.h) where an instance exists (rows of <= 8 entries, p <= 32)
    int persist_early = 0;     // persistent tCG: the neighbours' rows are gathered while reduction 2 is in flight -- sentinel-initialised exchange
                               //   halves, the rows are their own flags (0: at the top of the next trip, behind reduction 2 -- the round-4 trip;
                               //   n >= 1: n - 1 s_sleep units between the post of reduction 2 and the first gather)
    int affine_overlap = 0;  // affine Hess-vec: 2*eS*U on a second stream beside the A(.) / A'(.) chain.  Measured SLOWER (round 3: BQP d = 60
                             //   85 against 73 us, theta n = 5000 83 against 74 us per Hess-vec inside graph replays): every launch of the chain
                             //   already fills the chip, the fork / join only adds dependencies.  Kept as an A/B switch, default off.
    int dense_sk = 0;        // A/B switch: number of k slices of the dense contraction (0 = the plan's choice)
    int sweep_k = 2;         // 64-row steps a workgroup takes per window of the traversal (window = 32 * 64 * sweep_k rows per XCD)
    int sweep = 1;           // windowed row traversal of the large-vector gather kernels: 1 = from 2^21 vector entries per rank on (streaming accesses from 3 * 2^22 on), 2 always / without streaming accesses, 3 always / with them, 0 never
    int trip1 = 1;           // msdp_trip1.hip (sparse C / oblique): row-sharded handles -- one exchange + one all-reduce per tCG trip instead of one + two;
                             // one rank, chunked path -- the same two launches (14 vector passes, one gathered vector); 0: never
    int trip2 = 1;           // chunked path, sparse C / oblique / one rank: two launches per tCG trip (msdp_trip2.hip) instead of three
    int escape_method = 0;   // 0: block Chebyshev-filtered subspace iteration where it applies (msdp_blockeig.hip), else Lanczos;
                             //   1: Lanczos always (msdp_escape.hip); 2: block also below its size threshold (tests)
    int escape_rr = 0;       // block eigen-solver, dense algebra of a Rayleigh-Ritz stage: 0 = on the host (be_ritz), 1 = on the device
                             //   (k_be_ritz, msdp_beritz.hip) for panels of 32 / 64 columns; 128-wide panels and stages the kernel hands
                             //   back (dependent columns, breakdown) run on the host either way
    int be_width = 0;        // block eigen-solver: panel width 32 / 64 / 128 (0: 64, or 128 when the start block needs it)
    int be_degree = 0;       // ... filter degree per round (0: 200 warm, 400 cold)
    int be_grid = 0;         // ... workgroups of the filter step (0: by rows)
    int be_lpr = 0;          // ... lanes per row of the filter step (0: by rows per workgroup)
    int grid = 0;          // workgroups of the row-parallel launches (0: choose_grid; A/B switch)
    int blk_groups = 0;    // msdp_block_eigs_large: workgroups per block of order > 256 (0: by order; tests of the bit-identity across group sizes)
    int fail_block = 0;    // test hook (msdp_set_option "debug_fail_block"): the next block eigen-solver call reports itself unconverged
    int fail_xr = 0;       // test hook ("debug_xr_skip"): this member skips its next cross-rank persistent launch
    int fail_persist = 0;  // test hook (msdp_set_option "debug_fail_persist"): the next persistent launch reports a
                           //   grid-synchronisation time-out without running, to exercise the recovery path
    int block_persist = 0;       // block kinds (MANI_STIEFEL / COST_BLOCK): the tCG of a TR iteration in one persistent launch
                                 //   (msdp_blockpersist.hip) where a plan exists; 0 (default): the generic three-launch trips
    int block_persist_grid = 0;  // ... cap on its workgroups (0: planned; tests and tuning: a small grid takes the two-slot instances)
    int block_persist_wide = 0;  // ... A/B: 1 = the largest grid the plan allows at its row slots, not the fewest workgroups
    int round_order = 0;         // local search of msdp_round_hyperplane / msdp_round_phases: 0 = rows in index order, one wave per word (default);
                                 //   1 = rows in (colour, index) order, one launch per colour class over the whole grid (msdp_roundcolor.hip)
};

struct msdp_handle_s {
    int kind = 0;
    Tuning tune{};
    bool persist_failed = false;   // a persistent launch timed out on this handle: stay on the chunked path
    double* rtr_start = nullptr;   // copy of the start point of the running msdp_rtr call (persistent path: recovery)
    size_t rtr_start_cap = 0;
    Dev d{};
    int pcap = 0;
    int ldcap = 0;
    bool have_point = false;
    bool state_valid = false;      // cost/grad state computed at the resident point
    bool gradnorm_valid = false;   // h_ctl->norm_grad / fx describe the resident point
    bool dual_valid = false;       // d.Sdual holds the dual slack S of the last msdp_al_dual call
    double* vec_pool = nullptr;    // the one allocation behind Y, Gr, eta, Heta, r, md, Hmd, W0, W1 (msdp_alloc_vectors)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    Ctl* h_ctl = nullptr;          // pinned host mirror
    Frame* h_frame = nullptr;
    std::vector<void*> allocs;     // everything to hipFree
    // host copies needed for re-allocation / sharding
    int nranks = 1, rank = 0;
    void* comm = nullptr;          // ncclComm_t
    bool presharded = false;       // created per shard (dense synthetic): row0/n_loc fixed at creation
    double* full_buf = nullptr;    // gather buffer (nranks x cap rows) when the rows are sharded
    // halo exchange (sparse C, option "halo_exchange"): instead of all rows of the direction every rank receives only the rows
    // its rows of C reference (msdp_comm.hip, "Halo exchange")
    struct Halo* halo = nullptr;
    struct AffineState* affine = nullptr;  // affine, multiblock and dual kinds: the operator At and its operands (msdp_affine_dev.h;
                                           //   created by msdp_affine_setup[_blocked], deleted by msdp_affine_release)
    struct LocalGroup* lgroup = nullptr;   // in-process stand-in for the RCCL communicator (msdp_comm_init_local)
    unsigned long long* xr_paddr = nullptr; size_t xr_paddr_cap = 0; double* xr_paddr_key[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; int xr_paddr_ld = 0, xr_paddr_n = 0; const int* xr_paddr_pq = nullptr;   // cross-rank push addresses and what they were built from
    bool lgroup_is_ipc = false;                  // the handle's group is a process group (msdp_comm_init_ipc)
    unsigned long long* xr2_blk = nullptr;       // this member's two-level block (its own allocation), the members' blocks as mapped here (device array)
    unsigned long long** xr2_peers = nullptr;
    int xr2_share = 1; bool xr2_multi = false;   // process ranks (msdp_comm_init_ipc): the most members on one device, members on different devices
    bool xr_ok = false; int xr_halo_rows = 0;   // push exchange of the cross-rank kernels: usable (no row needed by more than two members), foreign rows referenced
    struct WinCache* win = nullptr;        // patch plans of the LDS-staged S*U (msdp_window.hip), one per lanes-per-row
    void* blk_ws = nullptr; size_t blk_ws_cap = 0;   // workspace of msdp_block_eigs (msdp_blockjacobi.hip) and msdp_block_eigs_large (msdp_blocktridiag.hip)
    int blk_launches = 0, blk_wgs = 0;               // launches and workgroups of the last msdp_block_eigs_large call
    std::vector<int64_t> mb_n; int mb_nob = 0;       // multiblock kinds: the block orders and the number of unit-diagonal blocks (msdp_block_reshape)
    double* lc_tmp = nullptr; size_t lc_tmp_cap = 0;   // its reduction scratch
    // row-sharded onlyunitdiag (sparse C): the escape runs replicated on full copies of C's CSR arrays and of z
    int* esc_rp = nullptr; int* esc_ci = nullptr; double* esc_cv = nullptr; double* esc_z = nullptr;
    double* yfull[2] = {nullptr, nullptr};   // row-sharded affine kinds: all rows of Y[slot] (the A(.) operator and the dense
                                             //   contraction read every row; msdp_affine.hip, "Row sharding")
    bool use_comm = false;         // route the exchanges through RCCL (set by msdp_comm_init, any nranks)
    std::vector<int> h_rowptr; std::vector<int> h_colind; std::vector<double> h_cval;
    // device-side sparse arrays owned by the handle
    int* d_rowptr = nullptr; int* d_colind = nullptr; double* d_cval = nullptr;
    int* d_ellc = nullptr; double* d_ellv = nullptr;
    msdp_rtr_opts last_opts{};
    double last_rtr_device_ms = -1.0; bool last_rtr_fused = false;   // msdp_debug_last_rtr_device_ms
    // tCG chunk graph (CH x {hess, upd1, upd2}) and its validity signature
    hipGraphExec_t chunk_exec = nullptr;          // the one to launch now (alias into chunk_execs)
    hipGraphExec_t chunk_execs[2] = {nullptr, nullptr};
    Dev chunk_sig{};
    int chunk_len = 0;
    volatile unsigned long long* h_status = nullptr;   // host view of Dev::status
    volatile int* h_flags = nullptr;                   // pinned copies of ctl->tcg_running, one per chunk in flight (lock-step path)
    hipEvent_t ev_flag[2] = {nullptr, nullptr};
    double* snap = nullptr;        // msdp_point_snapshot copy of the resident point
    size_t snap_cap = 0;
    int snap_p = 0;
    double* slab = nullptr;        // split-K partial slabs of the dense MFMA path
    bool blocked = false;          // multiblock kind with per-block storage: no N x N operand exists (msdp_affine_setup.hip)
    bool dense_symmetric = false;  // every dense operand of the contraction (C, eS, AyU) is symmetric (checked at set-up)
    unsigned long long* trace_buf = nullptr;   // device buffer behind Dev::trace (msdp_debug_persist_trace)
    void* symplans = nullptr;      // work-item plans of the symmetric contraction (msdp_densesym.hip)
    size_t slab_cap = 0;
    // escape workspace, kept between calls (freeing 3 GB after every call stalled the NEXT kernels on the stream
    // for ~60 ms while the driver unmapped it: gaps seen in the kernel trace of the G81 solve)
    double* esc_mem = nullptr;
    size_t esc_cap = 0;               // doubles
    unsigned long long* lz_slots = nullptr;   // grid-sync slots of the persistent Lanczos kernel (uncached device memory)
    double* esc_prev = nullptr;       // sum of the bottom eigenvectors found by the previous escape call (warm start)
    int esc_prev_n = 0;
    // outcome of the last escape call (msdp_escape_info): real pairs returned, every Lanczos run passed a stop test,
    // largest relative residual |S x - theta x| / max(|theta|, |lam_max|) among the runs that hit maxit instead
    int esc_nvalid = 0, esc_converged = 0;
    double esc_maxres = 0.0;
    double esc_lower = 0.0;           // lower estimate of lambda_min(S) from the last call (-inf: none), see msdp_escape_lower_bound
    void* be = nullptr;               // workspace and warm-start state of the block eigen-solver (msdp_blockeig.hip)
    double* esc_top = nullptr;        // top eigenvector of the previous escape call (warm start of the lambda_max run), esc_top_n entries
    int esc_top_n = 0;
    long long coll_calls = 0;         // collective calls issued so far (exchange, all-reduce, all-gather; a grouped call counts once)
    hipEvent_t xr_ev = nullptr;       // marks this member's stream in front of the combined cross-rank launch
    bool xpersist_last = false;       // the last trustregions() call ran the cross-rank persistent tCG (msdp_tcg_path reports 2)
    bool trip1_capture = false;       // enqueue_trips runs inside a graph capture (no count-dependent launches)
    int trip1_count = 0;              // msdp_trip1.hip: trips enqueued since the tCG began (refresh schedule)
    int esc_method_last = 0;          // what the last escape call ran: 0 Lanczos, 1 block
    // persistent tCG kernel (msdp_persist.hip): grid-sync slots, error flag, cached eligibility
    unsigned long long* psync_slots = nullptr;
    int* psync_err = nullptr;
    int persist_sig_lpr = 0, persist_sig_ew = 0, persist_sig_r = 0, persist_sig_G = 0, persist_sig_ok = 0;
    const void* persist_sig_fn = nullptr; const void* fused_sig_fn = nullptr;     // the kernel instance the cached answers are for
    int fused_sig_lpr = 0, fused_sig_ew = 0, fused_sig_G = 0, fused_sig_ok = 0;
    int slots_grid = 0;               // workgroups of the last persistent launch on psync_slots (a launch on another grid resets the slot lines first)
    bool ell_own_col = false;         // ELL copy: every local row has an entry in its own column or a padding slot (msdp_upload_sparse_rows)
    // persistent tCG kernel of the block kinds (msdp_blockpersist.hip): cached eligibility, the slot region of the next launch
    const void* blkpersist_sig_fn = nullptr; int blkpersist_sig_G = 0, blkpersist_sig_ok = 0; size_t blkpersist_sig_lds = 0;
    int blkpersist_region = 0;
    // option "precon" of the pose-graph kind (msdp_pose_precon.hip): the buffers behind Dev::pcM / Dev::pcz, allocated when the option is
    // first set and kept while it is off
    double* pc_minv = nullptr; double* pc_z = nullptr; size_t pc_z_cap = 0;
    // colouring of the rows of C for the colour-ordered rounding sweeps (msdp_roundcolor.hip): built on first use, kept with the handle.
    // rc_color[i] the colour of row i, rc_offs[c] .. rc_offs[c + 1] the positions of class c in the visiting order (device copies:
    // rc_order_d, n rows sorted by (colour, index), and rc_offs_d, rc_ncolors + 1 offsets)
    int rc_ncolors = -1; std::vector<int> rc_color, rc_offs; int* rc_order_d = nullptr; int* rc_offs_d = nullptr;
};

#define MSDP_CHECK_H(h)                                     \
    if (!(h)) { msdp_set_error("null handle"); return MSDP_EINVAL; }
#define MSDP_XS_MAX_RANKS 64
#define MSDP_TCG_CHUNK 8          // tCG trips per enqueued chunk (one hipGraph of 3 x 8 kernel nodes)

static inline bool msdp_dual_kind(msdp_handle h) { return h->kind == MSDP_KIND_DUAL_UNITDIAG || h->kind == MSDP_KIND_DUAL || h->kind == MSDP_KIND_DUAL_MULTIBLOCK; }
static inline int msdp_host_cur(msdp_handle h) { return h->h_ctl->cur; }
// equal per-rank row count so the all-gather is one uniform RCCL call
static inline int msdp_rows_capacity(msdp_handle h) { return (h->d.n + h->nranks - 1) / h->nranks; }

// --- every function one .hip unit defines and another calls, by defining unit (launchers: asynchronous on h->stream) ---
struct SideJob; struct AffineDev; struct AffineState;         // msdp_affine_dev.h
struct DualState;                                             // msdp_dual.hip
// msdp_api.hip
int msdp_alloc_vectors(msdp_handle h, int pcap);
int msdp_alloc_common(msdp_handle h);
int msdp_upload_sparse_rows(msdp_handle h);
int msdp_ensure_state(msdp_handle h);
int msdp_adopt_point(msdp_handle h, int slot, int p);         // the resident point now stands in Y[slot] with width p: width, stride, grid, flags
// msdp_mem.hip
int msdp_dev_alloc_bytes(msdp_handle h, void** out, size_t bytes);            // freed with the handle, or by msdp_dev_free
int msdp_dev_alloc_uncached_bytes(msdp_handle h, void** out, size_t bytes);   // from the pool of exchange memory (plain memory when that fails)
void msdp_dev_free(msdp_handle h, void* p);
void* msdp_uc_alloc(size_t bytes);                            // per-process pool of fine-grained blocks
bool msdp_uc_free(void* p);
void msdp_uc_release_pool();
bool msdp_host_kit_take(msdp_handle h);
void msdp_host_kit_give(msdp_handle h);
void msdp_host_kits_release();
template <typename T> inline int msdp_dev_alloc(msdp_handle h, T** out, size_t count) {
    void* p = nullptr;
    int rc = msdp_dev_alloc_bytes(h, &p, (count ? count : 1) * sizeof(T));
    if (!rc) *out = (T*)p;
    return rc;
}
template <typename T> inline int msdp_dev_alloc_uncached(msdp_handle h, T** out, size_t count) {
    void* p = nullptr;
    int rc = msdp_dev_alloc_uncached_bytes(h, &p, (count ? count : 1) * sizeof(T));
    if (!rc) *out = (T*)p;
    return rc;
}
// a device copy of a host array (freed with the handle)
template <typename T> inline int msdp_upload(msdp_handle h, const std::vector<T>& v, const T** out) {
    void* p = nullptr;
    int rc = msdp_dev_alloc_bytes(h, &p, v.size() * sizeof(T));
    if (rc) return rc;
    if (!v.empty()) HIPCHK(msdp_memcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (const T*)p;
    return 0;
}
// msdp_comm.hip
int msdp_allreduce_partials(msdp_handle h, int first, int count);   // no-op when nranks == 1
int msdp_allreduce_array(msdp_handle h, double* buf, size_t count);
int msdp_allgather_rows(msdp_handle h, const double* local_rows);   // local -> d.full
int msdp_allgather_vec(msdp_handle h, const double* local, double* all, size_t count_per_rank);
int msdp_exchange_rows(msdp_handle h, const double* local_rows);    // sparse C: halo rows only when option halo_exchange is set, else the all-gather
int msdp_exchange_rows_sums(msdp_handle h, const double* local_rows);
void msdp_comm_release(msdp_handle h);
void msdp_halo_release(msdp_handle h);
void msdp_local_leave(msdp_handle h);
int msdp_local_barrier(msdp_handle h);
int msdp_local_vote_min(msdp_handle h, int v, int* out);
int msdp_xr_begin(msdp_handle h, bool* use);
int msdp_xr_launch(msdp_handle h);
int msdp_xr_tail(msdp_handle h);
int msdp_xr_check(msdp_handle h);
// msdp_rtr.hip
int msdp_push_ctl(msdp_handle h);
void msdp_fill_ctl(msdp_handle h, const msdp_rtr_opts* o);
bool msdp_use_graphs(msdp_handle h);
int msdp_tcg_begin(msdp_handle h);
int msdp_enqueue_trips(msdp_handle h, int cnt);
int msdp_ensure_chunk_graph(msdp_handle h, int CH);
int msdp_launch_chunk(msdp_handle h, int CH, bool graph);
void msdp_restore_status_ptr(msdp_handle h);
// msdp_kernels.hip
int msdp_launch_costgrad(msdp_handle h, int slot);            // Y[slot] -> Gr[slot], eG[slot], P_F, P_GG
int msdp_launch_hess(msdp_handle h);
int msdp_launch_tcg_init(msdp_handle h);
int msdp_launch_upd1(msdp_handle h);
int msdp_launch_upd2(msdp_handle h);
int msdp_launch_retract(msdp_handle h);                       // Y[cur]+eta -> Y[1-cur], P_RD
int msdp_launch_rtr_begin(msdp_handle h);
int msdp_launch_rtr_decide(msdp_handle h);
int msdp_k_pack(msdp_handle h, const double* src, double* dst, int n, int p, int ld, bool colmajor);
int msdp_k_unpack(msdp_handle h, const double* src, double* dst, int n, int p, int ld, bool colmajor);
int msdp_k_proj_obl(msdp_handle h, const double* Y, const double* U, double* V);
int msdp_k_retr_obl(msdp_handle h, const double* Y, const double* U, double* Z, double alpha);
int msdp_k_set_active(msdp_handle h, int active);
int msdp_k_sum_to(msdp_handle h, int which, double* out);
int msdp_k_fgram(msdp_handle h, const double* Y, double* part, int nblk, double* out);
int msdp_k_frotate(msdp_handle h, int cap, int r, int ldn, const double* Y, const double* Q, double* Yn);
int msdp_k_fappend(msdp_handle h, int cap, int k, int ldn, const double* Y, const double* V, double alpha, int normalize, double* Yn);
// msdp_lowrank.hip
int msdp_lowrank_setup(msdp_handle h, int q, const double* V, const double* s);   // uploads V (row-major) and s, allocates T and its partials
int msdp_lowrank_project(msdp_handle h, const double* X);     // d.lrT = diag(s) V' X (X: n x ld gather source)
int msdp_lowrank_sv_add(msdp_handle h, const double* v, double* w);   // w += V (s .* (V' v)) for vectors of n entries (the escape's S*v; uses d.lrT / d.lrTp)
// msdp_hermitian.hip
int msdp_round_color_check(msdp_handle h, const char* who);    // 0 where the colour-ordered sweeps apply to the handle, else MSDP_EUNSUPPORTED with the kind named
int msdp_round_color_plan(msdp_handle h, const char* who);     // the colouring of the handle, built and uploaded on the first call (h->rc_*)
int msdp_hermitian_setup(msdp_handle h, const double* val);   // the complex CSR / ELL values of a COST_HERM handle (val: nnz (re, im) pairs in CSC order)
int msdp_hermitian_sv(msdp_handle h, const double* z, const double* v, double* w);   // w = C v - z .* v, v and w n complex entries (re, im interleaved)
int msdp_hermitian_jcopy(msdp_handle h, const double* v, double* w);                 // w = i * v: (re, im) -> (-im, re)
// msdp_stiefel.hip: the steps of a COST_BLOCK handle of either kind (d.efree = 0: unit-block-diagonal, 1: pose-graph)
int msdp_stiefel_setup(msdp_handle h, int blk, int efree, const int64_t* jc, const int64_t* ir, const double* val);   // block CSR (block order blk, of which efree free rows) of a COST_BLOCK handle from the caller's CSC arrays; Lam[0..1]
int msdp_stiefel_costgrad(msdp_handle h, int slot);           // Y[slot] -> Gr[slot], Lam[slot], eG[slot], P_F, P_GG (gather source: d.full)
int msdp_stiefel_hess(msdp_handle h);
int msdp_stiefel_upd2(msdp_handle h);
int msdp_stiefel_retract(msdp_handle h);
int msdp_stiefel_proj(msdp_handle h, const double* Y, const double* U, double* V);
int msdp_stiefel_retr(msdp_handle h, const double* Y, const double* U, double* Z, double alpha);
int msdp_stiefel_sv(msdp_handle h, const double* Lam, const double* v, double* w);   // w = C v - blockdiag(Lam (+) 0) v for vectors of n entries (the escape's S*v)
// msdp_pose_precon.hip: the block-Jacobi preconditioned tCG of a pose-graph handle (option "precon"; d.pcM != nullptr selects it)
int msdp_pose_precon_set(msdp_handle h, int on);              // the option: M_i^-1 on the host, once; MSDP_EUNSUPPORTED names the kind or the block
int msdp_pose_precon_vectors(msdp_handle h);                  // (re)allocates z for the handle's row capacity
int msdp_pose_precon_init(msdp_handle h);                     // tCG.m:102-157 with z = precon(r)
int msdp_pose_precon_upd1(msdp_handle h);                     // tCG.m:166-241, z = precon(r_new), <z, r_new>
int msdp_pose_precon_upd2(msdp_handle h);                     // tCG.m:227-287 with beta = z_r_new / z_r
int msdp_pose_precon_apply(msdp_handle h, const double* Y, const double* R, double* Z);   // Z = tangent_Y(blockdiag(M_i^-1) R)
// msdp_trip1.hip, msdp_trip2.hip
int msdp_trip1_ok(msdp_handle h);                             // sharded trip with one all-reduce applies to this handle
int msdp_launch_trip1_init(msdp_handle h);
int msdp_launch_trip1_head(msdp_handle h, bool direct);
int msdp_launch_trip1_upd(msdp_handle h);
int msdp_trip2_ok(msdp_handle h);                             // two-launch trip applies to this handle
int msdp_launch_trip2_init(msdp_handle h);
int msdp_launch_trip2_head(msdp_handle h);
int msdp_launch_trip2_upd(msdp_handle h);
// msdp_persist.hip
int msdp_persist_eligible(msdp_handle h);
int msdp_launch_tcg_persist(msdp_handle h, int reset_slots = 1);   // whole tCG of the current TR iteration, one launch
int msdp_persist_fused_ok(msdp_handle h);                     // whole trustregions() loop in one launch possible?
int msdp_launch_rtr_fused(msdp_handle h);
size_t msdp_psync_bytes();
int msdp_tr_tail_grid(msdp_handle h);                         // (persist_grid)
int msdp_fused_grid(msdp_handle h);                           // workgroups of the fused launch (fused_grid: the wide plan where it applies, else persist_grid)
int msdp_persist_trace_dims(msdp_handle h, int* G, int* nj, int* j0);
int msdp_xpersist_eligible(msdp_handle h, int nranks);
size_t msdp_xpersist_slot_bytes();
int msdp_xpersist_reset(hipStream_t stream, unsigned long long* slots, int* err);
int msdp_xpersist_member(msdp_handle h, int nranks, int rank, double* const* rows, int halo_rows, Dev* out, int* plan3);
int msdp_launch_tcg_xpersist_all(hipStream_t stream, int nranks, const Dev* devs, const int* plans, unsigned long long* slots, int* err);
int msdp_launch_tcg_xpersist_one(hipStream_t stream, const Dev& dv, const int* plan, unsigned long long* slots, int* err);
size_t msdp_xr2_block_bytes();
size_t msdp_xr2_err_offset();
int msdp_xr2_reset(hipStream_t stream, unsigned long long* blk);
// msdp_blockpersist.hip
int msdp_blockpersist_eligible(msdp_handle h);                // the persistent tCG of the block kinds applies (option "block_persist")
int msdp_blockpersist_plan_of(msdp_handle h, int* lpr, int* G, int* R, size_t* lds);   // its plan at the resident width (returns 0: none)
int msdp_launch_tcg_blockpersist(msdp_handle h, int reset_slots);   // whole tCG of the current TR iteration, one launch
// msdp_trtail.hip
int msdp_launch_tr_tail(msdp_handle h);                       // retract + cost/grad at the proposal + accept/reject, one launch
int msdp_launch_tr_tail_xr(hipStream_t stream, const Dev& dv, unsigned long long* slots, int* err);
// msdp_sphere.hip
int msdp_sphere_proj(msdp_handle h, const double* Y, const double* U, double* V);
int msdp_sphere_retr(msdp_handle h, const double* Y, const double* U, double* Z, double alpha);
int msdp_sphere_upd2(msdp_handle h);
int msdp_sphere_retract(msdp_handle h);
// msdp_window.hip
int msdp_window_eligible(msdp_handle h);
int msdp_window_hess(msdp_handle h);
void msdp_window_release(msdp_handle h);
// msdp_dense.hip
int msdp_dense_nS(int n);
int msdp_dense_setup(msdp_handle h, const double* C);
int msdp_dense_setup_synthetic(msdp_handle h, uint64_t seed);
int msdp_dense_reserve(msdp_handle h, int nmat);
int msdp_dense_ensure_slab(msdp_handle h, size_t need);
int msdp_dense_costgrad(msdp_handle h, int slot);
int msdp_dense_hess(msdp_handle h);
int msdp_dense_hess_epilogue_obl(msdp_handle h, const double* slab, int64_t stride, int SK);
int msdp_dense_gemm_slabs(msdp_handle h, int nmat);
int msdp_dense_gemm(msdp_handle h, int nmat, const double* const* M, const double* const* X, const double* scale,
                    const int* active_flag, const double** slab_out, int64_t* stride_out, int* SK_out);
int msdp_dense_gemm_at(msdp_handle h, hipStream_t stream, int slab_first, int slabs_reserve, int nmat, const double* const* M,
                       const double* const* X, const double* scale, const int* active_flag, const double** slab_out, int64_t* stride_out, int* SK_out);
int msdp_dense_gemm_side(msdp_handle h, const double* M, const double* X, double scale, const int* active_flag, SideJob sj,
                         int* njobs_out, const double** slab_out, int64_t* stride_out, int* SK_out);
// msdp_densesym.hip
int msdp_densesym_eligible(msdp_handle h, int nmat);
int msdp_densesym_reserve(msdp_handle h, int nmat, size_t* slabs_out);
int msdp_densesym_gemm(msdp_handle h, hipStream_t stream, int nmat, const double* const* M, const double* const* X, const double* scale, const int* active_flag);
void msdp_densesym_release(msdp_handle h);
// msdp_affine.hip: the closures of the affine kinds, and the operator's launchers (`a` is the caller's copy of AffineState::a with
// p and ld of the current factor; skipped when *flag == when)
int msdp_affine_costgrad(msdp_handle h, int slot);
int msdp_affine_hess(msdp_handle h);
int msdp_affine_linesearch_cost(msdp_handle h, const double* Yt, double* val);
int msdp_affine_al_primal(msdp_handle h, double* obj, double* Ax_host);
int msdp_affine_al_dual(msdp_handle h, const double* y_host, double* z_host);
void msdp_affine_algo_cost(msdp_handle h, double* bytes, double* flops);
int msdp_sphere_hess_raw(msdp_handle h, const double* slab, int64_t stride, int SK);
int msdp_affine_launch_A(msdp_handle h, AffineDev& a, int64_t nnz, const double* Ya, const double* Yb, const int* flag, int when,
                         int mode, double* axb_out, double sigma, int* G2_out = nullptr);                    // w = A(Ya Yb')
int msdp_affine_launch_adjoint(msdp_handle h, const AffineDev& a, const double* base, const double* vec, double scale, double* out,
                               const int* flag, int when, bool restricted_ok);                               // out = base + scale * At*vec
int msdp_affine_gemm(msdp_handle h, int nmat, const double* const* M, const double* const* X, const double* scale,
                     const int* active_flag, const double** slab_out, int64_t* stride_out, int* SK_out);      // sum_m scale_m M_m X_m -> slabs
int msdp_affine_gram(msdp_handle h, const double* Ya, const double* Yb, double* W, const int* flag, int when);   // W = Ya*Yb' in the handle's storage
int msdp_affine_rowdot_slabs(msdp_handle h, const double* Yl, const double* slab, int64_t stride, int SK, double scale_out,
                             double* dst, double* rowdot_out, int which);                                    // k_rowdot_slabs
int msdp_affine_grad_finish(msdp_handle h, bool oblique, int slot, double sigma, const double* f_given);     // k_obl_grad_finish / k_sph_grad_finish
// msdp_affine_setup.hip
int msdp_affine_setup(msdp_handle h, const int64_t* jc, const int64_t* ir, const double* pr, const double* b, const double* c);
int msdp_affine_setup_blocked(msdp_handle h, int nb, const int64_t* block_n, const int64_t* jc, const int64_t* ir, const double* pr,
                              const double* b, const double* c);   // multiblock kind, per-block storage
void msdp_affine_release(msdp_handle h);
int msdp_affine_set_multipliers(msdp_handle h, const double* y, double sigma);
int msdp_affine_get_block(msdp_handle h, int64_t row0, int64_t nbk, double* S);
int msdp_affine_block_source(msdp_handle h, int64_t row0, int64_t n, int64_t* off, int64_t* ld);   // per-block storage
// msdp_dual.hip
int msdp_dual_setup(msdp_handle h, const int64_t* at_jc, const int64_t* at_ir, const double* at_pr, const double* b, const double* c,
                    const double* dAAt, int32_t nf, const int64_t* b_jc, const int64_t* b_ir, const double* b_pr, const double* cf, bool generic);
void msdp_dual_release(DualState* ds);
int msdp_dual_costgrad(msdp_handle h, AffineState* st, int slot);      // what the msdp_affine_* closures run on a dual handle
int msdp_dual_hess(msdp_handle h, AffineState* st);
int msdp_dual_linesearch_cost(msdp_handle h, AffineState* st, const double* Yt, double* val);
int msdp_dual_set_zrows(msdp_handle h, int64_t zrows);
int msdp_dual_g_identity(msdp_handle h);
int msdp_dual_set_penalty_impl(msdp_handle h, double sigma, const double* wf_host);
int msdp_dual_outer_step_impl(msdp_handle h, double* scal_host, double* Af_host, double* z_host);
int msdp_dual_get_y_impl(msdp_handle h, double* y_host);
// msdp_escape.hip, msdp_lanczos.hip, msdp_blockeig.hip
int msdp_escape_impl(msdp_handle h, int k, double tol, int maxit, double* lam, double* V, double* lmax, int* iters, const double* Mdev);
void msdp_escape_workspace_park(double* ptr, size_t cap_doubles);
size_t msdp_lanczos_slot_bytes();
int msdp_lanczos_persist_ok(msdp_handle h, int nq, const int* full_csr);
int msdp_lanczos_persist_run(msdp_handle h, const double* z, const double* Q, int nq, double* V, double* X, double* dalpha,
                             double* dbeta, unsigned long long* slots, int* err, int m0, int m1, const int* rp, const int* ci, const double* cv);
int msdp_blockeig_eligible(msdp_handle h, const double* Mdev, bool w_loc);
int msdp_blockeig_run(msdp_handle h, int n, const int* rp, const int* ci, const double* cv, const double* z, bool own_rows,
                      const double* Ypt, int ld, int p, int k, double tol, int maxdeg, double lmax, double lmax_res, double lmin_est,
                      bool cold, bool use_y, double* lam, double* V_dev, int* degree_out, bool* conv_out, double* err_out, double* lower_out, const double* Mdense);
void msdp_blockeig_release(msdp_handle h);
// msdp_beritz.hip: H c = theta G c of a Rayleigh-Ritz stage in one workgroup; the status it leaves in its result record
#define MSDP_RITZ_OK 0
#define MSDP_RITZ_FALLBACK 1          // dependent columns (failed Cholesky pivot) or Jacobi not converged: the host stage decides
#define MSDP_RITZ_BREAKDOWN 2         // non-finite entry or max diag G <= 0
int msdp_beritz_supported(int b);
int msdp_beritz_launch(hipStream_t stream, int b, const double* gout, double* Wd, double* rec);
// msdp_blockjacobi.hip, msdp_blockreshape.hip
void msdp_block_eigs_release(msdp_handle h);                  // (the workspace is shared with msdp_block_reshape)
int msdp_block_reshape_run(msdp_handle h, int cur, int nb, const int64_t* nblk, const int32_t* p_in, const double* w, const double* V,
                           int k, double theta, int strict, int delta, double alpha, int min_facsize, int mode, int nob,
                           int32_t* p_out, int32_t* r_out, int32_t* nne_out, int* p_new);
int msdp_block_reshape_maxp();
