// msdp_device.h -- device-side helpers shared by the kernel translation units.
//
// Reductions use DPP (data-parallel primitives on the VALU) instead of __shfl:
// on gfx950 a __shfl_xor of a double is two ds_bpermute round trips through the
// LDS pipe per step (measured: three workgroup sums added 4 us to a 6.8 us
// streaming kernel); the DPP forms are plain VALU moves.
#pragma once
#include "msdp_common.h"
#include "msdp_tr_rules.h"

// Windowed row traversal for gather kernels on vectors larger than the L2s (sweep != 0).  With msdp_chunk_rows every workgroup
// streams through its own chunk: the 64 workgroups of an XCD walk 64 windows that lie one chunk apart, and a row a neighbour
// row's gather brought into the L2 is gone long before its owner reaches it -- the two-launch tCG head, which gathers three
// vectors, fetched 2.66 GB for 1.28 GB of vectors at n = 10^6 (profiles/r3_pmc_chunked_n1e6_p32.json).  Here the workgroups of
// an XCD that are resident TOGETHER (32: one 1024-thread workgroup per CU; a grid of 512 runs as two phases, each on its own
// half of the XCD's rows) take consecutive blocks of BR rows and advance by 32 blocks: one window of 32*BR rows plus the
// graph's halo per XCD, which its 4-MB L2 holds.  Loop shape: for (row0 = lo + wave*RPW; row0 < hi; row0 += stride).
__device__ __forceinline__ void msdp_sweep_rows(int n_loc, int G, int BR, int& lo, int& hi, int& stride) {
    const int X = blockIdx.x & 7, s = blockIdx.x >> 3, S = G >> 3;
    const int W = S < 32 ? S : 32, P = (S + W - 1) / W;
    const int phase = s / W, sp = s - phase * W;
    const int xlo = (int)((int64_t)n_loc * X / 8), xhi = (int)((int64_t)n_loc * (X + 1) / 8);
    // phases split the XCD's rows at multiples of BR so that no block straddles two phases
    const int nb = (xhi - xlo + BR - 1) / BR;
    const int b0 = (int)((int64_t)nb * phase / P), b1 = (int)((int64_t)nb * (phase + 1) / P);
    lo = xlo + (b0 + sp) * BR;
    hi = xlo + b1 * BR < xhi ? xlo + b1 * BR : xhi;
    stride = W * BR;
}

// Workgroup b -> row chunk.  Workgroups b and b+8 share an XCD (round-robin
// dispatch, observed; a pure speed heuristic), so XCD x gets the contiguous
// chunk range [x*G/8, (x+1)*G/8): its L2 then serves one contiguous 1/8 of the
// rows of every vector.  G is a multiple of 8.
__device__ __forceinline__ void msdp_chunk_rows(int n_loc, int G, int& lo, int& hi, int plain = 0, int bx = -1) {
    const int b = bx < 0 ? (int)blockIdx.x : bx;            // bx: the workgroup's index inside ITS rank's share of a combined launch
    const int c = plain ? b : (b & 7) * (G >> 3) + (b >> 3);
    // balanced split with one 32-bit division (a 64-bit n_loc*c/G costs ~350 instructions of preamble in
    // every launch): the first n_loc % G chunks get one extra row
    const unsigned q = (unsigned)n_loc / (unsigned)G, r = (unsigned)n_loc - q * (unsigned)G;
    lo = (int)(c * q + ((unsigned)c < r ? (unsigned)c : r));
    hi = lo + (int)q + ((unsigned)c < r ? 1 : 0);
}

// v moved by a DPP control (both halves of the double).
template <int CTRL>
__device__ __forceinline__ double msdp_dpp(double v) {
    const long long b = __double_as_longlong(v);
    int lo = (int)(b & 0xffffffffLL), hi = (int)(b >> 32);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}
// The same exchange where EVERY lane of the row is active (workgroup-uniform control flow) and CTRL is a permutation inside the row
// (quad_perm, row_mirror, row_half_mirror, row_ror): every lane receives a value, so the destination needs no initial contents -- with
// old = the source, as above, the compiler copies each half into the destination first (two v_mov_b32 per exchange on the dependent
// chain of a group sum).  Same values; bound_ctrl never applies since no source lane is invalid.
template <int CTRL>
__device__ __forceinline__ double msdp_dpp_all(double v) {
    const long long b = __double_as_longlong(v);
    int lo = (int)(b & 0xffffffffLL), hi = (int)(b >> 32);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}
#define MSDP_DPP_XOR1 0xB1          // quad_perm [1,0,3,2]
#define MSDP_DPP_XOR2 0x4E          // quad_perm [2,3,0,1]
#define MSDP_DPP_HALF_MIRROR 0x141  // lane i <-> 7-i inside each 8 lanes
#define MSDP_DPP_MIRROR 0x140       // lane i <-> 15-i inside each 16-lane row

__device__ __forceinline__ double msdp_readlane(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

template <int W>
__device__ __forceinline__ double msdp_rowpair_sum(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)(b & 0xffffffffLL), hi = (unsigned)((unsigned long long)b >> 32);
    unsigned l0, l1, h0, h1;
    if (W == 16) {
        const auto rl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto rh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        l0 = rl[0]; l1 = rl[1]; h0 = rh[0]; h1 = rh[1];
    } else {
        const auto rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        l0 = rl[0]; l1 = rl[1]; h0 = rh[0]; h1 = rh[1];
    }
    const double a = __longlong_as_double((long long)(((unsigned long long)h0 << 32) | l0));
    const double c = __longlong_as_double((long long)(((unsigned long long)h1 << 32) | l1));
    return a + c;
}

// Sum over the LPR consecutive lanes that serve one row; valid in every lane of the
// group.  All lanes of a group must be active together (they are: a group = a row).
template <int LPR>
__device__ __forceinline__ double msdp_group_sum(double v) {
    if (LPR >= 2) v += msdp_dpp<MSDP_DPP_XOR1>(v);
    if (LPR >= 4) v += msdp_dpp<MSDP_DPP_XOR2>(v);
    if (LPR >= 8) v += msdp_dpp<MSDP_DPP_HALF_MIRROR>(v);
    if (LPR >= 16) v += msdp_dpp<MSDP_DPP_MIRROR>(v);
    // gfx950: v_permlane16_swap / v_permlane32_swap exchange 16- / 32-lane rows in the VALU (a __shfl_xor across
    // rows is a ds_bpermute round trip through the LDS crossbar).  swap(v, v) returns {even-row value everywhere in
    // the pair, odd-row value everywhere in the pair}; both rows add them in the same order.
    if (LPR >= 32) v = msdp_rowpair_sum<16>(v);
    if (LPR >= 64) v = msdp_rowpair_sum<32>(v);
    return v;
}

// msdp_group_sum for callers in workgroup-uniform control flow (all lanes active): same exchanges, same order of the additions
template <int LPR>
__device__ __forceinline__ double msdp_group_sum_all(double v) {
    if (LPR >= 2) v += msdp_dpp_all<MSDP_DPP_XOR1>(v);
    if (LPR >= 4) v += msdp_dpp_all<MSDP_DPP_XOR2>(v);
    if (LPR >= 8) v += msdp_dpp_all<MSDP_DPP_HALF_MIRROR>(v);
    if (LPR >= 16) v += msdp_dpp_all<MSDP_DPP_MIRROR>(v);
    if (LPR >= 32) v = msdp_rowpair_sum<16>(v);
    if (LPR >= 64) v = msdp_rowpair_sum<32>(v);
    return v;
}

// Full-wave sum (all 64 lanes active), same value in every lane, fixed order.
__device__ __forceinline__ double msdp_wave_sum(double v) {
    v += msdp_dpp<MSDP_DPP_XOR1>(v);
    v += msdp_dpp<MSDP_DPP_XOR2>(v);
    v += msdp_dpp<MSDP_DPP_HALF_MIRROR>(v);
    v += msdp_dpp<MSDP_DPP_MIRROR>(v);
    const double r0 = msdp_readlane(v, 0), r1 = msdp_readlane(v, 16);
    const double r2 = msdp_readlane(v, 32), r3 = msdp_readlane(v, 48);
    return ((r0 + r1) + r2) + r3;
}

// Deterministic workgroup sum; result valid in every thread (one barrier pair).
__device__ __forceinline__ double msdp_block_sum(double v, double* sh /* >= MSDP_WAVES doubles */) {
    v = msdp_wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    double s = 0.0;
    const int nw = blockDim.x >> 6;
    for (int i = 0; i < nw; ++i) s += sh[i];
    return s;
}

// Up to three per-workgroup partial sums with ONE barrier.  sh (>= 3*MSDP_WAVES
// doubles) must not be in use by another phase of the kernel.
__device__ __forceinline__ void msdp_put_partials3(double* P, int w0, double a, int w1, double b, int w2, double c,
                                                   double* sh) {
    a = msdp_wave_sum(a);
    if (w1 >= 0) b = msdp_wave_sum(b);
    if (w2 >= 0) c = msdp_wave_sum(c);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[w] = a; sh[MSDP_WAVES + w] = b; sh[2 * MSDP_WAVES + w] = c; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int which = threadIdx.x == 0 ? w0 : (threadIdx.x == 1 ? w1 : w2);
        if (which >= 0) {
            double s = 0.0;
            const int nw = blockDim.x >> 6;
            for (int i = 0; i < nw; ++i) s += sh[threadIdx.x * MSDP_WAVES + i];
            P[which * MSDP_MAX_GRID + blockIdx.x] = s;
        }
    }
}
__device__ __forceinline__ void msdp_put_partial(double* P, int which, double v, double* sh) {
    msdp_put_partials3(P, which, v, -1, 0.0, -1, 0.0, sh);
}

// Every WAVE re-reduces the <= 512 partials of the previous launch in the same fixed
// order (no LDS, no barrier): all waves, workgroups and ranks obtain bit-identical
// sums and therefore take identical decisions without atomics or fences.
__device__ __forceinline__ double msdp_sum_partials(const double* P, int which, int G) {
    const double* a = P + which * MSDP_MAX_GRID;
    const int lane = threadIdx.x & 63;
    double v = 0.0;
    for (int i = lane; i < G; i += 64) v += a[i];
    return msdp_wave_sum(v);
}

// Block-level variant: wave 0 re-reduces, everyone reads the result from LDS (one barrier);
// 16x fewer same-address requests to the L2 channels that hold the partials.
__device__ __forceinline__ double msdp_sum_partials_block(const double* P, int which, int G, double* shb) {
    if (threadIdx.x < 64) {
        const double s = msdp_sum_partials(P, which, G);
        if (threadIdx.x == 0) shb[0] = s;
    }
    __syncthreads();
    return shb[0];
}
__device__ __forceinline__ void msdp_sum_partials3_block(const double* P, int w0, int w1, int w2, int G, double* shb,
                                                         double& s0, double& s1, double& s2) {
    if (threadIdx.x < 64) {
        const double a = msdp_sum_partials(P, w0, G), b = msdp_sum_partials(P, w1, G), c = msdp_sum_partials(P, w2, G);
        if (threadIdx.x == 0) { shb[0] = a; shb[1] = b; shb[2] = c; }
    }
    __syncthreads();
    s0 = shb[0]; s1 = shb[1]; s2 = shb[2];
}

__device__ __forceinline__ double2 ld2(const double* p) { return *reinterpret_cast<const double2*>(p); }
__device__ __forceinline__ void st2(double* p, double2 v) { *reinterpret_cast<double2*>(p) = v; }
// streaming accesses (nt: the line is not kept by the L2 beyond its use) for the operands a gather kernel touches exactly once,
// so that the rows other workgroups gather stay resident
typedef double msdp_d2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 ld2_nt(const double* p) {
    const msdp_d2v v = __builtin_nontemporal_load(reinterpret_cast<const msdp_d2v*>(p));
    return make_double2(v.x, v.y);
}
__device__ __forceinline__ void st2_nt(double* p, double2 v) {
    const msdp_d2v w = {v.x, v.y};
    __builtin_nontemporal_store(w, reinterpret_cast<msdp_d2v*>(p));
}

// Publish tCG progress to the host-mapped status word (one relaxed system-scope store by
// the lead thread): the host polls it to decide whether to enqueue another chunk.
__device__ __forceinline__ void msdp_publish(const Dev& d, int k, int j, int active) {
    if (!d.status) return;
    // bit 30 of the j field carries ctl->done so that the host can stop enqueuing TR iterations without a sync
    const unsigned jj = ((unsigned)j & 0x3fffffffu) | (d.ctl->done ? 0x40000000u : 0u);
    const unsigned long long v = ((unsigned long long)(unsigned)(k + 1) << 32) |
                                 ((unsigned long long)jj << 1) | (unsigned long long)(active & 1);
    __hip_atomic_store(d.status, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Frame fields are read one by one into scalars and written field by field by the lead
// thread: a by-value Frame copy is lowered through per-thread LDS/scratch by hipcc and
// cost 10 us per launch (measured: 19.3 -> 9.4 us for k_tcg_upd1).
__device__ __forceinline__ void frame_store(Frame* o, double z_r, double d_Pd, double e_Pd, double e_Pe,
                                            double model_value, double norm_r0, double alpha, double beta,
                                            int active, int j, int stop, int eta_idx, int md_idx = 0, int fresh = 0) {
    o->z_r = z_r; o->d_Pd = d_Pd; o->e_Pd = e_Pd; o->e_Pe = e_Pe; o->model_value = model_value;
    o->norm_r0 = norm_r0; o->alpha = alpha; o->beta = beta;
    o->active = active; o->j = j; o->stop = stop; o->eta_idx = eta_idx; o->md_idx = md_idx; o->fresh = fresh;
}


// Sum of the SK split-K slabs at offset o (two doubles), in slab order.  Four loads are requested together: with a
// plain loop hipcc keeps one load in flight per lane (SK is a run-time value), and the epilogues are latency-bound.
__device__ __forceinline__ double2 msdp_sum_slabs(const double* __restrict__ slab, int64_t slab_stride, int SK, int64_t o) {
    double2 acc = make_double2(0.0, 0.0);
    int s = 0;
    // eight, then four, then the last <= 3 loads in flight together; the additions stay in slab order (same bits as a plain loop).
    // Round 3: the affine Hess-vec of BQP d = 60 sums 26 slabs -- seven dependent round trips with batches of four.
    for (; s + 8 <= SK; s += 8) {
        double2 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = ld2(slab + (int64_t)(s + q) * slab_stride + o);
#pragma unroll
        for (int q = 0; q < 8; ++q) { acc.x += v[q].x; acc.y += v[q].y; }
    }
    if (s + 4 <= SK) {
        double2 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = ld2(slab + (int64_t)(s + q) * slab_stride + o);
#pragma unroll
        for (int q = 0; q < 4; ++q) { acc.x += v[q].x; acc.y += v[q].y; }
        s += 4;
    }
    if (s < SK) {
        double2 v[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) v[q] = (s + q < SK) ? ld2(slab + (int64_t)(s + q) * slab_stride + o) : make_double2(0.0, 0.0);
#pragma unroll
        for (int q = 0; q < 3; ++q) if (s + q < SK) { acc.x += v[q].x; acc.y += v[q].y; }
    }
    return acc;
}

// ------------------------------------------------------------------ sparse gather
// acc[ch] += sum_k C[row,k] * X[k, cols of this lane]; the LPR lanes of a row each
// fetch one (col,val) pair of the CSR row (coalesced) and broadcast it by shuffle.
#define MSDP_ELL_MAXW 8
template <int LPR, int NCH, bool ELL>
__device__ __forceinline__ void spmm_row(const Dev& d, int row, int sub, const double* __restrict__ X,
                                         double2 (&acc)[NCH]) {
    if (ELL) {
        // ELL slices ([w][row], padded with (row, 0.0)): no rowptr in the dependency chain, all (col,val)
        // loads of a row are independent and coalesced across the rows of a wave, and all W neighbour-row
        // gathers are in flight together: two dependent memory round trips instead of three.
        int c[MSDP_ELL_MAXW];
        double v[MSDP_ELL_MAXW];
#pragma unroll
        for (int w = 0; w < MSDP_ELL_MAXW; ++w) {
            const bool ok = w < d.ellW;
            c[w] = ok ? d.ellc[(int64_t)w * d.ell_stride + row] : row;
            v[w] = ok ? d.ellv[(int64_t)w * d.ell_stride + row] : 0.0;
        }
#pragma unroll
        for (int w = 0; w < MSDP_ELL_MAXW; ++w) {
            if (w < d.ellW) {
                const double* src = X + (int64_t)c[w] * d.ld + 2 * sub;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    if (2 * sub + ch * 2 * LPR < d.ld) {
                        const double2 x = ld2(src + ch * 2 * LPR);
                        acc[ch].x = fma(v[w], x.x, acc[ch].x);
                        acc[ch].y = fma(v[w], x.y, acc[ch].y);
                    }
                }
            }
        }
        return;
    }
    // CSR: all LPR lanes of a row read the same (col,val) pair: one L1 line per row serves the
    // whole group, the loads are independent of each other (no shuffle in the chain) and
    // the compiler can keep 4 neighbour rows in flight per lane.
    const int start = d.rowptr[row], end = d.rowptr[row + 1];
    const int* __restrict__ ci = d.colind;
    const double* __restrict__ cv = d.cval;
#pragma unroll 4
    for (int k = start; k < end; ++k) {
        const int c = ci[k];
        const double v = cv[k];
        const double* src = X + (int64_t)c * d.ld + 2 * sub;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            if (2 * sub + ch * 2 * LPR < d.ld) {
                const double2 x = ld2(src + ch * 2 * LPR);
                acc[ch].x = fma(v, x.x, acc[ch].x);
                acc[ch].y = fma(v, x.y, acc[ch].y);
            }
        }
    }
}

// The same gather for a Hermitian C = A + iB (COST_HERM, msdp_hermitian.hip): the values are complex (d.hzv / d.hzell) and a
// double2 of X is one complex number, acc += c * x.  Entries in ascending column order, the real-part product first: with
// B = 0 the sums carry the bits of spmm_row.
template <int LPR, int NCH, bool ELL>
__device__ __forceinline__ void spmm_row_herm(const Dev& d, int row, int sub, const double* __restrict__ X,
                                              double2 (&acc)[NCH]) {
    if (ELL) {
        int c[MSDP_ELL_MAXW];
        double2 v[MSDP_ELL_MAXW];
#pragma unroll
        for (int w = 0; w < MSDP_ELL_MAXW; ++w) {
            const bool ok = w < d.ellW;
            c[w] = ok ? d.ellc[(int64_t)w * d.ell_stride + row] : row;
            v[w] = ok ? d.hzell[(int64_t)w * d.ell_stride + row] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int w = 0; w < MSDP_ELL_MAXW; ++w) {
            if (w < d.ellW) {
                const double* src = X + (int64_t)c[w] * d.ld + 2 * sub;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    if (2 * sub + ch * 2 * LPR < d.ld) {
                        const double2 x = ld2(src + ch * 2 * LPR);
                        acc[ch].x = fma(v[w].x, x.x, acc[ch].x); acc[ch].x = fma(-v[w].y, x.y, acc[ch].x);
                        acc[ch].y = fma(v[w].x, x.y, acc[ch].y); acc[ch].y = fma(v[w].y, x.x, acc[ch].y);
                    }
                }
            }
        }
        return;
    }
    const int start = d.rowptr[row], end = d.rowptr[row + 1];
    const int* __restrict__ ci = d.colind;
    const double2* __restrict__ cv = d.hzv;
#pragma unroll 4
    for (int k = start; k < end; ++k) {
        const int c = ci[k];
        const double2 v = cv[k];
        const double* src = X + (int64_t)c * d.ld + 2 * sub;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            if (2 * sub + ch * 2 * LPR < d.ld) {
                const double2 x = ld2(src + ch * 2 * LPR);
                acc[ch].x = fma(v.x, x.x, acc[ch].x); acc[ch].x = fma(-v.y, x.y, acc[ch].x);
                acc[ch].y = fma(v.x, x.y, acc[ch].y); acc[ch].y = fma(v.y, x.x, acc[ch].y);
            }
        }
    }
}

// ------------------------------------------------------------------ stacked Stiefel manifold (MANI_STIEFEL, msdp_stiefel.hip)
// The gather of a block row of a block-CSR cost matrix (COST_BLOCK): a lane group owns the D rows of block `blk`, NCH double2
// each.  Per entry the D x D values are read once (the same addresses in every lane of the group: one L1 line), the D
// contiguous rows of the neighbour block are gathered once and each is used D times: acc[a] += sum_b c[a][b] * x[b].
// Entries in ascending block-column order, b ascending inside an entry.  UN entries are in flight together (1 where the caller
// holds three vectors of the block in registers and D = 3: two would spill at 128 registers per lane).
template <int D, int LPR, int NCH, int UN = 2>
__device__ __forceinline__ void spmm_block(const Dev& d, int blk, int sub, const double* __restrict__ X,
                                           double2 (&acc)[D][NCH]) {
    const int start = d.brp[blk], end = d.brp[blk + 1];
    const int* __restrict__ ci = d.bci;
    const double* __restrict__ cv = d.bval;
#pragma unroll UN
    for (int k = start; k < end; ++k) {
        const int j = ci[k];
        double c[D][D];
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = 0; b < D; ++b) c[a][b] = cv[(int64_t)k * (D * D) + a * D + b];
        const double* src = X + (int64_t)j * D * d.ld + 2 * sub;
        double2 x[D][NCH];
#pragma unroll
        for (int b = 0; b < D; ++b)
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
                x[b][ch] = (2 * sub + ch * 2 * LPR < d.ld) ? ld2(src + (int64_t)b * d.ld + ch * 2 * LPR) : make_double2(0.0, 0.0);
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = 0; b < D; ++b)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    acc[a][ch].x = fma(c[a][b], x[b][ch].x, acc[a][ch].x);
                    acc[a][ch].y = fma(c[a][b], x[b][ch].y, acc[a][ch].y);
                }
    }
}

// The same gather (one double2 per lane and row, NCH = 1) where the rows of X are read through an accessor of the caller:
// ldx(byte offset) -> double2.  The persistent kernel of the block kinds (msdp_blockpersist.hip) gathers rows that other
// workgroups stored during the same launch and passes the agent-coherent load of msdp_psync.h; a plain ld2 may see an XCD's
// stale L2 line there.  [k0, k1) = the entries of the block row (empty for a lane group without a block), col_bytes = the byte
// offset of the lane's columns in a row, ld = the row stride in doubles.  Entries and products in the order of spmm_block.
// CB entries are in flight together: their CB column indices are loaded first, then their CB * D rows, and only then the
// values row by row -- a chain of two dependent round trips per BATCH where a loop over single entries pays them per entry (the
// caller holds the vectors of its blocks in registers and runs two waves per SIMD: nothing else hides the latency).  The tail
// of the last batch reads the row's last entry again and leaves it out of the sums.
typedef double msdp_d2u __attribute__((ext_vector_type(2), aligned(8)));      // two doubles at an 8-byte aligned address
template <int D, int CB, class LoadX>
__device__ __forceinline__ void spmm_block_via(const Dev& d, int k0, int k1, unsigned col_bytes, unsigned ld, LoadX ldx, double2 (&acc)[D]) {
    const int* __restrict__ ci = d.bci;
    const double* __restrict__ cv = d.bval;
    for (int k = k0; k < k1; k += CB) {
        int j[CB];
#pragma unroll
        for (int u = 0; u < CB; ++u) j[u] = ci[k + u < k1 ? k + u : k1 - 1];
        double2 x[CB][D];
#pragma unroll
        for (int u = 0; u < CB; ++u)
#pragma unroll
            for (int b = 0; b < D; ++b) x[u][b] = ldx(((unsigned)j[u] * (unsigned)D + (unsigned)b) * ld * 8u + col_bytes);
#pragma unroll
        for (int u = 0; u < CB; ++u) {
            if (k + u < k1) {
                // the D * D values of the entry, two doubles per load: every lane of a group reads the same addresses, and a wave
                // of 64 / LPR groups touches as many lines per load instruction -- the count of these instructions is what the
                // gather costs.  Even D: row by row (the caller's registers are full), 16-byte aligned pairs; odd D: the entry's
                // values as one run of D * D doubles, 8-byte aligned pairs and a last single
                const double* __restrict__ ce = cv + (int64_t)(k + u) * (D * D);
                if (D % 2 == 0) {
#pragma unroll
                    for (int a = 0; a < D; ++a) {
                        double c[D];
#pragma unroll
                        for (int b = 0; b < D; b += 2) { const double2 cc = ld2(ce + a * D + b); c[b] = cc.x; c[b + 1 < D ? b + 1 : b] = cc.y; }
#pragma unroll
                        for (int b = 0; b < D; ++b) {
                            acc[a].x = fma(c[b], x[u][b].x, acc[a].x);
                            acc[a].y = fma(c[b], x[u][b].y, acc[a].y);
                        }
                    }
                } else {
                    double c[D * D];
#pragma unroll
                    for (int q = 0; q + 1 < D * D; q += 2) { const msdp_d2u cc = *reinterpret_cast<const msdp_d2u*>(ce + q); c[q] = cc.x; c[q + 1] = cc.y; }
                    c[D * D - 1] = ce[D * D - 1];
#pragma unroll
                    for (int a = 0; a < D; ++a)
#pragma unroll
                        for (int b = 0; b < D; ++b) {
                            acc[a].x = fma(c[a * D + b], x[u][b].x, acc[a].x);
                            acc[a].y = fma(c[a * D + b], x[u][b].y, acc[a].y);
                        }
                }
            }
        }
    }
}

// T = sym(A B') of the leading D rows of two blocks held by a lane group (RA / RB = D, or D + 1 where a block ends in a free
// row: the pose-graph kind, d.efree = 1): T[a][b] = (<A_a, B_b> + <A_b, B_a>) / 2, D (D + 1) / 2 group sums; the same bits in
// every lane of the group
template <int D, int LPR, int NCH, int RA, int RB>
__device__ __forceinline__ void msdp_block_symdot(const double2 (&A)[RA][NCH], const double2 (&B)[RB][NCH], double (&T)[D][D]) {
    static_assert(RA >= D && RB >= D, "blocks of at least D rows");
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = a; b < D; ++b) {
            double s = 0.0;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                s += A[a][ch].x * B[b][ch].x + A[a][ch].y * B[b][ch].y;
                if (b != a) s += A[b][ch].x * B[a][ch].x + A[b][ch].y * B[a][ch].y;
            }
            s = msdp_group_sum<LPR>(s);
            T[a][b] = T[b][a] = (b != a) ? 0.5 * s : s;
        }
}

// Workgroup size of the row kernels of the block kinds (msdp_stiefel.hip, msdp_pose_precon.hip; B = the rows of a block): 16
// waves hide the gather latency where a block fits 128 registers per lane (NCH = 1, widths up to 128); two chunks per lane
// (widths up to 256) take 8 waves and twice the registers.  A kernel that keeps THREE vectors of a block resident beside the
// B x B values of an entry (the Hess-vec: w, u, y; the preconditioned first update: r, z, y) takes 126-137 registers at B = 4
// and spilled at the 128 of a 16-wave workgroup: its one-chunk instances run 8 waves there (DESIGN.md section 4 has the table)
template <int B, int NCH> struct BlockRows { static constexpr int threads = NCH == 1 ? 1024 : 512; };
template <int B, int NCH> struct BlockRows3 { static constexpr int threads = (NCH == 1 && B < 4) ? 1024 : 512; };

// The width ladder of the block kinds: one kernel instance <LPR_, NCH_> per lanes-per-block count of the row stride ld_, widths
// up to 2 * 64 * 2 = 256.  The arguments after ld_ are the caller's launch statement, which names LPR_ and NCH_.  The macro
// ends in `else`: the statement that follows it is what the caller does with a wider stride,
//     MSDP_BLOCK_WIDTH_LADDER(ld, hipLaunchKernelGGL((k<LPR_, NCH_>), ...)) { msdp_set_error(...); return MSDP_EUNSUPPORTED; }
#define MSDP_BLOCK_WIDTH_RUNG(L, N, ...) { constexpr int LPR_ = L, NCH_ = N; __VA_ARGS__; }
#define MSDP_BLOCK_WIDTH_LADDER(ld_, ...)                                    \
    if ((ld_) / 2 <= 1) MSDP_BLOCK_WIDTH_RUNG(1, 1, __VA_ARGS__)             \
    else if ((ld_) / 2 <= 2) MSDP_BLOCK_WIDTH_RUNG(2, 1, __VA_ARGS__)        \
    else if ((ld_) / 2 <= 4) MSDP_BLOCK_WIDTH_RUNG(4, 1, __VA_ARGS__)        \
    else if ((ld_) / 2 <= 8) MSDP_BLOCK_WIDTH_RUNG(8, 1, __VA_ARGS__)        \
    else if ((ld_) / 2 <= 16) MSDP_BLOCK_WIDTH_RUNG(16, 1, __VA_ARGS__)      \
    else if ((ld_) / 2 <= 32) MSDP_BLOCK_WIDTH_RUNG(32, 1, __VA_ARGS__)      \
    else if ((ld_) / 2 <= 64) MSDP_BLOCK_WIDTH_RUNG(64, 1, __VA_ARGS__)      \
    else if ((ld_) / 2 <= 128) MSDP_BLOCK_WIDTH_RUNG(64, 2, __VA_ARGS__)     \
    else

// R = G^(-1/2) of a symmetric positive definite D x D matrix in registers (the polar retraction: G = A A' of a block A = Y + eta,
// G = I + eta eta' >= I for tangent eta).  Symmetric eigen-decomposition by Jacobi rotations -- for D = 2 a single rotation is
// the closed form; D = 3 runs cyclic sweeps until the off-diagonal part is below rounding (|off|^2 <= 1e-32 |diag|^2), at most
// MSDP_JACOBI_SWEEPS of them (quadratic convergence: four or five in practice).  Every index is a compile-time constant after
// unrolling: the matrices stay in registers.
#define MSDP_JACOBI_SWEEPS 12
template <int D>
__device__ __forceinline__ void msdp_sym_invsqrt(const double (&G)[D][D], double (&R)[D][D]) {
    double A[D][D], V[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) { A[a][b] = G[a][b]; V[a][b] = (a == b) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < (D == 2 ? 1 : MSDP_JACOBI_SWEEPS); ++sweep) {
        if (D > 2) {
            double off = 0.0, dg = 0.0;
#pragma unroll
            for (int a = 0; a < D; ++a) {
                dg += A[a][a] * A[a][a];
#pragma unroll
                for (int b = a + 1; b < D; ++b) off += A[a][b] * A[a][b];
            }
            if (off <= 1e-32 * dg) break;
        }
#pragma unroll
        for (int p = 0; p < D; ++p)
#pragma unroll
            for (int q = p + 1; q < D; ++q) {
                const double apq = A[p][q];
                if (apq != 0.0) {
                    const double th = (A[q][q] - A[p][p]) / (2.0 * apq);
                    const double t = copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    A[p][p] -= t * apq; A[q][q] += t * apq;
                    A[p][q] = A[q][p] = 0.0;
#pragma unroll
                    for (int r = 0; r < D; ++r) {
                        if (r != p && r != q) {
                            const double arp = A[r][p], arq = A[r][q];
                            A[r][p] = A[p][r] = c * arp - s * arq;
                            A[r][q] = A[q][r] = s * arp + c * arq;
                        }
                        const double vrp = V[r][p], vrq = V[r][q];
                        V[r][p] = c * vrp - s * vrq;
                        V[r][q] = s * vrp + c * vrq;
                    }
                }
            }
    }
    double is[D];
#pragma unroll
    for (int k = 0; k < D; ++k) is[k] = 1.0 / sqrt(A[k][k]);
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = a; b < D; ++b) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) s += V[a][k] * is[k] * V[b][k];
            R[a][b] = R[b][a] = s;
        }
}

// The sibling of msdp_sym_invsqrt for a G that is only positive SEMI-definite in exact arithmetic (msdp_blockfactor.hip: the
// Gram matrix of a block after a rank cut, of a d x d block Y_i W): the same Jacobi iteration (a copy, so that the function
// above and its callers keep their bits), and beside R the eigenvalues lam[] in no particular order -- the caller decides from
// them whether R means anything.  R = V diag(s_k / sqrt(max(lam_k, tiny))) V': never a division by zero; s_k = -1 on the
// smallest eigenvalue when flip_smallest (the nearest ROTATION to a block of negative determinant), 1 elsewhere.
template <int D>
__device__ __forceinline__ void msdp_sym_invsqrt_eig(const double (&G)[D][D], double (&R)[D][D], double (&lam)[D], bool flip_smallest) {
    double A[D][D], V[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) { A[a][b] = G[a][b]; V[a][b] = (a == b) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < (D == 2 ? 1 : MSDP_JACOBI_SWEEPS); ++sweep) {
        if (D > 2) {
            double off = 0.0, dg = 0.0;
#pragma unroll
            for (int a = 0; a < D; ++a) {
                dg += A[a][a] * A[a][a];
#pragma unroll
                for (int b = a + 1; b < D; ++b) off += A[a][b] * A[a][b];
            }
            if (!(off > 1e-32 * dg)) break;                 // (also leaves on a NaN)
        }
#pragma unroll
        for (int p = 0; p < D; ++p)
#pragma unroll
            for (int q = p + 1; q < D; ++q) {
                const double apq = A[p][q];
                if (apq != 0.0) {
                    const double th = (A[q][q] - A[p][p]) / (2.0 * apq);
                    const double t = copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    A[p][p] -= t * apq; A[q][q] += t * apq;
                    A[p][q] = A[q][p] = 0.0;
#pragma unroll
                    for (int r = 0; r < D; ++r) {
                        if (r != p && r != q) {
                            const double arp = A[r][p], arq = A[r][q];
                            A[r][p] = A[p][r] = c * arp - s * arq;
                            A[r][q] = A[q][r] = s * arp + c * arq;
                        }
                        const double vrp = V[r][p], vrq = V[r][q];
                        V[r][p] = c * vrp - s * vrq;
                        V[r][q] = s * vrp + c * vrq;
                    }
                }
            }
    }
    double lmin = A[0][0];
#pragma unroll
    for (int k = 1; k < D; ++k) lmin = fmin(lmin, A[k][k]);
    double is[D];
    bool flipped = !flip_smallest;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        lam[k] = A[k][k];
        is[k] = 1.0 / sqrt(fmax(A[k][k], 2.2250738585072014e-308));
        if (!flipped && A[k][k] == lmin) { is[k] = -is[k]; flipped = true; }      // the first of equal smallest ones
    }
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = a; b < D; ++b) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) s += V[a][k] * is[k] * V[b][k];
            R[a][b] = R[b][a] = s;
        }
}

// tCG.m:227-287, the scalar part of the second update of a three-launch trip (everything an upd2 kernel decides before it
// touches a row): model check, convergence test, loop bound, the new frame -- the rules of msdp_tr_rules.h on the frame F[1]
// -> F[0].  The single reader of F[1] and writer of F[0] of these trips.  Returns true when a new direction
// mdelta = tangent(z + beta mdelta) is due, with beta; false when the tCG has ended (or was not running) -- the frame and the
// progress word are written either way.  PRECON: the fourth sum <z, r> of the preconditioned upd1 (P_ZRN) takes the place of
// r_r in the recurrences (tCG.m:270-287).  Called by every thread of the launch; shb: 4 doubles of LDS.
template <bool PRECON = false>
__device__ __forceinline__ bool msdp_tcg_upd2_scalars(const Dev& d, double* shb, double& beta_out) {
    const Frame* fi = &d.F[1];
    const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
    const int active = fi->active;
    const double z_r = fi->z_r, d_Pd = fi->d_Pd, e_Pd = fi->e_Pd, e_Pe = fi->e_Pe;
    const double model_value = fi->model_value, norm_r0 = fi->norm_r0, beta0 = fi->beta, alpha = fi->alpha;
    const int j0 = fi->j, stop0 = fi->stop, ix = fi->eta_idx;
    if (!active) {
        if (lead) {
            frame_store(&d.F[0], z_r, d_Pd, e_Pd, e_Pe, model_value, norm_r0, alpha, beta0, 0, j0, stop0, ix);
            d.ctl->tcg_running = 0;
            msdp_publish(d, d.ctl->k, j0, 0);
        }
        return false;
    }
    const Ctl* c = d.ctl;
    const bool bench = c->bench_mode != 0;
    double s1, s2, r_r, z_r_new;
    if (PRECON) {
        if (threadIdx.x < 64) {
            const double a = msdp_sum_partials(d.P, P_S1, d.G), b = msdp_sum_partials(d.P, P_S2, d.G);
            const double e = msdp_sum_partials(d.P, P_S3, d.G), f = msdp_sum_partials(d.P, P_ZRN, d.G);
            if (threadIdx.x == 0) { shb[0] = a; shb[1] = b; shb[2] = e; shb[3] = f; }
        }
        __syncthreads();
        s1 = shb[0]; s2 = shb[1]; r_r = shb[2]; z_r_new = shb[3];
    } else {
        msdp_sum_partials3_block(d.P, P_S1, P_S2, P_S3, d.G, shb, s1, s2, r_r);
        z_r_new = r_r;
    }
    const double new_model = s1 + 0.5 * s2;                 // :227
    const int j = j0 + 1;
    if (!bench && !tcg_model_decreased(new_model, model_value)) {
        if (lead) {
            frame_store(&d.F[0], z_r, d_Pd, e_Pd, e_Pe, model_value, norm_r0, alpha, beta0, 0, j, 6, ix);
            d.ctl->tcg_running = 0;
            msdp_publish(d, c->k, j, 0);
        }
        return false;
    }
    const int nix = ix ^ 1;                                 // :233-235 commit new_eta/new_Heta
    const double norm_r = sqrt(r_r);
    const double nr0t = tcg_nr0t(norm_r0, c->theta);
    if (!bench && !tcg_unconverged(j, c->mininner, norm_r, norm_r0, nr0t, c->kappa)) {
        if (lead) {
            frame_store(&d.F[0], z_r, d_Pd, e_Pd, e_Pe, new_model, norm_r0, alpha, beta0, 0, j, tcg_converged_stop(c->kappa, nr0t), nix);
            d.ctl->tcg_running = 0;
            msdp_publish(d, c->k, j, 0);
        }
        return false;
    }
    if (j >= c->maxinner) {                                 // loop bound :160 (stop stays 5)
        if (lead) {
            frame_store(&d.F[0], z_r, d_Pd, e_Pd, e_Pe, new_model, norm_r0, alpha, beta0, 0, j, stop0, nix);
            d.ctl->tcg_running = 0;
            msdp_publish(d, c->k, j, 0);
        }
        return false;
    }
    double n_z_r = z_r, n_e_Pd = e_Pd, n_d_Pd = d_Pd;
    const double beta = tcg_recurrences(z_r_new, alpha, n_z_r, n_e_Pd, n_d_Pd);
    if (lead) {
        frame_store(&d.F[0], n_z_r, n_d_Pd, n_e_Pd, e_Pe, new_model, norm_r0, alpha, beta, 1, j, stop0, nix);
        msdp_publish(d, c->k, j, 1);
    }
    beta_out = beta;
    return true;
}

// trustregions.m:548-729 of the routes whose RTR scalars live in Ctl: rho, the radius, accept or reject, the counters, the
// stopping test.  One thread.  fp, ggp, prd: cost and squared gradient norm at the proposal, <eta, grad + .5 Heta>.
__device__ __forceinline__ void msdp_rtr_decide(Ctl* c, const Frame& f, double fp, double ggp, double prd) {
    const int f_stop = f.stop, f_j = f.j;
    double Delta = c->Delta, rho, rhonum, rhoden;
    const bool accept = rtr_outcome(c->fx, fp, prd, c->rho_reg, c->rho_prime, c->Delta_bar, f_stop, Delta, rho, rhonum, rhoden);
    c->Delta = Delta;
    if (accept) {
        c->cur ^= 1;
        c->fx = fp; c->gg = ggp; c->norm_grad = sqrt(ggp);
        c->accepted++;
    } else {
        c->rejected++;
    }
    c->rho = rho; c->rhonum = rhonum; c->rhoden = rhoden; c->fx_prop = fp; c->gg_prop = ggp;
    c->k++;                                                              // :729
    c->hessvecs += f_j;
    c->cost_evals++;
    c->last_stop_inner = f_stop;
    c->done = rtr_done(c->norm_grad, c->tolgradnorm, c->k, c->maxiter);
}
