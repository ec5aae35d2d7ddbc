// msdp_round.hip -- hyperplane rounding of the unit-diagonal solution to +1/-1 vectors, with 1-opt local search
// (msdp_round_hyperplane).  Not part of the reference: ManiSDP_onlyunitdiag.m returns the bound and the factor only.
//
// Lane = trial.  A wave owns the 64 trials of one mask word and walks rows; whatever belongs to a row (the row of Y, the row of
// C, the neighbours' mask words) is the same for all 64 lanes.  Bit t of M[w * n + i] is set when x_i = -1 in trial 64 w + t.
// No kernel here synchronises across workgroups, no launch does more than one pass over the rows, and nothing of the handle
// is written: the masks, the partial sums and the copy of R live in allocations of the call.
#include "msdp_common.h"
#include <algorithm>

#define ROUND_KT 64          // columns of R per LDS tile (64 x 64 doubles = 32 KB)
#define ROUND_RB 8           // rows per wave and pass
#define ROUND_WAVES 4
#define ROUND_ROWS (ROUND_RB * ROUND_WAVES)

typedef unsigned long long u64;

// x = sign(Y r): lane t forms <Y_i, r_t>, the ballot of (dot < 0) is the mask word of row i (sign(0) = +1).  The row of Y is
// wave-uniform; r_t stays in registers for p <= 8 and is staged in LDS, ROUND_KT columns at a time, otherwise (one pass for
// p <= ROUND_KT).  Grid: (row groups, words); a workgroup takes ROUND_ROWS rows at a time, ROUND_RB per wave.
__global__ __launch_bounds__(ROUND_WAVES * 64) void k_round_signs(const double* __restrict__ Y, int ld, int p, int n,
                                                                  const double* __restrict__ R, u64* __restrict__ M) {
    __shared__ double rt[ROUND_KT * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int w = blockIdx.y;
    const double* Rw = R + (size_t)w * 64 * p;
    u64* Mw = M + (size_t)w * n;
    const int ngroups = (n + ROUND_ROWS - 1) / ROUND_ROWS;
    if (p <= 8) {
        double r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = k < p ? Rw[(size_t)lane * p + k] : 0.0;
        for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
#pragma unroll
            for (int q = 0; q < ROUND_RB; ++q) {
                const int i = g * ROUND_ROWS + wave * ROUND_RB + q;
                if (i >= n) break;
                const double* y = Y + (size_t)i * ld;
                double dot = 0.0;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < p) dot = fma(y[k], r[k], dot);
                const u64 m = __ballot(dot < 0.0);
                if (lane == 0) Mw[i] = m;
            }
        }
        return;
    }
    const int ntiles = (p + ROUND_KT - 1) / ROUND_KT;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        double acc[ROUND_RB];
        const double* yq[ROUND_RB];
#pragma unroll
        for (int q = 0; q < ROUND_RB; ++q) {
            acc[q] = 0.0;
            yq[q] = Y + (size_t)std::min(g * ROUND_ROWS + wave * ROUND_RB + q, n - 1) * ld;   // (rows past n: computed, not stored)
        }
        for (int tile = 0; tile < ntiles; ++tile) {
            const int k0 = tile * ROUND_KT, kn = std::min(ROUND_KT, p - k0);
            if (ntiles > 1 || g == (int)blockIdx.x) {       // one tile: staged once per workgroup
                __syncthreads();
                for (int idx = threadIdx.x; idx < kn * 64; idx += ROUND_WAVES * 64) {
                    const int k = idx >> 6, t = idx & 63;
                    rt[k * 64 + t] = Rw[(size_t)t * p + k0 + k];
                }
                __syncthreads();
            }
            for (int k = 0; k < kn; ++k) {
                const double rv = rt[k * 64 + lane];
#pragma unroll
                for (int q = 0; q < ROUND_RB; ++q) acc[q] = fma(yq[q][k0 + k], rv, acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < ROUND_RB; ++q) {
            const int i = g * ROUND_ROWS + wave * ROUND_RB + q;
            const u64 m = __ballot(acc[q] < 0.0);
            if (i < n && lane == 0) Mw[i] = m;
        }
    }
}

// The rows of C as the handle holds them: CSR (COST_SPARSE) or the dense rows d.Cd with stride nS (COST_DENSE); COST_SPLR: the
// CSR rows of Cs plus the low-rank term V diag(s) V' (V row-major n x q, the kernel instances with LR set).
struct RoundCost {
    int n, dense, nS;
    const int* rowptr; const int* colind; const double* cval;
    const double* Cd;
    int q; const double* V; const double* s;
};
// The low-rank term keeps lane = trial: lane t holds t_k = V_k' x of its trial in registers; row i of V is wave-uniform.
// t_k += x_i V_ik for the lane's sign of row i (bit `lane` of the row's mask word set: x_i = -1)
__device__ inline void round_lr_accum(const RoundCost& c, int i, u64 mi, int lane, double (&tk)[MSDP_LOWRANK_MAX]) {
    const double* __restrict__ vr = c.V + (size_t)i * c.q;
    const bool neg = ((mi >> lane) & 1ull) != 0;
#pragma unroll
    for (int k = 0; k < MSDP_LOWRANK_MAX; ++k)
        if (k < c.q) { const double v = vr[k]; tk[k] += neg ? -v : v; }
}

__device__ inline u64 round_readlane64(u64 v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}

// Row i of C as a range of stored entries: [e0, e1) of (ci, cv); ci == nullptr (dense row): entry e is column e.
struct RoundRow { int e0, e1; const int* ci; const double* cv; };
__device__ inline RoundRow round_row(const RoundCost& c, int i) {
    RoundRow r;
    if (c.dense) { r.e0 = 0; r.e1 = c.n; r.ci = nullptr; r.cv = c.Cd + (size_t)i * c.nS; }
    else { r.e0 = c.rowptr[i]; r.e1 = c.rowptr[i + 1]; r.ci = c.colind; r.cv = c.cval; }
    return r;
}
__device__ inline void round_uniform(RoundRow& r) {
    r.e0 = __builtin_amdgcn_readfirstlane(r.e0);
    r.e1 = __builtin_amdgcn_readfirstlane(r.e1);
}
// Lane l takes entry base + l of the row: its column j and the bits vb of its value; past the row's end (and, with skip_diag,
// on the diagonal) a zero that adds nothing, at column i.
__device__ inline void round_fetch(const RoundRow& r, int base, int i, bool skip_diag, int lane, int& j, u64& vb) {
    const int e = base + lane;
    const bool ok = e < r.e1;
    j = ok ? (r.ci ? r.ci[e] : e) : i;
    double v = ok ? r.cv[e] : 0.0;
    if (skip_diag && j == i) v = 0.0;
    vb = (u64)__double_as_longlong(v);
}
// acc + sum over the cnt entries the lanes hold of +-C_ij: every entry is broadcast, lane t flips its sign bit by bit t of
// xw = M[i] ^ M[j].
__device__ inline double round_consume(double acc, u64 xw, u64 vb, int cnt, int lane) {
    for (int q = 0; q < cnt; ++q) {
        const u64 xq = round_readlane64(xw, q);
        const u64 vq = round_readlane64(vb, q);
        acc += __longlong_as_double((long long)(vq ^ (((xq >> lane) & 1ull) << 63)));
    }
    return acc;
}
// The mask word of column j.  LIVE: the wave itself rewrites the words between rows (k_round_1opt) -- relaxed wavefront-scope
// atomic loads, vector loads that see the wave's own earlier stores.
template <bool LIVE>
__device__ inline u64 round_word(const u64* Mw, int j) {
    if (LIVE) return __hip_atomic_load(&Mw[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    return Mw[j];
}
// sum_j C_ij x_i x_j over the entries [base, r.e1) of row i for the 64 trials of a word, in stored order, 64 entries and their
// columns' mask words fetched at once (as lanes of entries).
template <bool LIVE>
__device__ inline double round_row_sum(double acc, const RoundRow& r, int base, const u64* Mw, int i, u64 mi, bool skip_diag, int lane) {
    for (; base < r.e1; base += 64) {
        int j; u64 vb;
        round_fetch(r, base, i, skip_diag, lane, j, vb);
        acc = round_consume(acc, mi ^ round_word<LIVE>(Mw, j), vb, std::min(64, r.e1 - base), lane);
    }
    return acc;
}

// val_t = sum_i sum_j C_ij x_i x_j (diagonal included), deterministic: workgroup (g, w) -- one wave -- sums the rows of chunk g
// for word w in order and writes part[g][64 w + t]; k_round_sum adds the chunks in index order.  No floating-point atomics.
// LR: the same pass forms the chunk's partial of V_k' x per trial, partT[g][k][64 w + t]; k_round_sum adds the chunks in index order,
// squares, and adds sum_k s_k (V_k' x)^2 in k order.
template <bool LR>
__global__ __launch_bounds__(64) void k_round_values(RoundCost c, const u64* __restrict__ M, int rows_per, int T,
                                                     double* __restrict__ part, double* __restrict__ partT) {
    const int lane = threadIdx.x;
    const int g = blockIdx.x, w = blockIdx.y;
    const u64* Mw = M + (size_t)w * c.n;
    const int i0 = g * rows_per, i1 = std::min(c.n, i0 + rows_per);
    double acc = 0.0;
    double tk[MSDP_LOWRANK_MAX];
    if (LR) {
#pragma unroll
        for (int k = 0; k < MSDP_LOWRANK_MAX; ++k) tk[k] = 0.0;
    }
    for (int i = i0; i < i1; ++i) {
        RoundRow r = round_row(c, i);
        round_uniform(r);
        const u64 mi = Mw[i];
        acc += round_row_sum<false>(0.0, r, r.e0, Mw, i, mi, false, lane);
        if (LR) round_lr_accum(c, i, mi, lane, tk);
    }
    part[(size_t)g * T + w * 64 + lane] = acc;
    if (LR) {
#pragma unroll
        for (int k = 0; k < MSDP_LOWRANK_MAX; ++k)
            if (k < c.q) partT[((size_t)g * c.q + k) * T + w * 64 + lane] = tk[k];
    }
}

template <bool LR>
__global__ void k_round_sum(const double* __restrict__ part, const double* __restrict__ partT, int q, const double* __restrict__ sk,
                            int G, int T, double* __restrict__ val) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[(size_t)g * T + t];
    if (LR) {
        for (int k = 0; k < q; ++k) {
            double tk = 0.0;
            for (int g = 0; g < G; ++g) tk += partT[((size_t)g * q + k) * T + t];
            s += sk[k] * (tk * tk);
        }
    }
    val[t] = s;
}

// One Gauss-Seidel sweep of 1-opt: the wave of word w visits the rows in order, forms x_i s_i = sum_{j != i} C_ij x_i x_j per
// lane and flips x_i where it is > 0 (strict: a tie stays).  st[w] = sweeps this word has run, st[W + w] = flips of its last
// one; a word whose last sweep flipped nothing returns at once.  The wave is the only reader and writer of its words.
// LR: t_k = V_k' x per lane, formed by one ordered pass over the rows at the start of EVERY sweep launch (recomputed, never carried
// between launches or stored per word); x_i s_i gains sum_k s_k V_ik (x_i t_k - V_ik); a flipped lane takes t_k -= 2 V_ik x_i(old).
template <bool LR>
__global__ __launch_bounds__(64) void k_round_1opt(RoundCost c, u64* M, int* st, int W, int first) {
    const int lane = threadIdx.x;
    const int w = blockIdx.x;
    if (!first && st[W + w] == 0) return;
    u64* Mw = M + (size_t)w * c.n;
    int flips = 0;
    double tk[MSDP_LOWRANK_MAX];
    if (LR) {
#pragma unroll
        for (int k = 0; k < MSDP_LOWRANK_MAX; ++k) tk[k] = 0.0;
        for (int i = 0; i < c.n; ++i) round_lr_accum(c, i, round_word<true>(Mw, i), lane, tk);
    }
    // The rows of C are read-only: the first 64 entries of row i + 1 and the bounds of row i + 2 are fetched while the words of
    // row i are in flight, so that a row waits for its mask words only.
    const int last = c.n - 1;
    RoundRow cur = round_row(c, 0), nxt = round_row(c, std::min(1, last));
    round_uniform(cur);
    round_uniform(nxt);
    int j; u64 vb;
    round_fetch(cur, cur.e0, 0, true, lane, j, vb);
    for (int i = 0; i < c.n; ++i) {
        const u64 mi = round_word<true>(Mw, i);
        const u64 mj = round_word<true>(Mw, j);
        RoundRow nn = round_row(c, std::min(i + 2, last));
        int nj; u64 nvb;
        round_fetch(nxt, nxt.e0, std::min(i + 1, last), true, lane, nj, nvb);
        double xs = round_consume(0.0, mi ^ mj, vb, std::min(64, cur.e1 - cur.e0), lane);
        xs = round_row_sum<true>(xs, cur, cur.e0 + 64, Mw, i, mi, true, lane);
        const double xi = ((mi >> lane) & 1ull) ? -1.0 : 1.0;
        if (LR) {
            const double* __restrict__ vr = c.V + (size_t)i * c.q;
#pragma unroll
            for (int k = 0; k < MSDP_LOWRANK_MAX; ++k)
                if (k < c.q) { const double v = vr[k]; xs += (c.s[k] * v) * (xi * tk[k] - v); }
        }
        const u64 fl = __ballot(xs > 0.0);
        if (fl) {
            if (lane == 0) __hip_atomic_store(&Mw[i], mi ^ fl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            flips += __popcll(fl);
            if (LR && ((fl >> lane) & 1ull)) {
                const double* __restrict__ vr = c.V + (size_t)i * c.q;
#pragma unroll
                for (int k = 0; k < MSDP_LOWRANK_MAX; ++k)
                    if (k < c.q) tk[k] -= 2.0 * vr[k] * xi;
            }
        }
        round_uniform(nn);
        cur = nxt; nxt = nn; j = nj; vb = nvb;
    }
    if (lane == 0) { st[w] += 1; st[W + w] = flips; }
}

// One colour class of a 1-opt sweep in colour order (option "round_order" = 1): the rows order[offs[cls]] .. order[offs[cls + 1] - 1]
// for every word at once.  Grid: (row groups, words); a wave takes one row of the class at a time for the word of its workgroup,
// lane = trial.  The row's number and the flip rule are those of k_round_1opt.  No stored off-diagonal entry joins two rows of a
// class (msdp_roundcolor.hip), so no wave of the launch writes a word that another one reads, and the word of a wave's own row
// is read and written by that wave alone: plain loads, the kernel boundary orders the classes.  cur[w] gains the flips of word w
// (one integer atomic per wave: the sum does not depend on the order); a word whose previous sweep flipped nothing (prev[w] == 0)
// skips the sweep.  CSR rows only: the dense and the low-rank kinds have no colour order.
__global__ __launch_bounds__(ROUND_WAVES * 64) void k_round_1opt_color(RoundCost c, u64* M, const int* __restrict__ order,
                                                                       const int* __restrict__ offs, int cls, const int* __restrict__ prev,
                                                                       int* cur, int first) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int w = blockIdx.y;
    if (!first && prev[w] == 0) return;
    u64* Mw = M + (size_t)w * c.n;
    const int q1 = offs[cls + 1];
    int flips = 0;
    for (int q = offs[cls] + blockIdx.x * ROUND_WAVES + wave; q < q1; q += gridDim.x * ROUND_WAVES) {
        const int i = __builtin_amdgcn_readfirstlane(order[q]);
        RoundRow r = round_row(c, i);
        round_uniform(r);
        const u64 mi = Mw[i];
        const double xs = round_row_sum<false>(0.0, r, r.e0, Mw, i, mi, true, lane);
        const u64 fl = __ballot(xs > 0.0);
        if (fl) {
            if (lane == 0) Mw[i] = mi ^ fl;
            flips += __popcll(fl);
        }
    }
    if (flips && lane == 0) atomicAdd(&cur[w], flips);
}

static int round_values(msdp_handle h, const RoundCost& c, const u64* M, int W, int G, int rows_per, double* part, double* partT, double* val) {
    const int T = W * 64;
    if (c.q > 0) {
        hipLaunchKernelGGL(k_round_values<true>, dim3(G, W), dim3(64), 0, h->stream, c, M, rows_per, T, part, partT);
        hipLaunchKernelGGL(k_round_sum<true>, dim3((T + 255) / 256), dim3(256), 0, h->stream, (const double*)part, (const double*)partT, c.q, c.s, G, T, val);
    } else {
        hipLaunchKernelGGL(k_round_values<false>, dim3(G, W), dim3(64), 0, h->stream, c, M, rows_per, T, part, (double*)nullptr);
        hipLaunchKernelGGL(k_round_sum<false>, dim3((T + 255) / 256), dim3(256), 0, h->stream, (const double*)part, (const double*)nullptr, 0, (const double*)nullptr, G, T, val);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// Sweep s of the colour-ordered search: one launch per colour class on the handle's stream.  st holds two count rows of W
// words, alternated by the parity of s: the row of this sweep is cleared on the stream in front of its launches, the other one
// still holds the counts of sweep s - 1.  The host then reads the counts of this sweep, as after a serial sweep: hst[w] gains
// one for every word that ran (the first sweep, or flips in its previous one), hst[W + w] is the count of its last sweep.
static int round_sweep_color(msdp_handle h, const RoundCost& c, u64* M, int* st, int W, int s, std::vector<int>& hst) {
    int* cur = st + (size_t)(s & 1) * W;
    const int* prev = st + (size_t)((s & 1) ^ 1) * W;
    HIPCHK(hipMemsetAsync(cur, 0, (size_t)W * sizeof(int), h->stream));
    for (int cls = 0; cls < h->rc_ncolors; ++cls) {
        const int rows = h->rc_offs[(size_t)cls + 1] - h->rc_offs[(size_t)cls];
        const int Gc = std::max(1, std::min((rows + ROUND_WAVES - 1) / ROUND_WAVES, (4096 + W - 1) / W));   // about 16 384 waves per launch
        hipLaunchKernelGGL(k_round_1opt_color, dim3(Gc, W), dim3(ROUND_WAVES * 64), 0, h->stream, c, M, (const int*)h->rc_order_d,
                           (const int*)h->rc_offs_d, cls, prev, cur, s == 0 ? 1 : 0);
    }
    HIPCHK(hipGetLastError());
    std::vector<int> cnt((size_t)W);
    HIPCHK(msdp_memcpy_async(cnt.data(), cur, cnt.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int w = 0; w < W; ++w) {
        if (s == 0 || hst[(size_t)W + w] != 0) hst[(size_t)w] += 1;   // (a word that did not run left its zero in place)
        hst[(size_t)W + w] = cnt[(size_t)w];
    }
    return 0;
}

extern "C" int msdp_round_hyperplane(msdp_handle h, int32_t trials, const double* R, int32_t sweeps, double* values0, double* values,
                                     int32_t* info, uint64_t* masks, int32_t* best, int8_t* x) {
    MSDP_CHECK_H(h);
    if (trials <= 0 || trials % 64 || trials > MSDP_ROUND_MAX_TRIALS || sweeps < 0 || !R || !values || !best) {
        msdp_set_error("round_hyperplane: trials = %d (a multiple of 64 up to %d), sweeps = %d (>= 0), R, values and best not null",
                       trials, MSDP_ROUND_MAX_TRIALS, sweeps);
        return MSDP_EINVAL;
    }
    if (h->kind != MSDP_KIND_ONLYUNITDIAG) { msdp_set_error("round_hyperplane: the onlyunitdiag kind only"); return MSDP_EUNSUPPORTED; }
    if (h->nranks > 1 || h->use_comm || h->lgroup) { msdp_set_error("round_hyperplane: not on a handle that has joined a communicator"); return MSDP_EUNSUPPORTED; }
    Dev& d = h->d;
    if (d.costkind == COST_HERM) { msdp_set_error("round_hyperplane: not for a Hermitian handle (+1/-1 rounding is the real problem's)"); return MSDP_EUNSUPPORTED; }
    if (d.costkind == COST_BLOCK) { msdp_set_error("round_hyperplane: not for a %s handle (+1/-1 rounding is the unit-diagonal problem's; rotations are rounded on the host)", msdp_block_kind_name(d.efree)); return MSDP_EUNSUPPORTED; }
    if (d.costkind != COST_SPARSE && d.costkind != COST_DENSE && d.costkind != COST_SPLR) { msdp_set_error("round_hyperplane: no cost matrix"); return MSDP_EUNSUPPORTED; }
    if (!h->have_point) { msdp_set_error("round_hyperplane: no resident point"); return MSDP_ESTATE; }
    const int n = d.n, p = d.p, T = trials, W = T / 64;
    if (n < 1) { msdp_set_error("round_hyperplane: empty problem"); return MSDP_EINVAL; }
    const bool color = h->tune.round_order == 1 && sweeps > 0;
    if (color) {                                               // (the option is refused on the dense and the low-rank kinds)
        const int rcc = msdp_round_color_plan(h, "round_hyperplane");
        if (rcc) return rcc;
    }
    RoundCost c{};
    c.n = n; c.dense = d.costkind == COST_DENSE; c.nS = msdp_dense_nS(n);
    c.rowptr = d.rowptr; c.colind = d.colind; c.cval = d.cval; c.Cd = d.Cd;
    const bool lr = d.costkind == COST_SPLR;
    c.q = lr ? d.lrq : 0; c.V = lr ? d.lrV : nullptr; c.s = lr ? d.lrs : nullptr;
    // row chunks of the value sums: about 2048 waves in flight, at least ROUND_ROWS rows each
    const int G = std::max(1, std::min((n + ROUND_ROWS - 1) / ROUND_ROWS, (2048 + W - 1) / W));
    const int rows_per = (n + G - 1) / G;
    const int Gs = std::max(1, std::min((n + ROUND_ROWS - 1) / ROUND_ROWS, (1024 + W - 1) / W));   // workgroups per word of k_round_signs

    u64* M = nullptr; double* part = nullptr; double* partT = nullptr; double* val = nullptr; double* Rd = nullptr; int* st = nullptr;
    auto release = [&]() {
        (void)hipStreamSynchronize(h->stream);
        msdp_dev_free(h, M); msdp_dev_free(h, part); msdp_dev_free(h, partT); msdp_dev_free(h, val); msdp_dev_free(h, Rd); msdp_dev_free(h, st);
    };
    int rc = 0;
    if ((rc = msdp_dev_alloc<u64>(h, &M, (size_t)W * n)) || (rc = msdp_dev_alloc<double>(h, &part, (size_t)G * T)) ||
        (lr && (rc = msdp_dev_alloc<double>(h, &partT, (size_t)G * c.q * T))) ||
        (rc = msdp_dev_alloc<double>(h, &val, (size_t)T)) || (rc = msdp_dev_alloc<double>(h, &Rd, (size_t)T * p)) ||
        (rc = msdp_dev_alloc<int>(h, &st, (size_t)2 * W))) { release(); return rc; }
#define ROUND_HIP(expr)                                                                                           \
    do {                                                                                                          \
        hipError_t _e = (expr);                                                                                   \
        if (_e != hipSuccess) {                                                                                   \
            msdp_set_error("round_hyperplane: %s failed: %s", #expr, hipGetErrorString(_e));                      \
            release();                                                                                            \
            return MSDP_EHIP;                                                                                     \
        }                                                                                                         \
    } while (0)
    ROUND_HIP(msdp_memcpy_async(Rd, R, (size_t)T * p * sizeof(double), hipMemcpyHostToDevice, h->stream));
    ROUND_HIP(hipMemsetAsync(st, 0, (size_t)2 * W * sizeof(int), h->stream));
    hipLaunchKernelGGL(k_round_signs, dim3(Gs, W), dim3(ROUND_WAVES * 64), 0, h->stream, (const double*)d.Y[msdp_host_cur(h)], d.ld, p, n,
                       (const double*)Rd, M);
    ROUND_HIP(hipGetLastError());
    if ((rc = round_values(h, c, M, W, G, rows_per, part, partT, val))) { release(); return rc; }
    ROUND_HIP(msdp_memcpy_async(values, val, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    ROUND_HIP(hipStreamSynchronize(h->stream));
    if (values0) std::copy(values, values + T, values0);

    // the host reads the flip counts after every sweep: it stops when no word flipped anything, or after `sweeps` launches
    std::vector<int> hst((size_t)2 * W, 0);
    for (int s = 0; s < sweeps; ++s) {
        if (color) {
            if ((rc = round_sweep_color(h, c, M, st, W, s, hst))) { release(); return rc; }
        } else {
            if (lr) hipLaunchKernelGGL(k_round_1opt<true>, dim3(W), dim3(64), 0, h->stream, c, M, st, W, s == 0 ? 1 : 0);
            else hipLaunchKernelGGL(k_round_1opt<false>, dim3(W), dim3(64), 0, h->stream, c, M, st, W, s == 0 ? 1 : 0);
            ROUND_HIP(hipGetLastError());
            ROUND_HIP(msdp_memcpy_async(hst.data(), st, hst.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
            ROUND_HIP(hipStreamSynchronize(h->stream));
        }
        bool any = false;
        for (int w = 0; w < W; ++w) any = any || hst[(size_t)W + w] != 0;
        if (!any) break;
    }
    if (sweeps > 0) {                                          // never updated incrementally: all values again from the final masks
        if ((rc = round_values(h, c, M, W, G, rows_per, part, partT, val))) { release(); return rc; }
        ROUND_HIP(msdp_memcpy_async(values, val, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        ROUND_HIP(hipStreamSynchronize(h->stream));
    }
    if (info) for (size_t k = 0; k < hst.size(); ++k) info[k] = hst[k];
    int b = 0;
    for (int t = 1; t < T; ++t) if (values[t] < values[b]) b = t;       // the lowest index wins a tie
    *best = b;
    if (masks) ROUND_HIP(msdp_memcpy_async(masks, M, (size_t)W * n * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    if (x) {
        std::vector<u64> word((size_t)n);
        ROUND_HIP(msdp_memcpy_async(word.data(), M + (size_t)(b / 64) * n, (size_t)n * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
        ROUND_HIP(hipStreamSynchronize(h->stream));
        for (int i = 0; i < n; ++i) x[i] = ((word[(size_t)i] >> (b & 63)) & 1ull) ? -1 : 1;
    }
#undef ROUND_HIP
    release();
    return 0;
}
