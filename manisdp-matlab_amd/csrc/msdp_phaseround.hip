// msdp_phaseround.hip -- rounding of the complex unit-diagonal solution (COST_HERM, msdp_hermitian.hip) to phases: points of the
// unit circle (M = 0) or M-th roots of unity (M >= 2), with a coordinate-minimisation local search (msdp_round_phases).  Not
// part of the reference.  The complex analogue of msdp_round.hip, with the same shape: lane = trial, a wave owns the 64
// trials of one "word" and walks rows; whatever belongs to a row (the row of Y, the row of C) is the same for all 64 lanes.
//
// Phases live in an allocation of the call, Z[word][row][64 lanes] double2: the phases of one row for the 64 trials of a
// word are one coalesced 1-KB line.  The rows of C are read from the CSR form (d.rowptr / d.colind / d.hzv, row i already the
// conjugated column i); the fixed-width ELL copy (d.hzell) is never read here.  No kernel synchronises across workgroups, no
// launch does more than one pass over the rows, and nothing of the handle is written.
#include "msdp_common.h"
#include <algorithm>
#include <cmath>
#include <vector>

#define PHASE_REG_P 4         // complex widths up to this: a lane's row of R stays in registers (8 doubles)
#define PHASE_KT 32           // wider: complex columns of R per LDS tile (32 x 64 double2 = 32 KB); one pass for p <= PHASE_KT
#define PHASE_RB 8            // rows per wave and pass
#define PHASE_WAVES 4
#define PHASE_ROWS (PHASE_RB * PHASE_WAVES)

// Re(conj(a) b) = a.x b.x + a.y b.y, in ONE spelling: the local search compares this number for the phase a row holds with the
// same number for every table entry, and a phase that is a bit copy of entry k must reproduce entry k's number exactly.
__device__ inline double phase_dot(double2 a, double2 b) { return fma(a.x, b.x, a.y * b.y); }
// acc += c * z (complex, no conjugate), the real-part product first
__device__ inline void phase_cfma(double2& acc, double2 c, double2 z) {
    acc.x = fma(c.x, z.x, acc.x); acc.x = fma(-c.y, z.y, acc.x);
    acc.y = fma(c.x, z.y, acc.y); acc.y = fma(c.y, z.x, acc.y);
}
// The rounding of one number: M = 0: w / |w| (1 where |w| = 0); M >= 2: the table entry of the largest Re(conj(c_k) w), the
// lowest k at a tie.  The table is wave-uniform.
__device__ inline double2 phase_round_one(double2 w, int M, const double2* __restrict__ tab) {
    if (M == 0) {
        const double m = sqrt(w.x * w.x + w.y * w.y);
        return m == 0.0 ? make_double2(1.0, 0.0) : make_double2(w.x / m, w.y / m);
    }
    double2 z = tab[0];
    double best = phase_dot(z, w);
    for (int k = 1; k < M; ++k) {
        const double2 c = tab[k];
        const double v = phase_dot(c, w);
        if (v > best) { best = v; z = c; }
    }
    return z;
}

// z_i = round(sum_a Y_ia R_ta), ascending a.  The row of Y is wave-uniform; r_t stays in registers for p <= PHASE_REG_P and is
// staged in LDS, PHASE_KT columns at a time, otherwise.  Grid: (row groups, words); a workgroup takes PHASE_ROWS rows at a
// time, PHASE_RB per wave.
__global__ __launch_bounds__(PHASE_WAVES * 64) void k_phase_round(const double* __restrict__ Y, int ld, int p, int n,
                                                                  const double2* __restrict__ R, int M,
                                                                  const double2* __restrict__ tab, double2* __restrict__ Z) {
    __shared__ double2 rt[PHASE_KT * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int w = blockIdx.y;
    const double2* Rw = R + (size_t)w * 64 * p;
    double2* Zw = Z + (size_t)w * n * 64;
    const int ngroups = (n + PHASE_ROWS - 1) / PHASE_ROWS;
    if (p <= PHASE_REG_P) {
        double2 r[PHASE_REG_P];
#pragma unroll
        for (int k = 0; k < PHASE_REG_P; ++k) r[k] = k < p ? Rw[(size_t)lane * p + k] : make_double2(0.0, 0.0);
        for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
#pragma unroll
            for (int q = 0; q < PHASE_RB; ++q) {
                const int i = g * PHASE_ROWS + wave * PHASE_RB + q;
                if (i >= n) break;
                const double2* y = reinterpret_cast<const double2*>(Y + (size_t)i * ld);
                double2 acc = make_double2(0.0, 0.0);
#pragma unroll
                for (int k = 0; k < PHASE_REG_P; ++k)
                    if (k < p) phase_cfma(acc, y[k], r[k]);
                Zw[(size_t)i * 64 + lane] = phase_round_one(acc, M, tab);
            }
        }
        return;
    }
    const int ntiles = (p + PHASE_KT - 1) / PHASE_KT;
    for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
        double2 acc[PHASE_RB];
        const double2* yq[PHASE_RB];
#pragma unroll
        for (int q = 0; q < PHASE_RB; ++q) {
            acc[q] = make_double2(0.0, 0.0);
            // (rows past n: computed, not stored)
            yq[q] = reinterpret_cast<const double2*>(Y + (size_t)std::min(g * PHASE_ROWS + wave * PHASE_RB + q, n - 1) * ld);
        }
        for (int tile = 0; tile < ntiles; ++tile) {
            const int k0 = tile * PHASE_KT, kn = std::min(PHASE_KT, p - k0);
            if (ntiles > 1 || g == (int)blockIdx.x) {       // one tile: staged once per workgroup
                __syncthreads();
                for (int idx = threadIdx.x; idx < kn * 64; idx += PHASE_WAVES * 64) {
                    const int k = idx >> 6, t = idx & 63;
                    rt[k * 64 + t] = Rw[(size_t)t * p + k0 + k];
                }
                __syncthreads();
            }
            for (int k = 0; k < kn; ++k) {
                const double2 rv = rt[k * 64 + lane];
#pragma unroll
                for (int q = 0; q < PHASE_RB; ++q) phase_cfma(acc[q], yq[q][k0 + k], rv);
            }
        }
#pragma unroll
        for (int q = 0; q < PHASE_RB; ++q) {
            const int i = g * PHASE_ROWS + wave * PHASE_RB + q;
            if (i < n) Zw[(size_t)i * 64 + lane] = phase_round_one(acc[q], M, tab);
        }
    }
}

// The CSR rows of C as the Hermitian handle holds them.
struct PhaseCost { int n; const int* rowptr; const int* colind; const double2* cv; };
struct PhaseRow { int e0, e1; };
__device__ inline PhaseRow phase_row(const PhaseCost& c, int i) {
    PhaseRow r;
    r.e0 = __builtin_amdgcn_readfirstlane(c.rowptr[i]);
    r.e1 = __builtin_amdgcn_readfirstlane(c.rowptr[i + 1]);
    return r;
}
__device__ inline double phase_readlane(double v, int l) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// Lane l takes entry base + l of the row: its column j and its value v; past the row's end (and, with skip_diag, on the
// diagonal) a zero that adds nothing, at column i.
__device__ inline void phase_fetch(const PhaseCost& c, const PhaseRow& r, int base, int i, bool skip_diag, int lane, int& j, double2& v) {
    const int e = base + lane;
    const bool ok = e < r.e1;
    j = ok ? c.colind[e] : i;
    v = ok ? c.cv[e] : make_double2(0.0, 0.0);
    if (skip_diag && j == i) v = make_double2(0.0, 0.0);
}
// acc + sum over the cnt entries the lanes hold of C_ij z_j, in stored order: every entry is broadcast, lane t loads the phase
// of column j for its own trial (one 1-KB line per entry).  ZP: const double2* in the read-only passes, double2* in the sweep.
template <typename ZP>
__device__ inline double2 phase_consume(double2 acc, ZP Zw, int j, double2 v, int cnt, int lane) {
    for (int q = 0; q < cnt; ++q) {
        const int jq = __builtin_amdgcn_readlane(j, q);
        const double2 cq = make_double2(phase_readlane(v.x, q), phase_readlane(v.y, q));
        const double2 z = Zw[(size_t)jq * 64 + lane];
        phase_cfma(acc, cq, z);
    }
    return acc;
}
// the entries [base, r.e1) of row i, 64 at a time
template <typename ZP>
__device__ inline double2 phase_row_sum(double2 acc, const PhaseCost& c, const PhaseRow& r, int base, ZP Zw, int i, bool skip_diag, int lane) {
    for (; base < r.e1; base += 64) {
        int j; double2 v;
        phase_fetch(c, r, base, i, skip_diag, lane, j, v);
        acc = phase_consume(acc, Zw, j, v, std::min(64, r.e1 - base), lane);
    }
    return acc;
}

// val_t = sum_i Re(conj(z_i) sum_j C_ij z_j) (diagonal included), deterministic: workgroup (g, w) -- one wave -- sums the rows of
// chunk g for word w in order and writes part[g][64 w + t]; k_phase_sum adds the chunks in index order.  No floating-point
// atomics.
__global__ __launch_bounds__(64) void k_phase_values(PhaseCost c, const double2* __restrict__ Z, int rows_per, int T,
                                                     double* __restrict__ part) {
    const int lane = threadIdx.x;
    const int g = blockIdx.x, w = blockIdx.y;
    const double2* Zw = Z + (size_t)w * c.n * 64;
    const int i0 = g * rows_per, i1 = std::min(c.n, i0 + rows_per);
    double acc = 0.0;
    for (int i = i0; i < i1; ++i) {
        const PhaseRow r = phase_row(c, i);
        const double2 zi = Zw[(size_t)i * 64 + lane];
        const double2 s = phase_row_sum(make_double2(0.0, 0.0), c, r, r.e0, Zw, i, false, lane);
        acc += phase_dot(zi, s);
    }
    part[(size_t)g * T + w * 64 + lane] = acc;
}
__global__ void k_phase_sum(const double* __restrict__ part, int G, int T, double* __restrict__ val) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[(size_t)g * T + t];
    val[t] = s;
}
// the phases of one trial: lane `t` of every row of a word
__global__ void k_phase_column(int n, const double2* __restrict__ Zw, int t, double2* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = Zw[(size_t)i * 64 + t];
}

// One Gauss-Seidel sweep of the local search: the wave of word w visits the rows in order and forms s_i = sum_{j != i} C_ij z_j
// per lane.  CIRCLE (M = 0): z_i <- -s_i / |s_i| unless |s_i|^2 == 0.  Otherwise: z_i <- the table entry of the smallest
// Re(conj(c_k) s_i) (the lowest k at a tie) where that is strictly below the number of the phase the row holds.
// st[w] = sweeps this word has run, st[W + w] = changes of its last one (0 with CIRCLE, which never stops early); a word whose
// last sweep changed nothing returns at once.
//
// Z is read AND written here: row i's new phase is read back by later rows of the same launch, so Z must not be a const
// __restrict__ pointer (the compiler could then hoist or cache a load across the store).  Correctness rests on one property:
// lane t reads and writes only column t of its own word, so every load that must see an earlier store is a load of the SAME
// thread from the address that thread stored to -- per-thread program order, no fence, no cross-lane visibility.
template <bool CIRCLE>
__global__ __launch_bounds__(64) void k_phase_sweep(PhaseCost c, double2* Z, int M, const double2* __restrict__ tab, int* st, int W,
                                                    int first) {
    const int lane = threadIdx.x;
    const int w = blockIdx.x;
    if (!CIRCLE && !first && st[W + w] == 0) return;
    double2* Zw = Z + (size_t)w * c.n * 64;
    int changes = 0;
    // The rows of C are read-only: the first 64 entries of row i + 1 are fetched before the phases of row i are asked for, so
    // that a row waits for its phases only.
    const int last = c.n - 1;
    PhaseRow cur = phase_row(c, 0), nxt = phase_row(c, std::min(1, last));
    int j; double2 v;
    phase_fetch(c, cur, cur.e0, 0, true, lane, j, v);
    for (int i = 0; i < c.n; ++i) {
        const PhaseRow nn = phase_row(c, std::min(i + 2, last));
        int nj; double2 nv;
        phase_fetch(c, nxt, nxt.e0, std::min(i + 1, last), true, lane, nj, nv);
        double2 s = phase_consume(make_double2(0.0, 0.0), Zw, j, v, std::min(64, cur.e1 - cur.e0), lane);
        s = phase_row_sum(s, c, cur, cur.e0 + 64, Zw, i, true, lane);
        if (CIRCLE) {
            const double m2 = s.x * s.x + s.y * s.y;
            if (m2 != 0.0) {
                const double m = sqrt(m2);
                Zw[(size_t)i * 64 + lane] = make_double2(-s.x / m, -s.y / m);
            }
        } else {
            const double2 zi = Zw[(size_t)i * 64 + lane];
            const double now = phase_dot(zi, s);
            double2 zb = tab[0];
            double best = phase_dot(zb, s);
            for (int k = 1; k < M; ++k) {
                const double2 ck = tab[k];
                const double cand = phase_dot(ck, s);
                if (cand < best) { best = cand; zb = ck; }
            }
            const bool ch = best < now;
            if (ch) Zw[(size_t)i * 64 + lane] = zb;
            changes += __popcll(__ballot(ch));
        }
        cur = nxt; nxt = nn; j = nj; v = nv;
    }
    if (lane == 0) { st[w] += 1; st[W + w] = changes; }
}

// One colour class of a sweep in colour order (option "round_order" = 1): the rows order[offs[cls]] .. order[offs[cls + 1] - 1] for
// every word at once.  Grid: (row groups, words); a wave takes one row of the class at a time for the word of its workgroup,
// lane = trial.  s_i and both decision rules are those of k_phase_sweep.  No stored off-diagonal entry joins two rows of a class
// (msdp_roundcolor.hip), so no wave of the launch writes a phase line that another one reads, and lane t reads and writes only
// column t of its own row's line: plain loads, the kernel boundary orders the classes.  Z is read and written here as well: no
// const __restrict__.  cur[w] gains the changes of word w (one integer atomic per wave: the sum does not depend on the order); a
// word whose previous sweep changed nothing (prev[w] == 0) skips the sweep; CIRCLE counts nothing and never skips.
template <bool CIRCLE>
__global__ __launch_bounds__(PHASE_WAVES * 64) void k_phase_sweep_color(PhaseCost c, double2* Z, int M, const double2* __restrict__ tab,
                                                                        const int* __restrict__ order, const int* __restrict__ offs, int cls,
                                                                        const int* __restrict__ prev, int* cur, int first) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int w = blockIdx.y;
    if (!CIRCLE && !first && prev[w] == 0) return;
    double2* Zw = Z + (size_t)w * c.n * 64;
    const int q1 = offs[cls + 1];
    int changes = 0;
    for (int q = offs[cls] + blockIdx.x * PHASE_WAVES + wave; q < q1; q += gridDim.x * PHASE_WAVES) {
        const int i = __builtin_amdgcn_readfirstlane(order[q]);
        const PhaseRow r = phase_row(c, i);
        const double2 s = phase_row_sum(make_double2(0.0, 0.0), c, r, r.e0, Zw, i, true, lane);
        if (CIRCLE) {
            const double m2 = s.x * s.x + s.y * s.y;
            if (m2 != 0.0) {
                const double m = sqrt(m2);
                Zw[(size_t)i * 64 + lane] = make_double2(-s.x / m, -s.y / m);
            }
        } else {
            const double2 zi = Zw[(size_t)i * 64 + lane];
            const double now = phase_dot(zi, s);
            double2 zb = tab[0];
            double best = phase_dot(zb, s);
            for (int k = 1; k < M; ++k) {
                const double2 ck = tab[k];
                const double cand = phase_dot(ck, s);
                if (cand < best) { best = cand; zb = ck; }
            }
            const bool ch = best < now;
            if (ch) Zw[(size_t)i * 64 + lane] = zb;
            changes += __popcll(__ballot(ch));
        }
    }
    if (!CIRCLE && changes && lane == 0) atomicAdd(&cur[w], changes);
}

// c_k = (cos, sin)(2 pi k / M), the angle evaluated as ((2 * pi) * k) / M in double and passed to the C library's cos / sin;
// where 4 k is a multiple of M the entry is written as exactly (1, 0), (0, 1), (-1, 0), (0, -1) for 4 k / M = 0, 1, 2, 3.
static void phase_table(int M, std::vector<double2>& tab) {
    static const double ex[4][2] = {{1.0, 0.0}, {0.0, 1.0}, {-1.0, 0.0}, {0.0, -1.0}};
    tab.resize((size_t)std::max(M, 1));
    tab[0] = make_double2(1.0, 0.0);
    for (int k = 0; k < M; ++k) {
        if ((4 * k) % M == 0) { tab[(size_t)k] = make_double2(ex[4 * k / M][0], ex[4 * k / M][1]); continue; }
        const double a = ((2.0 * 3.141592653589793238462643383279502884) * (double)k) / (double)M;
        tab[(size_t)k] = make_double2(std::cos(a), std::sin(a));
    }
}

static int phase_values(msdp_handle h, const PhaseCost& c, const double2* Z, int W, int G, int rows_per, double* part, double* val) {
    const int T = W * 64;
    hipLaunchKernelGGL(k_phase_values, dim3(G, W), dim3(64), 0, h->stream, c, Z, rows_per, T, part);
    hipLaunchKernelGGL(k_phase_sum, dim3((T + 255) / 256), dim3(256), 0, h->stream, (const double*)part, G, T, val);
    HIPCHK(hipGetLastError());
    return 0;
}

// Sweep s of the colour-ordered search: one launch per colour class on the handle's stream.  st holds two count rows of W words,
// alternated by the parity of s: the row of this sweep is cleared on the stream in front of its launches, the other one still
// holds the counts of sweep s - 1.  With `read` the host then reads the counts of this sweep, as after a serial sweep: hst[w] gains
// one for every word that ran (the first sweep, or changes in its previous one), hst[W + w] is the count of its last sweep.
// M = 0: every word runs every sweep and counts nothing; the counts are read once, after the last one.
static int phase_sweep_color(msdp_handle h, const PhaseCost& c, double2* Z, int M, const double2* tab, int* st, int W, int s, bool read,
                             std::vector<int>& hst) {
    int* cur = st + (size_t)(s & 1) * W;
    const int* prev = st + (size_t)((s & 1) ^ 1) * W;
    HIPCHK(hipMemsetAsync(cur, 0, (size_t)W * sizeof(int), h->stream));
    for (int cls = 0; cls < h->rc_ncolors; ++cls) {
        const int rows = h->rc_offs[(size_t)cls + 1] - h->rc_offs[(size_t)cls];
        const int Gc = std::max(1, std::min((rows + PHASE_WAVES - 1) / PHASE_WAVES, (4096 + W - 1) / W));   // about 16 384 waves per launch
        if (M == 0)
            hipLaunchKernelGGL(k_phase_sweep_color<true>, dim3(Gc, W), dim3(PHASE_WAVES * 64), 0, h->stream, c, Z, 0, tab,
                               (const int*)h->rc_order_d, (const int*)h->rc_offs_d, cls, prev, cur, s == 0 ? 1 : 0);
        else
            hipLaunchKernelGGL(k_phase_sweep_color<false>, dim3(Gc, W), dim3(PHASE_WAVES * 64), 0, h->stream, c, Z, M, tab,
                               (const int*)h->rc_order_d, (const int*)h->rc_offs_d, cls, prev, cur, s == 0 ? 1 : 0);
    }
    HIPCHK(hipGetLastError());
    if (M == 0) for (int w = 0; w < W; ++w) hst[(size_t)w] += 1;
    if (!read) return 0;
    std::vector<int> cnt((size_t)W);
    HIPCHK(msdp_memcpy_async(cnt.data(), cur, cnt.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int w = 0; w < W; ++w) {
        if (M != 0 && (s == 0 || hst[(size_t)W + w] != 0)) hst[(size_t)w] += 1;   // (a word that did not run left its zero in place)
        hst[(size_t)W + w] = cnt[(size_t)w];
    }
    return 0;
}

extern "C" int msdp_round_phases(msdp_handle h, int32_t M, int32_t trials, const double* R, int32_t sweeps, double* values0,
                                 double* values, int32_t* info, double* phases, int32_t* best, double* z, int32_t* k) {
    MSDP_CHECK_H(h);
    Dev& d = h->d;
    if (d.costkind != COST_HERM || !d.hzv) {
        msdp_set_error("round_phases: for Hermitian handles only (msdp_create_onlyunitdiag_csc_hermitian); the real kinds take msdp_round_hyperplane, the block kinds msdp_blockfactor_round");
        return MSDP_EUNSUPPORTED;
    }
    if (trials <= 0 || trials % 64 || trials > MSDP_ROUND_PHASES_MAX_TRIALS || (M != 0 && (M < 2 || M > MSDP_ROUND_PHASES_MAX_M)) ||
        sweeps < 0 || !R || !values || !best || (k && M == 0)) {
        msdp_set_error("round_phases: M = %d (0, or 2 .. %d), trials = %d (a multiple of 64 up to %d), sweeps = %d (>= 0), R, values and best not null, k null with M = 0",
                       M, MSDP_ROUND_PHASES_MAX_M, trials, MSDP_ROUND_PHASES_MAX_TRIALS, sweeps);
        return MSDP_EINVAL;
    }
    if (!h->have_point) { msdp_set_error("round_phases: no resident point"); return MSDP_ESTATE; }
    const int n = d.n, p = d.p / 2, T = trials, W = T / 64;
    if (n < 1 || p < 1) { msdp_set_error("round_phases: empty problem"); return MSDP_EINVAL; }
    const bool color = h->tune.round_order == 1 && sweeps > 0;
    if (color) {
        const int rcc = msdp_round_color_plan(h, "round_phases");
        if (rcc) return rcc;
    }
    PhaseCost c{};
    c.n = n; c.rowptr = d.rowptr; c.colind = d.colind; c.cv = d.hzv;
    // row chunks of the value sums: about 2048 waves in flight, at least PHASE_ROWS rows each
    const int G = std::max(1, std::min((n + PHASE_ROWS - 1) / PHASE_ROWS, (2048 + W - 1) / W));
    const int rows_per = (n + G - 1) / G;
    const int Gs = std::max(1, std::min((n + PHASE_ROWS - 1) / PHASE_ROWS, (1024 + W - 1) / W));   // workgroups per word of k_phase_round
    std::vector<double2> htab;
    phase_table(M, htab);

    double2* Z = nullptr; double* part = nullptr; double* val = nullptr; double2* Rd = nullptr; double2* tab = nullptr; double2* col = nullptr;
    int* st = nullptr;
    auto release = [&]() {
        (void)hipStreamSynchronize(h->stream);
        msdp_dev_free(h, Z); msdp_dev_free(h, part); msdp_dev_free(h, val); msdp_dev_free(h, Rd); msdp_dev_free(h, tab);
        msdp_dev_free(h, col); msdp_dev_free(h, st);
    };
    int rc = 0;
    if ((rc = msdp_dev_alloc<double2>(h, &Z, (size_t)T * n)) || (rc = msdp_dev_alloc<double>(h, &part, (size_t)G * T)) ||
        (rc = msdp_dev_alloc<double>(h, &val, (size_t)T)) || (rc = msdp_dev_alloc<double2>(h, &Rd, (size_t)T * p)) ||
        (rc = msdp_dev_alloc<double2>(h, &tab, htab.size())) || (rc = msdp_dev_alloc<double2>(h, &col, (size_t)n)) ||
        (rc = msdp_dev_alloc<int>(h, &st, (size_t)2 * W))) { release(); return rc; }
#define PHASE_HIP(expr)                                                                                           \
    do {                                                                                                          \
        hipError_t _e = (expr);                                                                                   \
        if (_e != hipSuccess) {                                                                                   \
            msdp_set_error("round_phases: %s failed: %s", #expr, hipGetErrorString(_e));                          \
            release();                                                                                            \
            return MSDP_EHIP;                                                                                     \
        }                                                                                                         \
    } while (0)
    PHASE_HIP(msdp_memcpy_async(Rd, R, (size_t)T * p * sizeof(double2), hipMemcpyHostToDevice, h->stream));
    PHASE_HIP(msdp_memcpy_async(tab, htab.data(), htab.size() * sizeof(double2), hipMemcpyHostToDevice, h->stream));
    PHASE_HIP(hipMemsetAsync(st, 0, (size_t)2 * W * sizeof(int), h->stream));
    hipLaunchKernelGGL(k_phase_round, dim3(Gs, W), dim3(PHASE_WAVES * 64), 0, h->stream, (const double*)d.Y[msdp_host_cur(h)], d.ld, p, n,
                       (const double2*)Rd, (int)M, (const double2*)tab, Z);
    PHASE_HIP(hipGetLastError());
    if ((rc = phase_values(h, c, Z, W, G, rows_per, part, val))) { release(); return rc; }
    PHASE_HIP(msdp_memcpy_async(values, val, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PHASE_HIP(hipStreamSynchronize(h->stream));
    if (values0) std::copy(values, values + T, values0);

    // M >= 2: the host reads the change counts after every sweep and stops when no word changed anything, or after `sweeps`
    // launches; M = 0: exactly `sweeps` launches, the counts read once
    std::vector<int> hst((size_t)2 * W, 0);
    for (int s = 0; s < sweeps; ++s) {
        if (color) {
            if ((rc = phase_sweep_color(h, c, Z, (int)M, (const double2*)tab, st, W, s, M != 0 || s + 1 == sweeps, hst))) { release(); return rc; }
            if (M == 0) continue;
        } else if (M == 0) {
            hipLaunchKernelGGL(k_phase_sweep<true>, dim3(W), dim3(64), 0, h->stream, c, Z, 0, (const double2*)tab, st, W, s == 0 ? 1 : 0);
            PHASE_HIP(hipGetLastError());
            if (s + 1 < sweeps) continue;
        } else {
            hipLaunchKernelGGL(k_phase_sweep<false>, dim3(W), dim3(64), 0, h->stream, c, Z, (int)M, (const double2*)tab, st, W, s == 0 ? 1 : 0);
            PHASE_HIP(hipGetLastError());
        }
        if (!color) {
            PHASE_HIP(msdp_memcpy_async(hst.data(), st, hst.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
            PHASE_HIP(hipStreamSynchronize(h->stream));
        }
        bool any = false;
        for (int w = 0; w < W; ++w) any = any || hst[(size_t)W + w] != 0;
        if (M != 0 && !any) break;
    }
    if (sweeps > 0) {                                          // never updated incrementally: all values again from the final phases
        if ((rc = phase_values(h, c, Z, W, G, rows_per, part, val))) { release(); return rc; }
        PHASE_HIP(msdp_memcpy_async(values, val, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        PHASE_HIP(hipStreamSynchronize(h->stream));
    }
    if (info) for (size_t q = 0; q < hst.size(); ++q) info[q] = hst[q];
    int b = 0;
    for (int t = 1; t < T; ++t) if (values[t] < values[b]) b = t;       // the lowest index wins a tie
    *best = b;
    if (phases) PHASE_HIP(msdp_memcpy_async(phases, Z, (size_t)T * n * sizeof(double2), hipMemcpyDeviceToHost, h->stream));
    if (z || k) {
        std::vector<double2> zb((size_t)n);
        hipLaunchKernelGGL(k_phase_column, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, (const double2*)(Z + (size_t)(b / 64) * n * 64),
                           b & 63, col);
        PHASE_HIP(hipGetLastError());
        PHASE_HIP(msdp_memcpy_async(zb.data(), col, (size_t)n * sizeof(double2), hipMemcpyDeviceToHost, h->stream));
        PHASE_HIP(hipStreamSynchronize(h->stream));
        if (z) for (int i = 0; i < n; ++i) { z[2 * (size_t)i] = zb[(size_t)i].x; z[2 * (size_t)i + 1] = zb[(size_t)i].y; }
        if (k) {                                               // a phase is a bit copy of its table entry
            for (int i = 0; i < n; ++i) {
                int ki = -1;
                for (int q = 0; q < M && ki < 0; ++q)
                    if (zb[(size_t)i].x == htab[(size_t)q].x && zb[(size_t)i].y == htab[(size_t)q].y) ki = q;
                k[i] = ki;
            }
        }
    }
    PHASE_HIP(hipStreamSynchronize(h->stream));
#undef PHASE_HIP
    release();
    return 0;
}
