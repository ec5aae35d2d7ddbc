// msdp_blocktridiag.hip -- eig(S_i) of diagonal blocks of order up to 1024, several workgroups per block.
//
// The mathematics of k_block_tridiag (msdp_blockjacobi.hip; ManiSDP_multiblock.m:78-88): the symmetrised block 0.5 (S + S'),
// Householder tridiagonalisation with the reflectors kept, ALL eigenvalues by bisection on the Sturm count, the k <= 8 lowest
// eigenvectors by inverse iteration on T (modified Gram-Schmidt inside clusters) and back-transformation.  One workgroup streams an
// 8-MB block of order 1024 through one CU n times; here a GROUP of G workgroups shares a block:
//   rows       row i of the work matrix belongs to workgroup i mod G of the group, for the whole call: only its owner ever reads or
//              writes it (plain accesses, the L2 of the owner's XCD; 8 MB / G per workgroup).  What crosses workgroups is vectors:
//   step kk    (1) every owner publishes its entries of column kk (from the diagonal down)            -> group barrier 1
//              (2) every workgroup reads the column, forms the reflector v and tau for itself (the same instructions on the same
//                  numbers: the same bits), computes p_i = tau A(i, :) v for ITS rows and publishes them  -> group barrier 2
//              (3) every workgroup reads p, forms w = p - tau/2 (p'v) v for itself and updates its rows A(i, :) -= v_i w' + w_i v'.
//              Workgroup kk mod G stores the reflector (one contiguous row of Rf).
//   spectrum   every workgroup holds the whole tridiagonal matrix in LDS; eigenvalue j is bisected by workgroup j mod G (one thread
//              per eigenvalue), the k lowest and the largest by every workgroup for itself (the scale of the inverse iteration).
//   vectors    inverse iteration by the group's first workgroup (LDS; the LU factors of the k shifted matrices stream through a
//              private piece of global memory), published -> group barrier 3; vector c is back-transformed by one wave of
//              workgroup c mod G, the reflectors read as contiguous rows.
// Determinism, strong form: no sum is ever split between workgroups.  Every inner product over rows (|x|^2, p'v) is formed by
// every workgroup over ALL rows in one fixed order, the row products and the vector back-transformations by one wave each in lane
// order.  G and the other blocks of a launch therefore change who computes a number, never the number: a block's w and V have the
// same bits alone or among many, with any G.
// Visibility: the workgroups of a group may sit on different XCDs (one L2 each, not coherent).  Every published value is stored with
// an agent-scope (sc1, write-through) store into memory nobody accesses any other way, every storing wave waits for its stores,
// one lane per workgroup then adds to the group's counter behind a workgroup barrier; the readers poll the counter with sc1 loads
// and read the values with sc1 loads behind a workgroup barrier of their own (the protocol of the exchange buffers, msdp_psync.h).
// Co-residency and time-outs: the host never launches more workgroups than hipOccupancyMaxActiveBlocksPerMultiprocessor x CUs
// (more blocks = consecutive launches), every spin is bounded, a spin that runs out sets the launch's error word, which every
// other spin reads: all workgroups leave and the call returns MSDP_ECOMM.
#include "msdp_device.h"
#include "msdp_psync.h"
#include <algorithm>
#include <vector>

#define BTL_MAXN MSDP_BLOCK_EIGS_LARGE_MAXN
#define BTL_MAXK 8
#define BTL_THREADS 1024
#define BTL_WAVES (BTL_THREADS / 64)
#define BTL_MAXG 16
#define BTL_ONE_WG 256                   // orders up to this take one workgroup
#define BTL_ITERS 5
#define BTL_SPIN_LIMIT (1 << 22)
// exchange region of a block (doubles): [counter line 16] [X0 ld + 16] [X1 ld + 16] [P ld] [Z 8 ld] [U 24 ld]
#define BTL_EX(ld) (35 * (int64_t)(ld) + 48)

struct BtlBlock {                        // one per block of the call
    int64_t soff, sld;                   // S_b(i, j) = S[soff + i * sld + j]
    int64_t aoff;                        // its n x ld work matrix and reflector rows
    int64_t eoff;                        // its exchange region
    int64_t r0;                          // first row in the outputs
    int n, ld, G, pad;
};
struct BtlArgs {
    int k, kld;                          // vectors asked for; row length of vec (max(k, 1))
    const BtlBlock* blk;
    const int2* wg;                      // workgroup of the launch -> (block, member of its group)
    const double* S;
    double* A; double* Rf; double* E;
    double* w; double* vec;
    int* err;
};

typedef unsigned long long btl_u64;
__device__ __forceinline__ void btl_put(double* p, double v) {
    __hip_atomic_store(reinterpret_cast<btl_u64*>(p), (btl_u64)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double btl_get(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const btl_u64*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// Barrier of the G workgroups of one group: a monotonic counter, the nbar-th barrier waits for nbar * G arrivals.  False (in every
// thread) when the spin ran out or another workgroup of the launch has reported that.
__device__ __forceinline__ bool btl_barrier(btl_u64* cnt, unsigned& nbar, int G, int* err, int* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // this wave's published values have been performed
    __syncthreads();
    ++nbar;
    if (G == 1) return true;
    if (threadIdx.x < 64) {
        if (threadIdx.x == 0) __hip_atomic_fetch_add(cnt, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const btl_u64 want = (btl_u64)nbar * (unsigned)G;
        int spins = 0;
        bool fail = false;
        for (;;) {
            const btl_u64 v = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v >= want) break;
            ++spins;
            if (spins > BTL_SPIN_LIMIT || ((spins & 255) == 0 && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) { fail = true; break; }
            __builtin_amdgcn_s_sleep(2);
        }
        if (threadIdx.x == 0 && fail) { *flag = 1; __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    }
    __syncthreads();
    return *flag == 0;
}
__device__ __forceinline__ double btl_block_sum(double v, double* red, int tid) {
    v = msdp_wave_sum(v);
    __syncthreads();                                               // red is free again
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < BTL_WAVES; ++q) s += red[q];
    return s;
}
// eigenvalue number idx (ascending) of the tridiagonal matrix (dd, ee) by bisection on the Sturm count
__device__ __forceinline__ double btl_bisect(const double* dd, const double* ee, int n, int idx, double glo, double ghi, double pivmin) {
    double lo = glo, hi = ghi;
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (mid == lo || mid == hi) break;
        int cnt = 0;
        double q = dd[0] - mid;
        if (fabs(q) < pivmin) q = -pivmin;
        cnt += q < 0.0;
        for (int i = 1; i < n; ++i) {
            q = dd[i] - mid - ee[i - 1] * ee[i - 1] / q;
            if (fabs(q) < pivmin) q = -pivmin;
            cnt += q < 0.0;
        }
        if (cnt > idx) hi = mid; else lo = mid;
    }
    return 0.5 * (lo + hi);
}

__global__ __launch_bounds__(BTL_THREADS) void k_block_tridiag_group(BtlArgs a) {
    __shared__ double vv[BTL_MAXN], pw[BTL_MAXN], dd[BTL_MAXN], ee[BTL_MAXN], tt[BTL_MAXN];
    __shared__ double Z[BTL_MAXN * BTL_MAXK];                       // inverse iteration: [i * 8 + c]; back-transformation: [wave * BTL_MAXN + i]
    __shared__ double red[BTL_WAVES];
    __shared__ double wl[BTL_MAXK + 1], nrmv[BTL_MAXK];
    __shared__ double dk;
    __shared__ int flag;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int2 me = a.wg[blockIdx.x];
    const BtlBlock* B = a.blk + me.x;
    const int g = me.y, G = B->G, n = B->n, ld = B->ld;
    const int64_t so = B->soff, sl = B->sld, r0 = B->r0;
    double* __restrict__ A = a.A + B->aoff;
    double* Rf = a.Rf + B->aoff;
    double* E = a.E + B->eoff;
    btl_u64* cnt = reinterpret_cast<btl_u64*>(E);
    double* P = E + 16 + 2 * (ld + 16);
    double* Zg = P + ld;
    double* U = Zg + 8 * ld;
    unsigned nbar = 0;
    const int KZ = BTL_MAXK;
    const int k = min(min(a.k, n), KZ);
    if (tid == 0) flag = 0;
    {   // my rows of the symmetrised block (ManiSDP_multiblock.m:86 symmetrises too)
        const int mine = (n - g + G - 1) / G;
        for (int e = tid; e < mine * n; e += BTL_THREADS) {
            const int t = e / n, j = e - t * n, i = g + G * t;
            A[(int64_t)i * ld + j] = 0.5 * (a.S[so + (int64_t)i * sl + j] + a.S[so + (int64_t)j * sl + i]);
        }
    }
    __syncthreads();
    // ---- tridiagonalisation: A <- H_k A H_k, H_k = I - tau v v', v = (1, A[k+2:, k]) on rows / columns k+1 .. n-1
    for (int kk = 0; kk < n; ++kk) {
        double* Xb = E + 16 + (kk & 1) * (ld + 16);
        {   // my entries of column kk, from the diagonal down
            const int i0 = kk + ((g - kk) % G + G) % G;
            for (int i = i0 + G * tid; i < n; i += G * BTL_THREADS) btl_put(Xb + (i - kk), A[(int64_t)i * ld + kk]);
        }
        if (!btl_barrier(cnt, nbar, G, a.err, &flag)) return;
        for (int i = tid; i < n - kk; i += BTL_THREADS) {
            const double x = btl_get(Xb + i);
            if (i == 0) dk = x; else vv[i - 1] = x;
        }
        __syncthreads();
        if (kk + 2 >= n) {                                           // the last 2 x 2 corner: nothing to reflect
            if (tid == 0) { dd[kk] = dk; if (kk + 2 == n) ee[kk] = vv[0]; tt[kk] = 0.0; }
            __syncthreads();
            continue;
        }
        const int m = n - kk - 1;
        double part = 0.0;
        for (int i = tid; i < m; i += BTL_THREADS) if (i > 0) part += vv[i] * vv[i];
        const double tail = btl_block_sum(part, red, tid);
        const double x0 = vv[0];
        if (tail == 0.0) {                                          // nothing below the subdiagonal: H = I (every workgroup finds the same)
            if (tid == 0) { dd[kk] = dk; ee[kk] = x0; tt[kk] = 0.0; }
            __syncthreads();
            continue;
        }
        const double alpha = (x0 >= 0.0 ? -1.0 : 1.0) * sqrt(x0 * x0 + tail);
        const double beta = x0 - alpha, tau = -beta / alpha;
        __syncthreads();
        for (int i = tid; i < m; i += BTL_THREADS) vv[i] = (i == 0) ? 1.0 : vv[i] / beta;
        __syncthreads();
        if (kk % G == g) for (int i = tid; i < m; i += BTL_THREADS) btl_put(Rf + (int64_t)kk * ld + i, vv[i]);     // the reflector, v_0 = 1 included
        const int i0 = kk + 1 + ((g - kk - 1) % G + G) % G;         // my first row below kk
        // p = tau * A22 v, my rows: one wave per row
        for (int i = i0 + G * wave; i < n; i += G * BTL_WAVES) {
            const double* row = A + (int64_t)i * ld + kk + 1;
            double acc = 0.0;
            for (int j = lane; j < m; j += 64) acc = fma(row[j], vv[j], acc);
            acc = msdp_wave_sum(acc);
            if (lane == 0) btl_put(P + (i - kk - 1), tau * acc);
        }
        if (!btl_barrier(cnt, nbar, G, a.err, &flag)) return;
        for (int i = tid; i < m; i += BTL_THREADS) pw[i] = btl_get(P + i);
        __syncthreads();
        double pv = 0.0;
        for (int i = tid; i < m; i += BTL_THREADS) pv += pw[i] * vv[i];
        const double pdotv = btl_block_sum(pv, red, tid);
        for (int i = tid; i < m; i += BTL_THREADS) pw[i] -= 0.5 * tau * pdotv * vv[i];            // w
        __syncthreads();
        // my rows of the rank-2 update (four entries per lane and trip, their loads in front of the first store)
        for (int i = i0 + G * wave; i < n; i += G * BTL_WAVES) {
            double* row = A + (int64_t)i * ld + kk + 1;
            const double vi = vv[i - kk - 1], wi = pw[i - kk - 1];
            for (int j0 = lane; j0 < m; j0 += 256) {
                double x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) x[u] = (j0 + 64 * u < m) ? row[j0 + 64 * u] : 0.0;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + 64 * u;
                    if (j < m) row[j] = x[u] - (vi * pw[j] + wi * vv[j]);
                }
            }
        }
        if (tid == 0) { dd[kk] = dk; ee[kk] = alpha; tt[kk] = tau; }
        __syncthreads();
    }
    // ---- all eigenvalues: bisection on the Sturm count, one thread per eigenvalue, eigenvalue j by workgroup j mod G (waves 1 ..);
    // wave 0 of EVERY workgroup: the k lowest and the largest, which the inverse iteration's shifts and scale are
    double glo = 0.0, ghi = 0.0, pivmin = 0.0;
    {
        double lo = 1e300, hi = -1e300, emax = 0.0;
        for (int i = 0; i < n; ++i) {
            const double r = (i > 0 ? fabs(ee[i - 1]) : 0.0) + (i + 1 < n ? fabs(ee[i]) : 0.0);
            lo = fmin(lo, dd[i] - r); hi = fmax(hi, dd[i] + r);
            if (i + 1 < n) emax = fmax(emax, ee[i] * ee[i]);
        }
        const double span = fmax(hi - lo, 1e-300);
        glo = lo - 1e-12 * span - 1e-300; ghi = hi + 1e-12 * span + 1e-300;
        pivmin = fmax(1e-292, 2.2250738585072014e-308 * fmax(1.0, emax));
    }
    if (tid <= KZ) {
        if (tid < k || tid == KZ) wl[tid] = btl_bisect(dd, ee, n, tid < KZ ? tid : n - 1, glo, ghi, pivmin);
    } else if (tid >= 64) {
        for (int s = tid - 64; g + G * s < n; s += BTL_THREADS - 64) a.w[r0 + g + G * s] = btl_bisect(dd, ee, n, g + G * s, glo, ghi, pivmin);
    }
    if (a.k == 0) return;
    __syncthreads();
    if (g == 0) for (int e = tid; e < n * (a.k - k); e += BTL_THREADS) a.vec[(r0 + e / (a.k - k)) * a.kld + k + e % (a.k - k)] = 0.0;   // columns beyond the order
    // ---- eigenvectors of the k smallest: inverse iteration on T by the group's first workgroup.  Lane c < k solves (T - w_c I) z = y_c
    // (LU with partial pivoting, dgttrf / dgtts2: the forward sweep keeps its two active rows in registers and streams U to global
    // memory, [i][d, du, du2][c]; the back substitution reads it in batches of eight rows), wave 0 orthogonalises inside clusters
    double scale = fmax(fabs(wl[0]), fabs(wl[KZ]));
    if (!(scale > 0.0)) scale = 1.0;
    if (g == 0) {
        for (int e = tid; e < n * KZ; e += BTL_THREADS) {
            unsigned hsh = (unsigned)e * 2654435761u + 12345u; hsh ^= hsh >> 15; hsh *= 2246822519u; hsh ^= hsh >> 13;
            Z[e] = (double)(hsh & 0xffffff) / 16777216.0 - 0.5;
        }
        __syncthreads();
        for (int it = 0; it < BTL_ITERS; ++it) {
            if (tid < k) {
                const int c = tid;
                const double lam = wl[c];
                const double tiny = 2.220446049250313e-16 * scale;
                double di = dd[0] - lam, dui = n > 1 ? ee[0] : 0.0, xi = Z[c];
                for (int i = 0; i + 1 < n; ++i) {
                    const double dli = ee[i];
                    double dn = dd[i + 1] - lam, dun = (i + 2 < n) ? ee[i + 1] : 0.0, xn = Z[(i + 1) * KZ + c], du2 = 0.0;
                    if (fabs(di) >= fabs(dli)) {
                        if (di == 0.0) di = tiny;
                        const double f = dli / di;
                        dn -= f * dui;
                        xn -= f * xi;
                    } else {                                        // interchange rows i and i + 1
                        const double f = di / dli;
                        di = dli;
                        const double t1 = dn;
                        dn = dui - f * t1;
                        if (i + 2 < n) { du2 = dun; dun = -f * dun; }
                        dui = t1;
                        const double t2 = xi; xi = xn; xn = t2 - f * xi;
                    }
                    double* u = U + (int64_t)i * 3 * KZ + c;
                    u[0] = di; u[KZ] = dui; u[2 * KZ] = du2;
                    Z[i * KZ + c] = xi;
                    di = dn; dui = dun; xi = xn;
                }
                if (fabs(di) < tiny) di = (di < 0.0 ? -tiny : tiny);
                // back substitution with U (diagonals d, du, du2)
                double x1 = xi / di, x2 = 0.0, nrm = fabs(x1);
                Z[(n - 1) * KZ + c] = x1;
                for (int i1 = n - 2; i1 >= 0; i1 -= 8) {
                    double ud[8], uu[8], u2[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int i = i1 - q >= 0 ? i1 - q : 0;
                        const double* u = U + (int64_t)i * 3 * KZ + c;
                        ud[q] = u[0]; uu[q] = u[KZ]; u2[q] = u[2 * KZ];
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int i = i1 - q;
                        if (i >= 0) {
                            const double x = (Z[i * KZ + c] - uu[q] * x1 - u2[q] * x2) / ud[q];
                            Z[i * KZ + c] = x;
                            nrm = fmax(nrm, fabs(x));
                            x2 = x1; x1 = x;
                        }
                    }
                }
                if (!(nrm > 0.0)) nrm = 1.0;
                nrmv[c] = nrm;
            }
            __syncthreads();
            for (int e = tid; e < n * KZ; e += BTL_THREADS) if ((e & (KZ - 1)) < k) Z[e] /= nrmv[e & (KZ - 1)];
            __syncthreads();
            if (wave == 0) {                                        // modified Gram-Schmidt inside clusters, in eigenvalue order
                // (two passes per vector: where the solves of a cluster return nearly parallel vectors the first pass cancels most of
                // the vector and leaves |V'V - I| ~ eps / |what remains|; the second works on a normalised vector -- 2.4e-11 -> eps on a
                // rank-one block of order 3)
                for (int c = 0; c < k; ++c) {
                    for (int pass = 0; pass < 2; ++pass) {
                        for (int c2 = 0; c2 < c; ++c2) {
                            if (fabs(wl[c] - wl[c2]) > 1e-3 * scale) continue;
                            double dot = 0.0;
                            for (int i = lane; i < n; i += 64) dot += Z[i * KZ + c] * Z[i * KZ + c2];
                            dot = msdp_wave_sum(dot);
                            for (int i = lane; i < n; i += 64) Z[i * KZ + c] -= dot * Z[i * KZ + c2];
                        }
                        double nn = 0.0;
                        for (int i = lane; i < n; i += 64) nn += Z[i * KZ + c] * Z[i * KZ + c];
                        nn = sqrt(msdp_wave_sum(nn));
                        if (!(nn > 0.0)) nn = 1.0;
                        for (int i = lane; i < n; i += 64) Z[i * KZ + c] /= nn;
                    }
                }
            }
            __syncthreads();
        }
        for (int e = tid; e < n * KZ; e += BTL_THREADS) {
            const int i = e / KZ, c = e - i * KZ;
            if (c < k) btl_put(Zg + (int64_t)c * ld + i, Z[e]);
        }
    }
    if (!btl_barrier(cnt, nbar, G, a.err, &flag)) return;
    // ---- back-transformation z = H_0 H_1 ... H_{n-3} y: vector c by wave (c - g) / G of workgroup c mod G, the reflectors last one first,
    // a lane takes the entry pairs 2 lane + 128 q; the next reflector is requested before the present one is applied
    const int c = g + G * wave;
    if (c < k) {
        double* z = Z + wave * BTL_MAXN;
        for (int i = lane; i < n; i += 64) z[i] = btl_get(Zg + (int64_t)c * ld + i);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(Rf, 0, (unsigned)((int64_t)n * ld * 8), 0x00020000);
        v4u cur[8], nxt[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) { cur[q].x = 0u; cur[q].y = 0u; cur[q].z = 0u; cur[q].w = 0u; nxt[q] = cur[q]; }
        if (n >= 3) {
            const int qn = (n - (n - 3) - 1 + 127) / 128;
#pragma unroll
            for (int q = 0; q < 8; ++q) if (q < qn) cur[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)(((n - 3) * ld + 2 * lane + 128 * q) * 8), 0, MSDP_CPOL_SC1);
        }
        for (int kk = n - 3; kk >= 0; --kk) {
            const int m = n - kk - 1, qn = (m + 127) / 128;
            if (kk > 0) {
                const int qn1 = (m + 1 + 127) / 128;
#pragma unroll
                for (int q = 0; q < 8; ++q) if (q < qn1) nxt[q] = __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)(((kk - 1) * ld + 2 * lane + 128 * q) * 8), 0, MSDP_CPOL_SC1);
            }
            const double tau = tt[kk];
            if (tau != 0.0) {
                double vx[8], vy[8];
                double s = 0.0;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    if (q < qn) {
                        const int i = 2 * lane + 128 * q;
                        const double x = __longlong_as_double(((long long)cur[q].y << 32) | (long long)cur[q].x);
                        const double y = __longlong_as_double(((long long)cur[q].w << 32) | (long long)cur[q].z);
                        vx[q] = i < m ? x : 0.0; vy[q] = i + 1 < m ? y : 0.0;
                        const double z0 = i < m ? z[kk + 1 + i] : 0.0, z1 = i + 1 < m ? z[kk + 2 + i] : 0.0;
                        s += vx[q] * z0 + vy[q] * z1;
                    }
                }
                s = msdp_wave_sum(s) * tau;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    if (q < qn) {
                        const int i = 2 * lane + 128 * q;
                        if (i < m) z[kk + 1 + i] -= s * vx[q];
                        if (i + 1 < m) z[kk + 2 + i] -= s * vy[q];
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) cur[q] = nxt[q];
        }
        for (int i = lane; i < n; i += 64) a.vec[(r0 + i) * a.kld + c] = z[i];
    }
}

// workgroups of the kernel that are resident together on the CURRENT device (the handle's), kept per device
static int btl_capacity() {
    static int cap[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    const bool keep = dev >= 0 && dev < 64;
    if (keep && cap[dev]) return cap[dev];
    int cus = 0, per_cu = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1 ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_block_tridiag_group, BTL_THREADS, 0) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        return 0;
    }
    if (keep) cap[dev] = per_cu * cus;
    return per_cu * cus;
}

extern "C" int msdp_block_eigs_large(msdp_handle h, int32_t nb, const int64_t* row0, const int64_t* nblk, int32_t k, double* w, double* V) {
    if (!h) { msdp_set_error("null handle"); return MSDP_EINVAL; }
    if (nb < 1 || !row0 || !nblk || !w || (k > 0 && !V) || k < 0) { msdp_set_error("block_eigs_large: bad argument"); return MSDP_EINVAL; }
    if (k > BTL_MAXK) { msdp_set_error("block_eigs_large: at most %d eigenvectors per block (%d asked for)", BTL_MAXK, (int)k); return MSDP_EUNSUPPORTED; }
    if (h->d.costkind != COST_AFFINE || !h->dual_valid) { msdp_set_error("block_eigs_large: call msdp_al_dual first"); return MSDP_ESTATE; }
    const int N = h->d.n, nS = msdp_dense_nS(N);
    const int force = h->tune.blk_groups;
    std::vector<BtlBlock> blk(nb);
    int64_t atot = 0, etot = 0, rows = 0;
    int wgs = 0;
    for (int b = 0; b < nb; ++b) {
        if (nblk[b] < 1) { msdp_set_error("block_eigs_large: block %d has order %lld", b, (long long)nblk[b]); return MSDP_EINVAL; }
        if (nblk[b] > BTL_MAXN) { msdp_set_error("block_eigs_large: block orders up to %d (block %d has %lld)", BTL_MAXN, b, (long long)nblk[b]); return MSDP_EUNSUPPORTED; }
        if (row0[b] < 0 || row0[b] + nblk[b] > N) { msdp_set_error("block_eigs_large: block %d outside the matrix", b); return MSDP_EINVAL; }
        BtlBlock& B = blk[b];
        if (h->blocked) {
            int rc = msdp_affine_block_source(h, row0[b], nblk[b], &B.soff, &B.sld);
            if (rc == MSDP_EINVAL) msdp_set_error("block_eigs_large: rows %lld..%lld (block %d) are not one block of this handle", (long long)row0[b], (long long)(row0[b] + nblk[b]), b);
            if (rc) return rc;
        } else { B.soff = row0[b] * nS + row0[b]; B.sld = nS; }
        B.n = (int)nblk[b]; B.ld = (B.n + 15) & ~15; B.pad = 0;
        B.G = B.n <= BTL_ONE_WG ? 1 : (force > 0 ? std::min(force, BTL_MAXG) : std::min(BTL_MAXG, (B.n + 31) / 32));
        B.aoff = atot; B.eoff = etot; B.r0 = rows;
        atot += (int64_t)B.n * B.ld; etot += BTL_EX(B.ld); rows += B.n; wgs += B.G;
    }
    const int cap = btl_capacity();
    if (cap < BTL_MAXG) { msdp_set_error("block_eigs_large: the occupancy query failed"); return MSDP_EHIP; }
    // launches: blocks in call order, as many as are resident together
    std::vector<int2> wg;
    std::vector<int> first(1, 0);
    wg.reserve(wgs);
    for (int b = 0, used = 0; b < nb; ++b) {
        if (used + blk[b].G > cap) { first.push_back((int)wg.size()); used = 0; }
        for (int q = 0; q < blk[b].G; ++q) wg.push_back(make_int2(b, q));
        used += blk[b].G;
    }
    first.push_back((int)wg.size());
    const int kk = k > 0 ? k : 1;
    // one workspace, carved into 256-byte aligned pieces
    size_t need = 0;
    auto piece = [&](size_t bytes) { const size_t o = need; need += (bytes + 255) / 256 * 256; return o; };
    const size_t o_blk = piece(nb * sizeof(BtlBlock)), o_wg = piece(wg.size() * sizeof(int2));
    const size_t o_A = piece((size_t)atot * sizeof(double)), o_R = piece((size_t)atot * sizeof(double));
    const size_t e_bytes = (size_t)etot * sizeof(double) + 256;   // the exchange regions and the error word behind them
    const size_t o_E = piece(e_bytes);
    const size_t o_w = piece((size_t)rows * sizeof(double)), o_vec = piece((size_t)rows * kk * sizeof(double));
    if (h->blk_ws_cap < need) {
        msdp_block_eigs_release(h);
        if (hipMalloc(&h->blk_ws, need) != hipSuccess) { (void)hipGetLastError(); h->blk_ws = nullptr; msdp_set_error("block_eigs_large: device allocation of %zu bytes failed", need); return MSDP_ENOMEM; }
        h->blk_ws_cap = need;
    }
    char* base = (char*)h->blk_ws;
    BtlArgs a;
    a.k = k; a.kld = kk; a.S = h->d.Sdual;
    a.blk = (const BtlBlock*)(base + o_blk);
    a.A = (double*)(base + o_A); a.Rf = (double*)(base + o_R); a.E = (double*)(base + o_E);
    a.w = (double*)(base + o_w); a.vec = (double*)(base + o_vec);
    a.err = (int*)(base + o_E + (size_t)etot * sizeof(double));
    HIPCHK(msdp_memcpy_async(base + o_blk, blk.data(), nb * sizeof(BtlBlock), hipMemcpyHostToDevice, h->stream));
    HIPCHK(msdp_memcpy_async(base + o_wg, wg.data(), wg.size() * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(base + o_E, 0, e_bytes, h->stream));     // counters and the error word
    HIPCHK(hipStreamSynchronize(h->stream));                       // (the tables are locals of this call)
    hipError_t e = hipSuccess;
    for (size_t l = 0; l + 1 < first.size() && e == hipSuccess; ++l) {
        a.wg = (const int2*)(base + o_wg) + first[l];
        hipLaunchKernelGGL(k_block_tridiag_group, dim3(first[l + 1] - first[l]), dim3(BTL_THREADS), 0, h->stream, a);
        e = hipGetLastError();
    }
    h->blk_launches = (int)first.size() - 1; h->blk_wgs = wgs;
    int err = 0;
    if (e == hipSuccess) e = msdp_memcpy_async(w, a.w, rows * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && k > 0) e = msdp_memcpy_async(V, a.vec, rows * k * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = msdp_memcpy_async(&err, a.err, sizeof(int), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { msdp_set_error("block_eigs_large: %s", hipGetErrorString(e)); return MSDP_EHIP; }
    if (err) { msdp_set_error("block_eigs_large: a group barrier timed out (the workgroups of a block were not resident together)"); return MSDP_ECOMM; }
    return 0;
}

extern "C" int msdp_block_eigs_large_info(msdp_handle h, int32_t* launches, int32_t* workgroups) {
    if (!h) { msdp_set_error("null handle"); return MSDP_EINVAL; }
    if (launches) *launches = h->blk_launches;
    if (workgroups) *workgroups = h->blk_wgs;
    return 0;
}
