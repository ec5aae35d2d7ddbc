// msdp_beritz.hip -- the dense algebra of a Rayleigh-Ritz stage of the block eigen-solver (msdp_blockeig.hip) on the device.
//
// be_ritz (msdp_blockeig.hip) solves H c = theta G c for the b x b Gram matrices of the panel on ONE host thread: Cholesky of G,
// A = L^-1 H L^-T, tred2 / tql2 -- 0.45 ms at b = 64, behind a copy of 2 b^2 doubles and a synchronisation, in front of a copy of
// b^2 + b doubles back.  k_be_ritz<B> restates the Cholesky route of be_ritz step by step in ONE workgroup with the three b x b
// matrices (G -> L, H -> A, the rotation accumulator Q -> W) in LDS: 3 x 64 x 65 doubles = 97.5 KB at B = 64 (rows padded by one
// double), inside the 160 KB of a gfx950 workgroup.  B = 128 would need 387 KB and keeps the host stage.
//   * symmetrise G and H; any non-finite entry, or max diag G <= 0: status BREAKDOWN;
//   * lower Cholesky of G (right-looking, one column per step) with the host's pivot test s > 1e-11 max diag G; a failed pivot:
//     status FALLBACK (the host stage then takes the eigen-basis route that drops the dependent directions);
//   * A = L^-1 H L^-T by two forward substitutions (L^-1 H, transpose, L^-1 again), symmetrised;
//   * eig(A) by cyclic two-sided Jacobi with the round-robin pairing of k_block_jacobi (msdp_blockjacobi.hip): B/2 disjoint
//     rotations per round, B - 1 rounds per sweep.  Thread (k1, k2) of the (B/2)^2 applies the rotations of pairs k1 (rows) and
//     k2 (columns) to the 2 x 2 block they meet in; only k1 <= k2 compute, and write the mirrored block too, so A stays EXACTLY
//     symmetric and one barrier separates the rotation angles of a round from their application.  After the first stage of a
//     call the panel consists of filtered Ritz vectors and A is nearly diagonal: few sweeps (quadratic convergence).  Stop at
//     off(A)^2 <= 1e-30 |A|_F^2; 40 sweeps without it: status FALLBACK (and the bound that ends the loops on any data);
//   * eigenvalues ranked ascending by counting (ties by index), W = L^-T Q by back substitution, columns stored in rank order.
// Every sum runs in a fixed order and nothing is atomic: the same input gives the same bits on every run.
// Measured: about 1 ms per stage at B = 64 -- some 1 500 barrier-separated steps of one workgroup, each a few
// hundred cycles of dependent LDS reads and divide / square-root chains -- against 0.45 ms of host algebra plus two small copies:
// the option that selects it (escape_rr = 1) is off by default.
#include "msdp_device.h"
#include <cstring>
#include <vector>

#define BER_MAXSWEEP 40

// M <- L^-1 M (L lower triangular in the lower triangle of Lm, diagonal included; both B x B with row stride B + 1)
template <int B, int NT>
__device__ __forceinline__ void ber_forward(const double* __restrict__ Lm, double* __restrict__ M, int tid) {
    constexpr int LD = B + 1;
    for (int k = 0; k < B; ++k) {
        if (tid < B) M[k * LD + tid] /= Lm[k * LD + k];
        __syncthreads();
        const int m = B - 1 - k;
        for (int e = tid; e < m * B; e += NT) {
            const int a = e / B, c = e - a * B, i = k + 1 + a;
            M[i * LD + c] -= Lm[i * LD + k] * M[k * LD + c];
        }
        __syncthreads();
    }
}

// gin: G then H (B x B row-major each, as k_be_gram_sum leaves them; not modified).  Wd: W (B x B row-major, column j = Ritz
// vector j), then theta[B] -- the layout k_be_rotate reads.  rec: theta[B], (res[B]: k_be_res_sum), rank, status (all doubles).
template <int B>
__global__ __launch_bounds__((B / 2) * (B / 2)) void k_be_ritz(const double* __restrict__ gin, double* __restrict__ Wd, double* __restrict__ rec) {
    constexpr int HALF = B / 2, NT = HALF * HALF, NW = NT / 64, LD = B + 1;
    extern __shared__ double lds[];
    double* G = lds;                                   // G, then its Cholesky factor in the lower triangle
    double* A = G + B * LD;                            // H, then A = L^-1 H L^-T, then its diagonal form
    double* Q = A + B * LD;                            // the accumulated rotations, then W = L^-T Q
    __shared__ double cc[HALF], ss[HALF], tt[HALF], red[2 * NW], dg[B];
    __shared__ int pp[HALF], qq[HALF], rk[B];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int nbad = 0;
    for (int e = tid; e < B * B; e += NT) {
        const int i = e / B, j = e - i * B;
        const double g = 0.5 * (gin[i * B + j] + gin[j * B + i]);
        const double h = 0.5 * (gin[B * B + i * B + j] + gin[B * B + j * B + i]);
        G[i * LD + j] = g; A[i * LD + j] = h; Q[i * LD + j] = (i == j) ? 1.0 : 0.0;
        nbad += (isfinite(g) && isfinite(h)) ? 0 : 1;
    }
    const int anybad = __syncthreads_or(nbad);
    double dmax = 0.0;
    for (int i = 0; i < B; ++i) dmax = fmax(dmax, G[i * LD + i]);
    // (every exit below is taken by all threads together: the tests read LDS words behind a barrier)
    if (anybad || !(dmax > 0.0)) {
        if (tid == 0) { rec[2 * B] = 0.0; rec[2 * B + 1] = (double)MSDP_RITZ_BREAKDOWN; }
        return;
    }
    // ---- G = L L'
    for (int j = 0; j < B; ++j) {
        const double s = G[j * LD + j];
        if (!(s > 1e-11 * dmax)) {
            if (tid == 0) { rec[2 * B] = 0.0; rec[2 * B + 1] = (double)MSDP_RITZ_FALLBACK; }
            return;
        }
        const double ljj = sqrt(s);
        __syncthreads();
        if (tid == j) G[j * LD + j] = ljj;
        else if (tid > j && tid < B) G[tid * LD + j] /= ljj;
        __syncthreads();
        const int m = B - 1 - j;
        for (int e = tid; e < m * m; e += NT) {
            const int a = e / m, c = e - a * m;
            if (c <= a) { const int i = j + 1 + a, k = j + 1 + c; G[i * LD + k] -= G[i * LD + j] * G[k * LD + j]; }
        }
        __syncthreads();
    }
    // ---- A = L^-1 H L^-T
    ber_forward<B, NT>(G, A, tid);
    for (int e = tid; e < B * B; e += NT) {
        const int i = e / B, j = e - i * B;
        if (i < j) { const double x = A[i * LD + j]; A[i * LD + j] = A[j * LD + i]; A[j * LD + i] = x; }
    }
    __syncthreads();
    ber_forward<B, NT>(G, A, tid);
    for (int e = tid; e < B * B; e += NT) {
        const int i = e / B, j = e - i * B;
        if (i < j) { const double x = 0.5 * (A[i * LD + j] + A[j * LD + i]); A[i * LD + j] = x; A[j * LD + i] = x; }
    }
    __syncthreads();
    // ---- A <- J'AJ, Q <- QJ until A is diagonal
    bool conv = false;
    for (int sweep = 0; ; ++sweep) {
        double off = 0.0, tot = 0.0;
        for (int e = tid; e < B * B; e += NT) {
            const int i = e / B, j = e - i * B;
            const double v = A[i * LD + j] * A[i * LD + j];
            tot += v;
            if (i != j) off += v;
        }
        off = msdp_wave_sum(off); tot = msdp_wave_sum(tot);
        if (lane == 0) { red[wave] = off; red[NW + wave] = tot; }
        __syncthreads();
        double o2 = 0.0, t2 = 0.0;
        for (int q = 0; q < NW; ++q) { o2 += red[q]; t2 += red[NW + q]; }
        conv = o2 <= 1e-30 * t2;
        __syncthreads();                                  // (red is written again by the next sweep)
        if (conv || sweep == BER_MAXSWEEP) break;
        for (int r = 0; r < B - 1; ++r) {
            if (tid < HALF) {
                // round-robin pairing of B players: player B - 1 stays, the others rotate
                int p, q;
                if (tid == 0) { p = B - 1; q = r; }
                else { p = (r + tid) % (B - 1); q = (r - tid + (B - 1)) % (B - 1); }
                if (p > q) { const int t = p; p = q; q = t; }
                double c = 1.0, s = 0.0, t = 0.0;
                const double apq = A[p * LD + q];
                if (apq != 0.0) {
                    const double tau = (A[q * LD + q] - A[p * LD + p]) / (2.0 * apq);
                    t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = t * c;
                }
                pp[tid] = p; qq[tid] = q; cc[tid] = c; ss[tid] = s; tt[tid] = t;
            }
            __syncthreads();
            {
                const int k1 = tid / HALF, k2 = tid - k1 * HALF;
                if (k1 == k2) {
                    const int p = pp[k1], q = qq[k1];
                    const double d = tt[k1] * A[p * LD + q];
                    A[p * LD + p] -= d; A[q * LD + q] += d;
                    A[p * LD + q] = 0.0; A[q * LD + p] = 0.0;
                } else if (k1 < k2) {
                    const int p1 = pp[k1], q1 = qq[k1], p2 = pp[k2], q2 = qq[k2];
                    const double c1 = cc[k1], s1 = ss[k1], c2 = cc[k2], s2 = ss[k2];
                    const double a = A[p1 * LD + p2], b = A[p1 * LD + q2], c = A[q1 * LD + p2], d = A[q1 * LD + q2];
                    const double ra = c1 * a - s1 * c, rb = c1 * b - s1 * d, rc = s1 * a + c1 * c, rd = s1 * b + c1 * d;   // rows p1, q1
                    const double na = c2 * ra - s2 * rb, nb = s2 * ra + c2 * rb, nc = c2 * rc - s2 * rd, nd = s2 * rc + c2 * rd;   // columns p2, q2
                    A[p1 * LD + p2] = na; A[p1 * LD + q2] = nb; A[q1 * LD + p2] = nc; A[q1 * LD + q2] = nd;
                    A[p2 * LD + p1] = na; A[q2 * LD + p1] = nb; A[p2 * LD + q1] = nc; A[q2 * LD + q1] = nd;
                }
            }
            for (int e = tid; e < B * HALF; e += NT) {
                const int i = e / HALF, k = e - i * HALF;
                const int p = pp[k], q = qq[k];
                const double c = cc[k], s = ss[k];
                const double vp = Q[i * LD + p], vq = Q[i * LD + q];
                Q[i * LD + p] = c * vp - s * vq; Q[i * LD + q] = s * vp + c * vq;
            }
            __syncthreads();
        }
    }
    if (!conv) {
        if (tid == 0) { rec[2 * B] = 0.0; rec[2 * B + 1] = (double)MSDP_RITZ_FALLBACK; }
        return;
    }
    // ---- theta ascending (rank by counting, ties by index), W = L^-T Q
    if (tid < B) dg[tid] = A[tid * LD + tid];
    __syncthreads();
    if (tid < B) {
        const double v = dg[tid];
        int rnk = 0;
        for (int j = 0; j < B; ++j) rnk += (dg[j] < v || (dg[j] == v && j < tid)) ? 1 : 0;
        rk[tid] = rnk;
    }
    for (int k = B - 1; k >= 0; --k) {
        if (tid < B) Q[k * LD + tid] /= G[k * LD + k];
        __syncthreads();
        for (int e = tid; e < k * B; e += NT) {
            const int i = e / B, c = e - i * B;
            Q[i * LD + c] -= G[k * LD + i] * Q[k * LD + c];
        }
        __syncthreads();
    }
    for (int e = tid; e < B * B; e += NT) {
        const int i = e / B, j = e - i * B;
        Wd[i * B + rk[j]] = Q[i * LD + j];
    }
    if (tid < B) { Wd[B * B + rk[tid]] = dg[tid]; rec[rk[tid]] = dg[tid]; }
    if (tid == 0) { rec[2 * B] = (double)B; rec[2 * B + 1] = (double)MSDP_RITZ_OK; }
}

template <int B>
static int ber_launch(hipStream_t stream, const double* gout, double* Wd, double* rec) {
    constexpr int NT = (B / 2) * (B / 2);
    constexpr size_t lds = (size_t)3 * B * (B + 1) * sizeof(double);
    static bool attr_set = false;
    if (!attr_set) {
        HIPCHK(hipFuncSetAttribute((const void*)k_be_ritz<B>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set = true;
    }
    hipLaunchKernelGGL((k_be_ritz<B>), dim3(1), dim3(NT), lds, stream, gout, Wd, rec);
    HIPCHK(hipGetLastError());
    return 0;
}

int msdp_beritz_supported(int b) { return b == 32 || b == 64; }

int msdp_beritz_launch(hipStream_t stream, int b, const double* gout, double* Wd, double* rec) {
    if (b == 32) return ber_launch<32>(stream, gout, Wd, rec);
    if (b == 64) return ber_launch<64>(stream, gout, Wd, rec);
    msdp_set_error("device Rayleigh-Ritz stage: block widths 32 and 64 (got %d)", b);
    return MSDP_EUNSUPPORTED;
}

// ---------------------------------------------------------------- test-only entry point: the kernel alone, no handle, no fallback
extern "C" int msdp_debug_ritz_device(int32_t b, const double* G, const double* H, double* theta, double* W, int32_t* rank, int32_t* status) {
    if (!G || !H || !theta || !W || !rank || !status) { msdp_set_error("debug_ritz_device: bad argument"); return MSDP_EINVAL; }
    if (!msdp_beritz_supported(b)) { msdp_set_error("debug_ritz_device: block widths 32 and 64 (got %d)", b); return MSDP_EUNSUPPORTED; }
    const size_t bb = (size_t)b * b, nrec = (size_t)2 * b + 2, tot = 2 * bb + bb + b + nrec;
    double* dev = nullptr;
    if (hipMalloc((void**)&dev, tot * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); msdp_set_error("debug_ritz_device: device allocation failed"); return MSDP_ENOMEM; }
    double* Wd = dev + 2 * bb;
    double* rec = Wd + bb + b;
    std::vector<double> host(bb + b + nrec, 0.0);
    hipError_t e = msdp_memcpy(dev, G, bb * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = msdp_memcpy(dev + bb, H, bb * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = msdp_memcpy(Wd, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice);   // zeros: a stopped kernel writes no W
    int rc = 0;
    if (e == hipSuccess) rc = msdp_beritz_launch(nullptr, b, dev, Wd, rec);
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess && !rc) e = msdp_memcpy(host.data(), Wd, host.size() * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(dev);
    if (rc) return rc;
    if (e != hipSuccess) { msdp_set_error("debug_ritz_device: %s", hipGetErrorString(e)); return MSDP_EHIP; }
    memcpy(W, host.data(), bb * sizeof(double));
    memcpy(theta, host.data() + bb, (size_t)b * sizeof(double));
    *rank = (int32_t)host[bb + b + 2 * b];
    *status = (int32_t)host[bb + b + 2 * b + 1];
    return 0;
}
