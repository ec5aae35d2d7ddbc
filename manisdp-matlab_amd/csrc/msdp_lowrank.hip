// msdp_lowrank.hip -- the low-rank term of a sparse-plus-low-rank cost matrix C = Cs + V diag(s) V' (COST_SPLR,
// msdp_create_onlyunitdiag_csc_lowrank; ManiSDP_onlyunitdiag.m:6 with C held implicitly).
//
// A product C*X with a gather source X (n x ld) is the sparse product of the row kernels (msdp_kernels.hip) plus V*T with
// T = diag(s) V' X (q x ld).  T is formed here, in front of the row launch, by a deterministic two-stage reduction
// (per-workgroup partials, then a sum in index order: no floating-point atomics); the row kernels add sum_k V[row,k] T[k,:]
// to a row's accumulator right behind its sparse gather.  The projection writes only its own scratch (d.lrTp, d.lrT), so it
// runs unconditionally: the ctl->done / F[0].active gates of the row kernels need no counterpart.
#include "msdp_device.h"
#include <vector>

#define LR_THREADS 256

// part[b][k][col] = sum over the rows of workgroup b of V[row,k] * X[row,col].  CW = pow2 >= ld columns (at most LR_THREADS) are
// served side by side by RS = LR_THREADS / CW row slices; a thread holds the q sums of its column over the rows of its
// slice (X is read once), the slices are added in slice order through the LDS.
__global__ __launch_bounds__(LR_THREADS) void k_lr_part(int n, int ld, int q, const double* __restrict__ V, const double* __restrict__ X,
                                                        double* __restrict__ part) {
    __shared__ double sh[MSDP_LOWRANK_MAX * LR_THREADS];
    const int rows = (n + (int)gridDim.x - 1) / (int)gridDim.x;
    const int r0 = min(n, (int)blockIdx.x * rows), r1 = min(n, r0 + rows);
    int CW = 1;
    while (CW < ld && CW < LR_THREADS) CW <<= 1;
    const int RS = LR_THREADS / CW;
    const int tid = threadIdx.x, c = tid & (CW - 1), rs = tid / CW;
    for (int c0 = 0; c0 < ld; c0 += CW) {
        const int col = c0 + c;
        double acc[MSDP_LOWRANK_MAX];
#pragma unroll
        for (int k = 0; k < MSDP_LOWRANK_MAX; ++k) acc[k] = 0.0;
        if (col < ld) {
            // four row steps per trip, every load of the four issued before the first is consumed (a plain loop keeps one row in
            // flight per thread and the launch becomes a chain of memory round trips); the additions stay in row order
            int row = r0 + rs;
            for (; row + 3 * RS < r1; row += 4 * RS) {
                double x[4], v[4][MSDP_LOWRANK_MAX];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    x[u] = X[(int64_t)(row + u * RS) * ld + col];
                    const double* __restrict__ vr = V + (int64_t)(row + u * RS) * q;
#pragma unroll
                    for (int k = 0; k < MSDP_LOWRANK_MAX; ++k) v[u][k] = k < q ? vr[k] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int k = 0; k < MSDP_LOWRANK_MAX; ++k)
                        if (k < q) acc[k] = fma(v[u][k], x[u], acc[k]);
                }
            }
            for (; row < r1; row += RS) {
                const double x = X[(int64_t)row * ld + col];
                const double* __restrict__ vr = V + (int64_t)row * q;
#pragma unroll
                for (int k = 0; k < MSDP_LOWRANK_MAX; ++k)
                    if (k < q) acc[k] = fma(vr[k], x, acc[k]);
            }
        }
        __syncthreads();                               // the previous column block's sums have been read
#pragma unroll
        for (int k = 0; k < MSDP_LOWRANK_MAX; ++k) sh[k * LR_THREADS + tid] = acc[k];
        __syncthreads();
        if (rs == 0 && col < ld) {
            for (int k = 0; k < q; ++k) {
                double s = 0.0;
                for (int r = 0; r < RS; ++r) s += sh[k * LR_THREADS + r * CW + c];
                part[((int64_t)blockIdx.x * q + k) * ld + col] = s;
            }
        }
    }
}

// T[k][col] = s[k] * sum_b part[b][k][col], the workgroups' partials in index order
__global__ void k_lr_sum(int ld, int q, int nblk, const double* __restrict__ s, const double* __restrict__ part, double* __restrict__ T) {
    const int tot = q * ld;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += gridDim.x * blockDim.x) {
        // 32 partials requested together, added in index order (the same bits as a plain loop, which would keep one load in flight)
        double acc = 0.0;
        for (int b = 0; b < nblk; b += 32) {
            double v[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) v[u] = (b + u < nblk) ? part[(int64_t)(b + u) * tot + e] : 0.0;
#pragma unroll
            for (int u = 0; u < 32; ++u) if (b + u < nblk) acc += v[u];
        }
        T[e] = s[e / ld] * acc;
    }
}

// w[i] += sum_k V[i,k] * t[k]
__global__ void k_lr_vadd(int n, int q, const double* __restrict__ V, const double* __restrict__ t, double* __restrict__ w) {
    double tk[MSDP_LOWRANK_MAX];
#pragma unroll
    for (int k = 0; k < MSDP_LOWRANK_MAX; ++k) tk[k] = k < q ? t[k] : 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double* __restrict__ vr = V + (int64_t)i * q;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < MSDP_LOWRANK_MAX; ++k)
            if (k < q) acc = fma(vr[k], tk[k], acc);
        w[i] += acc;
    }
}

static int lr_project(msdp_handle h, int n, int ld, const double* X) {
    const Dev& d = h->d;
    const int nblk = std::max(1, std::min(MSDP_LR_PARTS, (n + 127) / 128));
    hipLaunchKernelGGL(k_lr_part, dim3(nblk), dim3(LR_THREADS), 0, h->stream, n, ld, d.lrq, d.lrV, X, d.lrTp);
    hipLaunchKernelGGL(k_lr_sum, dim3((d.lrq * ld + 255) / 256), dim3(256), 0, h->stream, ld, d.lrq, nblk, d.lrs, (const double*)d.lrTp, d.lrT);
    HIPCHK(hipGetLastError());
    return 0;
}

int msdp_lowrank_project(msdp_handle h, const double* X) {
    const Dev& d = h->d;
    if (d.costkind != COST_SPLR || !d.lrT) { msdp_set_error("low-rank projection: not a sparse-plus-low-rank handle"); return MSDP_ESTATE; }
    if (d.ld > 1024) { msdp_set_error("low-rank projection: row stride %d exceeds the 1024 columns T and its partials are sized for", d.ld); return MSDP_EUNSUPPORTED; }
    return lr_project(h, d.n_loc, d.ld, X);
}

int msdp_lowrank_sv_add(msdp_handle h, const double* v, double* w) {
    const Dev& d = h->d;
    if (d.costkind != COST_SPLR || !d.lrT) { msdp_set_error("low-rank product: not a sparse-plus-low-rank handle"); return MSDP_ESTATE; }
    int rc = lr_project(h, d.n, 1, v);                  // a vector is a gather source of one column: t = s .* (V' v) in d.lrT
    if (rc) return rc;
    hipLaunchKernelGGL(k_lr_vadd, dim3((d.n + 255) / 256), dim3(256), 0, h->stream, d.n, d.lrq, d.lrV, (const double*)d.lrT, w);
    HIPCHK(hipGetLastError());
    return 0;
}

// V arrives n x q column-major (the MATLAB layout); the device copy is row-major.  T and its partials are sized for the
// widest factor the row kernels serve (ld = 1024), so that a growing factor never reallocates them.
int msdp_lowrank_setup(msdp_handle h, int q, const double* V, const double* s) {
    Dev& d = h->d;
    if (q < 1 || q > MSDP_LOWRANK_MAX || !V || !s) { msdp_set_error("low-rank term: q = %d outside 1 .. %d, or null V / s", q, MSDP_LOWRANK_MAX); return MSDP_EINVAL; }
    if (h->nranks != 1 || h->use_comm || d.n_loc != d.n) { msdp_set_error("low-rank term: single-rank handles only"); return MSDP_EUNSUPPORTED; }
    const size_t n = (size_t)d.n;
    std::vector<double> vt(n * q);
    for (int k = 0; k < q; ++k)
        for (size_t i = 0; i < n; ++i) vt[i * q + k] = V[(size_t)k * n + i];
    double *dV = nullptr, *ds = nullptr, *dT = nullptr, *dTp = nullptr;
    int rc;
    if ((rc = msdp_dev_alloc<double>(h, &dV, n * q)) || (rc = msdp_dev_alloc<double>(h, &ds, (size_t)q)) ||
        (rc = msdp_dev_alloc<double>(h, &dT, (size_t)q * 1024)) || (rc = msdp_dev_alloc<double>(h, &dTp, (size_t)MSDP_LR_PARTS * q * 1024))) return rc;
    HIPCHK(msdp_memcpy(dV, vt.data(), n * q * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(msdp_memcpy(ds, s, (size_t)q * sizeof(double), hipMemcpyHostToDevice));
    d.lrq = q; d.lrV = dV; d.lrs = ds; d.lrT = dT; d.lrTp = dTp;
    return 0;
}
