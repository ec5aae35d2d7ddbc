// msdp_hermitian.hip -- the complex unit-diagonal problem  min <C, X>  s.t. X Hermitian PSD, X_ii = 1  with a sparse Hermitian
// cost matrix C = A + iB (COST_HERM, msdp_create_onlyunitdiag_csc_hermitian; manopt's elliptope_SDP_complex).
//
// A factor row of complex width p is a run of p double2, one complex number each, and crosses the C ABI as its real view of
// 2p doubles (d.p = d.ld = 2p).  Re<u, v> on C^p is the real inner product of the two views, so projection, retraction and all
// tCG / RTR bookkeeping kernels run unchanged; what differs is the product with C: the row kernels of msdp_kernels.hip gather
// through spmm_row_herm (msdp_device.h) instead of spmm_row, and the escape applies S = C - diag(z) to a complex vector here.
//
// Storage: the caller's CSC arrays are read as CSR, as for the real kinds, but row i of a Hermitian C is the CONJUGATE of
// column i -- invisible for real C, the sign of B otherwise.  The values live beside rowptr / colind as double2 (d.hzv), and in
// the fixed-width ELL form (d.hzell beside d.ellc, padded with (row, 0 + 0i)) where no row has more than 8 entries.  d.cval and
// d.ellv stay null on such a handle: nothing may read its values as real.
#include "msdp_device.h"
#include <algorithm>
#include <vector>

// w = C v - z .* v for a complex vector (v, w: n double2; z real).  One thread per row, entries in column order, the real-part
// product first (the order of spmm_row_herm).
__global__ void k_sv_herm(int n, const int* __restrict__ rp, const int* __restrict__ ci, const double2* __restrict__ cv,
                          const double* __restrict__ z, const double2* __restrict__ v, double2* __restrict__ w) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double2 acc = make_double2(0.0, 0.0);
        for (int t = rp[i]; t < rp[i + 1]; ++t) {
            const double2 c = cv[t], x = v[ci[t]];
            acc.x = fma(c.x, x.x, acc.x); acc.x = fma(-c.y, x.y, acc.x);
            acc.y = fma(c.x, x.y, acc.y); acc.y = fma(c.y, x.x, acc.y);
        }
        const double zi = z[i];
        const double2 vi = v[i];
        w[i] = make_double2(acc.x - zi * vi.x, acc.y - zi * vi.y);
    }
}

// w = i * v
__global__ void k_herm_jcopy(int n, const double2* __restrict__ v, double2* __restrict__ w) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double2 x = v[i];
        w[i] = make_double2(-x.y, x.x);
    }
}

int msdp_hermitian_sv(msdp_handle h, const double* z, const double* v, double* w) {
    const Dev& d = h->d;
    if (d.costkind != COST_HERM || !d.hzv) { msdp_set_error("Hermitian product: not a Hermitian handle"); return MSDP_ESTATE; }
    hipLaunchKernelGGL(k_sv_herm, dim3((d.n + 255) / 256), dim3(256), 0, h->stream, d.n, d.rowptr, d.colind, d.hzv, z,
                       reinterpret_cast<const double2*>(v), reinterpret_cast<double2*>(w));
    HIPCHK(hipGetLastError());
    return 0;
}

int msdp_hermitian_jcopy(msdp_handle h, const double* v, double* w) {
    const Dev& d = h->d;
    hipLaunchKernelGGL(k_herm_jcopy, dim3((d.n + 255) / 256), dim3(256), 0, h->stream, d.n, reinterpret_cast<const double2*>(v),
                       reinterpret_cast<double2*>(w));
    HIPCHK(hipGetLastError());
    return 0;
}

// h_rowptr / h_colind hold the pattern (column j of the CSC input = row j); val: nnz (re, im) pairs in the same order.
int msdp_hermitian_setup(msdp_handle h, const double* val) {
    Dev& d = h->d;
    if (h->nranks != 1 || h->use_comm || d.n_loc != d.n) { msdp_set_error("Hermitian cost: single-rank handles only"); return MSDP_EUNSUPPORTED; }
    const int n = d.n;
    const std::vector<int>& rp = h->h_rowptr;
    const int64_t nnz = rp[n];
    // row i = conj(column i)
    std::vector<double2> cv((size_t)nnz);
    for (int64_t t = 0; t < nnz; ++t) cv[(size_t)t] = make_double2(val[2 * t], -val[2 * t + 1]);
    int rc;
    double2* dzv = nullptr;
    if ((rc = msdp_dev_alloc<int>(h, &h->d_rowptr, (size_t)n + 1)) || (rc = msdp_dev_alloc<int>(h, &h->d_colind, (size_t)nnz)) ||
        (rc = msdp_dev_alloc<double2>(h, &dzv, (size_t)nnz))) return rc;
    HIPCHK(msdp_memcpy(h->d_rowptr, rp.data(), ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice));
    if (nnz) {
        HIPCHK(msdp_memcpy(h->d_colind, h->h_colind.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(msdp_memcpy(dzv, cv.data(), (size_t)nnz * sizeof(double2), hipMemcpyHostToDevice));
    }
    d.rowptr = h->d_rowptr; d.colind = h->d_colind; d.cval = nullptr; d.hzv = dzv; d.nnz = nnz;
    d.ellW = 0; d.ell_stride = 0; d.ellc = nullptr; d.ellv = nullptr; d.hzell = nullptr;
    // ELL copy when every row is short, stored width 5 or 8 as for the real kinds (msdp_upload_sparse_rows)
    int W = 0;
    for (int i = 0; i < n; ++i) W = std::max(W, rp[i + 1] - rp[i]);
    if (W >= 1 && W <= MSDP_ELL_MAXW) {
        W = W <= 5 ? 5 : 8;
        const size_t cap = (size_t)n;
        std::vector<int> ec((size_t)W * cap);
        std::vector<double2> ev((size_t)W * cap, make_double2(0.0, 0.0));
        for (int w = 0; w < W; ++w)
            for (size_t i = 0; i < cap; ++i) ec[(size_t)w * cap + i] = (int)i;
        for (int i = 0; i < n; ++i)
            for (int t = rp[i]; t < rp[i + 1]; ++t) {
                const int w = t - rp[i];
                ec[(size_t)w * cap + i] = h->h_colind[t];
                ev[(size_t)w * cap + i] = cv[(size_t)t];
            }
        double2* dze = nullptr;
        if ((rc = msdp_dev_alloc<int>(h, &h->d_ellc, ec.size())) || (rc = msdp_dev_alloc<double2>(h, &dze, ev.size()))) return rc;
        HIPCHK(msdp_memcpy(h->d_ellc, ec.data(), ec.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(msdp_memcpy(dze, ev.data(), ev.size() * sizeof(double2), hipMemcpyHostToDevice));
        d.ellW = W; d.ell_stride = (int64_t)cap; d.ellc = h->d_ellc; d.hzell = dze;
    }
    return 0;
}
