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

// ---- the factor between two trustregions() calls (msdp_hfactor_gram / _rotate / _append): the complex algebra is real algebra
// on the real view, so all three run the kernels of msdp_factor_gram / _rotate / _append (msdp_kernels.hip) at real width 2p;
// only the host-side packing of G, Q and V is complex.
static int hfactor_check(msdp_handle h, const char* call) {
    if (h->d.costkind != COST_HERM) {
        msdp_set_error("%s: for Hermitian handles only (the real kinds take msdp_factor_gram / _rotate / _append, the block kinds msdp_blockfactor_*)", call);
        return MSDP_EUNSUPPORTED;
    }
    if (!h->have_point) { msdp_set_error("%s: no resident point", call); return MSDP_ESTATE; }
    return 0;
}

// G = Y^H Y from the real Gram matrix Gr of the real view: Re G_ab = Gr[2a,2b] + Gr[2a+1,2b+1], Im G_ab = Gr[2a,2b+1] - Gr[2a+1,2b]
extern "C" int msdp_hfactor_gram(msdp_handle h, double* G) {
    MSDP_CHECK_H(h);
    int rc = hfactor_check(h, "hfactor_gram");
    if (rc) return rc;
    if (!G) { msdp_set_error("hfactor_gram: null out"); return MSDP_EINVAL; }
    Dev& d = h->d;
    const int ld = d.ld, p = d.p / 2;
    const int nblk = (int)std::min<int64_t>(64, std::max<int64_t>(1, (int64_t)(1 << 22) / ((int64_t)ld * ld)));
    double* buf = nullptr;
    if ((rc = msdp_dev_alloc<double>(h, &buf, ((size_t)nblk + 1) * ld * ld))) return rc;
    double* out = buf + (size_t)nblk * ld * ld;
    std::vector<double> Gr((size_t)ld * ld);
    rc = msdp_k_fgram(h, d.Y[msdp_host_cur(h)], buf, nblk, out);
    if (!rc && msdp_memcpy_async(Gr.data(), out, Gr.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess) {
        msdp_set_error("hfactor_gram: D2H failed"); rc = MSDP_EHIP;
    }
    (void)hipStreamSynchronize(h->stream);
    msdp_dev_free(h, buf);
    if (rc) return rc;
    for (int a = 0; a < p; ++a)
        for (int b = 0; b < p; ++b) {
            G[2 * ((size_t)a * p + b)] = Gr[(size_t)(2 * a) * ld + 2 * b] + Gr[(size_t)(2 * a + 1) * ld + 2 * b + 1];
            G[2 * ((size_t)a * p + b) + 1] = Gr[(size_t)(2 * a) * ld + 2 * b + 1] - Gr[(size_t)(2 * a + 1) * ld + 2 * b];
        }
    return 0;
}

// Y <- Y Q: the real view times the 2p x 2r matrix with the block [qr, qi; -qi, qr] per complex q_ab
extern "C" int msdp_hfactor_rotate(msdp_handle h, int32_t r, const double* Q) {
    MSDP_CHECK_H(h);
    int rc = hfactor_check(h, "hfactor_rotate");
    if (rc) return rc;
    Dev& d = h->d;
    const int p = d.p / 2;
    if (!Q || r < 1 || r > p) { msdp_set_error("hfactor_rotate: r = %d outside 1..p = %d, or null Q", r, p); return MSDP_EINVAL; }
    std::vector<double> Qr((size_t)4 * p * r);
    const size_t ldq = (size_t)2 * r;
    for (int a = 0; a < p; ++a)
        for (int b = 0; b < r; ++b) {
            const double qr = Q[2 * ((size_t)a * r + b)], qi = Q[2 * ((size_t)a * r + b) + 1];
            Qr[(size_t)(2 * a) * ldq + 2 * b] = qr;      Qr[(size_t)(2 * a) * ldq + 2 * b + 1] = qi;
            Qr[(size_t)(2 * a + 1) * ldq + 2 * b] = -qi; Qr[(size_t)(2 * a + 1) * ldq + 2 * b + 1] = qr;
        }
    const int cur = msdp_host_cur(h), rn = 2 * r;
    double* qd = nullptr;
    if ((rc = msdp_dev_alloc<double>(h, &qd, Qr.size()))) return rc;
    if (msdp_memcpy_async(qd, Qr.data(), Qr.size() * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess) {
        msdp_set_error("hfactor_rotate: H2D failed"); rc = MSDP_EHIP;
    }
    if (!rc) rc = msdp_k_frotate(h, msdp_rows_capacity(h), rn, rn, d.Y[cur], qd, d.Y[cur ^ 1]);
    (void)hipStreamSynchronize(h->stream);
    msdp_dev_free(h, qd);
    if (rc) return rc;
    return msdp_adopt_point(h, cur ^ 1, rn);
}

// Y <- rows_normalised([Y, alpha V]): k complex columns are 2k real ones (re, im of column c at real columns 2c, 2c + 1), and
// the real row norm is the complex one
extern "C" int msdp_hfactor_append(msdp_handle h, int32_t k, const double* V, double alpha) {
    MSDP_CHECK_H(h);
    int rc = hfactor_check(h, "hfactor_append");
    if (rc) return rc;
    Dev& d = h->d;
    if (!V || k < 1) { msdp_set_error("hfactor_append: k = %d, or null V", k); return MSDP_EINVAL; }
    if (d.p + 2 * k > h->pcap) {
        msdp_set_error("hfactor_append: width %d exceeds the allocated capacity %d (complex columns; use msdp_set_point)", d.p / 2 + k, h->pcap / 2);
        return MSDP_EUNSUPPORTED;
    }
    const int n = d.n, cur = msdp_host_cur(h), pn = d.p + 2 * k;
    std::vector<double> Vr((size_t)2 * k * n);
    for (int c = 0; c < k; ++c)
        for (int i = 0; i < n; ++i) {
            Vr[(size_t)(2 * c) * n + i] = V[2 * ((size_t)c * n + i)];
            Vr[(size_t)(2 * c + 1) * n + i] = V[2 * ((size_t)c * n + i) + 1];
        }
    double* vd = nullptr;
    if ((rc = msdp_dev_alloc<double>(h, &vd, Vr.size()))) return rc;
    if (msdp_memcpy_async(vd, Vr.data(), Vr.size() * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess) {
        msdp_set_error("hfactor_append: H2D failed"); rc = MSDP_EHIP;
    }
    if (!rc) rc = msdp_k_fappend(h, msdp_rows_capacity(h), 2 * k, pn, d.Y[cur], vd, alpha, 1, d.Y[cur ^ 1]);
    (void)hipStreamSynchronize(h->stream);
    msdp_dev_free(h, vd);
    if (rc) return rc;
    return msdp_adopt_point(h, cur ^ 1, pn);
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
