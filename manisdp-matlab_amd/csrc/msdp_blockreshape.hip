// msdp_blockreshape.hip -- rank cut and escape widening of every block of a multiblock factor, on the device.
//
// ManiSDP_multiblock.m:109-147 (ManiDSDP_multiblock.m:146-181) does, block by block and in every outer iteration: svd(Y_i), the rank
// r_i = #{e >= theta e_1} (the dual kinds: >), Y_i <- Y_i Q(:, 1:r_i), the number of escape directions from the negative eigenvalues
// of S_i, Y_i <- [Y_i, alpha V_i(:, 1:nne_i)] and the row normalisation of the blocks with unit diagonal.  With the factor packed
// as ONE (N, max p_i) array that is a download, nb small LAPACK calls, a re-pack and an upload per outer iteration.  Here one
// workgroup per block takes the decisions (k_breshape_decide: Gram matrix of the block's columns summed over its rows in row order,
// its eigen-decomposition by cyclic Jacobi in LDS, the counts) and one workgroup per block rewrites the block's rows
// (k_breshape_apply: one wave per row, a lane per column and its neighbour 64 further on).  The row stride of the resident factor is its width rounded up to
// even, and the width after the call is max_i p_i, known only when every block has decided: hence two launches with the counts
// read in between -- which is also where a growth beyond the allocated width is refused with nothing modified -- and hence the
// rows are written to the other point slot (as msdp_factor_rotate / msdp_factor_append do), not over themselves.
//
// The Jacobi iteration is k_block_jacobi's (msdp_blockjacobi.hip) on a p_i x p_i matrix in LDS: round-robin pairing, the
// rotations of a round in parallel, angle and stopping test from the symmetric part (the two triangles see
// different operation sequences and their difference does not shrink under the rotations).  A block's arithmetic depends on its
// own rows, its own width and its own eigen-data only: results are bit-reproducible and independent of the other blocks.
#include "msdp_device.h"
#include <vector>

#define BR_MAXP 64                 // G and Q of a block in LDS: 2 * 64 * 64 doubles = 64 KB of the CU's 160 KB (two workgroups per CU)
#define BR_THREADS 256
#define BR_WAVES (BR_THREADS / 64)
#define BR_MAXSWEEP 40

struct BrArgs {
    int k, strict, delta, min_facsize, mode, nob;
    double theta, alpha;
    const int64_t* r0;             // first row of block b in the factor (= in w and V)
    const int* n; const int* p_in;
    const int64_t* qoff;           // block b's p_in x p_in rotation: Q[qoff[b] + a * p_in + c], column c = c-th largest eigenvalue
    const double* w; const double* V;
    double* Q;
    int* p_out; int* r_out; int* nne_out; int* sweeps;
    const double* Y; int ld;       // resident point
    double* Yn; int ldn;           // the other slot, zero-filled, new row stride (k_breshape_apply only)
};

__global__ __launch_bounds__(BR_THREADS) void k_breshape_decide(BrArgs a) {
    extern __shared__ double br_lds[];                              // G (p x p), Q (p x p)
    __shared__ double cc[BR_MAXP / 2], ss[BR_MAXP / 2];
    __shared__ int pp[BR_MAXP / 2], qq[BR_MAXP / 2];
    __shared__ double red[2 * BR_WAVES];
    __shared__ double ev[BR_MAXP];
    __shared__ int rk[BR_MAXP];
    __shared__ int done, nneg_s, r_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n[b], p = a.p_in[b];
    const int64_t r0 = a.r0[b];
    if (tid == 0) { nneg_s = 0; r_s = p; }
    __syncthreads();
    if (n < a.min_facsize) {                                        // ManiSDP_multiblock.m:110: the block is left as it is
        if (tid == 0) { a.p_out[b] = p; a.r_out[b] = p; a.nne_out[b] = 0; a.sweeps[b] = 0; }
        return;
    }
    {
        int cnt = 0;
        for (int i = tid; i < n; i += BR_THREADS) cnt += a.w[r0 + i] < 0.0 ? 1 : 0;
        if (cnt) atomicAdd(&nneg_s, cnt);                           // (integers: the order does not matter)
    }
    int sweep = 0;
    if (p > 1) {
        double* __restrict__ G = br_lds;
        double* __restrict__ Q = br_lds + p * p;
        const double* __restrict__ Y = a.Y + r0 * a.ld;
        for (int e = tid; e < p * p; e += BR_THREADS) {
            const int i = e / p, j = e - i * p;
            double acc = 0.0;
            for (int t = 0; t < n; ++t) acc = fma(Y[(int64_t)t * a.ld + i], Y[(int64_t)t * a.ld + j], acc);
            G[e] = acc;
            Q[e] = (i == j) ? 1.0 : 0.0;
        }
        __syncthreads();
        const int m = p + (p & 1), half = m >> 1;
        for (; sweep < BR_MAXSWEEP; ++sweep) {
            double off = 0.0, tot = 0.0;
            for (int e = tid; e < p * p; e += BR_THREADS) {
                const int i = e / p, j = e - i * p;
                tot += G[e] * G[e];
                if (i != j) { const double o = 0.5 * (G[e] + G[j * p + i]); off += o * o; }
            }
            off = msdp_wave_sum(off); tot = msdp_wave_sum(tot);
            if (lane == 0) { red[wave] = off; red[BR_WAVES + wave] = tot; }
            __syncthreads();
            if (tid == 0) {
                double o2 = 0.0, t2 = 0.0;
                for (int q = 0; q < BR_WAVES; ++q) { o2 += red[q]; t2 += red[BR_WAVES + q]; }
                done = (o2 <= 1e-30 * t2) ? 1 : 0;
            }
            __syncthreads();
            if (done) break;
            for (int r = 0; r < m - 1; ++r) {
                if (tid < half) {
                    int u, v;
                    if (tid == 0) { u = m - 1; v = r; }
                    else { u = (r + tid) % (m - 1); v = (r - tid + (m - 1)) % (m - 1); }
                    if (u > v) { const int t = u; u = v; v = t; }
                    double c = 1.0, s = 0.0;
                    if (v < p) {                                    // (v == p: the dummy player of an odd width)
                        const double apq = 0.5 * (G[u * p + v] + G[v * p + u]);
                        if (apq != 0.0) {
                            const double tau = (G[v * p + v] - G[u * p + u]) / (2.0 * apq);
                            const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                            c = 1.0 / sqrt(1.0 + t * t);
                            s = t * c;
                        }
                    } else v = u;
                    pp[tid] = u; qq[tid] = v; cc[tid] = c; ss[tid] = s;
                }
                __syncthreads();
                for (int e = tid; e < p * half; e += BR_THREADS) {  // columns u, v of G and Q: every item owns its two entries per matrix
                    const int i = e / half, k2 = e - i * half;
                    const int u = pp[k2], v = qq[k2];
                    if (u == v) continue;
                    const double c = cc[k2], s = ss[k2];
                    const double gu = G[i * p + u], gv = G[i * p + v], qu = Q[i * p + u], qv = Q[i * p + v];
                    G[i * p + u] = c * gu - s * gv; G[i * p + v] = s * gu + c * gv;
                    Q[i * p + u] = c * qu - s * qv; Q[i * p + v] = s * qu + c * qv;
                }
                __syncthreads();
                for (int e = tid; e < half * p; e += BR_THREADS) {  // rows u, v of G
                    const int k2 = e / p, j = e - k2 * p;
                    const int u = pp[k2], v = qq[k2];
                    if (u == v) continue;
                    const double c = cc[k2], s = ss[k2];
                    const double gu = G[u * p + j], gv = G[v * p + j];
                    G[u * p + j] = c * gu - s * gv; G[v * p + j] = s * gu + c * gv;
                }
                __syncthreads();
            }
        }
        // e = sqrt(max(lambda, 0)), descending (ties by index); r = #{e >= theta e_1} or #{e > theta e_1}, at least 1 (:112-121)
        if (tid < p) ev[tid] = sqrt(fmax(G[tid * p + tid], 0.0));
        __syncthreads();
        if (tid < p) {
            const double v = ev[tid];
            int rnk = 0;
            for (int j = 0; j < p; ++j) rnk += (ev[j] > v || (ev[j] == v && j < tid)) ? 1 : 0;
            rk[tid] = rnk;
        }
        if (tid == 0) {
            double e1 = 0.0;
            for (int j = 0; j < p; ++j) e1 = fmax(e1, ev[j]);
            const double cutoff = a.theta * e1;
            int cnt = 0;
            for (int j = 0; j < p; ++j) cnt += (a.strict ? ev[j] > cutoff : ev[j] >= cutoff) ? 1 : 0;
            r_s = cnt > 1 ? cnt : 1;
        }
        __syncthreads();
        const int r = r_s;
        if (r < p) {
            double* __restrict__ Qo = a.Q + a.qoff[b];
            for (int e = tid; e < p * p; e += BR_THREADS) {
                const int i = e / p, j = e - i * p;
                if (rk[j] < r) Qo[i * p + rk[j]] = Q[e];
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int r = r_s, pn = r < p ? r : p;
        int nne = nneg_s < a.delta ? nneg_s : a.delta;               // :129-133
        const int least = b < a.nob ? 1 : 0;
        if (nne < least) nne = least;
        if (pn + nne > n) nne = 0;                                  // :134-136
        a.p_out[b] = pn + nne; a.r_out[b] = r; a.nne_out[b] = nne;
        a.sweeps[b] = sweep < BR_MAXSWEEP ? sweep : -1;
    }
}

// One wave per row, lane c = columns c and c + 64 of the new row (the new width r + nne reaches 64 + delta <= 128: an uncut block of
// width 64 that gains escape columns): the cut columns Y_i Q(:, c) (summed over the old columns in order), then the escape columns
// alpha V_i(:, c - p) (mode 0) or zeros (mode 1); mode 0 scales the rows of the blocks with unit diagonal to norm 1.  The row is read
// whole from the resident slot and written to the other one; columns beyond the block's new width stay zero.
__global__ __launch_bounds__(BR_THREADS) void k_breshape_apply(BrArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = a.n[b], p = a.p_in[b], po = a.p_out[b], nne = a.nne_out[b];
    const int pn = po - nne;
    const int64_t r0 = a.r0[b];
    const bool untouched = n < a.min_facsize, cut = pn < p;
    const double* __restrict__ Q = a.Q + a.qoff[b];
    for (int row = wave; row < n; row += BR_WAVES) {
        const double* __restrict__ y = a.Y + (r0 + row) * a.ld;
        double* __restrict__ yn = a.Yn + (r0 + row) * a.ldn;
        if (untouched) {                                            // (its width may exceed 64: p_i = n_i by default)
            for (int c = lane; c < p; c += 64) yn[c] = y[c];
            continue;
        }
        double v[2] = {0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int c = lane + 64 * q;
            if (c < pn) {
                if (cut) { double acc = 0.0; for (int t = 0; t < p; ++t) acc = fma(y[t], Q[t * p + c], acc); v[q] = acc; }
                else v[q] = y[c];
            } else if (c < po && a.mode == 0) v[q] = a.alpha * a.V[(r0 + row) * a.k + (c - pn)];
        }
        if (a.mode == 0 && b < a.nob) {                             // :142-146 (a zero row keeps its zeros)
            const double nn = msdp_wave_sum(v[0] * v[0] + v[1] * v[1]);   // (columns beyond the new width hold zeros)
            if (nn > 0.0) { v[0] = v[0] / sqrt(nn); v[1] = v[1] / sqrt(nn); }
        }
        if (lane < po) yn[lane] = v[0];
        if (lane + 64 < po) yn[lane + 64] = v[1];
    }
}

// Decide, check, apply.  `blocks` = the handle's own block orders.  On success the other point slot holds the new factor of width
// *p_new (the caller adopts it); on any error the resident slot is untouched.
int msdp_block_reshape_run(msdp_handle h, int cur, int nb, const int64_t* nblk, const int32_t* p_in, const double* w, const double* V,
                           int k, double theta, int strict, int delta, double alpha, int min_facsize, int mode, int nob,
                           int32_t* p_out, int32_t* r_out, int32_t* nne_out, int* p_new) {
    Dev& d = h->d;
    std::vector<int64_t> r0(nb), qoff(nb);
    std::vector<int> nn(nb), pin(nb);
    int64_t rows = 0, qtot = 0;
    int pmax = 1;
    for (int b = 0; b < nb; ++b) {
        r0[b] = rows; qoff[b] = qtot; nn[b] = (int)nblk[b]; pin[b] = p_in[b];
        rows += nblk[b];
        if (nblk[b] >= min_facsize && p_in[b] > 1) { qtot += (int64_t)p_in[b] * p_in[b]; pmax = std::max(pmax, (int)p_in[b]); }
    }
    const int kk = k > 0 ? k : 1;
    size_t need = 0;
    auto piece = [&](size_t bytes) { const size_t o = need; need += (bytes + 255) / 256 * 256; return o; };
    const size_t o_r0 = piece(nb * sizeof(int64_t)), o_qoff = piece(nb * sizeof(int64_t)), o_n = piece(nb * sizeof(int)), o_pin = piece(nb * sizeof(int));
    const size_t o_cnt = piece((size_t)4 * nb * sizeof(int));        // p_out, r_out, nne_out, sweeps
    const size_t o_w = piece((size_t)rows * sizeof(double)), o_V = piece((size_t)rows * kk * sizeof(double));
    const size_t o_Q = piece((size_t)std::max<int64_t>(qtot, 1) * sizeof(double));
    if (h->blk_ws_cap < need) {
        msdp_block_eigs_release(h);
        if (hipMalloc(&h->blk_ws, need) != hipSuccess) { (void)hipGetLastError(); h->blk_ws = nullptr; msdp_set_error("block_reshape: device allocation of %zu bytes failed", need); return MSDP_ENOMEM; }
        h->blk_ws_cap = need;
    }
    char* base = (char*)h->blk_ws;
    int* d_cnt = (int*)(base + o_cnt);
    HIPCHK(msdp_memcpy_async(base + o_r0, r0.data(), nb * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(msdp_memcpy_async(base + o_qoff, qoff.data(), nb * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(msdp_memcpy_async(base + o_n, nn.data(), nb * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(msdp_memcpy_async(base + o_pin, pin.data(), nb * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(msdp_memcpy_async(base + o_w, w, (size_t)rows * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (k > 0) HIPCHK(msdp_memcpy_async(base + o_V, V, (size_t)rows * k * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));                         // (the index vectors are locals of this call)
    BrArgs a;
    a.k = kk; a.strict = strict; a.delta = delta; a.min_facsize = min_facsize; a.mode = mode; a.nob = nob;
    a.theta = theta; a.alpha = alpha;
    a.r0 = (const int64_t*)(base + o_r0); a.qoff = (const int64_t*)(base + o_qoff); a.n = (const int*)(base + o_n); a.p_in = (const int*)(base + o_pin);
    a.w = (const double*)(base + o_w); a.V = (const double*)(base + o_V); a.Q = (double*)(base + o_Q);
    a.p_out = d_cnt; a.r_out = d_cnt + nb; a.nne_out = d_cnt + 2 * nb; a.sweeps = d_cnt + 3 * nb;
    a.Y = d.Y[cur]; a.ld = d.ld; a.Yn = nullptr; a.ldn = 0;
    const size_t lds = (size_t)2 * pmax * pmax * sizeof(double);
    // (set on every call: the attribute belongs to the current device, and a flag of the process would cover the first one only)
    HIPCHK(hipFuncSetAttribute((const void*)k_breshape_decide, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * BR_MAXP * BR_MAXP * (int)sizeof(double)));
    hipLaunchKernelGGL(k_breshape_decide, dim3(nb), dim3(BR_THREADS), lds, h->stream, a);
    HIPCHK(hipGetLastError());
    std::vector<int> cnt((size_t)4 * nb);
    HIPCHK(msdp_memcpy_async(cnt.data(), d_cnt, (size_t)4 * nb * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    int pn = 1;
    for (int b = 0; b < nb; ++b) {
        if (cnt[(size_t)3 * nb + b] < 0) { msdp_set_error("block_reshape: Jacobi iteration of block %d did not converge in %d sweeps", b, BR_MAXSWEEP); return MSDP_ESTATE; }
        pn = std::max(pn, cnt[b]);
    }
    for (int b = 0; b < nb; ++b)                                     // (cannot happen while delta <= k <= 64: r <= 64, nne <= delta)
        if (nblk[b] >= min_facsize && cnt[b] > 2 * BR_MAXP) { msdp_set_error("block_reshape: new width %d of block %d above %d", cnt[b], b, 2 * BR_MAXP); return MSDP_EUNSUPPORTED; }
    if (pn > h->pcap) {
        msdp_set_error("block_reshape: new width %d exceeds the allocated width %d (the point is unchanged; use msdp_set_point)", pn, h->pcap);
        return MSDP_EUNSUPPORTED;
    }
    // the other slot: zero everywhere, so that the columns beyond every block's new width and the pad column are exact zeros
    a.Yn = d.Y[cur ^ 1]; a.ldn = ((pn + 1) / 2) * 2;
    HIPCHK(hipMemsetAsync(a.Yn, 0, (size_t)d.n * h->ldcap * sizeof(double), h->stream));
    hipLaunchKernelGGL(k_breshape_apply, dim3(nb), dim3(BR_THREADS), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int b = 0; b < nb; ++b) { p_out[b] = cnt[b]; r_out[b] = cnt[(size_t)nb + b]; nne_out[b] = cnt[(size_t)2 * nb + b]; }
    *p_new = pn;
    return 0;
}
int msdp_block_reshape_maxp() { return BR_MAXP; }
