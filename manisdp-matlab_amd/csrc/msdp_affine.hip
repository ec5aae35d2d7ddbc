// msdp_affine.hip -- the sparse A(.) / A'(.) operators and the cost / gradient / Hess-vec
// of the two affine entry points, on the oblique (unitdiag) and sphere (unittrace) manifolds.
//
// Reference expressions (Y, U are n x p row-major here = MATLAB's p x n for unitdiag):
//   cost   ManiSDP_unitdiag.m:152-157   X=Y'*Y; Axb=A*x-b-y/sigma; f=c'*x+.5*sigma*(Axb'*Axb)
//   grad   ManiSDP_unitdiag.m:159-164   eS=reshape(c+sigma*At*Axb,n,n); eG=2*Y*eS; YeG=sum(Y.*eG); G=eG-Y.*YeG
//   hess   ManiSDP_unitdiag.m:166-171   YU=Y'*U; AyU=reshape(A'*(At'*YU(:)),n,n); eH=2*U*eS+4*sigma*(Y*AyU);
//                                       H=eH-Y.*sum(Y.*eH)-U.*YeG
//   cost   ManiSDP_unittrace.m:156-165  ... z=sum(X.*eS,'all'); G=2*eS*Y-2*z*Y
//   hess   ManiSDP_unittrace.m:171-177  H=2*eS*U+4*sigma*(AyU*Y); H=H-trace(H*Y')*Y-2*z*U
//
// The n x n matrices X, YU are never formed: A(Ya Yb') is an SDDMM over the pattern of At
// (one LPR-lane group per constraint column, p-wide row panels gathered from L2), A'(w) is a
// CSR-by-entry SpMV that writes the dense n x nS matrix the MFMA kernel then contracts.
// The constraint matrices A_k and C are symmetric (SeDuMi data), so row-major == column-major.
#include "msdp_device.h"
#include "msdp_affine_dev.h"
#include <math.h>
#include <algorithm>
#include <cstring>

// item value = sum over the item's nonzeros (i,j,val) of val * <Ya_i, Yb_j>   (one LPR-lane group per item)
template <int LPR, int NCH>
__global__ __launch_bounds__(MSDP_BLOCK) void k_sddmm(AffineDev a, const double* __restrict__ Ya,
                                                    const double* __restrict__ Yb, const int* skip_flag, int skip_when) {
    if (skip_flag && *skip_flag == skip_when) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int CPW = 64 / LPR;                       // items per wave
    const int sub = lane & (LPR - 1), csub = lane / LPR;
    const int64_t stride = (int64_t)gridDim.x * MSDP_WAVES * CPW;
    for (int64_t it = ((int64_t)blockIdx.x * MSDP_WAVES + wave) * CPW + csub; it < a.nitems; it += stride) {
        const int s0 = a.it0[it], s1 = a.it1[it];
        double acc = 0.0;
        // U nonzeros at a time (16 at a time was measured: 2x slower on BQP, whose constraints have ~4 nonzeros): their index loads and row gathers are independent, one at a time left a lane group
        // with a single request in flight (64 dependent round trips per item = 39 us for the trace row of a theta
        // problem, whatever the size of the rest)
        constexpr int U = NCH == 1 ? 4 : 2;
        for (int t = s0; t < s1; t += U) {
            int ii[U], jj[U];
            double vv[U], dd[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = t + u < s1;
                const int tt = in ? t + u : s1 - 1;
                ii[u] = a.ci[tt]; jj[u] = a.cj[tt];
                vv[u] = in ? a.cv[tt] : 0.0;
                dd[u] = 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double* ya = Ya + (int64_t)ii[u] * a.ld + 2 * sub;
                const double* yb = Yb + (int64_t)jj[u] * a.ld + 2 * sub;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    if (2 * sub + ch * 2 * LPR < a.ld) {
                        const double2 x = ld2(ya + ch * 2 * LPR), z = ld2(yb + ch * 2 * LPR);
                        dd[u] += x.x * z.x + x.y * z.y;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) acc = fma(vv[u], dd[u], acc);
        }
        acc = msdp_group_sum<LPR>(acc);
        if (sub == 0) a.ival[it] = acc;
    }
}
// w_k = sum of the items of constraint k (fixed order).  mode 0: store w.  mode 1 (cost): also
// Axb = w - b - y/sigma into axb_out and the partial sums of Axb^2 -> P_AXB (launch with MSDP_MAX_GRID workgroups).
__global__ __launch_bounds__(MSDP_BLOCK) void k_sddmm_finish(AffineDev a, int mode, double* axb_out, double sigma, double* P,
                                                           const int* skip_flag, int skip_when) {
    __shared__ double sh[3 * MSDP_WAVES];
    if (skip_flag && *skip_flag == skip_when) return;
    double pss = 0.0;
    // short constraints: one thread each
    for (int64_t k = (int64_t)blockIdx.x * MSDP_BLOCK + threadIdx.x; k < a.m; k += (int64_t)gridDim.x * MSDP_BLOCK) {
        const int i0 = a.kit[k], i1 = a.kit[k + 1];
        if (i1 - i0 > FIN_SHORT) continue;
        double acc = 0.0;
        for (int it = i0; it < i1; ++it) acc += a.ival[it];
        a.w[k] = acc;
        if (mode == 1) {
            const double r = acc - a.b[k] - a.y[k] / sigma;
            axb_out[k] = r;
            pss += r * r;
        }
    }
    // long constraints (the trace row of a theta problem, the all-ones constraint of a gpp problem: up to n^2/16
    // items): one wave each, lanes stride over the items
    {
        const int lane = threadIdx.x & 63;
        const int wv = blockIdx.x * (MSDP_BLOCK / 64) + (threadIdx.x >> 6), nwv = gridDim.x * (MSDP_BLOCK / 64);
        for (int q = wv; q < a.nlong; q += nwv) {
            const int k = a.longk[q];
            const int i0 = a.kit[k], i1 = a.kit[k + 1];
            double a0 = 0.0, a1 = 0.0;
            int it = i0 + lane;
            for (; it + 64 < i1; it += 128) { a0 += a.ival[it]; a1 += a.ival[it + 64]; }
            if (it < i1) a0 += a.ival[it];
            const double acc = msdp_wave_sum(a0 + a1);
            if (lane == 0) {
                a.w[k] = acc;
                if (mode == 1) {
                    const double r = acc - a.b[k] - a.y[k] / sigma;
                    axb_out[k] = r;
                    pss += r * r;
                }
            }
        }
    }
    if (mode == 1) msdp_put_partial(P, P_AXB, pss, sh);
}

// k_sddmm + k_sddmm_finish in ONE launch (one rank).  A lane group sums a short constraint whole (its nonzeros are contiguous)
// and writes w_k; the items of the long constraints (trace rows) go to ival with agent-coherent stores and the workgroup that
// arrives last sums them per constraint in item order -- the same order whichever workgroup it is.
//   mode 0: w.   mode 1 (cost): also Axb = w - b - y/sigma -> axb_out and the partial sums of Axb^2 -> P_AXB: launch with
//   MSDP_MAX_GRID - 1 workgroups, slot MSDP_MAX_GRID - 1 takes the long constraints.   mode 2 (sphere Hess-vec, Ya = Y, Yb = U):
//   also the partial sums of w_k (A x)_k -> P_T3 (slot gridDim.x: the long constraints) with (A x)_k = Axb_k + b_k + y_k/sigma of
//   the current point, and of <U, G>, <U, Y> over this workgroup's rows -> P_T1, P_T2: together they give the sphere's
//   tr(H Y') without a pass over H (k_sph_hess_fused).
template <int LPR, int NCH>
__global__ __launch_bounds__(MSDP_BLOCK) void k_sddmm1(AffineDev a, Dev d, const double* __restrict__ Ya, const double* __restrict__ Yb,
                                                     int mode, double* axb_out, double sigma, const int* skip_flag, int skip_when, int nbl) {
    __shared__ double sh[3 * MSDP_WAVES + 8];
    __shared__ int lastflag;
    if (skip_flag && *skip_flag == skip_when) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int CPW = 64 / LPR;
    const int sub = lane & (LPR - 1), csub = lane / LPR;
    const int64_t nunits = (int64_t)a.nshort + a.nlit;
    const int cur = mode == 2 ? d.ctl->cur : 0;
    const double* __restrict__ axc = cur ? a.Axb[1] : a.Axb[0];
    const int slotL = mode == 1 ? MSDP_MAX_GRID - 1 : (int)gridDim.x;
    double pacc = 0.0;
    int haslong = 0;
    const int64_t ustride = (int64_t)gridDim.x * MSDP_WAVES * CPW;
    // mode 2: the rows of <U, G>, <U, Y> are requested FIRST -- they depend on nothing and their latency hides behind the units'
    // chain (record -> nonzeros -> panel rows): every launch of this chain is a handful of dependent round trips, not bandwidth
    int lo = 0, hi = 0;
    double p1 = 0.0, p2 = 0.0;
    if (mode == 2) {
        const unsigned q = (unsigned)d.n_loc / gridDim.x, r = (unsigned)d.n_loc - q * gridDim.x, c = blockIdx.x;
        lo = (int)(c * q + (c < r ? c : r)); hi = lo + (int)q + (c < r ? 1 : 0);
        const double* __restrict__ Gr = cur ? d.Gr[1] : d.Gr[0];
        const int64_t e0 = (int64_t)lo * d.ld, e1 = (int64_t)hi * d.ld;
        for (int64_t i = e0 + 2 * threadIdx.x; i < e1; i += 2 * MSDP_BLOCK) {
            const double2 u = ld2(Yb + i), g = ld2(Gr + i), y = ld2(Ya + i);
            p1 += u.x * g.x + u.y * g.y;
            p2 += u.x * y.x + u.y * y.y;
        }
    }
    for (int64_t u = ((int64_t)blockIdx.x * MSDP_WAVES + wave) * CPW + csub; u < nunits; u += ustride) {
        const int s0 = a.us0[u], s1 = a.us1[u], kk = a.uk[u];
        const int k = kk >= 0 ? kk : -1, lq = kk >= 0 ? 0 : -1 - kk;
        if (kk < 0) haslong = 1;
        // what the constraint's value is combined with (known as soon as k is): requested together with the nonzeros
        double eb = 0.0, ey = 0.0, ea = 0.0;
        if (k >= 0 && mode != 0) { eb = a.b[k]; ey = a.y[k] / sigma; if (mode == 2) ea = axc[k]; }
        double acc = 0.0;
        constexpr int U = NCH == 1 ? 4 : 2;
        for (int t = s0; t < s1; t += U) {
            int ii[U], jj[U];
            double vv[U], dd[U];
#pragma unroll
            for (int u2 = 0; u2 < U; ++u2) {
                const bool in = t + u2 < s1;
                const int tt = in ? t + u2 : s1 - 1;
                ii[u2] = a.ci[tt]; jj[u2] = a.cj[tt];
                vv[u2] = in ? a.cv[tt] : 0.0;
                dd[u2] = 0.0;
            }
#pragma unroll
            for (int u2 = 0; u2 < U; ++u2) {
                const double* ya = Ya + (int64_t)ii[u2] * a.ld + 2 * sub;
                const double* yb = Yb + (int64_t)jj[u2] * a.ld + 2 * sub;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    if (2 * sub + ch * 2 * LPR < a.ld) {
                        const double2 x = ld2(ya + ch * 2 * LPR), z = ld2(yb + ch * 2 * LPR);
                        dd[u2] += x.x * z.x + x.y * z.y;
                    }
                }
            }
#pragma unroll
            for (int u2 = 0; u2 < U; ++u2) acc = fma(vv[u2], dd[u2], acc);
        }
        acc = msdp_group_sum<LPR>(acc);
        if (sub == 0) {
            if (k >= 0) {
                a.w[k] = acc;
                if (mode == 1) { const double r = acc - eb - ey; axb_out[k] = r; pacc += r * r; }      // ManiSDP_unitdiag.m:154, same order
                else if (mode == 2) pacc += acc * (ea + eb + ey);
            } else {
                __hip_atomic_store(a.ival + lq, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (mode == 2) {
        msdp_put_partials3(d.P, P_T1, p1, P_T2, p2, P_T3, pacc, sh);
    } else if (mode == 1) {
        msdp_put_partial(d.P, P_AXB, pacc, sh);
    }
    // ---- long constraints: the last workgroup to arrive sums their items
    if (a.nlit == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && mode != 0) d.P[(mode == 1 ? P_AXB : P_T3) * MSDP_MAX_GRID + slotL] = 0.0;
        return;
    }
    // only the `nbl` workgroups that summed items of long constraints (a host-known count: the items are consecutive units) take part
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!__syncthreads_or(haslong)) return;
    if (threadIdx.x == 0) lastflag = (__hip_atomic_fetch_add(a.cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nbl - 1u) ? 1 : 0;
    __syncthreads();
    if (!lastflag) return;
    double pl = 0.0;
    for (int q = wave; q < a.nlong; q += MSDP_WAVES) {
        const int k = a.longk[q];
        const int i0 = a.lkit[q], i1 = a.lkit[q + 1];
        // four agent-coherent loads in flight per lane and ONE wait (the compiler puts a full s_waitcnt behind every atomic load:
        // the trace row of a theta problem -- 313 items -- cost 7 us of serialized round trips that way)
        double a0 = 0.0;
        for (int base = i0; base < i1; base += 256) {
            const double* q0 = a.ival + min(base + lane, i1 - 1);
            const double* q1 = a.ival + min(base + lane + 64, i1 - 1);
            const double* q2 = a.ival + min(base + lane + 128, i1 - 1);
            const double* q3 = a.ival + min(base + lane + 192, i1 - 1);
            double v0, v1, v2, v3;
            asm volatile(
                "global_load_dwordx2 %0, %4, off sc1\n\t"
                "global_load_dwordx2 %1, %5, off sc1\n\t"
                "global_load_dwordx2 %2, %6, off sc1\n\t"
                "global_load_dwordx2 %3, %7, off sc1\n\t"
                "s_waitcnt vmcnt(0)"
                : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
                : "v"(q0), "v"(q1), "v"(q2), "v"(q3)
                : "memory");
            if (base + lane < i1) a0 += v0;
            if (base + lane + 64 < i1) a0 += v1;
            if (base + lane + 128 < i1) a0 += v2;
            if (base + lane + 192 < i1) a0 += v3;
        }
        const double acc = msdp_wave_sum(a0);
        if (lane == 0) {
            a.w[k] = acc;
            if (mode == 1) { const double r = acc - a.b[k] - a.y[k] / sigma; axb_out[k] = r; pl += r * r; }
            else if (mode == 2) pl += acc * (axc[k] + a.b[k] + a.y[k] / sigma);
        }
    }
    __syncthreads();                                       // sh is free again (msdp_put_partials3 above has finished)
    if (lane == 0) sh[wave] = pl;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < MSDP_WAVES; ++i) s += sh[i];
        if (mode != 0) d.P[(mode == 1 ? P_AXB : P_T3) * MSDP_MAX_GRID + slotL] = s;
        *a.cnt = 0u;
    }
}

// Sphere Hess-vec, everything behind the dense contraction in ONE launch (ManiSDP_unittrace.m:173-176, ManiSDP.m:160-162):
//   H_raw(i,:) = sum of the split-K slabs (2*eS*U, or 2*eS*U + 4 sigma AyU*Y when AyU is dense)
//              + 4 sigma * sum_j A'(w)_ij Y(j,:) over the entries At touches (k_support_spmm's sparse product, when nsup > 0)
//   H = H_raw - t*Y - 2 z U,  t = tr(H_raw Y'),   partial sums of <U, H> -> P_DHD.
// t needs no pass over H_raw: <2 eS U, Y> = <U, 2 eS Y> = <U, G> + 2 z <U, Y> (G = 2 eS Y - 2 z Y is the stored gradient, eS is
// symmetric) and <4 sigma A'(w) Y, Y> = 4 sigma <w, A(Y Y')> -- the three sums k_sddmm1 (mode 2) left in P_T1..P_T3.
// One wave per row; replaces k_support_spmm + k_sph_hess_raw + k_sph_hess_finish (20 us of launches at n = 5000).
template <int LPR, int NCH>
__global__ __launch_bounds__(MSDP_BLOCK) void k_sph_hess_fused(Dev d, AffineDev a, const double* slab, int64_t slab_stride, int SK,
                                                             double sigma, int G2, int support, int cur, int hetero) {
    __shared__ double sh[3 * MSDP_WAVES + 8];
    __shared__ double wl[MSDP_WAVES + 1];                      // values of the long constraints (<= 16), and their share of the third sum
    if (!d.F[0].active) return;
    const bool euc = d.manifold == MANI_EUCLID;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int RPW = 64 / LPR;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    // `cur` is the host's (the affine kinds bake the slot into their launches: one graph per slot).  The three sums of t are
    // requested by the LAST wave up front and consumed behind the row work (one barrier there): nothing waits for them early
    double z = 0.0;
    if (!euc) {
        z = d.ctl->z_sphere[cur];
        if (wave == MSDP_WAVES - 1) {
            const double s1 = msdp_sum_partials(d.P, P_T1, G2), s2 = msdp_sum_partials(d.P, P_T2, G2), s3 = msdp_sum_partials(d.P, P_T3, G2 + 1);
            if (lane == 0) { sh[0] = s1; sh[1] = s2; sh[2] = s3; }
        }
    }
    // Long constraints (a trace row): wave q provides the value of number q -- hetero (the SDDMM ran as a side job of the contraction
    // launch, msdp_sddmm_side): the sum of its item values, in item order, the same in every workgroup; else what k_sddmm1 left in w
    // (only the side-job route needs wl, and it is taken for nlong <= MSDP_WAVES only; otherwise k_sddmm1's last workgroup has written
    // w[longk[q]] and the records below read it there -- any number of long constraints)
    if (support && hetero && wave < a.nlong) {
        double a0 = 0.0;
        for (int it = a.lkit[wave] + lane; it < a.lkit[wave + 1]; it += 64) a0 += a.ival[it];
        const double v = msdp_wave_sum(a0);
        if (lane == 0) wl[wave] = v;
    }
    int lo, hi;
    msdp_chunk_rows(d.n_loc, d.G, lo, hi);
    const double* __restrict__ Yl = cur ? d.Y[1] : d.Y[0];
    const double* __restrict__ w = a.w;
    const double s4 = 4.0 * sigma;
    double pd = 0.0;
    // LPR lanes per row (one double2 each, NCH column chunks), 64 / LPR rows per wave: the lanes of a row take one touched entry
    // each (flattened record -> w), then the values and column indices are broadcast inside the group and all its lanes
    // accumulate v * Y(j, :).  raw = slabs + 4 sigma * sparse part; y, u = the row of the point and of the direction.
    // (eight column chunks per lane, p = 513..1024: only the sparse part is held across the row work; the slab sums and the rows of Y
    // and U are read in `finish` -- holding all four sets took 128 registers per lane and spilled 640 bytes)
    constexpr bool HOLD = NCH < 8;
    auto rowwork = [&](int i, bool rok, double2 (&raw)[NCH], double2 (&y)[HOLD ? NCH : 1], double2 (&u)[HOLD ? NCH : 1]) {
        double2 acc[NCH];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            acc[ch] = make_double2(0.0, 0.0); raw[ch] = acc[ch];
            if (HOLD) { y[HOLD ? ch : 0] = acc[ch]; u[HOLD ? ch : 0] = acc[ch]; }
            const int c = 2 * sub + ch * 2 * LPR;
            if (HOLD && rok && c < d.ld) {                         // independent of the sparse part: requested first
                const int64_t o = (int64_t)i * d.ld + c;
                raw[ch] = msdp_sum_slabs(slab, slab_stride, SK, o);
                y[HOLD ? ch : 0] = ld2(Yl + o); u[HOLD ? ch : 0] = ld2(d.md + o);
            }
        }
        if (support) {
            const int qb = rok ? a.suprow[i] : 0, qe = rok ? a.suprow[i + 1] : 0;
            for (int q0 = qb; __builtin_amdgcn_ballot_w64(q0 < qe) != 0ULL; q0 += LPR) {
                const int cnt = min(LPR, max(qe - q0, 0));
                int jl = 0;
                double vl = 0.0;
                if (sub < cnt) {
                    // flattened record of the entry: column, first (coefficient, constraint) pair; further pairs are rare
                    jl = a.sqj[q0 + sub];
                    const int k0 = a.sqk[q0 + sub], more = a.sqmore[q0 + sub];
                    vl = a.sqv[q0 + sub] * (k0 >= 0 ? w[k0] : (hetero ? wl[-1 - k0] : w[a.longk[-1 - k0]]));
                    if (more > 0) {
                        const int s0 = a.rp[a.sup[q0 + sub]] + 1;
                        for (int tt = s0; tt < s0 + more; ++tt) { const int kx = a.rkx[tt]; vl = fma(a.rv[tt], kx >= 0 ? w[kx] : (hetero ? wl[-1 - kx] : w[a.longk[-1 - kx]]), vl); }
                    }
                }
                for (int e0 = 0; __builtin_amdgcn_ballot_w64(e0 < cnt) != 0ULL; e0 += SPB) {      // until the longest row of the wave is done
                    int jj[SPB];
                    double v[SPB];
#pragma unroll
                    for (int q = 0; q < SPB; ++q) {
                        const int e = min(e0 + q, max(cnt - 1, 0));
                        jj[q] = __shfl(jl, e, LPR);
                        const double vv = __shfl(vl, e, LPR);
                        v[q] = (e0 + q < cnt) ? vv : 0.0;
                    }
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) {
                        const int c = 2 * sub + ch * 2 * LPR;
                        if (c < d.ld) {
                            double2 yy[SPB];
#pragma unroll
                            for (int q = 0; q < SPB; ++q) yy[q] = ld2(Yl + (int64_t)jj[q] * d.ld + c);
#pragma unroll
                            for (int q = 0; q < SPB; ++q) { acc[ch].x = fma(v[q], yy[q].x, acc[ch].x); acc[ch].y = fma(v[q], yy[q].y, acc[ch].y); }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) { raw[ch].x += s4 * acc[ch].x; raw[ch].y += s4 * acc[ch].y; }
    };
    double t = 0.0;
    auto finish = [&](int i, bool rok, const double2 (&raw)[NCH], const double2 (&y)[HOLD ? NCH : 1], const double2 (&u)[HOLD ? NCH : 1]) {
        if (!rok) return;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const int c = 2 * sub + ch * 2 * LPR;
            if (c < d.ld) {
                const int64_t o = (int64_t)i * d.ld + c;
                double2 rw = raw[ch];
                if (!HOLD) { const double2 sl = msdp_sum_slabs(slab, slab_stride, SK, o); rw.x += sl.x; rw.y += sl.y; }
                const double2 yy = HOLD ? y[HOLD ? ch : 0] : ld2(Yl + o), uu = HOLD ? u[HOLD ? ch : 0] : ld2(d.md + o);
                double2 hq;
                hq.x = rw.x - t * yy.x - 2.0 * z * uu.x;
                hq.y = rw.y - t * yy.y - 2.0 * z * uu.y;
                st2(d.Hmd + o, hq);
                pd += uu.x * hq.x + uu.y * hq.y;
            }
        }
    };
    if (support && hetero && a.nlong > 0) __syncthreads();         // wl is in place
    double2 raw[NCH], y[HOLD ? NCH : 1], u[HOLD ? NCH : 1];
    int row0 = lo + wave * RPW;                                    // wave-uniform
    const bool first = row0 < hi;
    if (first) rowwork(row0 + rsub, row0 + rsub < hi, raw, y, u);  // first pass in front of the barrier that hands out t
    if (!euc) {
        __syncthreads();
        double s3 = sh[2];
        if (hetero && support) {                                   // the long constraints' share of <w, A(YY')>, in constraint order
            const double* __restrict__ axc = cur ? a.Axb[1] : a.Axb[0];
            for (int q = 0; q < a.nlong; ++q) { const int k = a.longk[q]; s3 += wl[q] * (axc[k] + a.b[k] + a.y[k] / sigma); }
        }
        t = (sh[0] + 2.0 * z * sh[1]) + 4.0 * sigma * s3;
    }
    if (first) finish(row0 + rsub, row0 + rsub < hi, raw, y, u);
    for (row0 += MSDP_WAVES * RPW; row0 < hi; row0 += MSDP_WAVES * RPW) {
        rowwork(row0 + rsub, row0 + rsub < hi, raw, y, u);
        finish(row0 + rsub, row0 + rsub < hi, raw, y, u);
    }
    __syncthreads();                                               // sh[0..2] has been read by everybody
    msdp_put_partial(d.P, P_DHD, pd, sh + 8);
}

// fp64-MFMA version of k_gram (default): W = Ya * Yb' as 64 x 64 tiles, four waves per tile in a 2 x 2 arrangement,
// each wave 32 x 32 = 2 x 2 accumulator tiles of v_mfma_f64_16x16x4_f64.  Both operands are rows of a thin panel with k
// contiguous, so they are staged the same way (64 rows x 32 k per panel, row stride 36 doubles: the 16 rows of a
// fragment read start on distinct 32-byte bank groups) and read as fragments of 4 contiguous k per lane (two
// ds_read_b128), which feed four MFMAs -- the k order inside a 16-k step is permuted identically for A and B.
// In the BQP d = 60 solve the factor grows to p = 300 and the VALU kernel above was the largest single kernel of the
// RTR phase (228 us = 8.8 TFLOP/s at p = 300).  Prefetching the next tile's panel pieces into registers under the
// MFMAs was measured: 124 instead of 92 VGPRs (3 instead of 4 waves per SIMD) and 3 % slower.
typedef double gram_d4 __attribute__((ext_vector_type(4)));
#define GRAM_KT 32
#define GRAM_LDS (GRAM_KT + 4)
// sym != 0: Wsym = Ya*Yb' + Yb*Ya' on the tiles on and above the diagonal only -- the same flops as the full W, half the
// stores, and the gather that follows reads one entry per symmetric pair of a constraint.
// 512 threads = two groups of four waves, each with its own staging buffers: with the symmetric form group g computes
// product g (Ya_I*Yb_J' or Yb_I*Ya_J'); otherwise (one product) group g takes half of the k range.  The partial tiles
// are added through LDS at the end.  (Half as many workgroups as the full W would otherwise leave 1-2 four-wave
// workgroups per CU, too few to cover the staging latency: 79 instead of 57 us at p = 300.)
__global__ __launch_bounds__(512) void k_gram_mfma(int n, int nS, int ld, const double* __restrict__ Ya0,
                                                   const double* __restrict__ Yb0, double* __restrict__ W,
                                                   const int* skip_flag, int skip_when, int sym) {
    __shared__ __attribute__((aligned(16))) double Stage[2 * 2 * 64 * GRAM_LDS];      // [group][A|B][64 x GRAM_LDS]
    if (skip_flag && *skip_flag == skip_when) return;
    if (sym && blockIdx.y > blockIdx.x) return;
    const int ti = blockIdx.y * 64, tj = blockIdx.x * 64;
    const int grp = threadIdx.x >> 8, tid = threadIdx.x & 255;
    const bool two = sym && Ya0 != Yb0;                                 // two products, one per group
    const double post = (sym && Ya0 == Yb0) ? 2.0 : 1.0;
    const double* __restrict__ Ya = (two && grp) ? Yb0 : Ya0;
    const double* __restrict__ Yb = (two && grp) ? Ya0 : Yb0;
    const int nk = (ld + GRAM_KT - 1) / GRAM_KT;
    const int niter = two ? nk : (nk + 1) / 2;                          // the same trip count in both groups (barriers)
    const int kbeg = two ? 0 : grp * niter * GRAM_KT;
    const int kend = two ? ld : min(ld, (grp + 1) * niter * GRAM_KT);
    double* As = Stage + grp * (2 * 64 * GRAM_LDS);
    double* Bs = As + 64 * GRAM_LDS;
    const int lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, i = lane & 15;
    const int wr = wave >> 1, wc = wave & 1;
    gram_d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (gram_d4){0.0, 0.0, 0.0, 0.0};
    // staging: thread -> (row = tid / 16 + 16 * q, column pair = tid % 16), q = 0..3, both panels
    const int sr = tid >> 4, sc = 2 * (tid & 15);
    for (int it = 0; it < niter; ++it) {
        const int k0 = kbeg + it * GRAM_KT;
        double2 ra[4], rb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = sr + 16 * q;
            const bool ck = k0 + sc < kend;                         // ld is even: a pair is in or out as a whole
            const bool oa = ck && ti + r < n, ob = ck && tj + r < n;
            const double2 va = ld2(Ya + (oa ? (int64_t)(ti + r) * ld + k0 + sc : 0));
            const double2 vb = ld2(Yb + (ob ? (int64_t)(tj + r) * ld + k0 + sc : 0));
            ra[q] = oa ? va : make_double2(0.0, 0.0);
            rb[q] = ob ? vb : make_double2(0.0, 0.0);
        }
        __syncthreads();                                            // previous tile's fragment reads are done
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = sr + 16 * q;
            *reinterpret_cast<double2*>(&As[r * GRAM_LDS + sc]) = ra[q];
            *reinterpret_cast<double2*>(&Bs[r * GRAM_LDS + sc]) = rb[q];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < GRAM_KT / 16; ++s) {
            double2 fa[2][2], fb[2][2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const double* pa = &As[(wr * 32 + 16 * a + i) * GRAM_LDS + 16 * s + 4 * g];
                const double* pb = &Bs[(wc * 32 + 16 * a + i) * GRAM_LDS + 16 * s + 4 * g];
                fa[a][0] = *reinterpret_cast<const double2*>(pa); fa[a][1] = *reinterpret_cast<const double2*>(pa + 2);
                fb[a][0] = *reinterpret_cast<const double2*>(pb); fb[a][1] = *reinterpret_cast<const double2*>(pb + 2);
            }
#pragma unroll
            for (int t4 = 0; t4 < 4; ++t4) {
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const double av = (t4 == 0) ? fa[a][0].x : (t4 == 1) ? fa[a][0].y : (t4 == 2) ? fa[a][1].x : fa[a][1].y;
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const double bv = (t4 == 0) ? fb[b][0].x : (t4 == 1) ? fb[b][0].y : (t4 == 2) ? fb[b][1].x : fb[b][1].y;
                        acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[a][b], 0, 0, 0);
                    }
                }
            }
        }
    }
    // group 1 hands its partial tile to group 0 through LDS (4096 doubles, the staging space is 9216)
    __syncthreads();
    if (grp == 1) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) Stage[(((wave * 2 + a) * 2 + b) * 4 + r) * 64 + lane] = acc[a][b][r];
    }
    __syncthreads();
    if (grp == 1) return;
    // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4*reg
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int col = tj + wc * 32 + 16 * b + i;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = ti + wr * 32 + 16 * a + g + 4 * r;
                const double v = acc[a][b][r] + Stage[(((wave * 2 + a) * 2 + b) * 4 + r) * 64 + lane];
                if (row < n && col < nS) W[(int64_t)row * nS + col] = post * v;
            }
        }
}

// ---- Gram route for A(Ya Yb'): when At is dense in its rows (BQP moment relaxations: 4.8 M nonzeros for an
// 1831 x 1831 matrix) the SDDMM above gathers two p-wide rows per nonzero (2.5 GB of L2 traffic at p = 32,
// measured 154 us); forming W = Ya*Yb' once (n^2 p flops, 27 MB; k_gram_mfma above) and gathering ONE double per
// nonzero is what the reference does (ManiSDP_unitdiag.m:153,167: X = Y'*Y, YU = Y'*U) and moves 20x less.
// w_k = sum over the nonzeros of constraint k of val * W[cidx], straight from the Gram matrix: one thread per
// constraint (its nonzeros are contiguous), a whole wave for the few constraints with more than
// FIN_SHORT*SDDMM_CHUNK nonzeros (trace rows).  Four nonzeros are in flight per thread (one at a time left a thread
// with a single request outstanding: 33 us for the 1.16 M constraints of BQP d = 60).  mode as in k_sddmm_finish: the
// per-item partial values and the separate finish launch of the SDDMM route are not needed here.
__global__ __launch_bounds__(MSDP_BLOCK) void k_gram_apply(AffineDev a, const double* __restrict__ W, int mode, double* axb_out,
                                                         double sigma, double* P, const int* skip_flag, int skip_when) {
    __shared__ double sh[3 * MSDP_WAVES];
    if (skip_flag && *skip_flag == skip_when) return;
    double pss = 0.0;
    constexpr int LONG = FIN_SHORT * SDDMM_CHUNK;
    for (int64_t k = (int64_t)blockIdx.x * MSDP_BLOCK + threadIdx.x; k < a.m; k += (int64_t)gridDim.x * MSDP_BLOCK) {
        const int s0 = a.cjc[k], s1 = a.cjc[k + 1];
        if (s1 - s0 > LONG) continue;
        double acc = 0.0;
        for (int t = s0; t < s1; t += 4) {
            int cc[4];
            double vv[4], ww[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool in = t + u < s1;
                const int tt = in ? t + u : s1 - 1;
                cc[u] = a.cidx[tt];
                vv[u] = in ? a.cv[tt] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) ww[u] = W[cc[u]];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = fma(vv[u], ww[u], acc);
        }
        a.w[k] = acc;
        if (mode == 1) {
            const double r = acc - a.b[k] - a.y[k] / sigma;
            axb_out[k] = r;
            pss += r * r;
        }
    }
    {
        const int lane = threadIdx.x & 63;
        const int wv = blockIdx.x * (MSDP_BLOCK / 64) + (threadIdx.x >> 6), nwv = gridDim.x * (MSDP_BLOCK / 64);
        for (int q = wv; q < a.nlong; q += nwv) {
            const int k = a.longk[q];
            const int s0 = a.cjc[k], s1 = a.cjc[k + 1];
            double a0 = 0.0, a1 = 0.0;
            int t = s0 + lane;
            for (; t + 64 < s1; t += 128) { a0 = fma(a.cv[t], W[a.cidx[t]], a0); a1 = fma(a.cv[t + 64], W[a.cidx[t + 64]], a1); }
            if (t < s1) a0 = fma(a.cv[t], W[a.cidx[t]], a0);
            const double acc = msdp_wave_sum(a0 + a1);
            if (lane == 0) {
                a.w[k] = acc;
                if (mode == 1) {
                    const double r = acc - a.b[k] - a.y[k] / sigma;
                    axb_out[k] = r;
                    pss += r * r;
                }
            }
        }
    }
    if (mode == 1) msdp_put_partial(P, P_AXB, pss, sh);
}

// out[i][j] = (base ? base[i][j] : 0) + scale * sum_k At[(i,j),k] * vec[k]   (dense n x nS, zero pad)
__global__ void k_adjoint_dense(AffineDev a, const double* __restrict__ base, const double* __restrict__ vec,
                                double scale, double* __restrict__ out, const int* skip_flag, int skip_when) {
    if (skip_flag && *skip_flag == skip_when) return;
    const int64_t tot = (int64_t)a.n * a.nS;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(e / a.nS), j = (int)(e - (int64_t)i * a.nS);
        double v = 0.0;
        if (j < a.n) {
            const int64_t r = (int64_t)i * a.n + j;
            const int s0 = a.rp[r], s1 = a.rp[r + 1];
            double acc = 0.0;
            for (int t = s0; t < s1; ++t) acc = fma(a.rv[t], vec[a.rk[t]], acc);
            v = (base ? base[e] : 0.0) + scale * acc;
        }
        out[e] = v;
    }
}

// Same result for SYMMETRIC data (A_k = A_k', base = base': SeDuMi's convention, bqpmom.m:80-91, qsmom.m, fromsdpa.m),
// which is what the affine entry points are fed: only the 32 x 32 tiles on and above the diagonal are computed (half
// the (coefficient, constraint) reads and half the 8-byte gathers of `vec`) and every off-diagonal tile is stored
// twice, the second time transposed through LDS, so both stores are 256-byte row segments.  The CSR-by-entry
// arrays are laid out in tile order (trp/trk/trv), so a workgroup streams one contiguous range of them; each
// thread owns four entries of the tile and runs their chains of dependent loads (offsets -> coefficient and
// constraint -> vec) side by side.  The flat kernel above walked all n^2 entries with one chain per thread and a
// 64-bit division per entry: 85-104 us per call on BQP d = 60 (0.10 of the HBM roofline).
__global__ __launch_bounds__(256) void k_adjoint_tiled(AffineDev a, const double* __restrict__ base, const double* __restrict__ vec,
                                                       double scale, double* __restrict__ out, const int* skip_flag, int skip_when) {
    __shared__ double tile[ADJ_T][ADJ_T + 1];
    if (skip_flag && *skip_flag == skip_when) return;
    if ((int)blockIdx.x >= a.ntp) {
        // ---- long entries: one wave each, lanes stride over the (coefficient, constraint) pairs; both copies stored
        const int lane = threadIdx.x & 63;
        const int q = ((int)blockIdx.x - a.ntp) * 4 + (threadIdx.x >> 6);
        if (q >= a.nlong_e) return;
        const int t0 = a.ls0[q], t1 = a.ls1[q];
        double acc = 0.0;
        for (int t = t0 + lane; t < t1; t += 64) acc = fma(a.trv[t], vec[a.trk[t]], acc);
        acc = msdp_wave_sum(acc);
        if (lane == 0) {
            const int o = a.lpos[q], om = a.lmir[q];
            const double v = (base ? base[o] : 0.0) + scale * acc;
            out[o] = v;
            if (om != o) out[om] = v;
        }
        return;
    }
    const int bi = a.tp_i[blockIdx.x], bj = a.tp_j[blockIdx.x];
    const int lj = threadIdx.x & 31, li0 = threadIdx.x >> 5;          // rows li0 + 8 q, q = 0..3
    const int* __restrict__ trp = a.trp + (size_t)blockIdx.x * (ADJ_T * ADJ_T);
    int s0[4], s1[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = (li0 + 8 * q) * ADJ_T + lj;
        s0[q] = trp[e]; s1[q] = trp[e + 1];
    }
    bool lng[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { lng[q] = s1[q] - s0[q] > ADJ_LONG; if (lng[q]) s1[q] = s0[q]; }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    // the first two nonzeros of the four entries side by side (most entries have at most two); trk / trv carry one
    // padding element, so the clamped index of an exhausted entry is always readable
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        int kk[4];
        double vv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool in = s0[q] + r < s1[q];
            const int t = in ? s0[q] + r : s0[q];
            kk[q] = a.trk[t];
            vv[q] = in ? a.trv[t] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = fma(vv[q], vec[kk[q]], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int t = s0[q] + 2; t < s1[q]; ++t) acc[q] = fma(a.trv[t], vec[a.trk[t]], acc[q]);   // <= ADJ_LONG - 2 trips
    const int j = bj * ADJ_T + lj;
    double v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = bi * ADJ_T + li0 + 8 * q;
        v[q] = 0.0;
        if (i < a.n && j < a.nS && !lng[q]) {
            const size_t o = (size_t)i * a.nS + j;
            if (j < a.n) v[q] = (base ? base[o] : 0.0) + scale * acc[q];
            out[o] = v[q];                                           // pad columns are written as zeros
        }
    }
    if (bi == bj) return;                                            // diagonal tile: both triangles were computed
    // mirrored copy; long entries are marked with a NaN and skipped (the long-entry waves store both copies)
#pragma unroll
    for (int q = 0; q < 4; ++q) tile[li0 + 8 * q][lj] = lng[q] ? __longlong_as_double(0x7ff8000000000000LL) : v[q];
    __syncthreads();
    const int jm = bi * ADJ_T + lj;                                  // mirrored column = row index of the tile
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int im = bj * ADJ_T + li0 + 8 * q;                     // mirrored row = column index of the tile
        const double tv = tile[lj][li0 + 8 * q];
        if (im < a.n && jm < a.nS && tv == tv) out[(size_t)im * a.nS + jm] = (jm < a.n) ? tv : 0.0;
    }
}


// B route: out = scale * B * Wsym on the 32 x 32 tiles on and above the diagonal, mirrored like k_adjoint_tiled.  Wsym = Ya*Yb' +
// Yb*Ya' comes from k_gram_mfma (upper 64 x 64 tiles).  Replaces k_gram_apply (one gather per nonzero of the upper At, writes w)
// + k_adjoint_tiled (one gather of w per nonzero): for BQP d = 60 4.2 M coefficients instead of 2 x 2.4 M, two dependent round
// trips (ELL slice -> gather) instead of three + three, and no 9-MB m-vector in between.
template <int BW, bool PK>
__global__ __launch_bounds__(256) void k_adjoint_gram(AffineDev a, const double* __restrict__ Wsym, double scale, double* __restrict__ out,
                                                      const int* skip_flag, int skip_when) {
    __shared__ double tile[ADJ_T][ADJ_T + 1];
    __shared__ double dict[PK ? 256 : 1];
    if (skip_flag && *skip_flag == skip_when) return;
    if (PK && (int)blockIdx.x < a.ntp) { dict[threadIdx.x] = a.bdict[threadIdx.x]; __syncthreads(); }
    if ((int)blockIdx.x >= a.ntp) {
        const int lane = threadIdx.x & 63;
        const int q = ((int)blockIdx.x - a.ntp) * 4 + (threadIdx.x >> 6);
        if (q >= a.bnlong) return;
        const int t0 = a.bls0[q], t1 = a.bls1[q];
        double acc = 0.0;
        for (int t = t0 + lane; t < t1; t += 64) acc = fma(a.blv[t], Wsym[a.blk[t]], acc);
        acc = msdp_wave_sum(acc);
        if (lane == 0) {
            const int o = a.blpos[q], om = a.blmir[q];
            const double v = scale * acc;
            out[o] = v;
            if (om != o) out[om] = v;
        }
        return;
    }
    const int bi = a.tp_i[blockIdx.x], bj = a.tp_j[blockIdx.x];
    const int lj = threadIdx.x & 31, li0 = threadIdx.x >> 5;
    const size_t tb = (size_t)blockIdx.x * BW * (ADJ_T * ADJ_T);
    int idx[4][BW];
    double val[4][BW];
    bool lng[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = (li0 + 8 * q) * ADJ_T + lj;
        lng[q] = a.blong[(size_t)blockIdx.x * (ADJ_T * ADJ_T) + e] != 0;
#pragma unroll
        for (int w = 0; w < BW; ++w) {
            if (PK) {
                const unsigned pk = a.bpk[tb + (size_t)w * (ADJ_T * ADJ_T) + e];
                idx[q][w] = (int)(pk & 0xffffffu); val[q][w] = dict[pk >> 24];
            } else { idx[q][w] = a.bidx[tb + (size_t)w * (ADJ_T * ADJ_T) + e]; val[q][w] = a.bval[tb + (size_t)w * (ADJ_T * ADJ_T) + e]; }
        }
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int w = 0; w < BW; ++w)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = fma(val[q][w], Wsym[idx[q][w]], acc[q]);
    const int j = bj * ADJ_T + lj;
    double v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = bi * ADJ_T + li0 + 8 * q;
        v[q] = 0.0;
        if (i < a.n && j < a.nS && !lng[q]) {
            const size_t o = (size_t)i * a.nS + j;
            if (j < a.n) v[q] = scale * acc[q];
            out[o] = v[q];
        }
    }
    if (bi == bj) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) tile[li0 + 8 * q][lj] = lng[q] ? __longlong_as_double(0x7ff8000000000000LL) : v[q];
    __syncthreads();
    const int jm = bi * ADJ_T + lj;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int im = bj * ADJ_T + li0 + 8 * q;
        const double tv = tile[lj][li0 + 8 * q];
        if (im < a.n && jm < a.nS && tv == tv) out[(size_t)im * a.nS + jm] = (jm < a.n) ? tv : 0.0;
    }
}

// The same update restricted to the entries that occur in some constraint.  For the SDPLIB-type problems (theta, gpp:
// m = O(n) constraints of a few entries each) At touches a fraction of a percent of the n^2 entries, and `out` keeps
// its value everywhere else from one call to the next (eS = C there, AyU = 0 there), so the full sweep above moves
// 2-3 matrices through HBM to change 55 000 numbers (theta-like n = 5000: 55 us per call, 3 us here).
__global__ __launch_bounds__(256) void k_adjoint_support(AffineDev a, const double* __restrict__ base, const double* __restrict__ vec,
                                                         double scale, double* __restrict__ out, const int* skip_flag, int skip_when) {
    if (skip_flag && *skip_flag == skip_when) return;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < a.nsup; q += gridDim.x * blockDim.x) {
        const int r = a.sup[q];
        const int i = r / a.n, j = r - i * a.n;
        const int64_t e = (int64_t)i * a.nS + j;
        const int s0 = a.rp[r], s1 = a.rp[r + 1];
        double acc = 0.0;
        for (int t = s0; t < s1; ++t) acc = fma(a.rv[t], vec[a.rk[t]], acc);
        out[e] = (base ? base[e] : 0.0) + scale * acc;
    }
}

// out(i,:) = scale * sum_j (A'(w))_ij * Yp(j,:) over the entries (i,j) At touches: the product AyU*Y of the Hess-vec
// without forming AyU (ManiSDP_unitdiag.m:168-169, ManiSDP_unittrace.m:173-174).  One wave per matrix row; the
// adjoint values of the entries of a row are computed one per lane, the panel rows are read 16 bytes per lane.  The result is handed to the epilogue as one more split-K slab.
template <int NCH>
__global__ __launch_bounds__(256) void k_support_spmm(AffineDev a, const double* __restrict__ w, const double* __restrict__ Yp,
                                                      double scale, double* __restrict__ out, const int* skip_flag, int skip_when) {
    if (skip_flag && *skip_flag == skip_when) return;
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < a.n; i += gridDim.x * 4) {
        double2 acc[NCH];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) acc[ch] = make_double2(0.0, 0.0);
        // Phase 1: the lanes take one entry each (64 at a time) and run its chain of dependent loads -- entry -> row
        // pointer -> (coefficient, constraint) -> w -- side by side.  Phase 2: the values and column indices are
        // broadcast lane by lane and all lanes accumulate v * Yp(j,:); four panel rows are requested together.
        const int q1 = a.suprow[i + 1];
        for (int q0 = a.suprow[i]; q0 < q1; q0 += 64) {
            const int cnt = min(64, q1 - q0);
            int jl = 0;
            double vl = 0.0;
            if (lane < cnt) {
                const int r = a.sup[q0 + lane];
                jl = r - i * a.n;
                const int s0 = a.rp[r], s1 = a.rp[r + 1];
                for (int t = s0; t < s1; ++t) vl = fma(a.rv[t], w[a.rk[t]], vl);
            }
            for (int e0 = 0; e0 < cnt; e0 += SPB) {
                int jj[SPB];
                double v[SPB];
#pragma unroll
                for (int u = 0; u < SPB; ++u) {
                    const int e = min(e0 + u, cnt - 1);
                    jj[u] = __shfl(jl, e);
                    v[u] = (e0 + u < cnt) ? __shfl(vl, e) : 0.0;
                }
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const int c = 2 * lane + 128 * ch;
                    if (c < a.ld) {
                        double2 y[SPB];
#pragma unroll
                        for (int u = 0; u < SPB; ++u) y[u] = ld2(Yp + (int64_t)jj[u] * a.ld + c);
#pragma unroll
                        for (int u = 0; u < SPB; ++u) { acc[ch].x = fma(v[u], y[u].x, acc[ch].x); acc[ch].y = fma(v[u], y[u].y, acc[ch].y); }
                    }
                }
            }
        }
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const int c = 2 * lane + 128 * ch;
            if (c < a.ld) st2(out + (int64_t)i * a.ld + c, make_double2(scale * acc[ch].x, scale * acc[ch].y));
        }
    }
}

// rows: t_i = <S_i, Y_i> where S = sum of slabs (S = M*Y); writes optional S to dst and partial sum -> P[which]
template <int LPR, int NCH>
__global__ __launch_bounds__(MSDP_BLOCK) void k_rowdot_slabs(Dev d, const double* __restrict__ Yl, const double* slab,
                                                           int64_t slab_stride, int SK, double scale_out,
                                                           double* dst, double* rowdot_out, int which) {
    __shared__ double sh[3 * MSDP_WAVES];
    int lo, hi;
    msdp_chunk_rows(d.n_loc, d.G, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int RPW = 64 / LPR;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    double ps = 0.0;
    for (int row0 = lo + wave * RPW; row0 < hi; row0 += MSDP_WAVES * RPW) {
        const int row = row0 + rsub;
        if (row < hi) {
            double dot = 0.0;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const int col = 2 * sub + ch * 2 * LPR;
                if (col < d.ld) {
                    const int64_t o = (int64_t)row * d.ld + col;
                    const double2 acc = msdp_sum_slabs(slab, slab_stride, SK, o);
                    const double2 y = ld2(Yl + o);
                    dot += acc.x * y.x + acc.y * y.y;
                    if (dst) st2(dst + o, make_double2(scale_out * acc.x, scale_out * acc.y));
                }
            }
            dot = msdp_group_sum<LPR>(dot);
            // rows of a Euclidean block (multiblock kind) carry no diagonal multiplier: YeG / z stay 0 there
            // (ManiSDP_multiblock.m:80-84,225-228)
            const bool freerow = d.rowfree && d.rowfree[row];
            if (sub == 0) { if (rowdot_out) rowdot_out[row] = freerow ? 0.0 : scale_out * dot; ps += dot; }
        }
    }
    msdp_put_partial(d.P, which, ps, sh);
}

// unitdiag gradient finish: eG (n x ld, = 2*eS*Y) in Gr, YeG rows known -> G = eG - Y.*YeG, |G|^2; and f.
template <int LPR, int NCH>
__global__ __launch_bounds__(MSDP_BLOCK) void k_obl_grad_finish(Dev d, int slot, double sigma, const double* f_given) {
    __shared__ double sh[3 * MSDP_WAVES + 8];
    int lo, hi;
    msdp_chunk_rows(d.n_loc, d.G, lo, hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int RPW = 64 / LPR;
    const int sub = lane & (LPR - 1), rsub = lane / LPR;
    const double* __restrict__ Yl = slot ? d.Y[1] : d.Y[0];
    double* __restrict__ Gr = slot ? d.Gr[1] : d.Gr[0];
    const double* __restrict__ YeG = slot ? d.eG[1] : d.eG[0];
    double pgg = 0.0;
    for (int row0 = lo + wave * RPW; row0 < hi; row0 += MSDP_WAVES * RPW) {
        const int row = row0 + rsub;
        if (row < hi) {
            const double t = YeG[row];
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const int col = 2 * sub + ch * 2 * LPR;
                if (col < d.ld) {
                    const int64_t o = (int64_t)row * d.ld + col;
                    const double2 e = ld2(Gr + o), y = ld2(Yl + o);
                    const double2 gq = make_double2(e.x - y.x * t, e.y - y.y * t);
                    st2(Gr + o, gq);
                    pgg += gq.x * gq.x + gq.y * gq.y;
                }
            }
        }
    }
    // f = c'x + .5*sigma*|Axb|^2 : c'x partial sums are in P_S1 (sum <C*Y, Y>), |Axb|^2 in P_AXB
    const double cx = msdp_sum_partials_block(d.P, P_S1, d.G, sh);
    __syncthreads();
    const double ss = msdp_sum_partials_block(d.P, P_AXB, MSDP_MAX_GRID, sh);
    __syncthreads();
    double pf = 0.0;
    // f_given: the dual kind's cost.  Row-sharded runs: the value enters the all-reduced sum once (rank 0)
    if (blockIdx.x == 0 && threadIdx.x == 0 && d.row0 == 0) pf = f_given ? *f_given : cx + 0.5 * sigma * ss;
    msdp_put_partials3(d.P, P_F, pf, P_GG, pgg, -1, 0.0, sh + 8);
}

// sphere gradient finish: Gr holds 2*eS*Y, z = <eS*Y, Y> partials in P_S2: G = 2 eS Y - 2 z Y.
__global__ __launch_bounds__(MSDP_BLOCK) void k_sph_grad_finish(Dev d, int slot, double sigma, const double* f_given) {
    __shared__ double sh[3 * MSDP_WAVES + 8];
    // Euclidean manifold (generic ManiSDP.m:153-156): G = 2*S*Y, no projection term
    const double z = (d.manifold == MANI_EUCLID) ? 0.0 : msdp_sum_partials_block(d.P, P_S2, d.G, sh);
    __syncthreads();
    const double cx = msdp_sum_partials_block(d.P, P_S1, d.G, sh);
    __syncthreads();
    const double ss = msdp_sum_partials_block(d.P, P_AXB, MSDP_MAX_GRID, sh);
    __syncthreads();
    int lo, hi;
    msdp_chunk_rows(d.n_loc, d.G, lo, hi);
    const double* __restrict__ Yl = slot ? d.Y[1] : d.Y[0];
    double* __restrict__ Gr = slot ? d.Gr[1] : d.Gr[0];
    const int64_t e0 = (int64_t)lo * d.ld, e1 = (int64_t)hi * d.ld;
    double pgg = 0.0;
    for (int64_t i = e0 + 2 * threadIdx.x; i < e1; i += 2 * MSDP_BLOCK) {
        const double2 e = ld2(Gr + i), y = ld2(Yl + i);
        const double2 gq = make_double2(e.x - 2.0 * z * y.x, e.y - 2.0 * z * y.y);
        st2(Gr + i, gq);
        pgg += gq.x * gq.x + gq.y * gq.y;
    }
    double pf = 0.0;
    // f_given: the generic dual kind's cost
    if (blockIdx.x == 0 && threadIdx.x == 0) { if (d.row0 == 0) pf = f_given ? *f_given : cx + 0.5 * sigma * ss; d.ctl->z_sphere[slot] = z; }
    msdp_put_partials3(d.P, P_F, pf, P_GG, pgg, -1, 0.0, sh + 8);
}

// sphere Hess-vec finish (ManiSDP_unittrace.m:176): Hmd holds H_raw, t = <H_raw, Y> partials in P_AUX
__global__ __launch_bounds__(MSDP_BLOCK) void k_sph_hess_finish(Dev d) {
    __shared__ double sh[3 * MSDP_WAVES + 8];
    if (!d.F[0].active) return;
    // Euclidean manifold (generic ManiSDP.m:158-162): H = 2*S*U + 4*sigma*AyU*Y as is
    const bool euc = d.manifold == MANI_EUCLID;
    const double t = euc ? 0.0 : msdp_sum_partials_block(d.P, P_AUX, d.G, sh);
    __syncthreads();
    const int cur = d.ctl->cur;
    const double z = euc ? 0.0 : d.ctl->z_sphere[cur];
    int lo, hi;
    msdp_chunk_rows(d.n_loc, d.G, lo, hi);
    const double* __restrict__ Yl = cur ? d.Y[1] : d.Y[0];
    const int64_t e0 = (int64_t)lo * d.ld, e1 = (int64_t)hi * d.ld;
    double pd = 0.0;
    for (int64_t i = e0 + 2 * threadIdx.x; i < e1; i += 2 * MSDP_BLOCK) {
        const double2 hr = ld2(d.Hmd + i), y = ld2(Yl + i), u = ld2(d.md + i);
        const double2 hq = make_double2(hr.x - t * y.x - 2.0 * z * u.x, hr.y - t * y.y - 2.0 * z * u.y);
        st2(d.Hmd + i, hq);
        pd += u.x * hq.x + u.y * hq.y;
    }
    msdp_put_partial(d.P, P_DHD, pd, sh + 8);
}

__global__ void k_cost_only(Dev d, double sigma, double* out) {
    __shared__ double sh[8];
    const double cx = msdp_sum_partials_block(d.P, P_S1, d.G, sh);
    __syncthreads();
    const double ss = msdp_sum_partials_block(d.P, P_AXB, MSDP_MAX_GRID, sh);
    if (threadIdx.x == 0) *out = cx + 0.5 * sigma * ss;
}

// ------------------------------------------------------------------ multiblock kind, per-block storage (BlockedDev, msdp_affine_dev.h)

// W_b = Ya_b * Yb_b' for every block, in the per-block storage (row r of block b: W[rbase[r] + (c - rlo[r])]): the Gram route of
// A(Ya Yb') for many blocks -- one 8-byte gather per nonzero of At (k_gram_apply) instead of two panel rows of ld doubles
// (k_sddmm1: 6.8 GB through the L2 per call at ld = 128 for the 100 cliques of example_bqp_sparse.m, 795 us).  One wave per
// 16-row tile, v_mfma_f64_16x16x4_f64 over the ld columns, column tile after column tile of the block.
typedef double blkg_d4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_block_gram(BlockedDev bd, const double* __restrict__ Ya, const double* __restrict__ Yb, int ld,
                                                    double* __restrict__ W, const int* skip_flag, int skip_when) {
    if (skip_flag && *skip_flag == skip_when) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, i = lane & 15;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= bd.ntile) return;
    const int row0 = bd.tile_row0[tile];
    const int lo = bd.rlo[row0], hi = bd.rhi[row0];
    const int ra = min(row0 + i, hi - 1);
    const double* __restrict__ arow = Ya + (int64_t)ra * ld;
    for (int c0 = lo; c0 < hi; c0 += 16) {
        const int cb = min(c0 + i, hi - 1);
        const double* __restrict__ brow = Yb + (int64_t)cb * ld;
        blkg_d4 acc = (blkg_d4){0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < ld; k0 += 4) {
            const int kk = k0 + g;
            const double av = kk < ld ? arow[kk] : 0.0;               // A operand: lane (g, i) = Ya[row0 + i][k0 + g]
            const double bv = kk < ld ? brow[kk] : 0.0;               // B operand: lane (g, i) = Yb[c0 + i][k0 + g]
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
        const int col = c0 + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                 // D: row g + 4r, column i
            const int row = row0 + g + 4 * r;
            if (row < hi && col < hi) W[bd.rbase[row] + (col - lo)] = acc[r];
        }
    }
}

// out[q] = (base ? base[q] : 0) + scale * sum_k At[(position q), k] * vec[k]   over all stored positions
__global__ __launch_bounds__(256) void k_adjoint_blocked(BlockedDev bd, const double* __restrict__ base, const double* __restrict__ vec,
                                                         double scale, double* __restrict__ out, const int* skip_flag, int skip_when) {
    if (skip_flag && *skip_flag == skip_when) return;
    // A position that occurs in hundreds of constraints (the (1, 1) entry of a moment block: every `x_i^2 = 1` row) would keep ONE
    // thread in a chain of dependent gathers for the whole launch -- 362 us per call on the 100 cliques of example_bqp_sparse.m,
    // half of a Hess-vec, whatever the order or layout of the short positions: those go to a wave each (workgroups behind the
    // first `gmain`), lanes striding over the list.
    const int gmain = (int)gridDim.x - (bd.nlongq + 3) / 4;
    if ((int)blockIdx.x >= gmain) {
        const int lane = threadIdx.x & 63;
        const int lq = ((int)blockIdx.x - gmain) * 4 + (threadIdx.x >> 6);
        if (lq >= bd.nlongq) return;
        const int64_t q = bd.longq[lq];
        const int s0 = bd.prp[q], s1 = bd.prp[q + 1];
        double acc = 0.0;
        for (int t = s0 + lane; t < s1; t += 64) acc = fma(bd.prv[t], vec[bd.prk[t]], acc);
        acc = msdp_wave_sum(acc);
        if (lane == 0) out[q] = (base ? base[q] : 0.0) + scale * acc;
        return;
    }
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < bd.etot; q += (int64_t)gmain * blockDim.x) {
        const int s0 = bd.prp[q], s1 = bd.prp[q + 1];
        if (s1 - s0 > ADJB_LONG) continue;
        double acc = 0.0;
        for (int t = s0; t < s1; ++t) acc = fma(bd.prv[t], vec[bd.prk[t]], acc);
        out[q] = (base ? base[q] : 0.0) + scale * acc;
    }
}
typedef double blk_d4 __attribute__((ext_vector_type(4)));
// out(rows of a tile, :) = sum_m scale_m * M_m(block rows, block columns) * X_m(block rows, :): one wave per tile, A fragments
// straight from the block's storage rows, B fragments straight from the panel rows (they stay in the L1 / L2 of the CU: a block's
// panel is n_i x p doubles)
template <int NT>
__global__ __launch_bounds__(256) void k_block_contract(BlockedDev bd, BlockOp op, const int* active_flag) {
    if (active_flag && !*active_flag) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, i = lane & 15;
    const int tile = blockIdx.x * 4 + wave;
    if (tile >= bd.ntile) return;
    const int row0 = bd.tile_row0[tile];
    const int lo = bd.rlo[row0], hi = bd.rhi[row0], ns = bd.rns[row0];
    const int64_t abase = bd.rbase[min(row0 + i, hi - 1)] + 4 * g;
    blk_d4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = (blk_d4){0.0, 0.0, 0.0, 0.0};
    for (int m = 0; m < op.nmat; ++m) {
        const double* __restrict__ Mm = op.M[m] + abase;
        const double* __restrict__ Xm = op.X[m];
        const double sc = op.scale[m];
        for (int k = 0; k < ns; k += 16) {
            const double2 a01 = ld2(Mm + k), a23 = ld2(Mm + k + 2);
            const double av[4] = {a01.x * sc, a01.y * sc, a23.x * sc, a23.y * sc};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int xr = lo + k + 4 * g + t;
                const bool ok = xr < hi;                          // pad columns of the block hold zeros; keep the read inside the block
                const double* xp = Xm + (int64_t)(ok ? xr : lo) * op.ld + op.colofs + i;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const double bv = (ok && 16 * nt + i < op.ncols) ? xp[16 * nt] : 0.0;
                    acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t], bv, acc[nt], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = 16 * nt + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + g + 4 * r;
            if (row < hi && col < op.ncols) op.out[(int64_t)row * op.ld + op.colofs + col] = acc[nt][r];
        }
    }
}
__global__ void k_sub_diag_blocked(BlockedDev bd, double* __restrict__ S, const double* __restrict__ zrow) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < bd.N; i += gridDim.x * blockDim.x) S[bd.rbase[i] + (i - bd.rlo[i])] -= zrow[i];
}

// ------------------------------------------------------------------ host side
#define DISPATCH_LPR_A(KERNEL, h, GRID, ...)                                                         \
    do {                                                                                             \
        int half = (h)->d.ld / 2, lpr = 1;                                                           \
        while (lpr < half && lpr < 64) lpr <<= 1;                                                    \
        int nch = (half + lpr - 1) / lpr; if (nch < 1) nch = 1;                                      \
        dim3 grid(GRID), block(MSDP_BLOCK);                                                          \
        if (nch == 1) {                                                                              \
            switch (lpr) {                                                                           \
                case 1:  hipLaunchKernelGGL((KERNEL<1, 1>),  grid, block, 0, (h)->stream, __VA_ARGS__); break; \
                case 2:  hipLaunchKernelGGL((KERNEL<2, 1>),  grid, block, 0, (h)->stream, __VA_ARGS__); break; \
                case 4:  hipLaunchKernelGGL((KERNEL<4, 1>),  grid, block, 0, (h)->stream, __VA_ARGS__); break; \
                case 8:  hipLaunchKernelGGL((KERNEL<8, 1>),  grid, block, 0, (h)->stream, __VA_ARGS__); break; \
                case 16: hipLaunchKernelGGL((KERNEL<16, 1>), grid, block, 0, (h)->stream, __VA_ARGS__); break; \
                case 32: hipLaunchKernelGGL((KERNEL<32, 1>), grid, block, 0, (h)->stream, __VA_ARGS__); break; \
                default: hipLaunchKernelGGL((KERNEL<64, 1>), grid, block, 0, (h)->stream, __VA_ARGS__); break; \
            }                                                                                        \
        } else if (nch == 2) {                                                                       \
            hipLaunchKernelGGL((KERNEL<64, 2>), grid, block, 0, (h)->stream, __VA_ARGS__);           \
        } else if (nch <= 4) {                                                                       \
            hipLaunchKernelGGL((KERNEL<64, 4>), grid, block, 0, (h)->stream, __VA_ARGS__);           \
        } else if (nch <= 8) {                                                                       \
            hipLaunchKernelGGL((KERNEL<64, 8>), grid, block, 0, (h)->stream, __VA_ARGS__);           \
        } else {                                                                                     \
            msdp_set_error("factor width p = %d exceeds the supported maximum of 1024", (h)->d.p);    \
            return MSDP_EUNSUPPORTED;                                                                \
        }                                                                                            \
    } while (0)

// k_sddmm has no reductions, so its grid follows the number of work items, not the number of rows
static int sddmm_grid(const AffineDev& a, int ld) {
    int half = ld / 2, lpr = 1;
    while (lpr < half && lpr < 64) lpr <<= 1;
    const int64_t per_block = (int64_t)MSDP_WAVES * (64 / lpr);
    int64_t g = (a.nitems + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > 8192) g = 8192;
    return (int)g;
}
static bool sharded(msdp_handle h) { return h->use_comm || h->nranks > 1; }          // "Row sharding" below

// A(Ya Yb') -> item values.  SDDMM (gathers 2 p-wide rows per nonzero) or the Gram route (dense W = Ya*Yb' once,
// one double per nonzero), whichever moves fewer bytes; the option affine_route (msdp_set_option) overrides.
static bool use_gram_route(msdp_handle h, const AffineDev& a, int64_t nnz, int ld) {
    if (h->affine->blk) return false;                 // per-block storage: there is no N x N Gram matrix
    if (h->tune.affine_route) return h->tune.affine_route == 2;
    const double sddmm_bytes = (double)nnz * ld * 16.0;
    const double gram_bytes = 2.0 * a.n * (double)a.nS * 8.0 + (double)nnz * 20.0;
    return sddmm_bytes > 4.0 * gram_bytes && (double)a.n * a.nS * 8.0 <= 2.0e9;
}
// The constraints restricted to their entries i <= j (symmetric data): what the Gram route and the finish kernel
// that follows it iterate over.
static void upper_view(AffineDev& a) {
    a.nitems = a.unitems; a.it0 = a.uit0; a.it1 = a.uit1; a.kit = a.ukit; a.longk = a.ulongk; a.nlong = a.unlong;
    a.cidx = a.ucidx; a.cv = a.ucv; a.cjc = a.ucjc;
}
static bool sddmm1_ok(msdp_handle h, const AffineDev& a, int64_t nnz) {
    return h->tune.affine_fuse && !sharded(h) && !use_gram_route(h, a, nnz, a.ld);
}
// w = A(Ya Yb') (mode 0), or additionally Axb = w - b - y/sigma into axb_out and the partial sums of Axb^2 -> P_AXB
// (mode 1: exactly MSDP_MAX_GRID workgroups, the count the consumers re-reduce).  `a` is the caller's copy: on the
// symmetric Gram route it is switched to the upper view.
// mode 2 (k_sddmm1 only, see there): *G2_out = the number of workgroups whose partial sums P_T1..P_T3 carry
int msdp_affine_launch_A(msdp_handle h, AffineDev& a, int64_t nnz, const double* Ya, const double* Yb, const int* flag, int when,
                         int mode, double* axb_out, double sigma, int* G2_out) {
    int64_t gm = (a.m + MSDP_BLOCK - 1) / MSDP_BLOCK;           // mode 0: no reduction, size the grid by m
    if (gm > 2048) gm = 2048;
    const int G = mode == 1 ? MSDP_MAX_GRID : (int)gm;
    // per-block storage: the Gram route on the blocks' own storage once the panel is wide enough for the row gathers of the
    // SDDMM to cost four times the Gram matrix (the rule of use_gram_route, with sum n_i^2 in the place of n^2)
    const BlockedDev* blk = h->affine->blk;
    if (blk && a.W && a.cidx && mode != 2 && h->tune.affine_route != 1 &&
        ((double)nnz * a.ld * 16.0 > 4.0 * (2.0 * (double)blk->etot * 8.0 + (double)nnz * 20.0) || h->tune.affine_route == 2)) {
        hipLaunchKernelGGL(k_block_gram, dim3((blk->ntile + 3) / 4), dim3(256), 0, h->stream, *blk, Ya, Yb, a.ld, a.W, flag, when);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_gram_apply, dim3(G), dim3(MSDP_BLOCK), 0, h->stream, a, (const double*)a.W, mode, axb_out, sigma,
                           h->d.P, flag, when);
        HIPCHK(hipGetLastError());
        h->affine->last_A_route = 3;
        return 0;
    }
    if (sddmm1_ok(h, a, nnz)) {
        int half = a.ld / 2, lpr = 1;
        while (lpr < half && lpr < 64) lpr <<= 1;
        const int64_t per_block = (int64_t)MSDP_WAVES * (64 / lpr);
        int64_t g1 = ((int64_t)a.nshort + a.nlit + per_block - 1) / per_block;
        if (g1 < 1) g1 = 1;
        if (g1 > MSDP_MAX_GRID - 1) g1 = MSDP_MAX_GRID - 1;
        if (mode == 1) g1 = MSDP_MAX_GRID - 1;
        if (mode == 2 && g1 > h->d.n_loc) g1 = std::max(1, h->d.n_loc);
        if (G2_out) *G2_out = (int)g1;
        // workgroups that hold items of long constraints: unit u belongs to workgroup (u / per_block) mod g1
        int nbl = 0;
        if (a.nlit > 0) {
            const int64_t b0 = (int64_t)a.nshort / per_block, b1 = ((int64_t)a.nshort + a.nlit - 1) / per_block;
            nbl = (int)std::min<int64_t>(g1, b1 - b0 + 1);
        }
        DISPATCH_LPR_A(k_sddmm1, h, (int)g1, a, h->d, Ya, Yb, mode, axb_out, sigma, flag, when, nbl);
        HIPCHK(hipGetLastError());
        h->affine->last_A_route = 2;
        return 0;
    }
    if (mode == 2) { msdp_set_error("launch_A: mode 2 needs the fused SDDMM"); return MSDP_ESTATE; }
    if (use_gram_route(h, a, nnz, a.ld)) {
        dim3 grid((a.nS + 63) / 64, (a.n + 63) / 64);
        const int sym = a.usym ? 1 : 0;
        if (sym) upper_view(a);
        hipLaunchKernelGGL(k_gram_mfma, grid, dim3(512), 0, h->stream, a.n, a.nS, a.ld, Ya, Yb, a.W, flag, when, sym);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_gram_apply, dim3(G), dim3(MSDP_BLOCK), 0, h->stream, a, (const double*)a.W, mode, axb_out, sigma,
                           h->d.P, flag, when);
        HIPCHK(hipGetLastError());
        h->affine->last_A_route = 3;
        return 0;
    }
    DISPATCH_LPR_A(k_sddmm, h, sddmm_grid(a, a.ld), a, Ya, Yb, flag, when);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_sddmm_finish, dim3(G), dim3(MSDP_BLOCK), 0, h->stream, a, mode, axb_out, sigma, h->d.P, flag, when);
    HIPCHK(hipGetLastError());
    h->affine->last_A_route = 1;
    return 0;
}

static int adjoint_grid(const AffineDev& a) {
    int64_t tot = (int64_t)a.n * a.nS;
    int64_t g = (tot + 255) / 256;
    if (g > 4096) g = 4096;
    return (int)g;
}

// out = base + scale * At*vec.  `restricted_ok`: `out` already holds base (or 0) outside the entries At touches.
int msdp_affine_launch_adjoint(msdp_handle h, const AffineDev& a, const double* base, const double* vec, double scale, double* out,
                               const int* flag, int when, bool restricted_ok) {
    if (const BlockedDev* blk = h->affine->blk) {
        const int64_t g = std::min<int64_t>(4096, (blk->etot + 255) / 256) + (blk->nlongq + 3) / 4;
        hipLaunchKernelGGL(k_adjoint_blocked, dim3((int)g), dim3(256), 0, h->stream, *blk, base, vec, scale, out, flag, when);
        HIPCHK(hipGetLastError());
        return 0;
    }
    if (restricted_ok && a.nsup > 0) {
        int g = (a.nsup + 255) / 256;
        if (g > 4096) g = 4096;
        hipLaunchKernelGGL(k_adjoint_support, dim3(g), dim3(256), 0, h->stream, a, base, vec, scale, out, flag, when);
    } else if (a.ntp > 0) {
        hipLaunchKernelGGL(k_adjoint_tiled, dim3(a.ntp + (a.nlong_e + 3) / 4), dim3(256), 0, h->stream, a, base, vec, scale, out, flag, when);
    } else {
        hipLaunchKernelGGL(k_adjoint_dense, dim3(adjoint_grid(a)), dim3(256), 0, h->stream, a, base, vec, scale, out, flag, when);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// slab <- scale * (A'(vec) restricted to the touched entries) * Yp   (k_support_spmm; a.nsup > 0, ld <= 512)
static int launch_support_spmm(msdp_handle h, const AffineDev& a, const double* vec, const double* Yp, double scale,
                               double* out, const int* flag, int when) {
    const int nch = (a.ld + 127) / 128;
    const dim3 g(std::min((a.n + 3) / 4, 2048)), b(256);
    switch (nch) {
        case 1: hipLaunchKernelGGL(k_support_spmm<1>, g, b, 0, h->stream, a, vec, Yp, scale, out, flag, when); break;
        case 2: hipLaunchKernelGGL(k_support_spmm<2>, g, b, 0, h->stream, a, vec, Yp, scale, out, flag, when); break;
        case 3: hipLaunchKernelGGL(k_support_spmm<3>, g, b, 0, h->stream, a, vec, Yp, scale, out, flag, when); break;
        default: hipLaunchKernelGGL(k_support_spmm<4>, g, b, 0, h->stream, a, vec, Yp, scale, out, flag, when); break;
    }
    HIPCHK(hipGetLastError());
    return 0;
}


// The dense products of the closures: the MFMA contraction of msdp_dense.hip, or -- multiblock kind with per-block storage -- one
// wave per 16-row tile of a block, written to slab 0 (SK = 1)
int msdp_affine_gemm(msdp_handle h, int nmat, const double* const* M, const double* const* X, const double* scale, const int* active_flag,
                     const double** slab_out, int64_t* stride_out, int* SK_out) {
    AffineState* st = h->affine;
    if (!st || !st->blk) return msdp_dense_gemm(h, nmat, M, X, scale, active_flag, slab_out, stride_out, SK_out);
    Dev& d = h->d;
    const int64_t stride = (int64_t)d.n * d.ld;
    int rc = msdp_dense_ensure_slab(h, (size_t)2 * stride);
    if (rc) return rc;
    BlockOp op;
    memset(&op, 0, sizeof(op));
    op.nmat = nmat; op.ld = d.ld; op.out = h->slab;
    for (int m = 0; m < nmat; ++m) { op.M[m] = M[m]; op.X[m] = X[m]; op.scale[m] = scale[m]; }
    const dim3 grid((st->blk->ntile + 3) / 4), block(256);
    for (int colofs = 0; colofs < d.ld; colofs += 128) {
        op.colofs = colofs; op.ncols = std::min(128, d.ld - colofs);
        switch ((op.ncols + 15) / 16) {
            case 1: hipLaunchKernelGGL(k_block_contract<1>, grid, block, 0, h->stream, *st->blk, op, active_flag); break;
            case 2: hipLaunchKernelGGL(k_block_contract<2>, grid, block, 0, h->stream, *st->blk, op, active_flag); break;
            case 3: hipLaunchKernelGGL(k_block_contract<3>, grid, block, 0, h->stream, *st->blk, op, active_flag); break;
            case 4: hipLaunchKernelGGL(k_block_contract<4>, grid, block, 0, h->stream, *st->blk, op, active_flag); break;
            default: hipLaunchKernelGGL(k_block_contract<8>, grid, block, 0, h->stream, *st->blk, op, active_flag); break;
        }
    }
    HIPCHK(hipGetLastError());
    *slab_out = h->slab; *stride_out = stride; *SK_out = 1;
    return 0;
}
// W = Ya * Yb' in the handle's storage: n x nS, or block by block (per-block storage)
int msdp_affine_gram(msdp_handle h, const double* Ya, const double* Yb, double* W, const int* flag, int when) {
    const AffineState* st = h->affine;
    const AffineDev& a = st->a;
    const int ld = h->d.ld;
    if (st->blk)
        hipLaunchKernelGGL(k_block_gram, dim3((st->blk->ntile + 3) / 4), dim3(256), 0, h->stream, *st->blk, Ya, Yb, ld, W, flag, when);
    else
        hipLaunchKernelGGL(k_gram_mfma, dim3((a.nS + 63) / 64, (a.n + 63) / 64), dim3(512), 0, h->stream, a.n, a.nS, ld, Ya, Yb, W, flag, when, 0);
    HIPCHK(hipGetLastError());
    return 0;
}
// k_rowdot_slabs on the handle's rows, with the lanes per row its factor width asks for
int msdp_affine_rowdot_slabs(msdp_handle h, const double* Yl, const double* slab, int64_t stride, int SK, double scale_out,
                             double* dst, double* rowdot_out, int which) {
    Dev& d = h->d;
    DISPATCH_LPR_A(k_rowdot_slabs, h, d.G, d, Yl, slab, stride, SK, scale_out, dst, rowdot_out, which);
    HIPCHK(hipGetLastError());
    return 0;
}
// G from 2*eS*Y in Gr[slot]: the oblique finish (row dots in eG[slot]) or the sphere / Euclidean one; f_given: see the kernels
int msdp_affine_grad_finish(msdp_handle h, bool oblique, int slot, double sigma, const double* f_given) {
    Dev& d = h->d;
    if (oblique) {
        DISPATCH_LPR_A(k_obl_grad_finish, h, d.G, d, slot, sigma, f_given);
    } else {
        hipLaunchKernelGGL(k_sph_grad_finish, dim3(d.G), dim3(MSDP_BLOCK), 0, h->stream, d, slot, sigma, f_given);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ Row sharding of the affine kinds
// The rows of Y, U, G, H are split over the ranks as for the other kinds; the OPERATOR state is replicated: every rank
// holds At, the dense eS / AyU / S and computes A(Ya Yb'), Axb and the adjoint for the whole matrix itself -- the same
// kernels on the same inputs give the same bits on every rank, so no m-vector travels (for BQP d = 60 an all-reduce of
// the 9-MB A(U Y') per Hess-vec would cost more than recomputing it: 17 us).  What is shared is the dense contraction
// (each rank multiplies ITS rows of eS / AyU with the gathered panel) and every row-parallel kernel; their partial sums
// are all-reduced like those of the other kinds.  The operators read all rows of the point: yfull[slot] keeps the
// gathered copy of Y[slot] (the Hess-vec needs it next to the gathered direction).
// All n rows of Y[slot].  `gathered`: d.full holds them right now (the caller's all-gather) -> refresh the copy.
static int full_rows(msdp_handle h, int slot, const double* local, bool gathered, const double** out) {
    if (!sharded(h)) { *out = local; return 0; }
    if (!h->yfull[slot]) { msdp_set_error("row-sharded affine handle without gather buffers"); return MSDP_ESTATE; }
    if (!gathered) { int rc = msdp_allgather_rows(h, local); if (rc) return rc; }
    const size_t cap = (size_t)((h->d.n + h->nranks - 1) / h->nranks);
    HIPCHK(msdp_memcpy_async(h->yfull[slot], h->d.full, cap * h->nranks * (size_t)h->d.ld * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    *out = h->yfull[slot];
    return 0;
}
static const double* kept_rows(msdp_handle h, int slot) { return sharded(h) ? h->yfull[slot] : h->d.Y[slot]; }

// cost + gradient state at Y[slot]:  w = A(YY'), Axb, eS, eS*Y, C*Y  (see header comment)
int msdp_affine_costgrad(msdp_handle h, int slot) {
    AffineState* st = h->affine;
    if (!st) { msdp_set_error("affine state missing"); return MSDP_ESTATE; }
    if (st->dual) return msdp_dual_costgrad(h, st, slot);
    Dev& d = h->d;
    AffineDev a = st->a;
    a.p = d.p; a.ld = d.ld;
    const double sigma = st->sigma;
    const double* Ys = d.Y[slot];                         // my rows
    const double* Yf = nullptr;                           // all rows (the caller, msdp_launch_costgrad, has gathered them)
    { int rcf = full_rows(h, slot, Ys, true, &Yf); if (rcf) return rcf; }
    const size_t roff = (size_t)d.row0 * a.nS;            // my rows of the replicated n x nS matrices
    const int* done = &d.ctl->done;
    { int rc0 = msdp_affine_launch_A(h, a, st->nnz, Yf, Yf, done, 1, 1, a.Axb[slot], sigma); if (rc0) return rc0; }
    { int rca = msdp_affine_launch_adjoint(h, a, d.Cd, a.Axb[slot], sigma, d.eS[slot], done, 1, true); if (rca) return rca; }
    // c'x = <C*Y, Y>
    const double* slab; int64_t stride; int SK;
    {
        const double* M[1] = {d.Cd + roff}; const double* X[1] = {Yf}; const double sc[1] = {1.0};
        int rc = msdp_affine_gemm(h, 1, M, X, sc, nullptr, &slab, &stride, &SK);
        if (rc) return rc;
        { int rcd = msdp_affine_rowdot_slabs(h, Ys, slab, stride, SK, 1.0, (double*)nullptr, (double*)nullptr, P_S1); if (rcd) return rcd; }
    }
    // eG = 2*eS*Y -> Gr[slot]; row dots (YeG = sum(Y.*eG)) and their total (2z)
    if (a.nsup > 0 && !sharded(h) && d.ld <= 512) {
        // At touches few entries: eS*Y = C*Y (the slabs just computed) + sigma * (A'(Axb) on those entries) * Y,
        // appended as one more slab -- one dense product per cost/gradient evaluation instead of two
        double* extra = const_cast<double*>(slab) + (int64_t)SK * stride;
        int rc = launch_support_spmm(h, a, (const double*)a.Axb[slot], Ys, sigma, extra, done, 1);
        if (rc) return rc;
        ++SK;
        { int rcd = msdp_affine_rowdot_slabs(h, Ys, slab, stride, SK, 2.0, d.Gr[slot], d.eG[slot], P_S2); if (rcd) return rcd; }
    } else {
        const double* M[1] = {d.eS[slot] + roff}; const double* X[1] = {Yf}; const double sc[1] = {1.0};
        int rc = msdp_affine_gemm(h, 1, M, X, sc, nullptr, &slab, &stride, &SK);
        if (rc) return rc;
        { int rcd = msdp_affine_rowdot_slabs(h, Ys, slab, stride, SK, 2.0, d.Gr[slot], d.eG[slot], P_S2); if (rcd) return rcd; }
    }
    { int rcr = msdp_allreduce_partials(h, P_S1, 2); if (rcr) return rcr; }      // <C*Y, Y> and the row dots over all ranks
    return msdp_affine_grad_finish(h, d.manifold == MANI_OBLIQUE, slot, sigma, nullptr);
}

// Algorithmic traffic / work of one Hess-vec of the affine kinds (SURVEY.md 8d, A-operator): At is read twice (w = A(Y U'),
// A'(w): values + indices, 12 bytes per nonzero each), A'(w) is written and read once over the entries At touches (all n^2
// of them for BQP, 55 276 of 25 M for the theta-like problem), eS is read once, the three n x p panels once each.
void msdp_affine_algo_cost(msdp_handle h, double* bytes, double* flops) {
    AffineState* st = h->affine;
    *bytes = 0.0; *flops = 0.0;
    if (!st || st->dual) return;
    const AffineDev& a = st->a;
    const double n = a.n, p = h->d.p, nnz = (double)st->nnz;
    const double touched = a.nsup > 0 ? (double)a.nsup : n * n;
    *bytes = 2.0 * nnz * 12.0 + 16.0 * touched + 8.0 * n * n + 24.0 * n * p;
    *flops = 2.0 * n * n * p + 2.0 * touched * p + 2.0 * nnz * p + 4.0 * nnz;
}

int msdp_affine_hess(msdp_handle h) {
    AffineState* st = h->affine;
    if (!st) { msdp_set_error("affine state missing"); return MSDP_ESTATE; }
    if (st->dual) return msdp_dual_hess(h, st);
    Dev& d = h->d;
    AffineDev a = st->a;
    a.p = d.p; a.ld = d.ld;
    const double sigma = st->sigma;
    const int cur = h->h_ctl->cur;
    const int* act = &d.F[0].active;
    // all rows of the point (kept since its cost/gradient evaluation) and of the direction (gathered by msdp_launch_hess)
    const double* Yf = kept_rows(h, cur);
    const double* Uf = sharded(h) ? (const double*)d.full : (const double*)d.md;
    const size_t roff = (size_t)d.row0 * a.nS;
    const double* slab; int64_t stride; int SK;
    int rc;
    if (h->tune.affine_overlap) {
        st->last_hess_path = 1;
        // A/B switch, default OFF.  Two branches of the Hess-vec are independent until the epilogue sums their slabs: 2*eS*U (one
        // dense contraction) and the chain w = A(Y U') -> A'(w) -> 4 sigma A'(w)*Y.  Here they run side by side on two streams
        // (fork / join by events; inside a captured chunk the second stream joins the capture).  Measured in round 3: slower than
        // one stream (BQP d = 60: 85 against 73 us, theta n = 5000: 83 against 74 us) -- each launch of the chain fills the chip by
        // itself, the split contraction loses its two-matrix launch, and the fork / join adds graph dependencies.
        if (!st->s2) {
            HIPCHK(hipStreamCreateWithFlags(&st->s2, hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&st->ev_fork, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&st->ev_join, hipEventDisableTiming));
        }
        const int sk1 = msdp_dense_gemm_slabs(h, 1);
        const bool support = a.nsup > 0 && d.ld <= 512 && !sharded(h);
        const int total = support ? sk1 + 1 : 2 * sk1;
        int SKa = 0, SKb = 0;
        HIPCHK(hipEventRecord(st->ev_fork, h->stream));
        HIPCHK(hipStreamWaitEvent(st->s2, st->ev_fork, 0));
        {
            const double* M[1] = {d.eS[cur] + roff}; const double* X[1] = {Uf}; const double sc[1] = {2.0};
            if ((rc = msdp_dense_gemm_at(h, st->s2, 0, total, 1, M, X, sc, act, &slab, &stride, &SKa))) return rc;
        }
        HIPCHK(hipEventRecord(st->ev_join, st->s2));
        if ((rc = msdp_affine_launch_A(h, a, st->nnz, Yf, Uf, act, 0, 0, (double*)nullptr, sigma))) return rc;
        if (support) {
            double* extra = const_cast<double*>(slab) + (int64_t)SKa * stride;
            if ((rc = launch_support_spmm(h, a, (const double*)a.w, (const double*)d.Y[cur], 4.0 * sigma, extra, act, 0))) return rc;
            SKb = 1;
        } else {
            if ((rc = msdp_affine_launch_adjoint(h, a, (const double*)nullptr, a.w, 1.0, d.AyU, act, 0, true))) return rc;
            const double* M[1] = {d.AyU + roff}; const double* X[1] = {Yf}; const double sc[1] = {4.0 * sigma};
            const double* slab2;
            if ((rc = msdp_dense_gemm_at(h, h->stream, SKa, total, 1, M, X, sc, act, &slab2, &stride, &SKb))) return rc;
        }
        HIPCHK(hipStreamWaitEvent(h->stream, st->ev_join, 0));
        SK = SKa + SKb;
        if (d.manifold == MANI_OBLIQUE) return msdp_dense_hess_epilogue_obl(h, slab, stride, SK);
        return msdp_sphere_hess_raw(h, slab, stride, SK);
    }
    if (a.bW > 0 && h->tune.affine_broute && !sharded(h) && !(a.nsup > 0 && d.ld <= 512) && use_gram_route(h, a, st->nnz, a.ld)) {
        // B route: AyU = B * (Y U' + U Y') in one sparse pass over the upper entries (k_adjoint_gram) -- no w, At read once
        st->last_hess_path = 2;
        dim3 grid((a.nS + 63) / 64, (a.n + 63) / 64);
        hipLaunchKernelGGL(k_gram_mfma, grid, dim3(512), 0, h->stream, a.n, a.nS, a.ld, Yf, Uf, a.Wg, act, 0, 1);
        HIPCHK(hipGetLastError());
        const dim3 ga(a.ntp + (a.bnlong + 3) / 4), ba(256);
        const bool pk = a.bpk != nullptr;
#define AG(BW) do { if (pk) hipLaunchKernelGGL((k_adjoint_gram<BW, true>), ga, ba, 0, h->stream, a, (const double*)a.Wg, 1.0, d.AyU, act, 0); \
                    else hipLaunchKernelGGL((k_adjoint_gram<BW, false>), ga, ba, 0, h->stream, a, (const double*)a.Wg, 1.0, d.AyU, act, 0); } while (0)
        switch (a.bW) { case 1: AG(1); break; case 2: AG(2); break; case 3: AG(3); break; default: AG(4); break; }
#undef AG
        HIPCHK(hipGetLastError());
        const double* M[2] = {d.eS[cur] + roff, d.AyU + roff};
        const double* X[2] = {Uf, Yf};
        const double sc[2] = {2.0, 4.0 * sigma};
        if ((rc = msdp_affine_gemm(h, 2, M, X, sc, act, &slab, &stride, &SK))) return rc;
        if (d.manifold == MANI_OBLIQUE) return msdp_dense_hess_epilogue_obl(h, slab, stride, SK);
        return msdp_sphere_hess_raw(h, slab, stride, SK);
    }
    if (d.manifold != MANI_OBLIQUE && a.usym && d.ld <= 512 && sddmm1_ok(h, a, st->nnz)) {
        // sphere / Euclidean factor, SDDMM route, one rank: three launches + the contraction (k_sddmm1 mode 2, [adjoint,]
        // contraction, k_sph_hess_fused) instead of six
        int G2 = 0, hetero = 0;
        const bool support = a.nsup > 0;
        if (support && h->tune.affine_overlap) {
            // A/B (option affine_overlap): 2*eS*U needs neither w nor the sums -- it runs on a second stream beside k_sddmm1 and joins in
            // front of the epilogue
            if (!st->s2) {
                HIPCHK(hipStreamCreateWithFlags(&st->s2, hipStreamNonBlocking));
                HIPCHK(hipEventCreateWithFlags(&st->ev_fork, hipEventDisableTiming));
                HIPCHK(hipEventCreateWithFlags(&st->ev_join, hipEventDisableTiming));
            }
            const double* M[1] = {d.eS[cur]}; const double* X[1] = {d.md}; const double sc[1] = {2.0};
            HIPCHK(hipEventRecord(st->ev_fork, h->stream));
            HIPCHK(hipStreamWaitEvent(st->s2, st->ev_fork, 0));
            if ((rc = msdp_dense_gemm_at(h, st->s2, 0, 0, 1, M, X, sc, act, &slab, &stride, &SK))) return rc;
            HIPCHK(hipEventRecord(st->ev_join, st->s2));
            if ((rc = msdp_affine_launch_A(h, a, st->nnz, Yf, Uf, act, 0, 2, (double*)nullptr, sigma, &G2))) return rc;
            HIPCHK(hipStreamWaitEvent(h->stream, st->ev_join, 0));
        } else if (support) {
            // default: the SDDMM rides in the contraction launch as a side job (msdp_dense_gemm_side) -- where the shape allows it
            rc = MSDP_EUNSUPPORTED;
            if (h->tune.affine_side && a.nlong <= MSDP_WAVES) {
                SideJob sj;
                memset(&sj, 0, sizeof(sj));
                sj.a = a; sj.Ya = Yf; sj.Yb = Uf; sj.Gr = d.Gr[cur]; sj.axc = a.Axb[cur]; sj.P = d.P; sj.sigma = sigma;
                rc = msdp_dense_gemm_side(h, d.eS[cur], d.md, 2.0, act, sj, &G2, &slab, &stride, &SK);
                if (rc == 0) hetero = 1;
                else if (rc != MSDP_EUNSUPPORTED) return rc;
            }
            if (!hetero) {
                if ((rc = msdp_affine_launch_A(h, a, st->nnz, Yf, Uf, act, 0, 2, (double*)nullptr, sigma, &G2))) return rc;
                const double* M[1] = {d.eS[cur]}; const double* X[1] = {d.md}; const double sc[1] = {2.0};
                if ((rc = msdp_affine_gemm(h, 1, M, X, sc, act, &slab, &stride, &SK))) return rc;
            }
        } else {
            if ((rc = msdp_affine_launch_A(h, a, st->nnz, Yf, Uf, act, 0, 2, (double*)nullptr, sigma, &G2))) return rc;
            if ((rc = msdp_affine_launch_adjoint(h, a, (const double*)nullptr, a.w, 1.0, d.AyU, act, 0, true))) return rc;
            const double* M[2] = {d.eS[cur], d.AyU}; const double* X[2] = {Uf, Yf}; const double sc[2] = {2.0, 4.0 * sigma};
            if ((rc = msdp_affine_gemm(h, 2, M, X, sc, act, &slab, &stride, &SK))) return rc;
        }
        DISPATCH_LPR_A(k_sph_hess_fused, h, d.G, d, a, slab, stride, SK, sigma, G2, support ? 1 : 0, cur, hetero);
        HIPCHK(hipGetLastError());
        st->last_hess_path = hetero ? 3 : 4;
        return 0;
    }
    // w = A(Y U') ; AyU = A'(w)
    { int rc0 = msdp_affine_launch_A(h, a, st->nnz, Yf, Uf, act, 0, 0, (double*)nullptr, sigma); if (rc0) return rc0; }
    if (a.nsup > 0 && !sharded(h) && d.ld <= 512) {
        // At touches few entries: AyU*Y is a sparse product over those entries (appended as one more slab); only
        // 2*eS*U goes through the dense contraction
        const double* M[1] = {d.eS[cur]};
        const double* X[1] = {d.md};
        const double sc[1] = {2.0};
        if ((rc = msdp_affine_gemm(h, 1, M, X, sc, act, &slab, &stride, &SK))) return rc;
        double* extra = const_cast<double*>(slab) + (int64_t)SK * stride;
        if ((rc = launch_support_spmm(h, a, (const double*)a.w, (const double*)d.Y[cur], 4.0 * sigma, extra, act, 0))) return rc;
        ++SK;
        st->last_hess_path = 5;
    } else {
        { int rca = msdp_affine_launch_adjoint(h, a, (const double*)nullptr, a.w, 1.0, d.AyU, act, 0, true); if (rca) return rca; }
        const double* M[2] = {d.eS[cur] + roff, d.AyU + roff};
        const double* X[2] = {Uf, Yf};
        const double sc[2] = {2.0, 4.0 * sigma};
        if ((rc = msdp_affine_gemm(h, 2, M, X, sc, act, &slab, &stride, &SK))) return rc;
        st->last_hess_path = 6;
    }
    if (d.manifold == MANI_OBLIQUE) return msdp_dense_hess_epilogue_obl(h, slab, stride, SK);
    return msdp_sphere_hess_raw(h, slab, stride, SK);
}

// sphere: H_raw = sum slabs -> Hmd, partial <H_raw, Y> -> P_AUX; then the finish kernel.
template <int LPR, int NCH>
__global__ __launch_bounds__(MSDP_BLOCK) void k_sph_hess_raw(Dev d, const double* slab, int64_t slab_stride, int SK) {
    __shared__ double sh[3 * MSDP_WAVES];
    if (!d.F[0].active) return;
    int lo, hi;
    msdp_chunk_rows(d.n_loc, d.G, lo, hi);
    const int cur = d.ctl->cur;
    const double* __restrict__ Yl = cur ? d.Y[1] : d.Y[0];
    const int64_t e0 = (int64_t)lo * d.ld, e1 = (int64_t)hi * d.ld;
    double pt = 0.0;
    for (int64_t i = e0 + 2 * threadIdx.x; i < e1; i += 2 * MSDP_BLOCK) {
        const double2 acc = msdp_sum_slabs(slab, slab_stride, SK, i);
        const double2 y = ld2(Yl + i);
        st2(d.Hmd + i, acc);
        pt += acc.x * y.x + acc.y * y.y;
    }
    msdp_put_partial(d.P, P_AUX, pt, sh);
}

int msdp_sphere_hess_raw(msdp_handle h, const double* slab, int64_t stride, int SK) {
    Dev& d = h->d;
    hipLaunchKernelGGL((k_sph_hess_raw<1, 1>), dim3(d.G), dim3(MSDP_BLOCK), 0, h->stream, d, slab, stride, SK);
    HIPCHK(hipGetLastError());
    { int rcr = msdp_allreduce_partials(h, P_AUX, 1); if (rcr) return rcr; }     // <H_raw, Y> over all ranks
    hipLaunchKernelGGL(k_sph_hess_finish, dim3(d.G), dim3(MSDP_BLOCK), 0, h->stream, d);
    HIPCHK(hipGetLastError());
    return 0;
}

// co(Y) of the line search at the trial point Yt (device, n x ld): c'x + sigma/2 |A x - b - y/sigma|^2
int msdp_affine_linesearch_cost(msdp_handle h, const double* Yt, double* val) {
    AffineState* st = h->affine;
    if (!st) { msdp_set_error("affine state missing"); return MSDP_ESTATE; }
    if (st->dual) return msdp_dual_linesearch_cost(h, st, Yt, val);
    Dev& d = h->d;
    AffineDev a = st->a;
    a.p = d.p; a.ld = d.ld;
    const double sigma = st->sigma;
    const int other = h->h_ctl->cur ^ 1;
    const double* Yf = nullptr;
    { int rcf = full_rows(h, other, Yt, false, &Yf); if (rcf) return rcf; }
    { int rc0 = msdp_affine_launch_A(h, a, st->nnz, Yf, Yf, (const int*)nullptr, 0, 1, a.Axb[other], sigma); if (rc0) return rc0; }
    const double* slab; int64_t stride; int SK;
    const double* M[1] = {d.Cd + (size_t)d.row0 * a.nS}; const double* X[1] = {Yf}; const double sc[1] = {1.0};
    int rc = msdp_affine_gemm(h, 1, M, X, sc, nullptr, &slab, &stride, &SK);
    if (rc) return rc;
    { int rcd = msdp_affine_rowdot_slabs(h, Yt, slab, stride, SK, 1.0, (double*)nullptr, (double*)nullptr, P_S1); if (rcd) return rcd; }
    if ((rc = msdp_allreduce_partials(h, P_S1, 1))) return rc;
    hipLaunchKernelGGL(k_cost_only, dim3(1), dim3(MSDP_BLOCK), 0, h->stream, d, sigma, &d.ctl->fx_prop);
    HIPCHK(hipGetLastError());
    double v = 0.0;
    HIPCHK(msdp_memcpy_async(&v, &d.ctl->fx_prop, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *val = v;
    return 0;
}

// ------------------------------------------------------------------ AL bookkeeping on the device
// The host AL loop of the affine entry points needs, once per outer iteration (ManiSDP_unitdiag.m:59-70,
// ManiSDP_unittrace.m:59-70, ManiSDP.m:58-68): obj = c'x and Axb = A x - b at the new point, then with the NEW
// multipliers eS = reshape(c - At*y), z = sum(X.*eS) and S = eS - diag(z) (unit diagonal) / S = eS - z*I
// (unit trace) / S = eS (generic).  On the host that is n^2-sized NumPy/SciPy work (X = YY', two SpMVs with
// 4.8 M nonzeros, the dense eS): 49% of the BQP d = 60 solve.  Here the same quantities come from the kernels
// of the hot path: A(YY') (SDDMM or Gram route), the dense adjoint, the MFMA contraction and a row-dot.

// rows: S[i][j] -= (i == j) * (zrow ? zrow[i] : *zscalar)
__global__ void k_sub_diag(int n, int nS, double* __restrict__ S, const double* __restrict__ zrow, const double* __restrict__ zscalar) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        S[(int64_t)i * nS + i] -= zrow ? zrow[i] : *zscalar;
}

// obj = c'x, w = A x (m doubles to the host; the caller subtracts b)
int msdp_affine_al_primal(msdp_handle h, double* obj, double* Ax_host) {
    AffineState* st = h->affine;
    if (!st) { msdp_set_error("affine state missing"); return MSDP_ESTATE; }
    Dev& d = h->d;
    AffineDev a = st->a;
    a.p = d.p; a.ld = d.ld;
    const int cur = h->h_ctl->cur;
    const double* Ys = d.Y[cur];
    const double* Yf = nullptr;
    int rc = full_rows(h, cur, Ys, false, &Yf);
    if (rc) return rc;
    if ((rc = msdp_affine_launch_A(h, a, st->nnz, Yf, Yf, (const int*)nullptr, 0, 0, (double*)nullptr, 1.0))) return rc;
    const double* slab; int64_t stride; int SK;
    const double* M[1] = {d.Cd + (size_t)d.row0 * a.nS}; const double* X[1] = {Yf}; const double sc[1] = {1.0};
    if ((rc = msdp_affine_gemm(h, 1, M, X, sc, nullptr, &slab, &stride, &SK))) return rc;
    { int rcd = msdp_affine_rowdot_slabs(h, Ys, slab, stride, SK, 1.0, (double*)nullptr, (double*)nullptr, P_S1); if (rcd) return rcd; }
    if ((rc = msdp_allreduce_partials(h, P_S1, 1))) return rc;
    if ((rc = msdp_k_sum_to(h, P_S1, &d.ctl->fx_prop))) return rc;
    double v = 0.0;
    HIPCHK(msdp_memcpy_async(&v, &d.ctl->fx_prop, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(msdp_memcpy_async(Ax_host, a.w, (size_t)a.m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *obj = v;
    return 0;
}

// eS = c - At*y, z, S (left in d.Sdual for msdp_escape_eigs_dual); z -> host (n values, or 1 for the sphere, none for generic)
int msdp_affine_al_dual(msdp_handle h, const double* y_host, double* z_host) {
    AffineState* st = h->affine;
    if (!st) { msdp_set_error("affine state missing"); return MSDP_ESTATE; }
    Dev& d = h->d;
    AffineDev a = st->a;
    a.p = d.p; a.ld = d.ld;
    const int cur = h->h_ctl->cur;
    const double* Ys = d.Y[cur];
    HIPCHK(msdp_memcpy_async(a.w, y_host, (size_t)a.m * sizeof(double), hipMemcpyHostToDevice, h->stream));
    // full sweep: the diagonal of Sdual was modified by k_sub_diag after the previous call
    { int rca = msdp_affine_launch_adjoint(h, a, d.Cd, (const double*)a.w, -1.0, d.Sdual, (const int*)nullptr, 0, false); if (rca) return rca; }
    if (d.manifold == MANI_EUCLID) { HIPCHK(hipStreamSynchronize(h->stream)); return 0; }
    // t_i = <(eS*Y)_i, Y_i>  (= sum(X.*eS) per row); their total for the sphere
    const double* Yf = nullptr;
    int rc = full_rows(h, cur, Ys, false, &Yf);          // also what the escape deflates against (msdp_escape.hip)
    if (rc) return rc;
    const double* slab; int64_t stride; int SK;
    const double* M[1] = {d.Sdual + (size_t)d.row0 * a.nS}; const double* X[1] = {Yf}; const double sc[1] = {1.0};
    if ((rc = msdp_affine_gemm(h, 1, M, X, sc, nullptr, &slab, &stride, &SK))) return rc;
    { int rcd = msdp_affine_rowdot_slabs(h, Ys, slab, stride, SK, 1.0, (double*)nullptr, d.W0, P_S2); if (rcd) return rcd; }
    if (d.manifold == MANI_OBLIQUE) {
        const double* zall = d.W0;
        if (sharded(h)) {
            // z of all rows: one all-gather of the cap-long row blocks (the gather buffer is free here)
            if (!h->use_comm) { msdp_set_error("al_dual on a communicator-free shard"); return MSDP_ESTATE; }
            const size_t cap = (size_t)((d.n + h->nranks - 1) / h->nranks);
            if ((rc = msdp_allgather_vec(h, d.W0, h->full_buf, cap))) return rc;
            zall = h->full_buf;
        }
        if (st->blk) hipLaunchKernelGGL(k_sub_diag_blocked, dim3((a.n + 255) / 256), dim3(256), 0, h->stream, *st->blk, d.Sdual, zall);
        else hipLaunchKernelGGL(k_sub_diag, dim3((a.n + 255) / 256), dim3(256), 0, h->stream, a.n, a.nS, d.Sdual, zall, (const double*)nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(msdp_memcpy_async(z_host, zall, (size_t)a.n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    } else {
        if ((rc = msdp_allreduce_partials(h, P_S2, 1))) return rc;
        if ((rc = msdp_k_sum_to(h, P_S2, &d.ctl->fx_prop))) return rc;
        hipLaunchKernelGGL(k_sub_diag, dim3((a.n + 255) / 256), dim3(256), 0, h->stream, a.n, a.nS, d.Sdual, (const double*)nullptr, (const double*)&d.ctl->fx_prop);
        HIPCHK(hipGetLastError());
        HIPCHK(msdp_memcpy_async(z_host, &d.ctl->fx_prop, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
