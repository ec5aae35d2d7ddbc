// msdp_affine_plan.h -- the host index arithmetic of the affine set-ups (msdp_affine_setup.hip) as pure functions: host arrays
// in, a struct of std::vectors out, element for element what the set-up uploads (the single placeholder element of an array
// that would be empty included).  No HIP and nothing else of the project: tools/affine_plan_selftest.cpp runs all of it on the
// CPU, under the sanitizers.  AffineDev / BlockedDev (msdp_affine_dev.h) say what the kernels do with every array.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <utility>
#include <vector>

#define SDDMM_CHUNK 16        // nonzeros per work item of the SDDMM
#define FIN_SHORT 8           // constraints with more items than this are summed by a whole wave (k_sddmm_finish)
#define ADJ_T 32              // tile order of k_adjoint_tiled / k_adjoint_gram
#define ADJ_LONG 8            // entries in more constraints than this go to a wave each (k_adjoint_tiled)
#define ADJB_LONG 16          // the same for the stored positions of k_adjoint_blocked

// ---- SDDMM work: constraint k owns the nonzeros cjc[k] .. cjc[k+1]-1 (both set-ups, and the upper view below)
struct SddmmPlan {
    std::vector<int> it0, it1, kit;           // items of <= SDDMM_CHUNK nonzeros; items of constraint k: kit[k] .. kit[k+1]-1
    std::vector<int> longk;                   // constraints with more than FIN_SHORT items
    std::vector<int> sk, lit0, lit1, lkit;    // k_sddmm1: the short constraints; the items of the long ones, lkit[q] .. lkit[q+1]-1 of longk[q]
    std::vector<int> us0, us1, uk;            // units: the short constraints whole (uk = k), then the long items (uk = -1 - item)
    int64_t nitems = 0;
    int nlong = 0, nshort = 0, nlit = 0;
};
static inline void plan_items(int64_t m, const int* cjc, std::vector<int>& it0, std::vector<int>& it1, std::vector<int>& kit,
                              std::vector<int>& longk) {
    kit.assign((size_t)m + 1, 0);
    for (int64_t k = 0; k < m; ++k) {
        kit[k] = (int)it0.size();
        for (int t = cjc[k]; t < cjc[k + 1]; t += SDDMM_CHUNK) { it0.push_back(t); it1.push_back(std::min(t + SDDMM_CHUNK, cjc[k + 1])); }
        if ((int)it0.size() - kit[k] > FIN_SHORT) longk.push_back((int)k);
    }
    kit[m] = (int)it0.size();
}
static inline SddmmPlan plan_sddmm(int64_t m, const int* cjc) {
    SddmmPlan s;
    plan_items(m, cjc, s.it0, s.it1, s.kit, s.longk);
    s.nitems = (int64_t)s.it0.size();
    for (int64_t k = 0; k < m; ++k) {
        if (s.kit[k + 1] - s.kit[k] > FIN_SHORT) {
            s.lkit.push_back((int)s.lit0.size());
            for (int q = s.kit[k]; q < s.kit[k + 1]; ++q) { s.lit0.push_back(s.it0[q]); s.lit1.push_back(s.it1[q]); }
        } else s.sk.push_back((int)k);
    }
    s.lkit.push_back((int)s.lit0.size());
    s.nlong = (int)s.longk.size(); s.nshort = (int)s.sk.size(); s.nlit = (int)s.lit0.size();
    s.us0.assign((size_t)s.nshort + s.nlit + 1, 0); s.us1 = s.us0; s.uk = s.us0;
    for (int u = 0; u < s.nshort; ++u) { s.us0[u] = cjc[s.sk[u]]; s.us1[u] = cjc[s.sk[u] + 1]; s.uk[u] = s.sk[u]; }
    for (int q = 0; q < s.nlit; ++q) { s.us0[s.nshort + q] = s.lit0[q]; s.us1[s.nshort + q] = s.lit1[q]; s.uk[s.nshort + q] = -1 - q; }
    if (s.longk.empty()) s.longk.push_back(0);
    if (s.sk.empty()) s.sk.push_back(0);
    if (s.lit0.empty()) { s.lit0.push_back(0); s.lit1.push_back(0); }
    if (s.it0.empty()) { s.it0.push_back(0); s.it1.push_back(0); }
    return s;
}

// ---- At by constraint (CSC) and by matrix entry (CSR, r = i*n + j); ir is the column-major vec index i + j*n
struct EntryPlan {
    int64_t bad = -1;                         // first nonzero whose row index is outside [0, n*n), or -1
    std::vector<int> cjc, ci, cj, cidx;       // cidx = i*nS + j: the nonzero's position in the dense Gram matrix
    std::vector<double> cv;
    std::vector<int> rp, rk;                  // n*n + 1 row pointers; constraint and coefficient, by constraint inside an entry
    std::vector<double> rv;
};
static inline EntryPlan plan_entries(int n, int nS, int64_t m, const int64_t* jc, const int64_t* ir, const double* pr) {
    EntryPlan e;
    const int64_t nnz = jc[m], nn = (int64_t)n * n;
    for (int64_t t = 0; t < nnz; ++t) if (ir[t] < 0 || ir[t] >= nn) { e.bad = t; return e; }
    e.cjc.resize((size_t)m + 1); e.ci.resize((size_t)nnz); e.cj.resize((size_t)nnz); e.cidx.resize((size_t)nnz);
    e.cv.assign(pr, pr + nnz);
    for (int64_t k = 0; k <= m; ++k) e.cjc[k] = (int)jc[k];
    e.rp.assign((size_t)nn + 1, 0);
    for (int64_t t = 0; t < nnz; ++t) {
        const int i = (int)(ir[t] % n), j = (int)(ir[t] / n);      // column-major vec index (bqpmom.m:57, example_theta.m:20)
        e.ci[t] = i; e.cj[t] = j;
        e.cidx[t] = i * nS + j;
        e.rp[(int64_t)i * n + j + 1]++;
    }
    for (int64_t r = 0; r < nn; ++r) e.rp[r + 1] += e.rp[r];
    e.rk.resize((size_t)nnz); e.rv.resize((size_t)nnz);
    std::vector<int> fill(e.rp.begin(), e.rp.end() - 1);
    for (int64_t k = 0; k < m; ++k)
        for (int64_t t = jc[k]; t < jc[k + 1]; ++t) {
            const int pos = fill[(int64_t)e.ci[t] * n + e.cj[t]]++;
            e.rk[pos] = (int)k; e.rv[pos] = pr[t];
        }
    return e;
}

// ---- c and every A_k symmetric, entry by entry (c: n x n; SeDuMi data is)
static inline bool plan_symmetric(int n, const double* c, const EntryPlan& e) {
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            if (c[(size_t)i * n + j] != c[(size_t)j * n + i]) return false;
            const int64_t r = (int64_t)i * n + j, rt = (int64_t)j * n + i;
            const int len = e.rp[r + 1] - e.rp[r];
            if (len != e.rp[rt + 1] - e.rp[rt]) return false;
            for (int t = 0; t < len; ++t)
                if (e.rk[e.rp[r] + t] != e.rk[e.rp[rt] + t] || e.rv[e.rp[r] + t] != e.rv[e.rp[rt] + t]) return false;
        }
    return true;
}

// ---- upper view of symmetric data: the constraints over their entries i <= j, the coefficient halved on the diagonal
// (Wsym_ii = 2 W_ii), with SDDMM items of their own
struct UpperPlan {
    std::vector<int> ucjc, ucidx, uit0, uit1, ukit, ulongk;
    std::vector<double> ucv;
    int64_t unitems = 0;
    int unlong = 0;
};
static inline UpperPlan plan_upper(int nS, int64_t m, const EntryPlan& e) {
    UpperPlan u;
    u.ucjc.assign((size_t)m + 1, 0);
    u.ucidx.reserve(e.ci.size() / 2 + 1); u.ucv.reserve(e.ci.size() / 2 + 1);
    for (int64_t k = 0; k < m; ++k) {
        u.ucjc[k] = (int)u.ucidx.size();
        for (int t = e.cjc[k]; t < e.cjc[k + 1]; ++t) {
            if (e.ci[t] > e.cj[t]) continue;
            u.ucidx.push_back(e.ci[t] * nS + e.cj[t]);
            u.ucv.push_back(e.ci[t] == e.cj[t] ? 0.5 * e.cv[t] : e.cv[t]);
        }
    }
    u.ucjc[m] = (int)u.ucidx.size();
    plan_items(m, u.ucjc.data(), u.uit0, u.uit1, u.ukit, u.ulongk);
    u.unitems = (int64_t)u.uit0.size();
    u.unlong = (int)u.ulongk.size();
    if (u.ulongk.empty()) u.ulongk.push_back(0);
    if (u.ucidx.empty()) { u.ucidx.push_back(0); u.ucv.push_back(0.0); }
    if (u.uit0.empty()) { u.uit0.push_back(0); u.uit1.push_back(0); }
    return u;
}

// ---- Order of the upper tiles = order of the workgroups of k_adjoint_tiled / k_adjoint_gram.  Workgroups b, b + 8, ... share an
// XCD (round-robin dispatch, msdp_device.h), and what a tile gathers -- the Gram entries of the constraints its entries occur
// in -- is local to its tile ROW (BQP d = 60: 1.7 MB of the 13.6-MB Gram matrix per tile row, median): the tile rows are cut into
// 8 contiguous bands of equal tile count, band x feeds the positions x, x + 8, ...  With the plain row-major order every XCD
// gathered from the whole matrix: 114 MB fetched by k_adjoint_gram for 22 MB of B and 14 MB of W; banded 87 MB and 23.6 -> 20.4 us.
// (Streaming (nt) loads of B on top: 79-85 MB but 23.5 us -- they sit in the gather's dependency chain; not kept.)
static inline std::vector<std::pair<short, short>> plan_tile_order(int ntile) {
    std::vector<std::pair<short, short>> order;
    const int64_t tot = (int64_t)ntile * (ntile + 1) / 2;
    std::vector<std::vector<std::pair<short, short>>> band(8);
    int64_t seen = 0;
    for (int bi = 0; bi < ntile; ++bi) {
        const int cnt = ntile - bi;
        const int x = (int)std::min<int64_t>(7, (2 * seen + cnt) * 8 / (2 * tot));
        for (int bj = bi; bj < ntile; ++bj) band[x].push_back({(short)bi, (short)bj});
        seen += cnt;
    }
    std::vector<size_t> head(8, 0), tail(8);
    for (int x = 0; x < 8; ++x) tail[x] = band[x].size();
    order.reserve((size_t)tot);
    for (int64_t pos = 0; pos < tot; ++pos) {
        const int x = (int)(pos & 7);
        if (head[x] < tail[x]) { order.push_back(band[x][head[x]++]); continue; }
        int lx = 0;                                       // band x is used up: the last tile of the longest remaining band
        for (int q = 1; q < 8; ++q) if (tail[q] - head[q] > tail[lx] - head[lx]) lx = q;
        order.push_back(band[lx][--tail[lx]]);
    }
    return order;
}

// ---- tiled upper-triangle copy of the CSR-by-entry arrays (k_adjoint_tiled): the entries of tile pair tp are
// trp[tp*1024 + e], e = li*32 + lj; entries in more than ADJ_LONG constraints are listed once more (i <= j; a diagonal tile
// holds both (i,j) and (j,i): the upper one is kept, its mirror is stored too)
struct TiledPlan {
    std::vector<short> tpi, tpj;
    std::vector<int> trp, trk;
    std::vector<double> trv;
    std::vector<int> lpos, lmir, ls0, ls1;
    int ntp = 0, nlong_e = 0;
};
static inline TiledPlan plan_tiled(int n, int nS, const std::vector<std::pair<short, short>>& order, const EntryPlan& e) {
    TiledPlan t;
    t.trp.reserve(order.size() * ADJ_T * ADJ_T + 1);
    t.trk.reserve(e.rk.size() / 2 + n + 16); t.trv.reserve(e.rk.size() / 2 + n + 16);
    for (const auto& tb : order) {
        const int bi = tb.first, bj = tb.second;
        t.tpi.push_back((short)bi); t.tpj.push_back((short)bj);
        for (int li = 0; li < ADJ_T; ++li)
            for (int lj = 0; lj < ADJ_T; ++lj) {
                t.trp.push_back((int)t.trk.size());
                const int i = bi * ADJ_T + li, j = bj * ADJ_T + lj;
                if (i >= n || j >= n) continue;
                const int64_t r = (int64_t)i * n + j;
                for (int q = e.rp[r]; q < e.rp[r + 1]; ++q) { t.trk.push_back(e.rk[q]); t.trv.push_back(e.rv[q]); }
            }
    }
    t.trp.push_back((int)t.trk.size());
    t.trk.push_back(0); t.trv.push_back(0.0);                    // padding element (see the kernel)
    t.ntp = (int)t.tpi.size();
    for (size_t tp = 0; tp < t.tpi.size(); ++tp)
        for (int el = 0; el < ADJ_T * ADJ_T; ++el) {
            const size_t g = tp * (ADJ_T * ADJ_T) + el;
            if (t.trp[g + 1] - t.trp[g] <= ADJ_LONG) continue;
            const int i = t.tpi[tp] * ADJ_T + el / ADJ_T, j = t.tpj[tp] * ADJ_T + el % ADJ_T;
            if (i > j) continue;
            t.lpos.push_back(i * nS + j); t.lmir.push_back(j * nS + i);
            t.ls0.push_back(t.trp[g]); t.ls1.push_back(t.trp[g + 1]);
        }
    t.nlong_e = (int)t.lpos.size();
    if (t.lpos.empty()) { t.lpos.push_back(0); t.lmir.push_back(0); t.ls0.push_back(0); t.ls1.push_back(0); }
    return t;
}

// ---- B route (k_adjoint_gram): B[e][e'] = sum_k a_k[e] * c_k[e'] over the upper entries, in ELL slices of the tiled order,
// built when every constraint is short (at most 8 upper entries: a long one -- a trace row -- would fill B with its square) and
// At is dense in its rows (8 nnz >= n^2, the Gram route's case).  Rows longer than the ELL width go to a wave each.
struct BRoutePlan {
    int bW = 0;                               // ELL width, 0: not built (nothing below is filled)
    std::vector<int> bidx;                    // [ntp][bW][1024] position in Wsym; padding = position 0 with coefficient 0
    std::vector<double> bval;
    std::vector<unsigned char> blong;         // [ntp][1024]
    std::vector<int> blpos, blmir, bls0, bls1, blk;
    std::vector<double> blv;
    int bnlong = 0;
    bool packed = false;                      // bpk = position | code << 24 and the 256 coefficients bdict replace (bidx, bval),
    std::vector<unsigned> bpk;                //   which shrink to one placeholder element
    std::vector<double> bdict;
};
static inline BRoutePlan plan_broute(int n, int nS, int64_t m, const EntryPlan& e, const UpperPlan& u, const TiledPlan& t) {
    BRoutePlan b;
    const int64_t nnz = (int64_t)e.rk.size(), nn = (int64_t)n * n;
    int maxcol = 0;
    for (int64_t k = 0; k < m; ++k) maxcol = std::max(maxcol, u.ucjc[k + 1] - u.ucjc[k]);
    if (!(maxcol > 0 && maxcol <= 8 && nnz * 8 >= nn)) return b;
    const size_t TE = (size_t)ADJ_T * ADJ_T, ntp = t.tpi.size();
    std::vector<std::vector<std::pair<int, double>>> rows(ntp * TE);
    std::vector<int> hist(16, 0);
    size_t nonempty = 0;
    std::vector<std::pair<int, double>> acc;
    for (size_t tp = 0; tp < ntp; ++tp)
        for (size_t el = 0; el < TE; ++el) {
            const int i = t.tpi[tp] * ADJ_T + (int)(el / ADJ_T), j = t.tpj[tp] * ADJ_T + (int)(el % ADJ_T);
            if (i >= n || j >= n) continue;
            const int64_t r = (int64_t)std::min(i, j) * n + std::max(i, j);
            acc.clear();
            for (int q = e.rp[r]; q < e.rp[r + 1]; ++q) {
                const int k = e.rk[q];
                for (int s = u.ucjc[k]; s < u.ucjc[k + 1]; ++s) acc.push_back({u.ucidx[s], e.rv[q] * u.ucv[s]});
            }
            std::sort(acc.begin(), acc.end(), [](const std::pair<int, double>& x, const std::pair<int, double>& y) { return x.first < y.first; });
            auto& row = rows[tp * TE + el];
            for (size_t q = 0; q < acc.size(); ++q) {
                if (!row.empty() && row.back().first == acc[q].first) row.back().second += acc[q].second;
                else row.push_back(acc[q]);
            }
            if (!row.empty()) { ++nonempty; hist[std::min<size_t>(15, row.size())]++; }
        }
    int BW = 4;                                                   // the narrowest width that holds 99 % of the rows whole
    { size_t cum = 0; for (int w = 1; w <= 4; ++w) { cum += hist[w]; if (cum * 1000 >= nonempty * 990) { BW = w; break; } } }
    b.bidx.assign(ntp * TE * BW, 0);
    b.bval.assign(ntp * TE * BW, 0.0);
    b.blong.assign(ntp * TE, 0);
    for (size_t tp = 0; tp < ntp; ++tp)
        for (size_t el = 0; el < TE; ++el) {
            const auto& row = rows[tp * TE + el];
            if ((int)row.size() <= BW) {
                for (size_t q = 0; q < row.size(); ++q) {
                    b.bidx[(tp * BW + q) * TE + el] = row[q].first;
                    b.bval[(tp * BW + q) * TE + el] = row[q].second;
                }
                continue;
            }
            b.blong[tp * TE + el] = 1;
            const int i = t.tpi[tp] * ADJ_T + (int)(el / ADJ_T), j = t.tpj[tp] * ADJ_T + (int)(el % ADJ_T);
            if (i > j) continue;                         // diagonal tile: the upper copy stores both
            b.blpos.push_back(i * nS + j); b.blmir.push_back(j * nS + i);
            b.bls0.push_back((int)b.blk.size());
            for (const auto& pr : row) { b.blk.push_back(pr.first); b.blv.push_back(pr.second); }
            b.bls1.push_back((int)b.blk.size());
        }
    b.bnlong = (int)b.blpos.size();
    if (b.blpos.empty()) { b.blpos.push_back(0); b.blmir.push_back(0); b.bls0.push_back(0); b.bls1.push_back(0); }
    if (b.blk.empty()) { b.blk.push_back(0); b.blv.push_back(0.0); }
    // packed form: position (24 bits) | coefficient code (8 bits) when the data allows it
    bool ok = (int64_t)n * nS < (1 << 24);
    if (ok) {
        b.bpk.resize(b.bidx.size());
        for (size_t q = 0; q < b.bidx.size() && ok; ++q) {
            size_t c = 0;
            for (; c < b.bdict.size(); ++c) if (memcmp(&b.bdict[c], &b.bval[q], sizeof(double)) == 0) break;
            if (c == b.bdict.size()) { if (b.bdict.size() >= 256) { ok = false; break; } b.bdict.push_back(b.bval[q]); }
            b.bpk[q] = (unsigned)b.bidx[q] | ((unsigned)c << 24);
        }
    }
    if (ok) {
        b.bdict.resize(256, 0.0);
        b.bidx.assign(1, 0); b.bval.assign(1, 0.0);          // the packed arrays replace them on the device
    } else { b.bpk.clear(); b.bdict.clear(); }
    b.packed = ok;
    b.bW = BW;
    return b;
}

// ---- entries touched by At, when they are few (<= 1/8 of the matrix): the restricted adjoint and the sparse products.
// `kit` is the SDDMM plan's: a constraint with more than FIN_SHORT items is encoded as -1 - (its number among the long ones)
struct SupportPlan {
    int nsup = 0;                             // 0: not built (nothing below is filled)
    std::vector<int> sup, suprow;             // touched entries r = i*n + j in order; n + 1 row pointers into sup
    std::vector<int> sqj, sqk, sqmore;        // per touched entry: column, first constraint (encoded), number of further pairs
    std::vector<double> sqv;                  //   and first coefficient
    std::vector<int> rkx;                     // rk, encoded
};
static inline SupportPlan plan_support(int n, int64_t m, const EntryPlan& e, const std::vector<int>& kit) {
    SupportPlan s;
    const int64_t nn = (int64_t)n * n;
    int64_t ns = 0;
    for (int64_t r = 0; r < nn; ++r) ns += e.rp[r + 1] > e.rp[r];
    if (!(ns > 0 && ns * 8 <= nn)) return s;
    s.sup.reserve((size_t)ns);
    for (int64_t r = 0; r < nn; ++r) if (e.rp[r + 1] > e.rp[r]) s.sup.push_back((int)r);
    s.suprow.assign((size_t)n + 1, 0);
    for (int r : s.sup) s.suprow[r / n + 1]++;
    for (int i = 0; i < n; ++i) s.suprow[i + 1] += s.suprow[i];
    std::vector<int> longno((size_t)m, -1);
    { int ql = 0; for (int64_t k = 0; k < m; ++k) if (kit[k + 1] - kit[k] > FIN_SHORT) longno[k] = ql++; }
    auto enc = [&](int k) { return longno[k] >= 0 ? -1 - longno[k] : k; };
    s.sqj.resize(s.sup.size()); s.sqk.resize(s.sup.size()); s.sqmore.resize(s.sup.size()); s.sqv.resize(s.sup.size());
    for (size_t q = 0; q < s.sup.size(); ++q) {
        const int64_t r = s.sup[q];
        s.sqj[q] = (int)(r % n); s.sqk[q] = enc(e.rk[e.rp[r]]); s.sqv[q] = e.rv[e.rp[r]]; s.sqmore[q] = e.rp[r + 1] - e.rp[r] - 1;
    }
    s.rkx.resize(e.rk.size());
    for (size_t q = 0; q < e.rk.size(); ++q) s.rkx[q] = enc(e.rk[q]);
    if (s.rkx.empty()) s.rkx.push_back(0);
    s.nsup = (int)ns;
    return s;
}

// ---- every plan of msdp_affine_setup (n x n matrices, nS = padded row length of the dense operands; c: n x n)
struct AffinePlans {
    EntryPlan ent;
    SddmmPlan sd;
    bool sym = false;                         // symmetric data: upv is built (AffineDev::usym)
    UpperPlan upv;
    TiledPlan til;                            // til.ntp == 0: data not symmetric (flat adjoint kernel)
    BRoutePlan br;
    SupportPlan sp;
};
static inline AffinePlans plan_affine(int n, int nS, int64_t m, const int64_t* jc, const int64_t* ir, const double* pr, const double* c) {
    AffinePlans p;
    p.ent = plan_entries(n, nS, m, jc, ir, pr);
    if (p.ent.bad >= 0) return p;
    p.sd = plan_sddmm(m, p.ent.cjc.data());
    p.sym = plan_symmetric(n, c, p.ent);
    if (p.sym) p.upv = plan_upper(nS, m, p.ent);
    const int ntile = (nS + ADJ_T - 1) / ADJ_T;
    if (p.sym && ntile < 32768) {             // (tile coordinates are shorts)
        p.til = plan_tiled(n, nS, plan_tile_order(ntile), p.ent);
        p.br = plan_broute(n, nS, m, p.ent, p.upv, p.til);
    }
    p.sp = plan_support(n, m, p.ent, p.sd.kit);
    return p;
}

// ---- multiblock kind, per-block storage: block i (order bn[i]) is a bn[i] x bns[i] row-major array at off[i]; ir runs over the
// CONCATENATED column-major vecs of the blocks (e0[i] + a + b*bn[i])
struct BlockedPlan {
    int status = 0;                           // 1: sum n_i * nS_i does not fit an int; 2: a row index outside [0, sum n_i^2)
    int64_t etot = 0;                         // stored entries
    std::vector<int64_t> r0, e0, off;         // nb + 1: first row, first vec index, first stored position of every block
    std::vector<int> bn, bns;
    std::vector<int64_t> rbase;               // N: stored position of the first entry of row r
    std::vector<int> rlo, rhi, rns;           // N: the rows of r's block, its padded order
    std::vector<int> tile_row0;               // first row of every 16-row tile (tiles never straddle blocks)
    std::vector<int> cjc, ci, cj, pos;        // nonzeros: rows (i, j) of the direct sum, stored position off_i + a*nS_i + b
    std::vector<double> cv;
    std::vector<int> prp, prk;                // CSR by stored position -> (constraint, coefficient)
    std::vector<double> prv;
    std::vector<int> longq;                   // positions in more than ADJB_LONG constraints
    int nlongq = 0;
};
static inline BlockedPlan plan_blocked(int nb, const int64_t* block_n, const int* block_ns, int64_t m, const int64_t* jc,
                                       const int64_t* ir, const double* pr) {
    BlockedPlan p;
    const int64_t nnz = jc[m];
    p.r0.assign((size_t)nb + 1, 0); p.e0 = p.r0; p.off = p.r0;
    p.bn.resize(nb); p.bns.resize(nb);
    for (int i = 0; i < nb; ++i) {
        p.bn[i] = (int)block_n[i]; p.bns[i] = block_ns[i];
        p.r0[i + 1] = p.r0[i] + p.bn[i]; p.e0[i + 1] = p.e0[i] + (int64_t)p.bn[i] * p.bn[i]; p.off[i + 1] = p.off[i] + (int64_t)p.bn[i] * p.bns[i];
    }
    p.etot = p.off[nb];
    if (p.etot > 0x7fffffffLL) { p.status = 1; return p; }
    for (int64_t t = 0; t < nnz; ++t) if (ir[t] < 0 || ir[t] >= p.e0[nb]) { p.status = 2; return p; }
    const int64_t N = p.r0[nb];
    p.rbase.resize((size_t)N); p.rlo.resize((size_t)N); p.rhi.resize((size_t)N); p.rns.resize((size_t)N);
    for (int i = 0; i < nb; ++i) {
        for (int aa = 0; aa < p.bn[i]; ++aa) {
            const int64_t r = p.r0[i] + aa;
            p.rbase[r] = p.off[i] + (int64_t)aa * p.bns[i]; p.rlo[r] = (int)p.r0[i]; p.rhi[r] = (int)p.r0[i + 1]; p.rns[r] = p.bns[i];
        }
        for (int t = 0; t < p.bn[i]; t += 16) p.tile_row0.push_back((int)p.r0[i] + t);
    }
    p.cjc.resize((size_t)m + 1); p.ci.resize((size_t)nnz); p.cj.resize((size_t)nnz); p.pos.resize((size_t)nnz);
    p.cv.assign(pr, pr + nnz);
    for (int64_t k = 0; k <= m; ++k) p.cjc[k] = (int)jc[k];
    p.prp.assign((size_t)p.etot + 1, 0);
    for (int64_t t = 0; t < nnz; ++t) {
        const int64_t e = ir[t];
        const int i = (int)(std::upper_bound(p.e0.begin(), p.e0.end(), e) - p.e0.begin()) - 1;
        const int64_t l = e - p.e0[i];
        const int aa = (int)(l % p.bn[i]), bb = (int)(l / p.bn[i]);
        p.ci[t] = (int)p.r0[i] + aa; p.cj[t] = (int)p.r0[i] + bb;
        p.pos[t] = (int)(p.off[i] + (int64_t)aa * p.bns[i] + bb);
        p.prp[p.pos[t] + 1]++;
    }
    for (int64_t q = 0; q < p.etot; ++q) p.prp[q + 1] += p.prp[q];
    p.prk.assign((size_t)std::max<int64_t>(nnz, 1), 0);
    p.prv.assign((size_t)std::max<int64_t>(nnz, 1), 0.0);
    {
        std::vector<int> fill(p.prp.begin(), p.prp.end() - 1);
        for (int64_t k = 0; k < m; ++k)
            for (int64_t t = jc[k]; t < jc[k + 1]; ++t) { const int q = fill[p.pos[t]]++; p.prk[q] = (int)k; p.prv[q] = pr[t]; }
    }
    for (int64_t q = 0; q < p.etot; ++q) if (p.prp[q + 1] - p.prp[q] > ADJB_LONG) p.longq.push_back((int)q);
    p.nlongq = (int)p.longq.size();
    if (p.longq.empty()) p.longq.push_back(0);
    if (p.ci.empty()) { p.ci.push_back(0); p.cj.push_back(0); p.cv.push_back(0.0); }
    if (p.pos.empty()) p.pos.push_back(0);
    return p;
}
