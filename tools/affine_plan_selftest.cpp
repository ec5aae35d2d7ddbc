// Host-side check of the affine set-ups' index arithmetic (manisdp-matlab_amd/csrc/msdp_affine_plan.h): every plan is compared
// with brute force written here.  Stand-alone, no device and no HIP; tests/test_affine_plan_host.py builds and runs it plain.
// For a sanitizer run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imanisdp-matlab_amd/csrc
//       tools/affine_plan_selftest.cpp -o $OUT/affine_plan_selftest && $OUT/affine_plan_selftest
#include <cstdio>
#include <map>
#include <set>
#include "msdp_affine_plan.h"

static int failures = 0;
static void check(const char* group, const char* what, bool ok) {
    std::printf("%-18s %-72s %s\n", group, what, ok ? "ok" : "FAILED");
    if (!ok) ++failures;
}

// constraints as triplet lists -> CSC over the column-major vec index i + j*n
struct Trip { int i, j; double v; };
struct Csc { std::vector<int64_t> jc, ir; std::vector<double> pr; };
static Csc to_csc(int n, const std::vector<std::vector<Trip>>& A) {
    Csc s;
    s.jc.push_back(0);
    for (const auto& col : A) {
        for (const Trip& t : col) { s.ir.push_back(t.i + (int64_t)t.j * n); s.pr.push_back(t.v); }
        s.jc.push_back((int64_t)s.ir.size());
    }
    return s;
}
static std::vector<Trip> symmetric(const std::vector<Trip>& upper) {       // (i, j, v) with i <= j -> both triangles
    std::vector<Trip> out;
    for (const Trip& t : upper) { out.push_back(t); if (t.i != t.j) out.push_back({t.j, t.i, t.v}); }
    return out;
}

// ------------------------------------------------------------------ SDDMM items and units
static void sddmm_case(const char* name, const std::vector<int>& counts) {
    const int64_t m = (int64_t)counts.size();
    std::vector<int> cjc(m + 1, 0);
    for (int64_t k = 0; k < m; ++k) cjc[k + 1] = cjc[k] + counts[k];
    const SddmmPlan s = plan_sddmm(m, cjc.data());
    bool tiles = (int64_t)s.kit.size() == m + 1 && s.kit[0] == 0 && s.kit[m] == s.nitems;
    std::vector<int> longs, shorts;
    for (int64_t k = 0; k < m && tiles; ++k) {
        int cur = cjc[k];
        for (int q = s.kit[k]; q < s.kit[k + 1]; ++q) {
            tiles = tiles && s.it0[q] == cur && s.it1[q] > cur && s.it1[q] - cur <= 16 && s.it1[q] <= cjc[k + 1];
            cur = s.it1[q];
        }
        tiles = tiles && cur == cjc[k + 1];
        ((counts[k] + 15) / 16 > 8 ? longs : shorts).push_back((int)k);      // long: more than FIN_SHORT = 8 items
    }
    check(name, "items tile every constraint's range once, in order, <= 16 each", tiles);
    bool split = s.nlong == (int)longs.size() && s.nshort == (int)shorts.size();
    for (size_t q = 0; q < longs.size() && split; ++q) split = s.longk[q] == longs[q];
    for (size_t q = 0; q < shorts.size() && split; ++q) split = s.sk[q] == shorts[q];
    check(name, "sk and longk split the constraints", split);
    bool units = split && s.us0.size() == (size_t)s.nshort + s.nlit + 1 && s.us1.size() == s.us0.size() && s.uk.size() == s.us0.size() &&
                 (int)s.lkit.size() == s.nlong + 1;
    for (int u = 0; u < s.nshort && units; ++u) units = s.uk[u] == shorts[u] && s.us0[u] == cjc[shorts[u]] && s.us1[u] == cjc[shorts[u] + 1];
    int nlit = 0;
    for (size_t q = 0; q < longs.size() && units; ++q) {                       // the long items, constraint after constraint
        int cur = cjc[longs[q]];
        units = s.lkit[q] == nlit;
        for (; cur < cjc[longs[q] + 1] && units; ++nlit) {
            const int u = s.nshort + nlit, end = std::min(cur + 16, cjc[longs[q] + 1]);
            units = nlit < s.nlit && s.uk[u] == -1 - nlit && s.us0[u] == cur && s.us1[u] == end && s.lit0[nlit] == cur && s.lit1[nlit] == end;
            cur = end;
        }
    }
    units = units && nlit == s.nlit && s.lkit[longs.size()] == nlit;
    check(name, "units: short constraints whole (uk = k), then long items (uk = -1 - q)", units);
    check(name, "no array is empty",
          !s.it0.empty() && !s.it1.empty() && !s.kit.empty() && !s.longk.empty() && !s.sk.empty() && !s.lit0.empty() && !s.lit1.empty() &&
              !s.lkit.empty() && !s.us0.empty() && !s.us1.empty() && !s.uk.empty());
}

// ------------------------------------------------------------------ order of the upper tiles
static void tile_order_case(int ntile) {
    char name[32];
    std::snprintf(name, sizeof name, "tiles ntile=%d", ntile);
    const auto order = plan_tile_order(ntile);
    const int64_t tot = (int64_t)ntile * (ntile + 1) / 2;
    std::set<std::pair<int, int>> seen;
    bool perm = (int64_t)order.size() == tot;
    for (const auto& t : order) perm = perm && t.first >= 0 && t.first <= t.second && t.second < ntile && seen.insert({t.first, t.second}).second;
    check(name, "a permutation of the upper tiles", perm);
    // band of tile row bi: where the middle of its tiles falls in the row-major sequence, in eighths
    std::vector<int> band(ntile), left(8, 0);
    int64_t before = 0;
    for (int bi = 0; bi < ntile; ++bi) {
        const int cnt = ntile - bi;
        band[bi] = (int)std::min<int64_t>(7, (2 * before + cnt) * 8 / (2 * tot));
        left[band[bi]] += cnt;
        before += cnt;
    }
    bool ok = perm;
    for (int64_t pos = 0; pos < tot && ok; ++pos) {
        const int x = (int)(pos % 8), got = band[order[pos].first];
        if (left[x] > 0) ok = got == x;
        --left[got];
    }
    check(name, "position pos holds a tile of band pos mod 8 while that band has tiles left", ok);
}

// ------------------------------------------------------------------ tiled adjoint and B route
typedef std::map<int, double> Row;                                   // position i'*nS + j' -> coefficient
// B[e][e'] = sum_k a_k[e] * c_k[e'] from the triplets: a_k the coefficients of A_k, c_k those of its upper view (diagonal halved)
static std::map<int, Row> brute_B(int nS, const std::vector<std::vector<Trip>>& A) {
    std::map<int, Row> B;
    for (const auto& col : A)
        for (const Trip& s : col) {
            if (s.i > s.j) continue;
            for (const Trip& t : col) {
                if (t.i > t.j) continue;
                B[s.i * nS + s.j][t.i * nS + t.j] += s.v * (t.i == t.j ? 0.5 * t.v : t.v);
            }
        }
    return B;
}
static bool same_row(const Row& got, const Row* want) {
    Row g, w;
    for (const auto& pr : got) if (pr.second != 0.0) g.insert(pr);
    if (want) for (const auto& pr : *want) if (pr.second != 0.0) w.insert(pr);
    return g == w;
}
// every in-range element of every tile, expanded from the ELL slices (packed or not) or its long list, against brute force
static bool broute_matches(int n, int nS, const AffinePlans& p, const std::map<int, Row>& B) {
    const BRoutePlan& b = p.br;
    const size_t TE = 1024;
    bool ok = b.bW >= 1 && b.bW <= 4 && b.blong.size() == p.til.tpi.size() * TE;
    ok = ok && (b.packed ? b.bpk.size() == p.til.tpi.size() * TE * b.bW && b.bdict.size() == 256 && b.bidx.size() == 1 && b.bval.size() == 1
                         : b.bidx.size() == p.til.tpi.size() * TE * b.bW && b.bval.size() == b.bidx.size() && b.bpk.empty() && b.bdict.empty());
    for (size_t tp = 0; tp < p.til.tpi.size() && ok; ++tp)
        for (size_t el = 0; el < TE && ok; ++el) {
            const int i = p.til.tpi[tp] * 32 + (int)(el / 32), j = p.til.tpj[tp] * 32 + (int)(el % 32);
            Row got;
            if (b.blong[tp * TE + el]) {
                if (i >= n || j >= n) { ok = false; break; }
                int q = 0;
                while (q < b.bnlong && b.blpos[q] != std::min(i, j) * nS + std::max(i, j)) ++q;
                ok = q < b.bnlong && b.blmir[q] == std::max(i, j) * nS + std::min(i, j) && b.bls1[q] - b.bls0[q] > b.bW;
                for (int t = ok ? b.bls0[q] : 0; ok && t < b.bls1[q]; ++t) got[b.blk[t]] += b.blv[t];
            } else {
                for (int w = 0; w < b.bW; ++w) {
                    const size_t q = (tp * b.bW + w) * TE + el;
                    const int idx = b.packed ? (int)(b.bpk[q] & 0xffffffu) : b.bidx[q];
                    const double val = b.packed ? b.bdict[b.bpk[q] >> 24] : b.bval[q];
                    got[idx] += val;
                }
            }
            const auto it = (i < n && j < n) ? B.find(std::min(i, j) * nS + std::max(i, j)) : B.end();
            ok = ok && same_row(got, it == B.end() ? nullptr : &it->second);
        }
    return ok;
}
// the tiled CSR-by-entry arrays against the (constraint, coefficient) lists of every entry, and the list of long entries
static bool tiled_matches(int n, int nS, const AffinePlans& p, const std::vector<std::vector<Trip>>& A) {
    const TiledPlan& t = p.til;
    std::map<std::pair<int, int>, std::vector<std::pair<int, double>>> ent;
    for (size_t k = 0; k < A.size(); ++k) for (const Trip& s : A[k]) ent[{s.i, s.j}].push_back({(int)k, s.v});
    bool ok = t.trp.size() == (size_t)t.ntp * 1024 + 1 && t.trk.size() == (size_t)t.trp.back() + 1 && t.trv.size() == t.trk.size();
    int nlong = 0;
    for (int tp = 0; tp < t.ntp && ok; ++tp)
        for (int el = 0; el < 1024 && ok; ++el) {
            const int i = t.tpi[tp] * 32 + el / 32, j = t.tpj[tp] * 32 + el % 32;
            const auto it = ent.find({i, j});
            const size_t g = (size_t)tp * 1024 + el, len = (size_t)(t.trp[g + 1] - t.trp[g]);
            ok = len == (it == ent.end() ? 0 : it->second.size()) && (len == 0 || (i < n && j < n));
            for (size_t q = 0; q < len && ok; ++q) ok = t.trk[t.trp[g] + q] == it->second[q].first && t.trv[t.trp[g] + q] == it->second[q].second;
            if (ok && len > 8 && i <= j) {
                ok = nlong < t.nlong_e && t.lpos[nlong] == i * nS + j && t.lmir[nlong] == j * nS + i && t.ls0[nlong] == t.trp[g] && t.ls1[nlong] == t.trp[g + 1];
                ++nlong;
            }
        }
    return ok && nlong == t.nlong_e && !t.lpos.empty();
}
static void dense_cases() {
    const int n = 5, nS = 16;
    // symmetric, <= 8 upper entries per constraint, 8 nnz >= n^2; constraint 2 has six upper entries (rows of B longer than four),
    // entry (0,1) occurs in two constraints, entry (4,4) in nine (a long entry of the tiled adjoint); dyadic values: sums are exact
    std::vector<std::vector<Trip>> A;
    A.push_back(symmetric({{0, 0, 1.0}, {1, 1, 2.0}}));
    A.push_back(symmetric({{0, 1, 3.0}, {2, 2, 1.5}}));
    A.push_back(symmetric({{0, 2, 0.5}, {1, 2, -1.0}, {1, 3, 0.25}, {3, 3, 4.0}, {0, 4, -0.75}, {2, 4, 2.5}}));
    A.push_back(symmetric({{0, 1, 0.5}, {3, 4, -2.0}}));
    A.push_back({});
    for (int q = 0; q < 9; ++q) A.push_back(symmetric({{4, 4, 1.0 + 0.125 * q}}));
    std::vector<double> c((size_t)n * n);
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) c[(size_t)i * n + j] = 1.0 + std::min(i, j) + 0.5 * std::max(i, j);
    {
        const Csc s = to_csc(n, A);
        const AffinePlans p = plan_affine(n, nS, (int64_t)A.size(), s.jc.data(), s.ir.data(), s.pr.data(), c.data());
        check("dense n=5", "symmetric data: upper view, one tile pair", p.ent.bad < 0 && p.sym && p.til.ntp == 1);
        bool up = p.sym && p.upv.ucjc.size() == A.size() + 1;
        for (size_t k = 0; k < A.size() && up; ++k) {
            int q = p.upv.ucjc[k];
            for (const Trip& t : A[k]) {
                if (t.i > t.j) continue;
                up = up && q < p.upv.ucjc[k + 1] && p.upv.ucidx[q] == t.i * nS + t.j && p.upv.ucv[q] == (t.i == t.j ? 0.5 * t.v : t.v);
                ++q;
            }
            up = up && q == p.upv.ucjc[k + 1];
        }
        check("dense n=5", "upper view: entries i <= j in order, diagonal halved", up);
        check("dense n=5", "tiled adjoint arrays = entry lists; entry (4,4) (nine constraints) is long", tiled_matches(n, nS, p, A) && p.til.nlong_e == 1);
        check("dense n=5", "B route built, some row in the long list", p.br.bW > 0 && p.br.bnlong > 0);
        check("dense n=5", "<= 256 coefficients: packed, bpk / bdict unpack to B exactly", p.br.packed && broute_matches(n, nS, p, brute_B(nS, A)));
    }
    {
        std::vector<std::vector<Trip>> As = A;
        As[2][1].v = 0.625;                                        // the (2,0) copy of the (0,2) coefficient
        const Csc s = to_csc(n, As);
        const AffinePlans p = plan_affine(n, nS, (int64_t)As.size(), s.jc.data(), s.ir.data(), s.pr.data(), c.data());
        check("dense n=5", "asymmetric in one coefficient: no upper view (usym = 0), ntp = 0, no B route",
              p.ent.bad < 0 && !p.sym && p.til.ntp == 0 && p.br.bW == 0 && p.upv.ucidx.empty());
    }
    {
        // 257 distinct coefficients need 256 nonzeros of B inside the ELL slices (plus the padding's zero): at n = 5 B has 15 rows of at
        // most four slices each, so this case takes n = 16: the 136 upper entries in 34 constraints of four, every coefficient different
        const int n2 = 16;
        std::vector<std::vector<Trip>> A2;
        std::vector<Trip> cur;
        int e = 0;
        for (int i = 0; i < n2; ++i)
            for (int j = i; j < n2; ++j) {
                cur.push_back({i, j, 1.0 + (1 + e) / 1024.0}); ++e;
                if (cur.size() == 4) { A2.push_back(symmetric(cur)); cur.clear(); }
            }
        std::vector<double> c2((size_t)n2 * n2, 0.0);
        const auto B = brute_B(nS, A2);
        std::set<double> vals;
        for (const auto& r : B) for (const auto& pr : r.second) vals.insert(pr.second);
        const Csc s = to_csc(n2, A2);
        const AffinePlans p = plan_affine(n2, nS, (int64_t)A2.size(), s.jc.data(), s.ir.data(), s.pr.data(), c2.data());
        check("dense n=16", "the instance has >= 256 distinct nonzero coefficients in rows of four", cur.empty() && vals.size() >= 256 && p.br.bW == 4 && p.br.bnlong == 0);
        check("dense n=16", "257 coefficients: packed form refused, (bidx, bval) kept and equal to B", !p.br.packed && broute_matches(n2, nS, p, B));
    }
}

// ------------------------------------------------------------------ support list
static void support_cases() {
    const int n = 8, nS = 16;
    // constraint 1 is long: 129 nonzeros (nine items) cycling over four entries
    std::vector<std::vector<Trip>> A(3);
    A[0] = {{0, 0, 1.0}, {1, 2, 2.0}};
    const int cyc[4][2] = {{1, 2}, {3, 3}, {5, 1}, {7, 7}};
    for (int t = 0; t < 129; ++t) A[1].push_back({cyc[t % 4][0], cyc[t % 4][1], 1.0 + t});
    A[2] = {{2, 1, -3.0}, {7, 7, 0.5}};
    std::vector<double> c((size_t)n * n, 0.0);
    for (int variant = 0; variant < 2; ++variant) {
        if (variant == 1) { A[2].push_back({4, 0, 1.0}); A[2].push_back({4, 5, 1.0}); A[2].push_back({6, 6, 1.0}); }
        const Csc s = to_csc(n, A);
        const AffinePlans p = plan_affine(n, nS, 3, s.jc.data(), s.ir.data(), s.pr.data(), c.data());
        if (variant == 1) {
            check("support n=8", "9 touched entries (9 * 8 > 64): not built", p.sp.nsup == 0 && p.sp.sup.empty() && p.sp.rkx.empty());
            continue;
        }
        std::map<int, std::vector<std::pair<int, double>>> ent;          // r = i*n + j -> (constraint, coefficient) in constraint order
        for (int k = 0; k < 3; ++k) for (const Trip& t : A[k]) ent[t.i * n + t.j].push_back({k, t.v});
        const SupportPlan& sp = p.sp;
        check("support n=8", "6 touched entries: built, sup sorted and complete", sp.nsup == 6 && ent.size() == 6 && sp.sup.size() == 6 &&
              std::is_sorted(sp.sup.begin(), sp.sup.end()) && std::equal(sp.sup.begin(), sp.sup.end(), ent.begin(), [](int r, const auto& pr) { return r == pr.first; }));
        bool rows = sp.suprow.size() == (size_t)n + 1 && sp.suprow[0] == 0 && sp.suprow[n] == 6;
        for (int i = 0; i < n && rows; ++i)
            for (int q = sp.suprow[i]; q < sp.suprow[i + 1] && rows; ++q) rows = sp.sup[q] / n == i;
        check("support n=8", "suprow are row pointers into sup", rows);
        auto enc = [](int k) { return k == 1 ? -1 : k; };                // the one long constraint is number 0 among the long ones
        bool rec = sp.nsup == 6, anylong = false;
        std::vector<int> rkx;
        size_t q = 0;
        for (const auto& pr : ent) {
            rec = rec && sp.sqj[q] == pr.first % n && sp.sqk[q] == enc(pr.second[0].first) && sp.sqv[q] == pr.second[0].second &&
                  sp.sqmore[q] == (int)pr.second.size() - 1 && p.ent.rp[pr.first] == (int)rkx.size();
            anylong = anylong || sp.sqk[q] == -1;
            for (const auto& kv : pr.second) rkx.push_back(enc(kv.first));
            ++q;
        }
        check("support n=8", "sqj / sqk / sqv / sqmore; the long constraint is -1 - 0 in sqk and rkx", rec && anylong && sp.rkx == rkx && p.sd.nlong == 1 && p.sd.longk[0] == 1);
    }
}

// ------------------------------------------------------------------ multiblock kind, per-block storage
static void blocked_cases() {
    const int nb = 3;
    const int64_t bn[3] = {1, 16, 17};
    const int bns[3] = {16, 16, 32};
    const int64_t e0[4] = {0, 1, 257, 546}, off[4] = {0, 16, 272, 816}, r0[4] = {0, 1, 17, 34};
    // 17 constraints: all hold the entry (2, 3) of block 1, the first 16 also (5, 16) of block 2, the first the one entry of block 0
    const int64_t m = 17;
    Csc s;
    s.jc.push_back(0);
    for (int k = 0; k < m; ++k) {
        if (k == 0) { s.ir.push_back(0); s.pr.push_back(7.0); }
        s.ir.push_back(e0[1] + 2 + 3 * 16); s.pr.push_back(1.0 + k);
        if (k < 16) { s.ir.push_back(e0[2] + 5 + 16 * 17); s.pr.push_back(-1.0 - k); }
        s.jc.push_back((int64_t)s.ir.size());
    }
    const BlockedPlan p = plan_blocked(nb, bn, bns, m, s.jc.data(), s.ir.data(), s.pr.data());
    check("blocked 1,16,17", "accepted; offsets of rows, vec indices and stored positions", p.status == 0 && p.etot == 816 &&
          std::equal(p.r0.begin(), p.r0.end(), r0) && std::equal(p.e0.begin(), p.e0.end(), e0) && std::equal(p.off.begin(), p.off.end(), off));
    const std::vector<int> tiles = {0, 1, 17, 33};
    bool tl = p.tile_row0 == tiles && p.rlo.size() == 34;
    for (size_t t = 0; t < p.tile_row0.size() && tl; ++t) {
        const int row = p.tile_row0[t], last = std::min(row + 16, p.rhi[row]) - 1;
        tl = p.rlo[last] == p.rlo[row] && p.rhi[last] == p.rhi[row] && (row == p.rlo[row] || (t > 0 && p.tile_row0[t - 1] == row - 16));
    }
    check("blocked 1,16,17", "tiles per block 1, 1, 2; none straddles a block", tl);
    bool rt = tl;
    for (int i = 0; i < nb && rt; ++i)
        for (int a = 0; a < bn[i] && rt; ++a) {
            const int64_t r = r0[i] + a;
            rt = p.rbase[r] == off[i] + (int64_t)a * bns[i] && p.rlo[r] == r0[i] && p.rhi[r] == r0[i + 1] && p.rns[r] == bns[i];
        }
    check("blocked 1,16,17", "row tables rbase / rlo / rhi / rns", rt);
    const int pos0 = 0, pos1 = (int)off[1] + 2 * 16 + 3, pos2 = (int)off[2] + 5 * 32 + 16;
    bool ps = p.pos.size() == s.ir.size();
    std::map<int, std::vector<std::pair<int, double>>> at;
    for (int k = 0; k < m && ps; ++k)
        for (int64_t t = s.jc[k]; t < s.jc[k + 1] && ps; ++t) {
            const int blk = s.ir[t] >= e0[2] ? 2 : s.ir[t] >= e0[1] ? 1 : 0;
            const int want = blk == 0 ? pos0 : blk == 1 ? pos1 : pos2, a = blk == 0 ? 0 : blk == 1 ? 2 : 5, b = blk == 0 ? 0 : blk == 1 ? 3 : 16;
            ps = p.pos[t] == want && p.ci[t] == r0[blk] + a && p.cj[t] == r0[blk] + b && p.cv[t] == s.pr[t];
            at[want].push_back({k, s.pr[t]});
        }
    check("blocked 1,16,17", "an ir in every block maps to off_i + a * nS_i + b", ps);
    bool csr = p.prp.size() == 817 && p.prp[816] == (int)s.ir.size();
    for (int q = 0; q < 816 && csr; ++q) {
        const auto it = at.find(q);
        const size_t len = (size_t)(p.prp[q + 1] - p.prp[q]);
        csr = len == (it == at.end() ? 0 : it->second.size());
        for (size_t t = 0; t < len && csr; ++t) csr = p.prk[p.prp[q] + t] == it->second[t].first && p.prv[p.prp[q] + t] == it->second[t].second;
    }
    check("blocked 1,16,17", "CSR by stored position", csr);
    check("blocked 1,16,17", "the position in 17 constraints is in longq, the one in 16 is not", p.nlongq == 1 && p.longq.size() == 1 && p.longq[0] == pos1);
    s.ir[1] = 546;
    const BlockedPlan bad = plan_blocked(nb, bn, bns, m, s.jc.data(), s.ir.data(), s.pr.data());
    check("blocked 1,16,17", "ir = sum n_i^2 is refused", bad.status == 2);
    s.ir[1] = -1;
    check("blocked 1,16,17", "ir = -1 is refused", plan_blocked(nb, bn, bns, m, s.jc.data(), s.ir.data(), s.pr.data()).status == 2);
}

int main() {
    sddmm_case("sddmm mixed", {0, 1, 16, 17, 128, 129});              // 129 nonzeros = nine items: the first long constraint
    sddmm_case("sddmm no long", {0, 1, 16, 17, 128});
    sddmm_case("sddmm only long", {129, 129, 145});
    sddmm_case("sddmm empty", {0, 0});
    for (int ntile : {1, 2, 7, 9, 40}) tile_order_case(ntile);
    dense_cases();
    support_cases();
    blocked_cases();
    {
        const int64_t jc[2] = {0, 1}, ir[1] = {25};
        const double pr[1] = {1.0};
        check("dense n=5", "ir = n^2 is refused", plan_entries(5, 16, 1, jc, ir, pr).bad == 0);
    }
    std::printf("%s\n", failures ? "FAILED" : "all checks passed");
    return failures ? 1 : 0;
}
