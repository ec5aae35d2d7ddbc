// msdp_roundcolor.hip -- the colouring behind the colour-ordered local search of msdp_round_hyperplane and msdp_round_phases
// (option "round_order" = 1; msdp_round_coloring).  Host code only: the sweep kernels that visit a colour class per launch live
// beside the serial ones in msdp_round.hip and msdp_phaseround.hip.
//
// A Gauss-Seidel sweep needs an order only between rows that a stored off-diagonal entry joins.  Rows of one colour are joined by
// none, so a launch may update all of them at once, and the colours taken one after another give exactly the serial sweep that
// visits the rows in (colour, index) order.  That rests on a structurally symmetric pattern -- row i must be a neighbour of
// every row it reads -- which is checked here, not assumed.
#include "msdp_common.h"
#include <algorithm>
#include <vector>

static const char* rc_kind_name(msdp_handle h) {
    if (h->d.costkind == COST_BLOCK) return msdp_block_kind_name(h->d.efree);
    switch (h->kind) {
        case MSDP_KIND_ONLYUNITDIAG: break;
        case MSDP_KIND_UNITDIAG: return "unitdiag";
        case MSDP_KIND_UNITTRACE: return "unittrace";
        case MSDP_KIND_GENERIC: return "generic";
        case MSDP_KIND_MULTIBLOCK: return "multiblock";
        case MSDP_KIND_DUAL_UNITDIAG: return "dual unitdiag";
        case MSDP_KIND_DUAL: return "dual";
        case MSDP_KIND_DUAL_MULTIBLOCK: return "dual multiblock";
        default: return "unknown";
    }
    if (h->d.costkind == COST_DENSE) return "dense onlyunitdiag";
    if (h->d.costkind == COST_SPLR) return "sparse-plus-low-rank onlyunitdiag";
    return "onlyunitdiag";
}

// Colour order applies to a single-rank onlyunitdiag handle whose cost matrix is held as sparse rows and nothing else.
int msdp_round_color_check(msdp_handle h, const char* who) {
    const int ck = h->d.costkind;
    if (h->kind != MSDP_KIND_ONLYUNITDIAG || ck == COST_BLOCK) {
        msdp_set_error("%s: colour order is the sparse and the Hermitian onlyunitdiag kinds', this is a handle of the %s kind", who, rc_kind_name(h));
        return MSDP_EUNSUPPORTED;
    }
    if (ck == COST_DENSE || ck == COST_SPLR) {
        msdp_set_error("%s: no colour order for a handle of the %s kind (every row is coupled to every other)", who, rc_kind_name(h));
        return MSDP_EUNSUPPORTED;
    }
    if (ck != COST_SPARSE && ck != COST_HERM) { msdp_set_error("%s: no cost matrix", who); return MSDP_EUNSUPPORTED; }
    if (h->nranks > 1 || h->use_comm || h->lgroup) {
        msdp_set_error("%s: no colour order on a handle of the %s kind that has joined a communicator", who, rc_kind_name(h));
        return MSDP_EUNSUPPORTED;
    }
    return 0;
}

// Greedy first-fit in index order: colour(i) = the smallest colour no neighbour j < i holds (the neighbours are the stored
// entries of row i, the diagonal left out; an empty row gets 0).  Then the rows sorted by (colour, index) and the class offsets.
int msdp_round_color_plan(msdp_handle h, const char* who) {
    if (h->rc_ncolors >= 0) return 0;
    int rc = msdp_round_color_check(h, who);
    if (rc) return rc;
    const int n = h->d.n;
    if (n < 1) { msdp_set_error("%s: empty problem", who); return MSDP_EINVAL; }
    // the pattern: the host copy the handle keeps, else one copy down from the device
    std::vector<int> rp_dev, ci_dev;
    const int* rp = h->h_rowptr.data();
    const int* ci = h->h_colind.data();
    if (h->h_rowptr.size() != (size_t)n + 1) {
        if (!h->d.rowptr || !h->d.colind) { msdp_set_error("%s: the handle holds no sparse rows", who); return MSDP_EUNSUPPORTED; }
        rp_dev.resize((size_t)n + 1);
        HIPCHK(msdp_memcpy(rp_dev.data(), h->d.rowptr, rp_dev.size() * sizeof(int), hipMemcpyDeviceToHost));
        ci_dev.resize((size_t)rp_dev[(size_t)n]);
        if (!ci_dev.empty()) HIPCHK(msdp_memcpy(ci_dev.data(), h->d.colind, ci_dev.size() * sizeof(int), hipMemcpyDeviceToHost));
        rp = rp_dev.data(); ci = ci_dev.data();
    }
    // every stored (i, j) needs a stored (j, i): looked up in the sorted copy of row j
    std::vector<int> sorted(ci, ci + rp[n]);
    for (int i = 0; i < n; ++i) std::sort(sorted.begin() + rp[i], sorted.begin() + rp[i + 1]);
    for (int i = 0; i < n; ++i)
        for (int e = rp[i]; e < rp[i + 1]; ++e) {
            const int j = ci[e];
            if (j < 0 || j >= n) { msdp_set_error("%s: column index %d of row %d out of range", who, j, i); return MSDP_EINVAL; }
            if (j != i && !std::binary_search(sorted.begin() + rp[j], sorted.begin() + rp[j + 1], i)) {
                msdp_set_error("%s: the pattern of C is not symmetric: entry (%d, %d) is stored, entry (%d, %d) is not (colour order needs both)", who, i, j, j, i);
                return MSDP_EINVAL;
            }
        }
    std::vector<int> color((size_t)n, 0), mark((size_t)n + 1, -1);
    int nc = 0;
    for (int i = 0; i < n; ++i) {
        for (int e = rp[i]; e < rp[i + 1]; ++e)
            if (ci[e] < i) mark[(size_t)color[(size_t)ci[e]]] = i;
        int c = 0;
        while (mark[(size_t)c] == i) ++c;                      // (at most deg(i) colours are marked: c <= deg(i) < n)
        color[(size_t)i] = c;
        nc = std::max(nc, c + 1);
    }
    std::vector<int> offs((size_t)nc + 1, 0), order((size_t)n);
    for (int i = 0; i < n; ++i) offs[(size_t)color[(size_t)i] + 1] += 1;
    for (int c = 0; c < nc; ++c) offs[(size_t)c + 1] += offs[(size_t)c];
    std::vector<int> next(offs.begin(), offs.end() - 1);
    for (int i = 0; i < n; ++i) order[(size_t)next[(size_t)color[(size_t)i]]++] = i;
    int* od = nullptr; int* fd = nullptr;
    if ((rc = msdp_dev_alloc<int>(h, &od, order.size())) || (rc = msdp_dev_alloc<int>(h, &fd, offs.size()))) {
        msdp_dev_free(h, od);
        return rc;
    }
    hipError_t e = msdp_memcpy(od, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = msdp_memcpy(fd, offs.data(), offs.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        msdp_set_error("%s: upload of the colouring failed: %s", who, hipGetErrorString(e));
        msdp_dev_free(h, od); msdp_dev_free(h, fd);
        return MSDP_EHIP;
    }
    h->rc_color.swap(color); h->rc_offs.swap(offs);
    h->rc_order_d = od; h->rc_offs_d = fd;
    h->rc_ncolors = nc;
    return 0;
}

extern "C" int msdp_round_coloring(msdp_handle h, int32_t* ncolors, int32_t* color) {
    MSDP_CHECK_H(h);
    if (!ncolors) { msdp_set_error("round_coloring: ncolors is null"); return MSDP_EINVAL; }
    int rc = msdp_round_color_plan(h, "round_coloring");
    if (rc) return rc;
    *ncolors = h->rc_ncolors;
    if (color) std::copy(h->rc_color.begin(), h->rc_color.end(), color);
    return 0;
}
