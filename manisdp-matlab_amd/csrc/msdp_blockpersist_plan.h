// msdp_blockpersist_plan.h -- host arithmetic of the persistent tCG kernel of the block kinds (msdp_blockpersist.hip): how many
// lanes serve a block, how many workgroups run, how many blocks a lane group holds and what that takes in LDS.  Nothing of HIP
// in here: tools/block_persist_plan_selftest.cpp includes this header alone and compares every plan with brute force.
//
// A workgroup has MSDP_BP_THREADS = 512 threads = 8 waves.  A lane group of LPR lanes owns one block per row slot; a wave holds
// 64 / LPR groups, a workgroup RSTEP = 8 * 64 / LPR blocks per slot and R * RSTEP blocks in all.  Workgroup b of G owns the
// block chunk msdp_bp_chunk gives it (the arithmetic of msdp_chunk_rows); (wave w, group g, slot r) of it owns block
// lo + r * RSTEP + w * (64 / LPR) + g where that is below hi.
// LDS per workgroup: the D = B - efree rotation rows of Y and the B rows of the gradient, one double2 per thread, row and slot
// ((D + B) * R * 512 * 16 bytes), and the D x D multiplier block of every owned block (R * RSTEP * D * D * 8 bytes).
#pragma once
#include <stddef.h>

#define MSDP_BP_THREADS 512
#define MSDP_BP_WAVES (MSDP_BP_THREADS / 64)
#define MSDP_BP_MAXLPR 16                 // widths up to 2 * 16 = 32
#define MSDP_BP_MAXR 2                    // row slots per lane group
#define MSDP_BP_MAXGRID 256               // the grid reductions poll 4 x 64 slots
#define MSDP_BP_LDS_MAX (160 * 1024)      // per CU
#define MSDP_BP_LDS_STATIC 256            // the kernel's static arrays (wave sums, reduction results)

struct BlockPersistPlan {
    int ok;        // 0: no plan (the handle stays on the chunked path)
    int lpr;       // lanes per block: the smallest power of two with 2 * lpr >= p
    int G;         // workgroups: a multiple of 8, >= 8, <= min(256, CUs)
    int R;         // row slots per lane group
    int rstep;     // blocks per slot of a workgroup
    size_t lds;    // dynamic LDS bytes of a workgroup
};

static inline int msdp_bp_lpr(int p) {
    int l = 1;
    while (2 * l < p) l *= 2;
    return l;
}
static inline int msdp_bp_rstep(int lpr) { return MSDP_BP_WAVES * (64 / lpr); }
static inline size_t msdp_bp_lds(int B, int efree, int lpr, int R) {
    const size_t D = (size_t)(B - efree);
    return (size_t)R * ((D + (size_t)B) * MSDP_BP_THREADS * 16 + (size_t)msdp_bp_rstep(lpr) * D * D * 8);
}

// the block chunk [lo, hi) of workgroup b of G (G a multiple of 8): msdp_chunk_rows of msdp_device.h, restated for the host
static inline void msdp_bp_chunk(int nb, int G, int b, int* lo, int* hi) {
    const int c = (b & 7) * (G >> 3) + (b >> 3);
    const unsigned q = (unsigned)nb / (unsigned)G, r = (unsigned)nb - q * (unsigned)G;
    *lo = (int)((unsigned)c * q + ((unsigned)c < r ? (unsigned)c : r));
    *hi = *lo + (int)q + ((unsigned)c < r ? 1 : 0);
}

// nb blocks of order B (efree of its rows free), factor width p, a device of `cus` compute units; grid_cap > 0 caps the grid
// (tests, tuning).  The grid is the fewest workgroups that need the same number of row slots: fewer slots to poll in every
// grid reduction, and a workgroup with a half-empty slot takes as long as a full one.  wide != 0 (A/B switch): the LARGEST grid
// allowed at that number of row slots instead -- the blocks spread over more compute units, each gathers fewer rows.
static inline BlockPersistPlan msdp_blockpersist_plan(int nb, int B, int efree, int p, int cus, int grid_cap, int wide = 0) {
    BlockPersistPlan pl = {0, 0, 0, 0, 0, 0};
    if (nb < 1 || B < 2 || B > 4 || efree < 0 || efree > 1 || B - efree < 2 || B - efree > 3 || p < 1 || p > 2 * MSDP_BP_MAXLPR) return pl;
    int gmax = cus < MSDP_BP_MAXGRID ? cus : MSDP_BP_MAXGRID;
    if (grid_cap > 0 && grid_cap < gmax) gmax = grid_cap < 8 ? 8 : grid_cap;
    gmax = (gmax / 8) * 8;
    if (gmax < 8 || gmax > cus) return pl;
    const int lpr = msdp_bp_lpr(p), rstep = msdp_bp_rstep(lpr);
    for (int R = 1; R <= MSDP_BP_MAXR; ++R) {
        const size_t lds = msdp_bp_lds(B, efree, lpr, R);
        if (lds + MSDP_BP_LDS_STATIC > MSDP_BP_LDS_MAX) break;
        const long long cap = (long long)R * rstep;              // blocks of a workgroup
        if (cap * gmax < nb) continue;
        int G = (int)((((nb + cap - 1) / cap + 7) / 8) * 8);
        if (G < 8) G = 8;
        if (wide) G = gmax;
        pl.ok = 1; pl.lpr = lpr; pl.G = G; pl.R = R; pl.rstep = rstep; pl.lds = lds;
        return pl;
    }
    return pl;
}
