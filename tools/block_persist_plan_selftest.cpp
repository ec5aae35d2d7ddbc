// Host-side check of the plan of the block kinds' persistent tCG (manisdp-matlab_amd/csrc/msdp_blockpersist_plan.h): every plan
// is compared with brute force written here.  Stand-alone, no device and no HIP; tests/test_block_persist_plan_host.py builds
// and runs it plain.  For a sanitizer run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imanisdp-matlab_amd/csrc
//       tools/block_persist_plan_selftest.cpp -o $OUT/block_persist_plan_selftest && $OUT/block_persist_plan_selftest
#include <cstdio>
#include <string>
#include <vector>
#include "msdp_blockpersist_plan.h"

static int failures = 0;
static void check(const char* group, const char* what, bool ok) {
    std::printf("%-28s %-76s %s\n", group, what, ok ? "ok" : "FAILED");
    if (!ok) ++failures;
}

// LDS of a workgroup, counted row by row and block by block
static size_t brute_lds(int B, int efree, int lpr, int R) {
    const int D = B - efree;
    size_t bytes = 0;
    for (int r = 0; r < R; ++r) {
        for (int t = 0; t < 512; ++t) bytes += (size_t)(D + B) * 16;              // a double2 of every row of Y and the gradient
        for (int w = 0; w < 8; ++w)
            for (int g = 0; g < 64 / lpr; ++g) bytes += (size_t)D * D * 8;        // the multiplier block of (wave, group, slot)
    }
    return bytes;
}

// does ANY number of row slots fit: capacity for nb blocks on the largest grid, within the LDS?
static int brute_slots(int nb, int B, int efree, int lpr, int gmax) {
    for (int R = 1; R <= MSDP_BP_MAXR; ++R) {
        if (brute_lds(B, efree, lpr, R) + MSDP_BP_LDS_STATIC > (size_t)160 * 1024) continue;
        long long cap = 0;
        for (int g = 0; g < gmax; ++g) cap += (long long)R * 8 * (64 / lpr);
        if (cap >= nb) return R;
    }
    return 0;
}

// --plans: the header's answer to the queries "nb B efree p cus cap wide" of the standard input, one line "ok lpr G R rstep lds"
// each (tests/test_block_persist_cases_host.py holds the Python restatement of the plan to them)
static int print_plans() {
    int nb, B, ef, p, cus, cap, wide;
    while (std::scanf("%d %d %d %d %d %d %d", &nb, &B, &ef, &p, &cus, &cap, &wide) == 7) {
        const BlockPersistPlan pl = msdp_blockpersist_plan(nb, B, ef, p, cus, cap, wide);
        std::printf("%d %d %d %d %d %zu\n", pl.ok, pl.lpr, pl.G, pl.R, pl.rstep, pl.lds);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "--plans") return print_plans();
    const int Bs[4] = {2, 3, 3, 4}, EFs[4] = {0, 0, 1, 1};
    const int CUs[3] = {64, 256, 304}, CAPs[3] = {0, 8, 16};
    std::vector<int> nbs;
    for (int nb = 1; nb <= 40; ++nb) nbs.push_back(nb);
    for (int nb = 41; nb <= 20000; nb += (nb < 1200 ? 7 : 211)) nbs.push_back(nb);
    const int edge[] = {64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 20000};
    for (int e : edge) nbs.push_back(e);
    for (int k = 0; k < 4; ++k)
        for (int cu : CUs)
            for (int cap : CAPs) {
                const int B = Bs[k], ef = EFs[k];
                char name[64];
                std::snprintf(name, sizeof name, "B=%d free=%d CUs=%d cap=%d", B, ef, cu, cap);
                bool own = true, grid = true, room = true, lds = true, elig = true, lanes = true, fewest = true, widest = true;
                long plans = 0;
                for (int p = 1; p <= 64; ++p)
                    for (int nb : nbs) {
                        const BlockPersistPlan pl = msdp_blockpersist_plan(nb, B, ef, p, cu, cap);
                        int gmax = cu < 256 ? cu : 256;
                        if (cap > 0 && cap < gmax) gmax = cap;
                        gmax = gmax / 8 * 8;
                        int lpr = 1;
                        while (2 * lpr < p) lpr *= 2;
                        const int want = (p <= 32 && gmax >= 8) ? brute_slots(nb, B, ef, lpr, gmax) : 0;
                        elig = elig && (pl.ok != 0) == (want != 0);                 // ineligible exactly where no R fits
                        if (!pl.ok) continue;
                        ++plans;
                        lanes = lanes && pl.lpr == lpr && 2 * pl.lpr >= p && (pl.lpr == 1 || 2 * (pl.lpr / 2) < p) && pl.rstep == 8 * (64 / lpr);
                        grid = grid && pl.G % 8 == 0 && pl.G >= 8 && pl.G <= (cu < 256 ? cu : 256) && pl.G <= gmax;
                        room = room && (long long)pl.G * pl.R * pl.rstep >= nb && pl.R == want;
                        lds = lds && pl.lds == brute_lds(B, ef, lpr, pl.R) && pl.lds + MSDP_BP_LDS_STATIC <= (size_t)160 * 1024;
                        // the fewest workgroups that need the same R: eight fewer would not hold the blocks
                        fewest = fewest && (pl.G == 8 || (long long)(pl.G - 8) * pl.R * pl.rstep < nb);
                        // the A/B form: the largest grid, everything else as planned
                        const BlockPersistPlan pw = msdp_blockpersist_plan(nb, B, ef, p, cu, cap, 1);
                        widest = widest && pw.ok && pw.G == gmax && pw.R == pl.R && pw.lpr == pl.lpr && pw.rstep == pl.rstep && pw.lds == pl.lds;
                        // every block is owned by exactly one (workgroup, wave, group, slot)
                        std::vector<unsigned char> seen((size_t)nb, 0);
                        const int bpw = 64 / pl.lpr;
                        int covered = 0;
                        for (int b = 0; b < pl.G && own; ++b) {
                            int lo, hi;
                            msdp_bp_chunk(nb, pl.G, b, &lo, &hi);
                            own = own && lo >= 0 && hi >= lo && hi <= nb && hi - lo <= pl.R * pl.rstep;
                            for (int r = 0; r < pl.R; ++r)
                                for (int w = 0; w < 8; ++w)
                                    for (int g = 0; g < bpw; ++g) {
                                        const int blk = lo + r * pl.rstep + w * bpw + g;
                                        if (blk < hi) { own = own && blk < nb && !seen[(size_t)blk]; if (blk < nb) seen[(size_t)blk] = 1; ++covered; }
                                    }
                        }
                        own = own && covered == nb;
                    }
                check(name, "a plan exists exactly where one or two row slots fit (p <= 32, LDS, capacity)", elig && plans > 0);
                check(name, "LPR = the smallest power of two with 2 LPR >= p", lanes);
                check(name, "G is a multiple of 8 in [8, min(256, CUs)] and within the cap", grid);
                check(name, "capacity G * R * RSTEP >= nb with the smallest R that fits", room);
                check(name, "G is the fewest workgroups that need that R", fewest);
                check(name, "wide: the largest grid at the same R, lanes and LDS", widest);
                check(name, "LDS bytes match the brute count and stay within 160 KB", lds);
                check(name, "every block is owned by exactly one (workgroup, wave, group, slot)", own);
            }
    std::printf("%s\n", failures ? "FAILED" : "all checks passed");
    return failures ? 1 : 0;
}
