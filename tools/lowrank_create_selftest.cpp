// Host-side check of msdp_create_onlyunitdiag_csc_lowrank's argument validation: every path that returns before a device is
// needed, and the call with valid arguments (on a machine without a device it must end in MSDP_EHIP with nothing leaked).
// Meant for a sanitizer build of the library's host code, as a stand-alone program:
//   for f in manisdp-matlab_amd/csrc/*.hip; do hipcc -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 \
//       -Xarch_host -fsanitize=address,undefined -c $f -o $OUT/$(basename $f .hip).o; done
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude -c tools/lowrank_create_selftest.cpp -o $OUT/selftest_main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined $OUT/*.o -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib \
//       -o $OUT/lowrank_create_selftest && $OUT/lowrank_create_selftest
#include <cstdio>
#include <cstring>
#include <vector>
#include "manisdp_hip.h"

static int failures = 0;
static void expect(const char* what, int got, int want) {
    const bool ok = got == want;
    std::printf("%-44s rc %d (%s)%s\n", what, got, msdp_last_error(), ok ? "" : "   <-- UNEXPECTED");
    if (!ok) ++failures;
}

int main() {
    const int64_t n = 6;
    // a 6-cycle with quarter weights, CSC
    std::vector<int64_t> jc(n + 1), ir;
    std::vector<double> pr;
    for (int64_t j = 0; j < n; ++j) {
        jc[j] = (int64_t)ir.size();
        const int64_t a = (j + n - 1) % n, b = (j + 1) % n;
        ir.push_back(a < b ? a : b); pr.push_back(0.25);
        ir.push_back(a < b ? b : a); pr.push_back(-0.5);
    }
    jc[n] = (int64_t)ir.size();
    std::vector<double> V(n * MSDP_LOWRANK_MAX, 0.5), s(MSDP_LOWRANK_MAX, -0.25);
    msdp_handle h = nullptr;
    expect("q = 0", msdp_create_onlyunitdiag_csc_lowrank(n, jc.data(), ir.data(), pr.data(), 0, V.data(), s.data(), 8, &h), MSDP_EINVAL);
    expect("q = MSDP_LOWRANK_MAX + 1", msdp_create_onlyunitdiag_csc_lowrank(n, jc.data(), ir.data(), pr.data(), MSDP_LOWRANK_MAX + 1, V.data(), s.data(), 8, &h), MSDP_EINVAL);
    expect("q = -3", msdp_create_onlyunitdiag_csc_lowrank(n, jc.data(), ir.data(), pr.data(), -3, V.data(), s.data(), 8, &h), MSDP_EINVAL);
    expect("V = NULL", msdp_create_onlyunitdiag_csc_lowrank(n, jc.data(), ir.data(), pr.data(), 3, nullptr, s.data(), 8, &h), MSDP_EINVAL);
    expect("s = NULL", msdp_create_onlyunitdiag_csc_lowrank(n, jc.data(), ir.data(), pr.data(), 3, V.data(), nullptr, 8, &h), MSDP_EINVAL);
    expect("out = NULL", msdp_create_onlyunitdiag_csc_lowrank(n, jc.data(), ir.data(), pr.data(), 3, V.data(), s.data(), 8, nullptr), MSDP_EINVAL);
    expect("n = 0", msdp_create_onlyunitdiag_csc_lowrank(0, jc.data(), ir.data(), pr.data(), 3, V.data(), s.data(), 8, &h), MSDP_EINVAL);
    expect("jc = NULL", msdp_create_onlyunitdiag_csc_lowrank(n, nullptr, ir.data(), pr.data(), 3, V.data(), s.data(), 8, &h), MSDP_EINVAL);
    expect("ir = NULL", msdp_create_onlyunitdiag_csc_lowrank(n, jc.data(), nullptr, pr.data(), 3, V.data(), s.data(), 8, &h), MSDP_EINVAL);
    if (h) { std::printf("a refused call wrote the handle\n"); ++failures; }
    int32_t ndev = 0;
    msdp_device_count(&ndev);
    int rc = msdp_create_onlyunitdiag_csc_lowrank(n, jc.data(), ir.data(), pr.data(), 3, V.data(), s.data(), 8, &h);
    if (ndev == 0) expect("valid arguments, no device", rc, MSDP_EHIP);
    else {
        expect("valid arguments", rc, 0);
        if (!rc) msdp_destroy(h);
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
