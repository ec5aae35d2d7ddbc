"""The planning rule of the wide plan of the fused own-column launch (fused_grid in msdp_persist.hip; option `pipe_wide`), as host
arithmetic through `msdp_debug_fused_wide_rule` -- no device, no handle: the smallest multiple of 8, at least 8 and at most
min(256, CUs / 8 * 8), whose chunks hold at most 80 rows (two row slots of 32 and the first half of the third), else 0."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def test_rule_against_brute_force(lib):
    for cus in (1, 7, 8, 15, 16, 100, 104, 216, 255, 256, 304):
        gmax = 256 if cus >= 256 else (cus // 8) * 8
        for n in (1, 79, 80, 81, 600, 640, 641, 736, 1221, 1280, 1281, 10000, 17280, 17281, 20000, 20480, 20481, 40000):
            brute = next((g for g in range(8, gmax + 1, 8) if -(-n // g) <= 80), 0)
            assert lib.fused_wide_rule(n, cus) == (brute, cus), (n, cus)


def test_rule_on_the_named_sizes(lib):
    assert [lib.fused_wide_rule(n, 256)[0] for n in (600, 736, 1221, 10000, 20000, 20481)] == [8, 16, 16, 128, 256, 0]
