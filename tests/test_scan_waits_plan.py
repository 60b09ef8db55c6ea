"""Which wait schedule the mirror scan takes (crag_search_plan.h: pf_waits_for), host side, no GPU.  The choice is a
pure function of (mirror bytes, has_mirror, nt, CRAG_PF_WAITS): per-fragment waits for a mirror with plain loads up
to PF_FRAG_WAITS_MAX_BYTES, whole-tile waits above it; never for an index without the mirror or with the streaming
cache policy, whose kernels exist under one schedule only -- the switch cannot force it there."""
import ctypes as C

import pytest

from cadence_rag_amd import _native

TILE, FRAGMENT = 0, 1
ROW = 1024 * 2   # bytes of one mirror row


@pytest.fixture(scope="module")
def lib():
    lib = _native.load()
    lib.crag_pf_waits_.restype = C.c_int
    lib.crag_pf_waits_.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int]
    lib.crag_pf_frag_waits_max_bytes_.restype = C.c_int64
    lib.crag_pf_frag_waits_max_bytes_.argtypes = []
    return lib


def test_the_limit_covers_the_benchmark_and_not_more_than_the_infinity_cache(lib):
    limit = lib.crag_pf_frag_waits_max_bytes_()
    assert 125_000 * ROW <= limit <= 256 << 20 < 150_000 * ROW   # (the measured win ends between those two sizes)


def test_by_size_on_both_sides_of_the_limit(lib):
    limit = lib.crag_pf_frag_waits_max_bytes_()
    for size, want in ((0, FRAGMENT), (32_768 * ROW, FRAGMENT), (100_000 * ROW, FRAGMENT), (limit - 1, FRAGMENT),
                       (limit, FRAGMENT), (limit + 1, TILE), (limit + ROW, TILE), (500_000 * ROW, TILE),
                       (1_000_000 * ROW, TILE), (1 << 40, TILE)):
        assert lib.crag_pf_waits_(size, 1, 0, -1) == want, size


@pytest.mark.parametrize("switch", [-1, TILE, FRAGMENT])
def test_no_mirror_or_streaming_loads_always_wait_by_tile(lib, switch):
    limit = lib.crag_pf_frag_waits_max_bytes_()
    for size in (0, 100_000 * ROW, limit, limit + 1, 1_000_000 * ROW):
        assert lib.crag_pf_waits_(size, 0, 0, switch) == TILE
        assert lib.crag_pf_waits_(size, 1, 1, switch) == TILE
        assert lib.crag_pf_waits_(size, 0, 1, switch) == TILE


def test_the_switch_forces_either_schedule_at_any_size(lib):
    limit = lib.crag_pf_frag_waits_max_bytes_()
    for size in (0, 100_000 * ROW, limit, limit + 1, 1_000_000 * ROW):
        assert lib.crag_pf_waits_(size, 1, 0, TILE) == TILE
        assert lib.crag_pf_waits_(size, 1, 0, FRAGMENT) == FRAGMENT


def test_the_search_plan_keeps_its_layout(lib):
    """the chooser has a C entry of its own: crag_search_plan_ and SearchPlan (16 ints) are what they were"""
    fn = lib.crag_search_plan_
    fn.restype = C.c_int
    fn.argtypes = [C.c_int64] + [C.c_int] * 11 + [C.c_int64, C.c_void_p]
    assert fn(100_000, 256, 64, 10, 1, 0, 0, 0, 0, 2, 4, -1, 1536 << 20, None) == 16 * 4
