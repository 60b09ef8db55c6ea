"""The four list operators' result BITS against a recording from the commit before they shared their Gram block, id
lookup and row view (crag_gram.h, crag_rows.h): tests/golden/list_ops_bits.npz, written by
scripts/probes/record_list_ops_golden.py with the library of commit ea3d586.  The suites of the operators compare dedupe
with MMR and both with fp64 oracles under a tolerance; with one shared body a slip would move both alike, so here
nothing but array_equal on uint32 views, in both row layouts (with the fp16 mirror and with CRAG_NO_FP16_MIRROR=1).

The inputs come from integer arithmetic alone -- a 64-bit mixer over (row, dim) gives a sign, a full 23-bit mantissa
and one of six exponents --, so every machine rebuilds the same floats and the order of the MFMA chain and of the
slice sums shows in the low bits.  96 rows (three tiles of 32: the block pairs (0,0) (0,1) (1,1) (0,2) (1,2) (2,2)),
ids 10 + 3 * position, a zero row and a NaN row, dims 1024 and 768."""
import os
from pathlib import Path

import numpy as np
import pytest
import torch

from cadence_rag_amd.dense_index import DenseIndex

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "list_ops_bits.npz"
DIMS = (1024, 768)
N_ROWS, ZERO_ROW, NAN_ROW = 96, 37, 70          # the two odd rows lie in different tiles
NQ, QUERY_ROW0 = 3, 1000                        # the queries are "rows" 1000.. of the same hash
N_GROUPS, PER_GROUP, GROUP_K = 8, 2, 16
DEDUPE_TAU = -0.99


def mix64(x: np.ndarray) -> np.ndarray:
    """the splitmix64 finaliser on a uint64 array (the products wrap)"""
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def hashed_rows(first: int, n: int, dim: int) -> np.ndarray:
    """float32 [n, dim]: sign, mantissa and exponent (2^-3 ... 2^2) of element (row, d) from mix64 of its number"""
    r = np.arange(first, first + n, dtype=np.uint64)[:, None]
    d = np.arange(dim, dtype=np.uint64)[None, :]
    h = mix64((r * np.uint64(4096) + d + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))
    sign = (h >> np.uint64(63)).astype(np.uint32) << np.uint32(31)
    mant = ((h >> np.uint64(40)) & np.uint64(0x7FFFFF)).astype(np.uint32)
    expo = (np.uint32(124) + ((h >> np.uint64(8)) % np.uint64(6)).astype(np.uint32)) << np.uint32(23)
    return np.ascontiguousarray((sign | expo | mant).view(np.float32))


def inputs(dim: int) -> dict:
    rows = hashed_rows(0, N_ROWS, dim)
    rows[ZERO_ROW] = 0.0
    rows[NAN_ROW] = np.nan
    ids = 10 + 3 * np.arange(N_ROWS, dtype=np.int64)
    return {"rows": rows, "ids": ids, "queries": hashed_rows(QUERY_ROW0, NQ, dim),
            # the 96 ids, two that are not stored (one between two stored ids, one above them all) and a -1
            "listed": np.concatenate([ids, np.asarray([11, 10 + 3 * N_ROWS + 5, -1], dtype=np.int64)]),
            "row_group": (np.arange(N_ROWS) % N_GROUPS).astype(np.int32)}


def open_index(inp: dict, mirror: bool) -> DenseIndex:
    """(the switch is read when the index is created; the environment is left as it was)"""
    old = os.environ.pop("CRAG_NO_FP16_MIRROR", None)
    try:
        if not mirror:
            os.environ["CRAG_NO_FP16_MIRROR"] = "1"
        ix = DenseIndex(inp["rows"].shape[1], capacity=N_ROWS + 8, device=0)
        ix.add(inp["rows"], inp["ids"])
        return ix
    finally:
        os.environ.pop("CRAG_NO_FP16_MIRROR", None)
        if old is not None:
            os.environ["CRAG_NO_FP16_MIRROR"] = old


def u32(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint32)


def run_ops(ix: DenseIndex, inp: dict) -> dict:
    """The four operators on `inp` -> uint32 views of what the golden holds.  MMR: one 96-wide list, lambda = 1, k = 96,
    relevances descending with the slot, so pick t is slot t and out_sim_rows is the whole Gram matrix; the golden keeps
    its upper triangle and the test asserts the symmetry."""
    dev = torch.device("cuda", 0)
    n = N_ROWS
    d_ids = torch.from_numpy(inp["ids"][None, :].copy()).to(dev)
    d_rel = torch.from_numpy((1.0 - np.arange(n, dtype=np.float32) / 128.0)[None, :].copy()).to(dev)
    d_ct = torch.tensor([n], dtype=torch.int32, device=dev)
    o_ids = torch.empty(1, n, dtype=torch.int64, device=dev)
    o_rel = torch.empty(1, n, dtype=torch.float32, device=dev)
    o_ct = torch.empty(1, dtype=torch.int32, device=dev)
    o_slots = torch.empty(1, n, dtype=torch.int32, device=dev)
    o_sim = torch.empty(1, n, n, dtype=torch.float32, device=dev)
    ix.mmr_async(d_ids, d_rel, d_ct, 1.0, n, o_ids, o_rel, o_ct, d_out_slots=o_slots, d_out_sim_rows=o_sim,
                 stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert int(o_ct[0]) == n and np.array_equal(o_slots.cpu().numpy()[0], np.arange(n)), "the picks are the slots in order"
    gram = u32(o_sim.cpu().numpy()[0])
    _, dup_of, sim = ix.dedupe(inp["ids"], DEDUPE_TAU)
    *_, slot_scores = ix.search_ids(inp["queries"], inp["listed"], 10, slot_scores=True)
    g_ids, g_scores, g_groups, g_counts = ix.search_grouped(inp["queries"], GROUP_K, inp["row_group"], N_GROUPS, PER_GROUP)
    return {"gram": gram, "dedupe_dup_of": u32(dup_of), "dedupe_sim": u32(sim), "subset_slot_scores": u32(slot_scores),
            "group_ids": u32(g_ids), "group_scores": u32(g_scores), "group_groups": u32(g_groups),
            "group_counts": u32(g_counts)}


def golden_view(out: dict) -> dict:
    """what the file stores of run_ops' output: the Gram matrix as its upper triangle, the rest as it is"""
    kept = {name: a for name, a in out.items() if name != "gram"}
    kept["gram_upper"] = out["gram"][np.triu_indices(N_ROWS)]
    return kept


@pytest.fixture(scope="module")
def golden(gpu):
    with np.load(GOLDEN) as z:
        return {name: z[name] for name in z.files}


@pytest.mark.parametrize("mirror", [True, False], ids=["mirror", "no_mirror"])
@pytest.mark.parametrize("dim", DIMS)
def test_bits_are_the_recorded_ones(golden, dim, mirror):
    inp = inputs(dim)
    ix = open_index(inp, mirror)
    try:
        out = run_ops(ix, inp)
    finally:
        ix.close()
    assert np.array_equal(out["gram"], out["gram"].T), "cos(i, j) and cos(j, i) are the same bits"
    nan = np.isnan(out["gram"].view(np.float32))
    odd = np.zeros(N_ROWS, dtype=bool)
    odd[[ZERO_ROW, NAN_ROW]] = True
    assert np.array_equal(nan, odd[:, None] | odd[None, :]), "NaN exactly where a row is not comparable"
    got = golden_view(out)
    assert {f"{name}_{dim}" for name in got} == {name for name in golden if name.endswith(f"_{dim}")}
    for name, a in got.items():
        want = golden[f"{name}_{dim}"]
        assert want.dtype == np.uint32 and a.shape == want.shape, name
        assert np.array_equal(a, want), (name, dim, mirror, int((a != want).sum()))
