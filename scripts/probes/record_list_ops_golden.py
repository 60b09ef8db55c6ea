"""Records tests/golden/list_ops_bits.npz: the result bits of MMR's similarity rows, dedupe, search_ids' slot scores and
the grouped search on the hashed inputs of tests/test_list_ops_bits_gpu.py, dims 1024 and 768, uint32 views only.
Both row layouts (with the fp16 mirror, and CRAG_NO_FP16_MIRROR=1) are run and must give the same bits: one recording
serves both.  Run it on the GPU with the library of the commit whose results are to be pinned -- the golden in the
repository was recorded from commit ea3d586, the one BEFORE the list operators shared crag_gram.h and crag_rows.h:

   CRAG_DENSE_LIB=<that build>/libcrag_dense.so python scripts/probes/record_list_ops_golden.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from cadence_rag_amd import _native
from tests.test_list_ops_bits_gpu import DIMS, GOLDEN, golden_view, inputs, open_index, run_ops

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(GOLDEN))
args = ap.parse_args()
record = {}
for dim in DIMS:
    inp = inputs(dim)
    views = []
    for mirror in (True, False):
        ix = open_index(inp, mirror)
        try:
            out = run_ops(ix, inp)
        finally:
            ix.close()
        assert np.array_equal(out["gram"], out["gram"].T), "the Gram matrix is not symmetric in its bits"
        views.append(golden_view(out))
    for name, a in views[0].items():
        assert a.dtype == np.uint32 and np.array_equal(a, views[1][name]), f"{name}: the two row layouts differ"
        record[f"{name}_{dim}"] = a
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
np.savez(args.out, **record)
size = os.path.getsize(args.out)
assert size < 64 * 1024, size
print(f"library {_native.LIB_PATH}: {len(record)} arrays, {size} bytes -> {args.out}")
