"""Records tests/golden/selection_qnorm_k24.npz: ids and score bits of the 64-query, k = 24 case of
tests/test_selection_short_list_gpu.py (query norms spread over 1e-3 ... 1e3), with a digest of the generated inputs.
Run it on the GPU with the library of the commit whose results are to be pinned -- the golden in the repository was
recorded from the commit BEFORE the query-norm butterfly moved to the VALU:

   CRAG_DENSE_LIB=<that build>/libcrag_dense.so python scripts/probes/record_qnorm_golden.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from cadence_rag_amd import _native
from cadence_rag_amd.dense_index import DenseIndex
from tests.test_selection_short_list_gpu import GOLDEN, GOLDEN_K, base_case, inputs_digest

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(GOLDEN))
args = ap.parse_args()
corpus, queries = base_case()
with DenseIndex(corpus.shape[1], capacity=len(corpus)) as ix:
    ix.add(corpus)
    ids, scores, counts = ix.search(queries, GOLDEN_K)
    kernel = ix.last_scan_kernel()
assert "prefilter" in kernel, kernel
assert np.all(counts == GOLDEN_K)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
np.savez(args.out, ids=ids, score_bits=scores.view(np.uint32), inputs_sha256=inputs_digest(corpus, queries))
print(f"library {_native.LIB_PATH}: {kernel}, {ids.shape} -> {args.out}")
