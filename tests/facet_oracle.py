"""The facet rule restated with dense loops, independent of cadence_rag_amd.filters.facets_host: numpy arrays indexed by
(namespace, value), one pass per row, Python `sorted` for the order.

count(a) = the number of row positions i with mask bit i set whose attribute list holds a at least once; per requested
namespace the attributes with count > 0 by count descending, then value ascending (str order), cut at `top`; `distinct`
is their number before the cut; `rows` the number of set bits."""
import numpy as np


def unpack(packed, n):
    """Bits of a packed mask run (bit i % 8 of byte i // 8) as a bool array [n]; junk beyond n is dropped."""
    return np.unpackbits(np.asarray(packed, dtype=np.uint8), bitorder="little")[:n].astype(bool)


def facets(row_attrs, bits, namespaces, top):
    """row_attrs: per row (namespace, value) pairs in normal form; bits: bool [n] or None (every row); namespaces: the
    requested names in normal form.  Returns (rows, {namespace: ([(value, count)], distinct)})."""
    n = len(row_attrs)
    bits = np.ones(n, dtype=bool) if bits is None else np.asarray(bits, dtype=bool)[:n]
    universe = sorted({a for attrs in row_attrs for a in attrs})
    column = {a: j for j, a in enumerate(universe)}
    holds = np.zeros((n, len(universe)), dtype=bool)
    for i, attrs in enumerate(row_attrs):
        for a in attrs:
            holds[i, column[a]] = True          # a duplicate inside the row sets the same cell again
    count = holds[bits].sum(axis=0) if n else np.zeros(len(universe), dtype=np.int64)
    out = {}
    for ns in namespaces:
        live = [(value, int(count[column[(space, value)]])) for space, value in universe
                if space == ns and count[column[(space, value)]] > 0]
        out[ns] = (sorted(live, key=lambda vc: (-vc[1], vc[0]))[:top], len(live))
    return int(bits.sum()), out
