"""The contract of range_query_tagged and exact_range_query_tagged in plain Python: for every distinct mask m the
queries with query_tags == m are answered by the filtered call of the reference's restatement -- filtered_range_model's
filtered_range_batch on the CPU oracle's graph, or exact_range_model's exact_range -- with the allow-set tag_mask(row_tags, m,
match), and the lists are put back in the caller's query order.  HeapEmpty propagates: the loop of filtered calls fails at the
first mask whose call throws."""
import numpy as np

from exact_range_model import exact_range
from filtered_range_model import HeapEmpty, filtered_range_batch, heap_empty_closed_form  # noqa: F401  (re-exported for the tests)
from tagged_query_model import check_tag_args, tag_mask  # noqa: F401


def _per_mask(n_rows, queries, row_tags, query_tags, match, answer):
    q = np.asarray(queries, dtype=np.float32)
    qt = check_tag_args(query_tags, match, q.shape[0])
    ids, dists = [None] * q.shape[0], [None] * q.shape[0]
    for m in np.unique(qt):
        which = np.flatnonzero(qt == m)
        a, d = answer(q[which], tag_mask(row_tags, int(m), match, n_rows))
        for w, ai, di in zip(which, a, d):
            ids[w], dists[w] = ai, di
    return ids, dists


def tagged_range(ix, rows, metric, queries, radius, row_tags, query_tags, match="any"):
    """(ids, dists): per query the filtered RangeQuery of its mask on the oracle index ix, in the caller's order."""
    return _per_mask(rows.shape[0], queries, row_tags, query_tags, match, lambda q, mask: filtered_range_batch(ix, rows, metric, q, radius, mask))


def exact_range_tagged(metric, x, queries, radius, row_tags, query_tags, match="any", live=None):
    """(ids, dists): per query the exact range scan over its mask's ids (those of `live`, when given), in the caller's order."""
    return _per_mask(np.shape(x)[0], queries, row_tags, query_tags, match, lambda q, mask: exact_range(metric, x, q, radius, mask, live))
