"""The collapsed k-NN contract in plain Python, and models of how the device keeps it.

The contract: walk a query's candidates in ascending (distance, id) order, keep an id while fewer than m kept ids have its label,
stop at k.  `walk` states it; `collapsed_rows` applies it to the complete ordered lists that exact_range_query(q, inf) / knn_query
return and pads the rows like the library.

The device never sees the whole order.  A scan block keeps, per (query, chunk of the id list), a COLLAPSED list of at most k keys and
inserts keys into it in whatever order they arrive (`CollapsedList.offer`, the model of exact_list_insert_collapsed: drop, evict the
largest entry of the label, or the ordinary insert); a merge then feeds the chunks' lists, in order, into one more such list
(`merge`, the model of exact_merge_collapsed_kernel, which leaves a list at its first key that is not below the current k-th).
`chunked` runs both over a set of keys cut into chunks.  tests/test_collapse_model.py holds them against `walk`.

A key is the integer (distance key << 32) | id, as on the device: comparing keys compares (distance, id)."""
import numpy as np

EMPTY = (1 << 64) - 1


def walk(order, label_of, k, m):
    """The contract: `order` is the candidates in ascending order; the first k of those that have fewer than m kept
    predecessors of their own label."""
    kept, per = [], {}
    for x in order:
        g = label_of(x)
        if per.get(g, 0) < m:
            per[g] = per.get(g, 0) + 1
            kept.append(x)
            if len(kept) == k:
                break
    return kept


def collapsed_rows(id_lists, d_lists, row_group, k, m):
    """(ids [n, k] int32, dists [n, k] float32): per query the walk over its complete ordered list (ids, distances), padded with
    -1 / NaN.  Entries of -1 in a list are padding and are skipped."""
    n = len(id_lists)
    ids = np.full((n, k), -1, np.int32)
    d = np.full((n, k), np.nan, np.float32)
    for i in range(n):
        li, ld = np.asarray(id_lists[i]), np.asarray(d_lists[i], np.float32)
        pos = [p for p in range(li.shape[0]) if li[p] >= 0]
        kept = walk(pos, lambda p: int(row_group[li[p]]), k, m)
        ids[i, :len(kept)] = li[kept]
        d[i, :len(kept)] = ld[kept]
    return ids, d


def same(a, b):
    """(ids, distances) pairs with equal shapes, equal ids and byte-equal distances."""
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == np.ascontiguousarray(b[1]).tobytes()


# The case in which the traversal at a beam of the whole index and the flat scan must agree (tests/test_gpu_knn_collapsed_edges.py):
# a graph small enough that a beam of FULL_N holds every row.  tests/test_collapse_model.py checks on the CPU oracle that at this
# seed and M, built one row at a time, every query's traversal returns all FULL_N rows, no two at the same distance.
FULL_N, FULL_DIM, FULL_NQ, FULL_M, FULL_SEED = 300, 20, 48, 8, 40
FULL_METRICS = ("sq_euclid", "cosine", "sq_euclid_i8")


def full_case():
    """(rows, queries) of that case: uniform, as everywhere."""
    rng_x, rng_q = np.random.default_rng(FULL_SEED), np.random.default_rng(FULL_SEED + 1000)
    return rng_x.random((FULL_N, FULL_DIM), dtype=np.float32), rng_q.random((FULL_NQ, FULL_DIM), dtype=np.float32)


def reached_from_entry(ref, layer=0):
    """How many nodes of an oracle.OracleIndex the entry point reaches over the out-edges of `layer`."""
    seen, todo = {ref.entry_point}, [ref.entry_point]
    while todo:
        for j in ref.edges(todo.pop(), layer).tolist():
            if j not in seen:
                seen.add(j)
                todo.append(j)
    return len(seen)


class CollapsedList:
    """One (query, chunk) list of the scan, or the merge's: k slots of (key, label), ascending, EMPTY where there is none."""

    def __init__(self, k, m):
        self.k, self.m = k, m
        self.keys = [EMPTY] * k
        self.labels = [None] * k          # the label of an empty slot is never read
        self.dropped = self.evicted = 0

    def kth(self):
        return self.keys[self.k - 1]

    def offer(self, x, g):
        """exact_list_insert_collapsed: the counts the wave takes with ballots, then drop / evict / ordinary insert."""
        k, m, keys, labels = self.k, self.m, self.keys, self.labels
        ins = below = total = 0
        last = -1
        for i in range(k):
            if keys[i] == EMPTY:
                break
            same = labels[i] == g
            ins += keys[i] < x
            below += same and keys[i] < x
            total += same
            if same:
                last = i
        if below >= m:
            self.dropped += 1
            return
        if total >= m:
            self.evicted += 1
            end = last                    # the largest entry of the label leaves; the list's last entry stays
        elif x < keys[k - 1]:
            filled = sum(1 for v in keys if v != EMPTY)
            end = min(filled, k - 1)      # the ordinary insert: the first empty slot is taken, or the last entry drops out
        else:
            return
        assert ins <= end
        keys[ins + 1:end + 1] = keys[ins:end]
        labels[ins + 1:end + 1] = labels[ins:end]
        keys[ins], labels[ins] = x, g

    def entries(self):
        return [x for x in self.keys if x != EMPTY]


def scan_chunk(keys, label_of, k, m, rng=None):
    """One chunk's list: the keys offered in a random order (rng) or as given, through the scan's filter -- a key that is not
    below the list's current k-th is never offered."""
    keys = list(keys)
    if rng is not None:
        keys = [keys[i] for i in rng.permutation(len(keys))]
    L = CollapsedList(k, m)
    for x in keys:
        if x < L.kth():
            L.offer(x, label_of(x))
    return L


def merge(lists, label_of, k, m):
    """The chunks' lists (each ascending, EMPTY-padded to k) into the final list; a list is left at its first key that is not below
    the current k-th."""
    out = CollapsedList(k, m)
    for keys in lists:
        for x in keys:
            if x >= out.kth():
                break
            out.offer(x, label_of(x))
    return out


def chunked(keys, label_of, k, m, chunk, rng=None):
    """What the device returns for the candidates `keys` (in id-list order) cut into chunks of `chunk`: the entries of the merged list."""
    lists = [scan_chunk(keys[lo:lo + chunk], label_of, k, m, rng).keys for lo in range(0, len(keys), chunk)]
    return merge(lists, label_of, k, m).entries()
