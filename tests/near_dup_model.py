"""The contracts of the near-duplicate calls (include/hnsw_mi355x.h, hnsw_mi355x_exact_range_query_by_id /
hnsw_mi355x_duplicate_groups) in numpy and plain Python.

The range list of a stored item: query i is the stored row of ids[i]; its candidates are the live ids (those of `allowed`, when one is
given) except ids[i] itself; the answer is every candidate whose distance is <= radius -- the float32 compare, so a NaN distance or a
NaN radius admits nothing -- ascending by (distance, id).  A duplicate of the row under another id is a candidate like any other.

The groups: the members are the candidates above; members a < b are joined when the distance with the stored row of a as the query
and row b as the candidate is <= radius; the groups are the connected components, and the label of a member is the smallest id of
its group.  Every other id below `length` has the label -1.

Distances come from the caller (dist_to(own, cand) -> the float32 distances of the stored row of `own` to the candidates `cand`), so
the model says nothing about arithmetic."""
import numpy as np

from by_id_model import candidates


def within_by_distance_and_id(d, cand, radius):
    """(ids, dists): the entries with d <= radius (float32 compare), ascending by (distance, id)."""
    d, cand = np.asarray(d, np.float32), np.asarray(cand, np.int32)
    with np.errstate(invalid="ignore"):
        keep = d <= np.float32(radius)
    d, cand = d[keep], cand[keep]
    key = np.where(d == 0, np.float32(0), d)                 # -0 and +0 are equal: the id decides
    order = np.lexsort((cand, key))
    return cand[order], d[order]


def exact_range_by_id(dist_to, live_ids, ids, radius, allowed=None):
    """(list of ids, list of dists) of the contract.  dist_to(id, cand) -> float32[len(cand)]."""
    cand = candidates(live_ids, allowed)
    out_ids, out_d = [], []
    for own in np.asarray(ids, np.int32):
        c = cand[cand != own]
        a, b = within_by_distance_and_id(dist_to(int(own), c), c, radius)
        out_ids.append(a)
        out_d.append(b)
    return out_ids, out_d


def groups_from_pairs(length, members, pairs):
    """labels[length] of the components of the graph (members, pairs): a plain union-find, the smaller root kept; -1 off the members."""
    parent = {int(v): int(v) for v in members}

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for a, b in pairs:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    labels = np.full(length, -1, np.int32)
    for v in parent:
        labels[v] = find(v)
    return labels


def pairs_within(dist_to, members, radius):
    """The pairs (a, b), a < b both members, with dist_to(a, [b]) <= radius: the row of the SMALLER id is the query."""
    members = np.sort(np.asarray(members, np.int32))
    out = []
    for i, a in enumerate(members[:-1]):
        later = members[i + 1:]
        ids, _ = within_by_distance_and_id(dist_to(int(a), later), later, radius)
        out += [(int(a), int(b)) for b in ids]
    return out


def labels_and_info(length, members, pairs):
    """(labels[length], info) of the graph (members, pairs): info as hnsw_mi355x_duplicate_groups' out_info, by name."""
    labels = groups_from_pairs(length, members, pairs)
    m = int(len(members))
    info = {"members": m, "groups": int((labels[np.asarray(members, np.int64)] == np.asarray(members)).sum()) if m else 0,
            "pairs_within": len(pairs), "pairs_measured": m * (m - 1) // 2}
    return labels, info


def duplicate_groups(dist_to, length, live_ids, radius, allowed=None):
    """(labels[length], info) of the contract."""
    members = candidates(live_ids, allowed)
    pairs = pairs_within(dist_to, members, radius)
    return labels_and_info(length, members, pairs)


def groups_from_range_lists(length, members, lists):
    """The same from range lists: lists[i] holds the ids within the radius of members[i] (its own id absent); only b > a counts."""
    pairs = [(int(a), int(b)) for a, l in zip(members, lists) for b in np.asarray(l) if b > a]
    return labels_and_info(length, members, pairs)


def all_but(n, own, base=None):
    """The allow-set "every id below n (of `base`, a bool mask, when given) except `own`" as a bool mask."""
    m = np.ones(n, bool) if base is None else np.asarray(base, bool).copy()
    m[own] = False
    return m


def range_by_id_loop(ix, ids, radius, allowed=None, n=None):
    """exact_range_query_by_id's contract on an Index, by the calls it replaces: one get_vectors and one exact_range_query per id."""
    n = ix.length if n is None else n
    live = np.zeros(n, bool)
    live[ix.ids()] = True
    base = live if allowed is None else live & np.isin(np.arange(n), candidates(np.arange(n), allowed))
    out_ids, out_d = [], []
    for own in np.asarray(ids, np.int32):
        a, b = ix.exact_range_query(ix.get_vectors([own]), radius, allowed=all_but(n, int(own), base))
        out_ids.append(a[0])
        out_d.append(b[0])
    return out_ids, out_d
