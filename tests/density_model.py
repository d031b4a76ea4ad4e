"""The contract of the density clusters (include/hnsw_mi355x.h, hnsw_mi355x_density_clusters) in numpy and plain
Python: DBSCAN over the members and the pair rule of duplicate_groups (tests/near_dup_model.py).

Members a < b are WITHIN when the distance with the stored row of a as the query and row b as the candidate is <= radius (the
float32 compare: a NaN distance or a NaN radius admits nothing).  counts[v] is the number of within pairs that hold v, -1 where v is
no member.  A member is CORE when counts[v] + 1 >= min_samples.  The clusters are the connected components of the core members
under the within pairs between two of them, and a cluster's label is its smallest core id.  A member that is not core and has a core
within-neighbour is a BORDER: it takes the label of the core neighbour of smallest (distance, id) -- the pair's own distance, -0 equal
to +0.  Every other member is NOISE, label -1, as is every non-member.

Distances come from the caller (dist_to(own, cand) -> the float32 distances of the stored row of `own` to the candidates `cand`), so
the model says nothing about arithmetic."""
import numpy as np

from by_id_model import candidates
from near_dup_model import groups_from_pairs, within_by_distance_and_id

INFO = ("members", "clusters", "core", "border", "noise", "pairs_within", "pairs_measured", "scans")


def pairs_within_d(dist_to, members, radius):
    """near_dup_model.pairs_within with every pair's distance kept: (a, b, d), a < b both members, d = dist_to(a, [b]) <= radius."""
    members = np.sort(np.asarray(members, np.int32))
    out = []
    for i, a in enumerate(members[:-1]):
        later = members[i + 1:]
        ids, d = within_by_distance_and_id(dist_to(int(a), later), later, radius)
        out += [(int(a), int(b), np.float32(x)) for b, x in zip(ids, d)]
    return out


def neighbor_counts(length, members, pairs):
    """counts[length]: the pairs that hold each member, -1 off the members.  pairs: (a, b, ...) tuples."""
    counts = np.full(length, -1, np.int32)
    counts[np.asarray(members, np.int64)] = 0
    for p in pairs:
        counts[p[0]] += 1
        counts[p[1]] += 1
    return counts


def clusters_from_pairs(length, members, pairs_d, min_samples, scans=1):
    """(labels[length], counts[length], info) of the graph (members, within pairs (a, b, d) with a < b).  scans: how often the device
    is expected to walk the triangle (the model cannot know; it only enters pairs_measured and the slot of its own)."""
    if min_samples < 1:
        raise ValueError("min_samples = %d is below 1" % min_samples)
    members = [int(v) for v in members]
    m = len(members)
    counts = neighbor_counts(length, members, pairs_d)
    core = {v for v in members if int(counts[v]) + 1 >= min_samples}
    labels = groups_from_pairs(length, sorted(core), [(a, b) for a, b, _ in pairs_d if a in core and b in core])
    best = {}                                                    # a member that is not core -> the smallest (distance, core id) offered
    for a, b, d in pairs_d:
        if (a in core) == (b in core):
            continue
        c, v = (a, b) if a in core else (b, a)
        key = (0.0 if d == 0 else float(d), c)                   # -0 and +0 are equal: the id decides
        if v not in best or key < best[v]:
            best[v] = key
    for v, (_, c) in best.items():
        labels[v] = labels[c]
    scans = scans if m >= 2 else 0
    info = {"members": m, "clusters": sum(1 for v in core if labels[v] == v), "core": len(core), "border": len(best),
            "noise": m - len(core) - len(best), "pairs_within": len(pairs_d), "pairs_measured": scans * (m * (m - 1) // 2), "scans": scans}
    return labels, counts, info


def density_clusters(dist_to, length, live_ids, radius, min_samples, allowed=None, scans=1):
    """(labels[length], counts[length], info) of the contract."""
    members = candidates(live_ids, allowed)
    return clusters_from_pairs(length, members, pairs_within_d(dist_to, members, radius), min_samples, scans)


def pairs_from_range_lists(members, lists, dists):
    """The within pairs from range lists: lists[i] / dists[i] hold the ids within the radius of members[i] and their distances with
    members[i] as the query (its own id absent); a pair counts once, from its smaller id's list."""
    return [(int(a), int(b), np.float32(d)) for a, l, ds in zip(members, lists, dists) for b, d in zip(np.asarray(l), np.asarray(ds)) if b > a]


def counts_only_info(info):
    """What the call reports when no labels are asked for: the slots that need them are 0."""
    return {**info, "clusters": 0, "core": 0, "border": 0, "noise": 0}
