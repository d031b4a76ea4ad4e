"""The contract of the near-duplicate calls over the graph's edges (include/hnsw_mi355x.h, hnsw_mi355x_graph_duplicate_groups /
hnsw_mi355x_near_edges) in numpy and plain Python.

Three inputs: edges_of(i) -> the ids of i's layer-0 list, in list order; the members (the live ids an allow-set allows); and
dist_to(own, cand) -> the float32 distances of the stored row of `own`, taken as the query, to the rows of `cand`.  An EDGE is a
pair (i, j): i a member, j in edges_of(i), j a member -- directed, so that two items which list each other give two edges.  It is
WITHIN the radius when dist_to(i, [j]) <= radius, the float32 compare (NaN admits nothing).  near_edges returns the within-edges,
ascending by the owner and, inside one owner, by (distance, id); the groups are the components of the members under the within-edges
read both ways, labelled with their smallest id.  Distances come from the caller: the model says nothing about arithmetic."""
import numpy as np

from near_dup_model import groups_from_pairs, within_by_distance_and_id


def near_edges(edges_of, members, dist_to, radius):
    """(src int32[], dst int32[], dist float32[], edges_measured) of the contract."""
    members = np.sort(np.asarray(members, np.int32))
    is_member = set(members.tolist())
    src, dst, dist, measured = [], [], [], 0
    for i in members.tolist():
        cand = np.asarray([j for j in np.asarray(edges_of(i)).tolist() if j in is_member], np.int32)
        measured += cand.size
        if cand.size == 0:
            continue
        ids, d = within_by_distance_and_id(dist_to(i, cand), cand, radius)
        src.append(np.full(ids.size, i, np.int32))
        dst.append(ids.astype(np.int32))
        dist.append(d.astype(np.float32))
    cat = lambda parts, t: np.concatenate(parts).astype(t) if parts else np.zeros(0, t)
    return cat(src, np.int32), cat(dst, np.int32), cat(dist, np.float32), measured


def graph_duplicate_groups(edges_of, length, members, dist_to, radius):
    """(labels int32[length], info) of the contract; info as hnsw_mi355x_graph_duplicate_groups' out_info, by name -- but for
    `launches`, which the model cannot know."""
    members = np.sort(np.asarray(members, np.int32))
    src, dst, _, measured = near_edges(edges_of, members, dist_to, radius)
    labels = groups_from_pairs(length, members, zip(src.tolist(), dst.tolist()))
    m = int(members.size)
    info = {"members": m, "groups": int((labels[members.astype(np.int64)] == members).sum()) if m else 0,
            "edges_within": int(src.size), "edges_measured": int(measured)}
    return labels, info


def dist_from_range_lists(members, lists_ids, lists_d):
    """dist_to over the lists exact_range_query_by_id(members, radius) returned: the distance of a listed id, +inf for any other --
    an id that is not in own's list is farther than the radius the lists were taken with, so +inf decides as its distance would
    for that radius and any smaller one."""
    table = {int(o): dict(zip(np.asarray(i).tolist(), np.asarray(d, np.float32).tolist())) for o, i, d in zip(members, lists_ids, lists_d)}
    return lambda own, cand: np.asarray([table[int(own)].get(int(c), np.inf) for c in cand], np.float32)
