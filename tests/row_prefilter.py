"""The half-precision row prefilter of KnnQuery (csrc/dk_sorted_top.h) restated in numpy: the shadow rows h(x), the
bound E on ||x - h(x)||_2 as pack_shadow_rows_kernel computes it, the rounding allowance g, the lower bound lb on the f32 distance
and the threshold form the kernel tests.  Shared by the CPU model test and the GPU test's inputs.

Below that: search_model, the lean search with the prefilter in it, and GADGETS -- hand-made graphs on which the answer is one
decision of the prefilter at the edge of its bound (class Gadget), several to an index (GadgetIndex), and the catalogue of them that
tests/test_row_prefilter_inputs.py checks on the CPU and tests/test_gpu_row_prefilter_tight.py runs on the device.  Every search
for a gadget is seeded and bounded (N_CANDIDATES probes, a fixed number of steps); all kinds -- every element, chosen element sets,
list lengths, a partial repack -- are found at every dim asked for.  There is NO gadget for the rounding allowance g: at stretch
5000, dims 128 and 256, lb with g = 0 exceeds D_x by at most 2e-7 of it, but the kernel's threshold is raised by 2^-18 = 3.8e-6 for
its own roundings, so a kernel with g = 0 turns no candidate probe away at ANY farthest key above its D_x
(test_no_input_can_tell_g_from_zero_in_the_kernels_form): g is left to tests/test_row_prefilter_model.py."""
import numpy as np

U = 2.0 ** -24                      # unit roundoff of binary32
F32 = np.float32


def h(x):
    """The shadow of rows x: rounded to binary16, widened again (exact)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def gamma(dim):
    """g: relative allowance for the roundings of one f32 sum of squares over `dim` elements (row_prefilter_c's g)."""
    return F32(1.001) * F32((dim >> 3) + 16) * F32(U)


def c_of(dim):
    """1 + 1.5 g >= 1 / (1 - g), in f32 as the kernel computes it."""
    return F32(1.0) + F32(1.5) * gamma(dim)


def row_bounds(x):
    """Per row an upper bound of ||x - h(x)||_2, pack_shadow_rows_kernel's way: the squares summed in double, the root rounded up
    to f32, raised by 2^-20 (+ 1e-37); +inf for a row with an element that is not finite or does not round to a finite half."""
    x = np.asarray(x, dtype=np.float32)
    hx = h(x)
    bad = ~(np.isfinite(x) & np.isfinite(hx)).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.sqrt(((x.astype(np.float64) - hx.astype(np.float64)) ** 2).sum(axis=1))
        f = e.astype(np.float32)
        f = np.where(f.astype(np.float64) < e, np.nextafter(f, F32(np.inf)), f).astype(np.float32)
        f = f * F32(1.0 + 2.0 ** -20) + F32(1e-37)
    f[bad] = np.inf
    return f.astype(np.float32)


def e_of(x):
    """E: the index-wide word, the largest row bound."""
    return F32(row_bounds(x).max())


def lower_bound(d_h, e, dim, g=None):
    """lb = (sqrt(D_h) (1 - g) - E)^2 (1 - g), 0 when sqrt(D_h) <= E; evaluated in double.  `e` may be per row."""
    g = float(gamma(dim)) if g is None else float(g)
    with np.errstate(invalid="ignore"):
        r = np.sqrt(np.asarray(d_h, dtype=np.float64)) * (1.0 - g) - np.asarray(e, dtype=np.float64)
    r = np.where(r > 0, r, 0.0)          # (NaN compares false: 0, the row is kept)
    return r * r * (1.0 - g)


def threshold(far, e, dim, g=None):
    """T of row_prefilter_threshold, in f32 with the kernel's operations: a row is turned away iff D_h > T.  `g`: another allowance
    than gamma(dim) (a mutated model)."""
    c = c_of(dim) if g is None else F32(1.0) + F32(1.5) * F32(g)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.sqrt(np.maximum(np.asarray(far, dtype=np.float32), F32(1e-30)) * c, dtype=np.float32) + np.asarray(e, dtype=np.float32)
        t = (s * c).astype(np.float32)
        return (t * t * F32(1.0 + 2.0 ** -18)).astype(np.float32)


def turned_away(d_h, far, e, dim):
    """The kernel's decision for a full list whose farthest distance is `far` (NaN or inf anywhere: kept)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(d_h, dtype=np.float32) > threshold(far, e, dim)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def representable_rows(n, dim, seed):
    """Rows that ARE binary16 values: E = 0 (up to its 1e-37)."""
    return h(np.random.default_rng(seed).random((n, dim), dtype=np.float32))


def worst_case(n, dim, seed, stretch):
    """(rows x, one query per row): q = h + stretch (x - h), so x lies on the segment from h(x) to q and the rounding of EVERY
    element moves the distance the same way: ||x - q|| = ||h - q|| - ||x - h||, the triangle bound with equality (up to the
    rounding of q itself)."""
    x = np.random.default_rng(seed).random((n, dim), dtype=np.float32)
    hx = h(x)
    q = (hx.astype(np.float64) + stretch * (x.astype(np.float64) - hx.astype(np.float64))).astype(np.float32)
    return x, q


# ---- the search, restated ------------------------------------------------------------------------------------------------------
KEEP_MARGIN = 1.0 - 2.0 ** -20      # a decision with D_h <= T (1 - 2^-20) stays a "keep" if T's six f32 operations round otherwise (8 ulps)


def adjacency(layers):
    """[(counts, edges)] per layer, import_graph's form -> per layer a list of id lists."""
    return [[np.asarray(e)[i, :int(c[i])].tolist() if c[i] > 0 else [] for i in range(len(c))] for c, e in layers]


def search_model(rows, layers, levels, entry, q, ef, e, g=None):
    """KnnQuery's lean search with the row prefilter (traverse_sorted<.., LEAN, PF>), plainly: the reference's greedy descent to
    layer 1, then tests/test_novis_model.py's search_on_one_list -- ONE list of at most `ef` entries, no visited set -- in which
    every listed neighbour of an expansion is measured on the shadow (D_h) and, ONCE THE LIST IS FULL, turned away when
    D_h > T(farthest key at the start of that expansion); the others are measured from f32 (D_x), and D_x is all the list ever
    holds.  D_x and D_h are the oracle's AVX-order sums.  `e`, `g`: the bound's parameters, so that a mutated model can be run.
    -> dict(ids, dists: the list ascending; rows_on_shadow, rows_reread: the kernel's counters; rows_reread_sure: the keeps that a
    threshold a few ulps off would not undo; log: one dict per decision; popped)."""
    import oracle
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, dim = rows.shape
    ids = np.arange(n, dtype=np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = oracle.dist_query_rows("sq_euclid", rows, q, ids, use_avx=True)
        dh = oracle.dist_query_rows("sq_euclid", h(rows), q, ids, use_avx=True)
    adj = adjacency(layers)
    best = int(entry)
    for layer in range(int(levels[best]), 0, -1):          # GraphNavigator.cs:57-71
        changed = True
        while changed:
            changed = False
            for nb in list(adj[layer][best]):
                if dx[nb] < dx[best]:
                    best, changed = nb, True
    lst = [[dx[best], best, False]]
    popped, log = [], []
    on_shadow = reread = sure = 0
    while True:
        open_ = [t for t in lst if not t[2]]
        if not open_:
            break
        c = min(open_, key=lambda t: (t[0], t[1]))
        c[2] = True
        popped.append(c[1])
        full = len(lst) >= ef
        far = max(t[0] for t in lst)
        thr = threshold(far, e, dim, g) if full else F32(np.inf)
        kept = []
        for nb in adj[0][c[1]]:
            on_shadow += 1
            with np.errstate(invalid="ignore"):
                away = bool(full and dh[nb] > thr)
            log.append(dict(expansion=len(popped) - 1, of=c[1], id=nb, full=full, far=far, d_h=dh[nb], d_x=dx[nb], thr=thr, away=away))
            if not away:
                reread += 1
                kept.append(nb)
                with np.errstate(invalid="ignore"):
                    sure += int(not full or bool(np.float64(dh[nb]) <= np.float64(thr) * KEEP_MARGIN))
        for nb in kept:
            if any(t[1] == nb for t in lst):
                continue
            if len(lst) < ef or dx[nb] < far:
                lst.append([dx[nb], nb, False])
                if len(lst) > ef:
                    lst.remove(max(lst, key=lambda t: (t[0], -t[1])))
                far = max(t[0] for t in lst)
        # (a neighbour turned away carries +inf: never below the farthest key)
    lst.sort(key=lambda t: (t[0], t[1]))
    return dict(ids=[t[1] for t in lst], dists=np.array([t[0] for t in lst], dtype=np.float32), rows_on_shadow=on_shadow,
                rows_reread=reread, rows_reread_sure=sure, log=log, popped=popped, d_x=dx, d_h=dh)


# ---- gadgets: hand-made graphs on which ONE prefilter decision is the answer -----------------------------------------------------
HUB_VALUE = 4.0                     # the hub row: far from the unit cube, a binary16 value


def _d32(row, q):
    import oracle
    return oracle.dist_query_rows("sq_euclid", np.asarray(row, dtype=np.float32).reshape(1, -1), q, np.zeros(1, dtype=np.int32), use_avx=True)[0]


def _bump(c, i, up):
    c[i] = np.nextafter(c[i], np.float16(np.inf if up else -np.inf))


def _weights(c):
    """Coordinates with a fine binary16 grid are proposed more often: they are the fine steps of the search."""
    w = 1.0 / np.maximum(np.spacing(np.abs(c).astype(np.float16)).astype(np.float64), 2.0 ** -24)
    return w / w.sum()


def grid_point_in(q, lo, hi, rng, tries=6000):
    """A binary16-valued row f with lo <= D(f, q) <= hi (the oracle's f32 value), by a crude greedy walk from h(q): a random
    coordinate moves by one binary16 step when that brings the distance nearer to the middle of the window.  None if not found."""
    c = np.asarray(q, dtype=np.float32).astype(np.float16)
    q64 = np.asarray(q, dtype=np.float64)
    d = float(((c.astype(np.float64) - q64) ** 2).sum())
    mid = 0.5 * (float(lo) + float(hi))
    for t in range(tries):
        if lo <= d <= hi:
            d32 = _d32(c, q)
            if lo <= d32 <= hi:
                return c.astype(np.float32)
        if t % 64 == 0:
            w = _weights(c)
        i = int(rng.choice(c.size, p=w))
        c2 = c.copy()
        _bump(c2, i, rng.random() < 0.5)
        if not np.isfinite(c2[i]):
            continue
        d2 = d - (float(c[i]) - q64[i]) ** 2 + (float(c2[i]) - q64[i]) ** 2
        if abs(d2 - mid) < abs(d - mid) or (lo <= d <= hi):
            c, d = c2, d2
    return None


def grid_points_below(q, count, below, taken, rng, tries=40000):
    """`count` binary16-valued rows nearer to q than `below` (f32), their distances distinct from each other and from `taken`."""
    base = np.asarray(q, dtype=np.float32).astype(np.float16)
    q64 = np.asarray(q, dtype=np.float64)
    w = _weights(base)
    out, seen = [], set(float(t) for t in taken)
    for t in range(tries):
        if len(out) == count:
            break
        c = base.copy()
        for _ in range(int(rng.integers(0, 4)) if t else 0):      # (the first proposal is h(q) itself)
            _bump(c, int(rng.choice(c.size, p=w)), rng.random() < 0.5)
        if not np.isfinite(c).all() or float(((c.astype(np.float64) - q64) ** 2).sum()) >= float(below) * (1.0 - 1e-3):
            continue
        d32 = float(_d32(c, q))
        if d32 < float(below) and d32 not in seen:
            seen.add(d32)
            out.append((d32, c.astype(np.float32)))
    return out if len(out) == count else None


class Gadget:
    """One probe row p with its query q (worst_case: p on the segment from h(p) to q), K decoys that are binary16 values -- K - 1 of
    them nearer to q than p, one (f, the farthest) with D(f, q) in the middle half of (D_x(p), lb_mut) -- and the lists: the entry
    decoy d1 (local id 0, the nearest) lists the first `first_list` of the others; where that does not fill a list of K, the next
    nearest decoys list the rest, 2 M at a time; every other decoy lists `first_list` - 2 decoys, the hub (local id -1: a row that
    every bound turns away) and, last, p (local id K) -- `first_list` ids, so p's shadow value comes from the same measure pass.  So the
    list is full (K entries, f the farthest) before p is met, a correct kernel keeps p, p displaces f; a kernel whose bound is
    `e_mut` turns p away and answers with f.  Local ids: decoys 0 .. K - 1 ascending by distance, p = K."""

    def __init__(self, name, p, q, decoys, first_list, m):
        self.name, self.p, self.q, self.decoys, self.k, self.m = name, p, q, decoys, len(decoys), m
        K, cap = self.k, 2 * m
        rest = list(range(1, K))
        lists = {0: rest[:first_list]}
        owner, at = 1, first_list
        while at < len(rest):
            lists[owner] = rest[at:at + cap]
            owner, at = owner + 1, at + cap
        assert owner <= first_list + 1, "the decoys that fill the list must be listed by d1"
        for i in range(owner, K):
            lists[i] = [j for j in range(K) if j != i][:first_list - 2] + [-1, K]
        lists[K] = []
        assert all(len(v) <= cap for v in lists.values())
        self.lists = lists

    def rows(self):
        return np.concatenate([self.decoys, self.p.reshape(1, -1)]).astype(np.float32)


def make_gadget(name, cands_x, cands_q, start, k, first_list, m, e_index, e_mut, seed, g_mut=None):
    """The first candidate probe at or after `start` for which the decoys are found -> (Gadget, candidate index), or (None, None).
    e_index: the E the index will have (>= this probe's bound); e_mut, g_mut: the mutated bound that the gadget is to catch."""
    dim = cands_x.shape[1]
    for i in range(start, cands_x.shape[0]):
        p, q = cands_x[i], cands_q[i]
        if row_bounds(p.reshape(1, -1))[0] > e_index:
            continue
        rng = np.random.default_rng([seed, i])
        d_x, d_h = _d32(p, q), _d32(h(p), q)
        lb_mut = float(lower_bound(d_h, e_mut, dim, g_mut))
        if not lb_mut > float(d_x):
            continue
        quarter = 0.25 * (lb_mut - float(d_x))
        f = grid_point_in(q, float(d_x) + quarter, lb_mut - quarter, rng)
        if f is None:
            continue
        d_f = _d32(f, q)
        if turned_away(d_h, d_f, e_index, dim) or not bool(np.asarray(d_h, dtype=np.float32) > threshold(d_f, e_mut, dim, g_mut)):
            continue                                               # (the f32 threshold form must decide as lb does, both ways)
        near = grid_points_below(q, k - 1, d_x, [d_x, d_f, d_h], rng)
        if near is None:
            continue
        near.sort(key=lambda t: t[0])
        return Gadget(name, p, q, np.stack([c for _, c in near] + [f]), first_list, m), i
    return None, None


class GadgetIndex:
    """Several gadgets of one dim and M in one graph: id 0 is a far-away hub, the entry point, level 1, whose layer-1 list holds each
    gadget's d1 (level 1 too, at most M of them); the descent picks the gadget of the query.  E is index-wide: the largest probe bound."""

    def __init__(self, dim, m, gadgets):
        assert 0 < len(gadgets) <= m
        self.dim, self.m, self.gadgets = dim, m, gadgets
        rows, self.base = [np.full((1, dim), HUB_VALUE, dtype=np.float32)], []
        for gd in gadgets:
            self.base.append(sum(r.shape[0] for r in rows))
            rows.append(gd.rows())
        self.rows = np.concatenate(rows)
        n = self.rows.shape[0]
        self.levels = np.zeros(n, dtype=np.int32)
        self.levels[[0] + self.base] = 1
        c0, e0 = np.zeros(n, dtype=np.int32), np.zeros((n, 2 * m + 2), dtype=np.int32)
        c1, e1 = np.full(n, -1, dtype=np.int32), np.zeros((n, m + 2), dtype=np.int32)
        c1[[0] + self.base] = 0
        c1[0] = len(gadgets)
        e1[0, :len(gadgets)] = self.base
        for gd, b in zip(gadgets, self.base):
            for i, l in gd.lists.items():
                c0[b + i] = len(l)
                e0[b + i, :len(l)] = [b + j if j >= 0 else 0 for j in l]
        self.entry, self.layers = 0, [(c0, e0), (c1, e1)]
        self.e = e_of(self.rows)

    def probe_id(self, j):
        return self.base[j] + self.gadgets[j].k

    def far_id(self, j):
        return self.base[j] + self.gadgets[j].k - 1

    def model(self, j, e=None, g=None, rows=None, layers=None, levels=None):
        gd = self.gadgets[j]
        return search_model(self.rows if rows is None else rows, self.layers if layers is None else layers,
                            self.levels if levels is None else levels, self.entry, gd.q, gd.k, self.e if e is None else e, g)


# ---- the catalogue ------------------------------------------------------------------------------------------------------------
N_CANDIDATES = 48                    # probe candidates per gadget: the bounded length of every seeded search here
A_DIMS = [8, 24, 100, 128, 136, 200, 255, 256]
A_STRETCHES = [3.0, 5.0]
B_SETS = {                           # name -> (dim, the elements that carry the rounding error)
    "b_tail_136": (136, range(128, 136)), "b_tail_200": (200, range(128, 200)), "b_tail_256": (256, range(128, 256)),
    "b_block_100": (100, range(96, 100)), "b_block_255": (255, range(240, 255)), "b_elem0_100": (100, range(0, 1)),
}
C_LISTS = {                          # M -> [(K, ids in d1's list)]: one to four measure passes, the second 32-block, four register sets
    4: [(4, 3)], 16: [(13, 12), (21, 20), (32, 31)], 32: [(41, 40), (65, 64), (130, 64)],
}
C_DIMS = {4: 24, 16: 100, 32: 136}


def error_on(x, elements):
    """x with every element outside `elements` replaced by its binary16 value."""
    y = h(x)
    idx = np.fromiter(elements, dtype=np.int64)
    y[:, idx] = x[:, idx]
    return y


def worst_case_on(n, dim, seed, stretch, elements):
    """worst_case whose rows carry their rounding error on `elements` alone."""
    x = error_on(np.random.default_rng(seed).random((n, dim), dtype=np.float32), elements)
    hx = h(x)
    return x, (hx.astype(np.float64) + stretch * (x.astype(np.float64) - hx.astype(np.float64))).astype(np.float32)


def _by_bound(x, q):
    """Candidates ordered by how close their bound is to the batch's median: the gadgets of one index get probes of similar ||x - h(x)||."""
    b = row_bounds(x)
    order = np.argsort(np.abs(b - np.median(b)), kind="stable")
    return x[order], q[order]


def build_index(dim, m, specs, seed, mutation):
    """specs: [(name, candidate rows, candidate queries, K, ids in d1's list)].  mutation(E, probe rows) -> (e_mut, g_mut).  The probes
    are chosen first (E is index-wide and the decoys' window depends on it); a gadget whose decoys are not found moves on to its
    next candidate and the index starts over.  None when some gadget runs out of candidates."""
    at = [0] * len(specs)
    for _ in range(N_CANDIDATES * len(specs)):
        probes = np.stack([s[1][a] for s, a in zip(specs, at)])
        e = e_of(probes)
        e_mut, g_mut = mutation(e, probes)
        gadgets, moved = [], False
        for j, (name, cx, cq, k, first) in enumerate(specs):
            gd, i = make_gadget(name, cx, cq, at[j], k, first, m, e, e_mut, seed + j, g_mut)
            if gd is None:
                return None
            if i != at[j]:
                at[j], moved = i, True
                break
            gadgets.append(gd)
        if not moved:
            gi = GadgetIndex(dim, m, gadgets)
            gi.e_mut, gi.g_mut = e_mut, g_mut
            return gi
    return None


def half_e(e, probes):
    return F32(0.5) * e, None


def catalogue():
    """name -> GadgetIndex (or None where the seeded search found no gadget), built once per process."""
    global _CATALOGUE
    if _CATALOGUE is None:
        out = {}
        for dim in A_DIMS:                                          # (a) rounding error on every element
            specs = [(f"a_{dim}_s{int(s)}", *_by_bound(*worst_case(N_CANDIDATES, dim, 2100 + dim + int(s), s)), 6, 5) for s in A_STRETCHES]
            out[f"a_{dim}"] = build_index(dim, 16, specs, 3100 + dim, half_e)
        for name, (dim, elements) in B_SETS.items():                # (b) error on a chosen element set: E computed without that set is E of binary16 rows
            specs = [(f"{name}_s{int(s)}", *_by_bound(*worst_case_on(N_CANDIDATES, dim, 2300 + dim + int(s), s, elements)), 6, 5) for s in A_STRETCHES]
            without = lambda e, probes, el=elements: (e_of(error_on(probes, [i for i in range(probes.shape[1]) if i not in el])), None)
            out[name] = build_index(dim, 16, specs, 3300 + dim, without)
        for m, cases in C_LISTS.items():                            # (c) list lengths
            dim = C_DIMS[m]
            specs = [(f"c_m{m}_k{k}_l{first}", *_by_bound(*worst_case(N_CANDIDATES, dim, 2500 + m + k, 4.0)), k, first) for k, first in cases]
            out[f"c_m{m}"] = build_index(dim, m, specs, 3500 + m, half_e)
        # (d) partial repack: rows added after the first pack are binary16 values, so E of the last pack alone is E of such rows
        specs = [(f"d_100_s{int(s)}", *_by_bound(*worst_case(N_CANDIDATES, 100, 2700 + int(s), s)), 6, 5) for s in A_STRETCHES]
        out["d_100"] = build_index(100, 16, specs, 3700, lambda e, probes: (e_of(added_rows(100)), None))
        _CATALOGUE = out
    return _CATALOGUE


_CATALOGUE = None


def added_rows(dim, n=5):
    """(d)'s Add after the first pack: binary16-valued rows far from the unit cube."""
    return h(np.float32(40.0) + np.float32(8.0) * np.random.default_rng(2900 + dim).random((n, dim), dtype=np.float32))


def oracle_of(gi, extra=0):
    """The gadget index in the oracle (MinNN 1: a query's list holds k entries), with room for `extra` rows more."""
    import oracle
    ref = oracle.OracleIndex(gi.dim, "sq_euclid", max_edges=gi.m, min_nn=1, collection_size=gi.rows.shape[0] + extra, allow_removals=False)
    ref.import_graph(gi.rows, gi.levels, gi.entry, gi.layers)
    ref.rng_skip(gi.rows.shape[0])
    return ref


def graph_of(ref, m):
    """(levels, layers) of an oracle index as it stands, import_graph's form."""
    lv = ref.levels()
    layers = []
    for layer in range(int(lv.max()) + 1):
        cnt = np.where(lv >= layer, 0, -1 if layer else 0).astype(np.int32)
        ed = np.zeros((lv.size, (2 * m if layer == 0 else m) + 2), dtype=np.int32)
        for i in np.nonzero(lv >= layer)[0]:
            e = ref.edges(int(i), layer)
            cnt[i] = e.size
            ed[i, :e.size] = e
        layers.append((cnt, ed))
    return lv, layers
