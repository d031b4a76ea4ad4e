"""The 8-bit shadow of KnnQuery's row prefilter (kFormLeanPF8Fixed) restated in numpy: the index-wide grid (lo, step)
as shadow8_grid_kernel derives it, the shadow value of a code -- BY DEFINITION the f32 number fmaf(step, c, lo) --, the per-row bounds
and E8 as pack_shadow8_rows_kernel computes them, and search_model8: tests/row_prefilter.py's search_model with the shadow rows as an
argument.  gamma, c_of, threshold and adjacency are that file's (the 8-bit measure pass has a shorter lane chain than the f16 one:
the same allowance g holds).  The encoder here (nearest grid point, clamped) is the CPU tests' own: nothing in the proof needs the
device's encoder specified, and the GPU tests decode the codes they read back.

Below that: GADGETS for the 8-bit bound, in row_prefilter.Gadget's shape.  The hub row holds 0 and 4, so the grid is known up front
(lo = 0, step = 4 / 255 rounded up); the decoys ARE grid values (they decode exactly: E8 comes from the probes alone), and a probe p
lies on the segment from h8(p) to its query.  A correct kernel keeps p, which displaces the farthest decoy f; a kernel with half of
E8 answers with f."""
from fractions import Fraction

import numpy as np

from row_prefilter import F32, Gadget, GadgetIndex, adjacency, c_of, gamma, lower_bound, threshold   # noqa: F401  (re-exported)

DIM = 128                            # the one row length the 8-bit form is built for (kPfFixedDim)


# ---- the grid, the codes, the bound --------------------------------------------------------------------------------------------
def grid_of(x):
    """(lo, step) of a FULL pack of rows x: lo the smallest finite element, step = (hi - lo) / 255 in double, rounded UP to f32;
    step 1 when hi == lo or nothing is finite."""
    x = np.asarray(x, dtype=np.float32)
    fin = x[np.isfinite(x)]
    if fin.size == 0:
        return F32(0.0), F32(1.0)
    lo, hi = F32(fin.min()), F32(fin.max())
    if lo == 0 and np.signbit(fin[fin == 0]).any():
        lo = F32(-0.0)                                                   # (the ordered key puts -0 below +0)
    s = (np.float64(hi) - np.float64(lo)) / 255.0
    if not s > 0:
        return lo, F32(1.0)
    with np.errstate(over="ignore"):
        step = F32(s)
    if np.float64(step) < s:
        step = np.nextafter(step, F32(np.inf))
    return lo, F32(step)


def _round_f32(v):
    """A Fraction -> the nearest binary32 (ties to even)."""
    f = F32(float(v))                                                    # within one ulp of the answer
    best = None
    for c in (np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))):
        if not np.isfinite(c):
            continue
        err = abs(Fraction(float(c)) - v)
        even = (int(np.array([c], dtype=np.float32).view(np.uint32)[0]) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, c)
    return F32(best[1])


def table(lo, step):
    """The 256 shadow values of a grid: fmaf(step, (float)c, lo) exactly -- the product and the sum as ONE rounding."""
    if not (np.isfinite(lo) and np.isfinite(step)):
        with np.errstate(invalid="ignore", over="ignore"):
            return (np.float64(step) * np.arange(256) + np.float64(lo)).astype(np.float32)
    return np.array([_round_f32(Fraction(float(step)) * c + Fraction(float(lo))) for c in range(256)], dtype=np.float32)


def encode(x, lo, step):
    """The nearest grid point, clamped to [0, 255] (NaN: 0)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(x, dtype=np.float32).astype(np.float64) - np.float64(lo)) / np.float64(step)
        c = np.where(t > 0, np.where(t < 255, np.rint(t), 255), 0)
    return c.astype(np.uint8)


def decode(codes, lo, step):
    """The shadow rows of code bytes: f32."""
    return table(lo, step)[np.asarray(codes, dtype=np.uint8)]


def row_bounds8(x, shadow):
    """Per row an upper bound of ||x - h8(x)||_2, pack_shadow8_rows_kernel's way: the squares summed in double, the root rounded up
    to f32, raised by 2^-20 (+ 1e-37); +inf for a row with an element or a shadow value that is not finite."""
    x, shadow = np.asarray(x, dtype=np.float32), np.asarray(shadow, dtype=np.float32)
    bad = ~(np.isfinite(x) & np.isfinite(shadow)).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.sqrt(((x.astype(np.float64) - shadow.astype(np.float64)) ** 2).sum(axis=1))
        f = e.astype(np.float32)
        f = np.where(f.astype(np.float64) < e, np.nextafter(f, F32(np.inf)), f).astype(np.float32)
        f = f * F32(1.0 + 2.0 ** -20) + F32(1e-37)
    f[bad] = np.inf
    return f.astype(np.float32)


def pack(x, grid=None):
    """(lo, step, codes, shadow rows, E8) of rows x packed on `grid` (None: a full pack, the grid of x itself)."""
    lo, step = grid_of(x) if grid is None else grid
    codes = encode(x, lo, step)
    shadow = decode(codes, lo, step)
    return lo, step, codes, shadow, F32(row_bounds8(x, shadow).max())


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def worst_case8(x, shadow, stretch):
    """One query per row: q = h8 + stretch (x - h8) -- x on the segment from h8(x) to q, the triangle bound with equality."""
    return (shadow.astype(np.float64) + stretch * (x.astype(np.float64) - shadow.astype(np.float64))).astype(np.float32)


# ---- the search, restated ------------------------------------------------------------------------------------------------------------
def search_model8(rows, shadow, layers, levels, entry, q, ef, e, g=None):
    """row_prefilter.search_model with the shadow rows as an argument (D_8: the oracle's f32 sum on them) and E, g mutable.  Beside its
    counters: rows_reread_lo / rows_reread_hi, the re-reads with every threshold moved by a factor 1 -+ 2 g -- the kernel sums D_8 in
    another order than the oracle does, each within g of the exact value."""
    import oracle
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, dim = rows.shape
    ids = np.arange(n, dtype=np.int32)
    g2 = 2.0 * float(gamma(dim))
    with np.errstate(over="ignore", invalid="ignore"):
        dx = oracle.dist_query_rows("sq_euclid", rows, q, ids, use_avx=True)
        dh = oracle.dist_query_rows("sq_euclid", np.ascontiguousarray(shadow, dtype=np.float32), q, ids, use_avx=True)
    adj = adjacency(layers)
    best = int(entry)
    for layer in range(int(levels[best]), 0, -1):
        changed = True
        while changed:
            changed = False
            for nb in list(adj[layer][best]):
                if dx[nb] < dx[best]:
                    best, changed = nb, True
    lst = [[dx[best], best, False]]
    popped = []
    on_shadow = reread = lo = hi = 0
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
            with np.errstate(invalid="ignore", over="ignore"):
                away = bool(full and dh[nb] > thr)
                lo += int(not (full and np.float64(dh[nb]) > np.float64(thr) * (1.0 - g2)))
                hi += int(not (full and np.float64(dh[nb]) > np.float64(thr) * (1.0 + g2)))
            if not away:
                reread += 1
                kept.append(nb)
        for nb in kept:
            if any(t[1] == nb for t in lst):
                continue
            if len(lst) < ef or dx[nb] < far:
                lst.append([dx[nb], nb, False])
                if len(lst) > ef:
                    lst.remove(max(lst, key=lambda t: (t[0], -t[1])))
                far = max(t[0] for t in lst)
    lst.sort(key=lambda t: (t[0], t[1]))
    return dict(ids=[t[1] for t in lst], dists=np.array([t[0] for t in lst], dtype=np.float32), rows_on_shadow=on_shadow,
                rows_reread=reread, rows_reread_lo=lo, rows_reread_hi=hi, popped=popped, d_x=dx, d_8=dh)


# ---- gadgets -------------------------------------------------------------------------------------------------------------------------
HUB_TOP = 4.0                        # row_prefilter.HUB_VALUE; the hub's element 0 is 0, so the grid is [0, 4]
GRID = (F32(0.0), grid_of(np.array([0.0, HUB_TOP], dtype=np.float32))[1])
STRETCH = 4.0
C_LISTS8 = {4: [(4, 3)], 16: [(13, 12), (21, 20), (32, 31)], 32: [(41, 40), (65, 64), (130, 64)]}   # M -> [(K, ids in d1's list)]
N_CANDIDATES = 24


def _d32(row, q):
    import oracle
    return float(oracle.dist_query_rows("sq_euclid", np.asarray(row, dtype=np.float32).reshape(1, -1), q, np.zeros(1, dtype=np.int32), use_avx=True)[0])


def _walk(q, want, rng, tab, tries=4000):
    """Code bytes whose shadow row f has want(D(f, q)) true (the oracle's f32 distance), by a greedy walk from the nearest grid point:
    a random coordinate moves by one step when that brings the squared distance nearer to the middle of the window (lo, hi) = want.window."""
    lo, hi = want
    mid = 0.5 * (lo + hi)
    c = encode(q, *GRID).astype(np.int64)
    q64 = q.astype(np.float64)
    d = float(((tab[c].astype(np.float64) - q64) ** 2).sum())
    for _ in range(tries):
        if lo <= d <= hi and lo <= _d32(tab[c], q) <= hi:
            return c.astype(np.uint8)
        i = int(rng.integers(0, c.size))
        c2 = int(np.clip(c[i] + (1 if rng.random() < 0.5 else -1), 0, 255))
        d2 = d - (float(tab[c[i]]) - q64[i]) ** 2 + (float(tab[c2]) - q64[i]) ** 2
        if abs(d2 - mid) < abs(d - mid):
            c[i], d = c2, d2
    return None


def make_gadget8(name, p, q, k, first_list, m, e_index, seed):
    """A Gadget around probe p and its query q, or None: K - 1 grid-valued decoys nearer to q than p, and f with D(f, q) in the middle
    half of (D_x(p), lb with half of e_index)."""
    tab = table(*GRID)
    rng = np.random.default_rng(seed)
    d_x, d_8 = _d32(p, q), _d32(decode(encode(p, *GRID), *GRID), q)
    lb_half = float(lower_bound(d_8, 0.5 * float(e_index), DIM))
    if not lb_half > d_x:
        return None
    quarter = 0.25 * (lb_half - d_x)
    f = _walk(q, (d_x + quarter, lb_half - quarter), rng, tab)
    if f is None:
        return None
    d_f = _d32(tab[f], q)
    if bool(F32(d_8) > threshold(d_f, e_index, DIM)) or not bool(F32(d_8) > threshold(d_f, F32(0.5) * F32(e_index), DIM)):
        return None                                                      # (the f32 threshold form must decide as lb does, both ways)
    d_near = _d32(tab[encode(q, *GRID)], q)
    near, seen = [], {d_x, d_f, d_8}
    for t in range(40 * k):
        if len(near) == k - 1:
            break
        target = d_near + (0.9 * d_x - d_near) * rng.random()
        c = _walk(q, (min(target, 0.95 * d_x) * 0.98, min(target * 1.02, 0.97 * d_x)), rng, tab, tries=600) if t else encode(q, *GRID)
        if c is None:
            continue
        d = _d32(tab[c], q)
        if d < d_x and d not in seen:
            seen.add(d)
            near.append((d, tab[c]))
    if len(near) != k - 1:
        return None
    near.sort(key=lambda t: t[0])
    return Gadget(name, p, q, np.stack([r for _, r in near] + [tab[f]]).astype(np.float32), first_list, m)


class GadgetIndex8(GadgetIndex):
    """row_prefilter.GadgetIndex whose hub row starts with 0 (the grid's lower end); e8: E8 of a full pack of its rows."""

    def __init__(self, m, gadgets):
        super().__init__(DIM, m, gadgets)
        self.rows[0, 0] = 0.0
        self.grid = grid_of(self.rows)
        assert self.grid[0] == GRID[0] and self.grid[1] == GRID[1]
        _, _, self.codes, self.shadow, self.e8 = pack(self.rows)

    def model8(self, j, e=None):
        gd = self.gadgets[j]
        return search_model8(self.rows, self.shadow, self.layers, self.levels, self.entry, gd.q, gd.k, self.e8 if e is None else e)


def build_index8(m, seed):
    """The gadgets of C_LISTS8[m] in one index: probes of similar ||p - h8(p)|| (E8 is index-wide), chosen before their decoys."""
    x = np.random.default_rng(seed).random((N_CANDIDATES, DIM), dtype=np.float32)
    _, _, _, shadow, _ = pack(x, GRID)
    b = row_bounds8(x, shadow)
    order = np.argsort(np.abs(b - np.median(b)), kind="stable")
    cases = C_LISTS8[m]
    at = 0
    while at + len(cases) <= N_CANDIDATES:
        pick = order[at:at + len(cases)]
        e_index = F32(b[pick].max())
        q = worst_case8(x[pick], shadow[pick], STRETCH)
        gadgets = [make_gadget8(f"m{m}_k{k}_l{first}", x[i], q[j], k, first, m, e_index, seed + 17 * j)
                   for j, (i, (k, first)) in enumerate(zip(pick, cases))]
        if all(g is not None for g in gadgets):
            return GadgetIndex8(m, gadgets)
        at += 1
    return None


_CATALOGUE8 = {}


def catalogue8(m):
    if m not in _CATALOGUE8:
        _CATALOGUE8[m] = build_index8(m, 8100 + m)
    return _CATALOGUE8[m]
