"""The half-precision row prefilter of KnnQuery (csrc/dk_sorted_top.h) restated in numpy: the shadow rows h(x), the
bound E on ||x - h(x)||_2 as pack_shadow_rows_kernel computes it, the rounding allowance g, the lower bound lb on the f32 distance
and the threshold form the kernel tests.  Shared by the CPU model test and the GPU test's inputs."""
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


def threshold(far, e, dim):
    """T of row_prefilter_threshold, in f32 with the kernel's operations: a row is turned away iff D_h > T."""
    c = c_of(dim)
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
