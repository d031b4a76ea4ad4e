"""CPU tier: stage 1 of the int8 tile (csrc/dk_exact_mfma_i8.h) restated in numpy -- the f32 lower bound never lies above
the library's distance, on records with extreme scales, the largest sums of squares the form serves and the dot product at both ends
of Cauchy-Schwarz.  (The two FMAs are formed in float64 and rounded once more: at most a last bit beside the device's, the proof's 16 u
against the 11.2 u it needs covers it.)"""
import numpy as np

F = np.float32
NMAX = 127 * 127 * 4 * 206      # the sum of squares of a record of kExactI8MaxPitch words


def term(s, n):
    t = (s * s).astype(F) * n.astype(F)
    return np.where(np.isfinite(t), t, F(np.nan))


def lower_bound(sa, na, sb, nb, dot):
    S = term(sa, na) + term(sb, nb)
    p = sa * (F(2) * sb)
    est = (-p.astype(np.float64) * dot.astype(F) + S).astype(F)
    return est - (np.float64(2.0 ** -20) * S + 2.0 ** -96).astype(F)


def library(sa, na, sb, nb, dot):   # i8_epilogue (csrc/dk_metric.h)
    sa, sb = sa.astype(np.float64), sb.astype(np.float64)
    return ((sa * sa * na + sb * sb * nb) - 2.0 * (sa * sb * dot)).astype(F)


def test_the_bound_is_never_above_the_distance():
    scales = np.array([0.0, 1e-45, 1e-30, 1e-20, 1e-3, 1.0 / 127, 0.333, 1e10, 1.2e15, 1.8e19, np.inf], dtype=F)
    sums = np.array([0, 127 * 127, 1234567, NMAX], dtype=np.int64)
    frac = np.array([-1.0, -0.5, -1e-7, 0.0, 1e-7, 0.5, 0.999999, 1.0])   # of sqrt(na nb), the largest |dot|
    with np.errstate(all="ignore"):
        sa, sb, na, nb, f = (a.ravel() for a in np.meshgrid(scales, scales, sums, sums, frac, indexing="ij"))
        dot = np.trunc(f * np.floor(np.sqrt(na.astype(np.float64) * nb))).astype(np.int64)
        lb, dist = lower_bound(sa, na, sb, nb, dot), library(sa, na, sb, nb, dot)
        assert not (lb > dist).any(), [(a[lb > dist][0]) for a in (sa, na, sb, nb, dot, lb, dist)]   # a NaN keeps the pair
        worth = np.isfinite(dist) & (dist > 1e-20) & (dot <= 0)
        assert worth.sum() > 1000 and (lb[worth] > F(0.9999) * dist[worth]).all()   # within 1e-4 of the distance wherever nothing cancels
