"""CPU tier: the bound of the cosine family's MFMA prefilter (csrc/dk_exact_mfma_ip.h), restated in numpy with the
constants 3.38 states and held against the oracle's distances: S_ub -- the float64 dot product of the operands rounded to halves,
moved up by beta |a| |b|, the worst the matrix core may return -- gives a lower bound that no pair's distance is below.  No library
code runs here: this is the check of the constants that does not depend on which inputs the GPU cases happen to draw."""
import numpy as np
import pytest

from common import normalize_f32, uniform
from exact_knn_model import distances

U = 2.0 ** -24


def lower_bounds(metric, x, q, e_scale=1.0, dot_up=1.0):
    """[nq, n] float32: the tile's lower bound on the distance of every pair, the dot product at the upper end of what the matrix core
    may return (dot_up = 0: as if it had returned the exact one)."""
    K = x.shape[1]
    beta, gamma = (2 * K + 32) * U, 1.001 * (K / 8 + 4) * U
    with np.errstate(over="ignore"):
        a, b = x.astype(np.float16).astype(np.float64), q.astype(np.float16).astype(np.float64)
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    na, nb, nq = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1), np.linalg.norm(q64, axis=1)
    ex, eq = e_scale * np.linalg.norm(x64 - a, axis=1), e_scale * np.linalg.norm(q64 - b, axis=1)
    dot = b @ a.T + dot_up * beta * nb[:, None] * na[None, :]
    P = (beta + 8 * U) * nb + eq + gamma * nq
    s_ub = dot + na[None, :] * P[:, None] + (ex * (1 + gamma))[None, :] * nq[:, None] + (K + 8) * 2.0 ** -149
    s_ub = np.nextafter(s_ub.astype(np.float32), np.float32(np.inf))     # (the kernel's S_ub is a float at or above this)
    if metric != "cosine":
        return np.float32(1) - s_ub
    sn = lambda v: np.sqrt((v * v).sum(axis=1, dtype=np.float32).astype(np.float64))   # noqa: E731
    denom = (sn(q)[:, None] * sn(x)[None, :]).astype(np.float32)
    return np.where(denom < np.float32(1e-30), np.float32(1), np.float32(1) - s_ub / denom)


def tables(dim):
    rng = np.random.default_rng(dim)
    v = rng.random(dim, dtype=np.float32)
    near = lambda n: normalize_f32(v + np.float32(1e-4) * rng.standard_normal((n, dim)).astype(np.float32))   # noqa: E731
    xu, qu = normalize_f32(uniform(300, dim, 1)), normalize_f32(uniform(9, dim, 2))
    # every rounding to half moves the dot product upward, and as far as Cauchy-Schwarz allows: x = a + c q, a and q halves
    qh = rng.uniform(0.0625, 0.09, (1, dim)).astype(np.float16).astype(np.float32)
    up = rng.uniform(0.0625, 0.09, (300, dim)).astype(np.float16).astype(np.float32) + np.float32(3e-4) * qh
    return {"uniform": ("ucosine", xu, qu), "f16": ("ucosine_f16", xu, qu), "near": ("ucosine", near(300), near(9)),
            "tiny": ("cosine", xu * np.float32(2.0 ** -20), qu), "long": ("cosine", xu * np.float32(300), qu), "up": ("ucosine", up, qh)}


@pytest.mark.parametrize("dim", [64, 768])
def test_the_bound_is_below_every_distance_and_needs_its_error_terms(dim):
    for name, (metric, x, q) in tables(dim).items():
        d = distances(metric, x, q, np.arange(x.shape[0], dtype=np.int32))
        if metric.endswith("_f16"):
            x = x.astype(np.float16).astype(np.float32)
        assert (lower_bounds(metric, x, q) <= d).all(), (name, dim)
        if name == "up":   # with e halved a matrix core that happens to be exact turns a pair away that belongs to the answer
            assert (lower_bounds(metric, x, q, e_scale=0.5, dot_up=0.0) > d).any(), dim
