"""CPU tier: the bound behind the flat scan's MFMA prefilter (csrc/dk_exact_mfma.h), restated in numpy, and the
surface of its counters.  lb must never exceed the oracle's f32 distance, whichever way the matrix core rounds its sum -- the dot
product of the rounded vectors is taken in f64 and moved by +-beta |a| |b| -- and it must be no looser than it has to be: with e
halved, and with eps = 0, it breaks on pairs of the same families."""
import ctypes as ct

import numpy as np
import pytest

from common import uniform
from exact_knn_model import distances
from row_prefilter import U, gamma, h, representable_rows, row_bounds, worst_case

DIMS = [64, 160]
N = 48


def eps_of(dim):
    return 1.01 * (3 * dim + 36) * U


def lower_bound(x, q, sign, e_scale=1.0, eps=None):
    """lb [nq, n] of every (query, row) pair as the kernel forms it: n_x, n_q and the two operations of D~ in f32, the dot product
    the exact one of the rounded vectors moved by sign * beta |a| |b|."""
    dim = x.shape[1]
    eps = eps_of(dim) if eps is None else eps
    a, b = h(x).astype(np.float64), h(q).astype(np.float64)
    e_x, e_q = row_bounds(x).astype(np.float64) * e_scale, row_bounds(q).astype(np.float64) * e_scale
    n_x, n_q = (a * a).sum(axis=1).astype(np.float32), (b * b).sum(axis=1).astype(np.float32)
    beta = (2 * dim + 32) * U
    dot = (b @ a.T + sign * beta * np.sqrt(n_q.astype(np.float64))[:, None] * np.sqrt(n_x.astype(np.float64))[None, :]).astype(np.float32)
    n = (n_x[None, :] + n_q[:, None]).astype(np.float32)
    d = (n - np.float32(2.0) * dot).astype(np.float32)
    r = np.sqrt(np.maximum(d.astype(np.float64) - eps * n.astype(np.float64), 0.0)) - e_x[None, :] - e_q[:, None]
    r = np.where(r > 0, r, 0.0)
    return r * r * (1.0 - float(gamma(dim)))


def families(dim):
    rng = np.random.default_rng(dim)
    near100 = lambda n: (100.0 + 0.1 * rng.standard_normal((n, dim))).astype(np.float32)   # noqa: E731
    out = {"uniform": (uniform(N, dim, 1), uniform(N, dim, 2)),
           "binary16 rows": (representable_rows(N, dim, 3), uniform(N, dim, 4)),
           "offset 100": (near100(N), near100(N)),
           "scaled 2^-20": (uniform(N, dim, 5) * np.float32(2.0 ** -20), uniform(N, dim, 6) * np.float32(2.0 ** -20)),
           "scaled 300": (uniform(N, dim, 7) * np.float32(300.0), uniform(N, dim, 8) * np.float32(300.0))}
    # every element's rounding moves the distance the same way: pair (i, i) is the tight one.  At a stretch in the thousands the
    # distance is large enough that eps N~ costs sqrt(R) less than e_x / 2; the query is then rounded to binary16 (e_q = 0), which
    # moves it off the line by far less than that
    out["one way, stretch 3"] = worst_case(N, dim, 9, 3.0)
    for stretch in (2000.0, 5000.0):
        x, q = worst_case(N, dim, 9, stretch)
        out[f"one way, stretch {stretch}, binary16 query"] = (x, h(q))
    return out


@pytest.fixture(scope="module")
def measured():
    """family -> (x, q, the oracle's distances [nq, n]) per dim: computed once, never written."""
    out = {}
    for dim in DIMS:
        for name, (x, q) in families(dim).items():
            d = distances("sq_euclid", x, q, np.arange(x.shape[0], dtype=np.int32))
            d.setflags(write=False)
            out[(dim, name)] = (x, q, d)
    return out


@pytest.mark.parametrize("sign", [-1.0, 1.0])
def test_lb_never_exceeds_the_oracles_distance(measured, sign):
    for (dim, name), (x, q, d) in measured.items():
        lb = lower_bound(x, q, sign)
        assert (lb <= d.astype(np.float64)).all(), (dim, name, float((lb - d).max()))


@pytest.mark.parametrize("mutation", [dict(e_scale=0.5), dict(eps=0.0)])
def test_the_bound_breaks_without_e_or_eps(measured, mutation):
    broken = [key for key, (x, q, d) in measured.items() if (lower_bound(x, q, -1.0, **mutation) > d.astype(np.float64)).any()]
    assert broken, mutation


def test_getters_signatures_and_null_handle_answers():
    import importlib

    import hnswindex
    bindings = importlib.import_module(hnswindex.net_amd.Index.__module__)
    slots = ("launches", "pairs_on_tile", "pairs_remeasured", "reserved")
    for name in ("hnsw_mi355x_exact_prefilter_stats", "hnswdev_exact_prefilter_stats"):
        fn = getattr(bindings.lib, name)
        assert fn.restype is ct.c_int and list(fn.argtypes) == [ct.c_void_p, ct.POINTER(ct.c_uint64)], name
        out = (ct.c_uint64 * 4)(7, 7, 7, 7)
        assert fn(None, out) == -1 and list(out) == [7, 7, 7, 7], name       # a NULL handle: an error, nothing written
    ix = hnswindex.Index.__new__(hnswindex.Index)
    ix._h = None
    assert ix.exact_prefilter_stats() == dict.fromkeys(slots, 0)
    assert callable(hnswindex.DeviceBackend.exact_prefilter_stats)
