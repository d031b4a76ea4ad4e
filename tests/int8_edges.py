"""The edge rows of the int8 quantiser (oracle/hnsw_oracle.c "int8 rows": scale = max|x| / 127, q = clamp(rintf(x / scale)), 0 when
the scale is not positive), shared by the CPU tier (tests/test_int8.py: the oracle against the numpy statement) and the GPU tier
(tests/test_gpu_int8_edges.py: quantize_rows_kernel, rows and queries, against the oracle).  At dim 300 a lane of the kernel's
wave walks a second 256-element stretch: one row carries its maximum at the last index, another at index 256."""
import numpy as np

EDGE_DIMS = [7, 24, 300]


def _ordinary(dim):
    """A fixed row without ties: multiples of 1/4 in [-2.75, 2.75], the largest magnitude (-2.75) at index 0."""
    return ((np.arange(dim) * 37 % 23 - 11) / 4).astype(np.float32)


def edge_rows(dim):
    """(finite [n, dim], non_finite [3, dim]) float32.  hi = dim - 1; mid = 256 beyond 256 elements, dim // 2 otherwise."""
    hi, mid = dim - 1, 256 if dim > 256 else dim // 2
    i = np.arange(dim)
    rows = []
    ties = (i % 24 - 11.5).astype(np.float32)                    # 1: scale exactly 1, every other element a rintf tie
    ties[hi] = 127.0
    rows.append(ties)
    small = (i % 24 - 11.5).astype(np.float32)                   # 2: the same ties under the scale 2^-20, the maximum at mid
    small[mid] = 127.0
    rows.append(small * np.float32(2.0 ** -20))
    den = np.full(dim, 1e-40, np.float32)                        # 3: a denormal scale (3e-39 / 127 = 2.36e-41)
    den[mid] = -3e-39
    rows.append(den)
    rows.append(np.full(dim, 1e-45, np.float32))                 # 4: max / 127 rounds to 0: an all-zero record
    rows.append((np.float32(127.0) * np.float32(2.0 ** -126) * np.linspace(-1, 1, dim)).astype(np.float32))   # 5: the smallest normal scale
    big = np.full(dim, 3e38, np.float32)                         # 6: near the largest float
    big[hi] = -3.4e38
    rows.append(big)
    rows.append(np.full(dim, -0.0, np.float32))                  # 7: negative zeros: scale 0
    rows.append(_ordinary(dim))                                  # 8: an ordinary row and its negation
    rows.append(-_ordinary(dim))
    a = _ordinary(dim); a[mid] = np.inf                          # 9: non-finite rows
    b = _ordinary(dim); b[hi] = np.nan
    c = _ordinary(dim); c[0] = -np.inf; c[mid] = np.nan
    return np.stack(rows), np.stack([a, b, c])
