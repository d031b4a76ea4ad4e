"""CPU tier: the half-precision metric names (sq_euclid_f16, ucosine_f16) at the boundary -- the header's codes are the
bindings', the names are accepted by hnsw_create (it gets as far as looking for a device), and cosine_f16, which does not
exist, fails like any unknown metric."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def net():
    import hnswindex
    return hnswindex.net_amd


def test_header_codes_equal_the_bindings(net):
    text = (ROOT / "include" / "hnsw_mi355x.h").read_text()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bHNSWDEV_([A-Z0-9_]+_F16)\s*=\s*(\d+)", text)}
    assert codes == {"sq_euclid_f16": 4, "ucosine_f16": 5}
    assert {k: net.bindings.METRICS[k] for k in codes} == codes
    assert sorted(net.bindings.METRICS.values()) == list(range(6))


@pytest.mark.parametrize("name", [b"sq_euclid_f16", b"ucosine_f16"])
def test_the_names_are_known_to_hnsw_create(net, name):
    h = net.lib.hnsw_create(name)
    if net.lib.hnswdev_device_count() > 0:
        assert h
        net.lib.hnsw_free(h)
    else:   # the name was understood: what is missing is the device
        assert not h
        assert "no HIP device" in net.last_error() and "Unsupported distance metric" not in net.last_error()


def test_cosine_f16_is_not_a_metric(net):
    assert not net.lib.hnsw_create(b"cosine_f16")
    assert "Unsupported distance metric" in net.last_error() and "cosine_f16" in net.last_error()
    with pytest.raises(KeyError):
        net.DeviceBackend(8, "cosine_f16")
