"""CPU tier: the table of translation units (build.py units()) and the copies of the metric list -- C++ (HNSW_FOR_EACH_METRIC), the
build recipe (METRICS), the bindings (METRICS) and the ABI header (HNSWDEV_*) -- agree, and the build id covers the table."""
import importlib.util
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hnswindex.net_amd" / "csrc"


@pytest.fixture()
def build():
    spec = importlib.util.spec_from_file_location("hnsw_build_units", ROOT / "hnswindex.net_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def _macro_body(text, name):
    """The replacement text of a #define, its continuation lines joined."""
    m = re.search(r"^#define " + name + r"\([^)]*\)((?:.*\\\n)*.*)$", text, flags=re.M)
    assert m, name
    return m.group(1).replace("\\\n", " ")


def _metric_rows():
    """(id name, unit tag, ABI name) of every row of HNSW_FOR_EACH_METRIC, in order."""
    body = _macro_body((CSRC / "device_backend.h").read_text(), "HNSW_FOR_EACH_METRIC")
    rows = re.findall(r'X\(\s*(\w+)\s*,\s*(\w+)\s*,\s*"([^"]*)"\s*\)', body)
    assert len(rows) == body.count("X("), body
    return rows


def test_table_shape(build):
    us = build.units()
    assert len(build.METRICS) == 6 and len(build.KINDS) == 7
    assert len(us) == 6 * 8 + 4                                                # the table's rows, device_backend.hip, the three host sources
    assert sum(src.endswith(".hip") for _, src, _ in us) == 6 * 8 + 1           # the units that hold device code
    names = [name for name, _, _ in us]
    assert len(set(names)) == len(names)                                       # unit names, and with them the objects <name>.o
    assert {src for _, src, _ in us} == {"device_backend.hip", "kernel_unit.hip", "exact_unit.hip", "search_engine.cpp", "hnsw_index.cpp", "exports.cpp"}
    for _, src, _ in us:
        assert (CSRC / src).is_file(), src
    per_source = {}
    for name, src, defs in us:
        assert all(d.startswith("-DHNSW_UNIT_") for d in defs), (name, defs)   # the kind and the metric tag, nothing else
        assert tuple(defs) not in per_source.setdefault(src, set()), (name, defs)  # no two units are the same compilation
        per_source[src].add(tuple(defs))
    # no per-metric stub is left: the only exact_*.hip is the generic unit source
    assert [p.name for p in sorted(CSRC.glob("traverse_*.hip")) + sorted(CSRC.glob("exact_*.hip"))] == ["exact_unit.hip"]
    # the one-unit diagnostic build drops the seven traversal kinds and keeps the rest
    single = build.units(single_tu=True)
    assert [u for u in us if u[1] != "kernel_unit.hip"] == single and len(single) == 6 + 4


def test_kinds_agree_with_the_kernel_header(build):
    text = (CSRC / "device_kernels.h").read_text()
    kinds = re.findall(r"X\((\w+), __VA_ARGS__\)", _macro_body(text, "HNSW_FOR_EACH_KIND"))
    assert tuple(kinds) == tuple(build.KINDS)
    for k in kinds:
        assert re.search(r"^#define HNSW_UNIT_" + k + r"\(DO, M\) ", text, flags=re.M), k


def test_metric_lists_agree(build):
    import hnswindex
    rows = _metric_rows()
    assert [(tag, name) for _, tag, name in rows] == list(build.METRICS)                  # content and order
    assert list(hnswindex.net_amd.bindings.METRICS.items()) == [(name, i) for i, (_, _, name) in enumerate(rows)]
    # the ids: M_* = HNSWDEV_* (device_backend.h), HNSWDEV_* = value (the ABI header); a row's id is its place in the list
    m_enum = dict(re.findall(r"\b(M_\w+) = (HNSWDEV_\w+)", (CSRC / "device_backend.h").read_text()))
    abi = {k: int(v) for k, v in re.findall(r"\b(HNSWDEV_[A-Z0-9_]+) = (\d+)", (ROOT / "include" / "hnsw_mi355x.h").read_text())}
    assert [abi[m_enum[mid]] for mid, _, _ in rows] == list(range(len(rows)))
    assert len(abi) == len(rows)                                                        # and the ABI has no metric the list lacks


def test_build_id_covers_the_table(build, monkeypatch):
    base = build.source_id()
    assert build.source_id() == base and len(base) == 64                                 # stable
    monkeypatch.setattr(build, "KINDS", build.KINDS[:-1] + ("multilayer2",))             # one unit's name and -D flag change
    changed = build.source_id()
    assert changed != base
    monkeypatch.setattr(build, "KINDS", build.KINDS[:-1])                                # a unit leaves the table
    assert build.source_id() not in (base, changed)
    monkeypatch.undo()
    assert build.source_id() == base
    # the one-unit diagnostic build has another table, and its id says so beyond the flag itself
    assert build.source_id(["-DHNSW_SINGLE_TU"]) != base
