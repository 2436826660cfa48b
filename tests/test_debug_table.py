"""--debug-scores on the host side (no GPU): the Markdown renderer against the reference's own expected table
(tests/golden/debug_scores.json: the ten plugins' scores for four nodes and the string frameworkext/debug_test.go expects),
and the ABI surface of kg_debug_topn (row layout, exported symbol, plugin column names)."""
import ctypes
import json
import os

from koordinator_amd import abi, framework as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "debug_scores.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _rows(g):
    """Plain-Python rows in the reference's order: the totals summed per node, sorted descending (debug.go:66-75;
    the four totals are distinct, so the unstable sort has one outcome)."""
    names = sorted(g["plugin_scores"])
    cols = dict(enumerate(names))
    rows = [{"node_idx": i, "total": sum(g["plugin_scores"][p][i] for p in names),
             "plugin": [g["plugin_scores"][p][i] for p in names]} for i in range(len(g["nodes"]))]
    rows.sort(key=lambda r: -r["total"])
    return rows[:g["topn"]], cols


def test_render_reproduces_reference_markdown():
    g = _golden()
    rows, cols = _rows(g)
    assert [r["total"] for r in rows] == g["expected_totals"] == [577, 574, 541, 487]
    out = F.render_debug_table(rows, cols, g["pod_ref"], g["nodes"])
    assert out == g["expected_markdown"]


def test_render_takes_device_rows_and_sorts_plugin_names():
    import numpy as np
    rows = np.zeros(2, dtype=abi.TOPN_ROW_DTYPE)
    rows["node_idx"] = [3, 1]
    rows["total"] = [150, 120]
    rows["plugin"][:] = -1
    rows["plugin"][:, abi.PL_FIT] = [90, 70]
    rows["plugin"][:, abi.PL_LOADAWARE] = [60, 50]
    cols = {abi.PL_FIT: F.PLUGIN_COLUMNS[abi.PL_FIT], abi.PL_LOADAWARE: F.PLUGIN_COLUMNS[abi.PL_LOADAWARE]}
    out = F.render_debug_table(rows, cols, "ns/p", ["n0", "n1", "n2", "n3"])
    assert out.split("\n") == ["| # | Pod | Node | Score | LoadAwareScheduling | NodeResourcesFit |",
                               "| --- | --- | --- | ---:| ---:| ---:|",
                               "| 0 | ns/p | n3 | 150 | 60 | 90 |",
                               "| 1 | ns/p | n1 | 120 | 50 | 70 |"]


def test_plugin_columns_name_every_kg_pl():
    assert F.PLUGIN_COLUMNS == {abi.PL_FIT: "NodeResourcesFit", abi.PL_LOADAWARE: "LoadAwareScheduling",
                                abi.PL_NUMA: "NodeNUMAResource", abi.PL_DEVICESHARE: "DeviceShare",
                                abi.PL_RESERVATION: "Reservation", abi.PL_TAINT: "TaintToleration",
                                abi.PL_NODE_AFFINITY: "NodeAffinity",
                                abi.PL_BALANCED: "NodeResourcesBalancedAllocation",
                                abi.PL_IMAGE_LOCALITY: "ImageLocality"}
    assert max(F.PLUGIN_COLUMNS) < abi.PL_COLUMNS


def test_topn_row_layout_and_symbol():
    lib = abi.load_library()
    assert abi.ABI_VERSION == 18 and lib.kg_abi_version() == 18
    assert abi.TOPN_ROW_DTYPE.itemsize == lib.kg_abi_struct_size(11) == 16 + 8 * abi.PL_COLUMNS
    assert abi.STRUCT_DTYPES[11] is abi.TOPN_ROW_DTYPE
    assert "kg_debug_topn" in abi.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(abi.LIB_PATH), "kg_debug_topn")


def test_null_arguments_rejected_without_device():
    """kg_debug_topn rejects null arguments before touching the engine (the topn range needs an engine: GPU file)."""
    lib = abi.load_library()
    assert lib.kg_debug_topn(None, None, 10, None, None, None) == abi.E_INVALID
