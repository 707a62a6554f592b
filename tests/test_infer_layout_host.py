"""CPU: the byte layout of the inference workspace and the int layout of its table slot are what they were before both were declared
in one place (csrc/infer_workspace.h).  tests/golden/infer_layout_golden.json holds what that earlier library returned from
sir_model_workspace_bytes / sir_model_workspace_offsets and what the table arithmetic then kept in ops.py gave: odd widths, tab2
with and without its 8-byte alignment bump, S = 1 and S = 256, and the batch limit (a workspace above 2^31 bytes).  No call here
needs a device."""
import ctypes as C
import json
import os

import pytest

from sir_amd import _native

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "infer_layout_golden.json")))
TABLES = ("e0", "d1", "d3", "rows", "tab2", "tab3", "record", "nonfinite", "ints")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.lib()


def test_golden_covers_the_shape_set():
    # (2, 16) is there for the alignment bump of tab2: the count in front of it is n (3 + k2max + k3max + S) + 2 ints with
    # n = B + 1, and none of the other shapes makes that odd
    assert [(g["batch"], g["t_frames"]) for g in GOLDEN["shapes"]] == [
        (1, 8), (1, 9), (2, 15), (3, 16), (5, 24), (4, 200), (7, 201), (256, 200), (17, 2055), (1041, 24), (65535, 8), (2, 16)]
    assert GOLDEN["refused"] == [[2, 2056], [0, 200]]
    by_shape = {(g["batch"], g["t_frames"]): g for g in GOLDEN["shapes"]}
    assert by_shape[(4, 200)]["bytes"] == 19345152 and by_shape[(4, 200)]["offsets"][7] == 4769792
    assert by_shape[(256, 200)]["bytes"] == 290901248 and by_shape[(256, 200)]["offsets"][7] == 250431488
    assert by_shape[(4, 200)]["tables"] == {"e0": 0, "d1": 4, "d3": 9, "rows": 116, "tab2": 242, "tab3": 374, "record": 446,
                                            "nonfinite": 448, "ints": 452}
    assert by_shape[(65535, 8)]["bytes"] > 2 ** 31
    assert {g["tables"]["tab2"] - (g["tables"]["rows"] + 1 + (g["batch"] + 1) * (g["t_frames"] // 8)) for g in GOLDEN["shapes"]} == {0, 1}


@pytest.mark.parametrize("g", GOLDEN["shapes"], ids=lambda g: f"{g['batch']}x{g['t_frames']}")
def test_layout_is_the_recorded_one(lib, g):
    b, t = g["batch"], g["t_frames"]
    assert lib.sir_model_workspace_bytes(None, b, t, 0) == g["bytes"]
    offs = (C.c_size_t * 16)()
    assert lib.sir_model_workspace_offsets(None, b, t, 0, offs, 16) == 16
    assert list(offs) == g["offsets"]
    vals = (C.c_size_t * 10)()
    assert lib.sir_model_infer_table_offsets(None, b, t, vals, 10) == 10
    assert dict(zip(TABLES, vals)) == g["tables"]
    assert vals[9] == 7
    assert g["offsets"][7] + 4 * g["tables"]["ints"] <= g["offsets"][8]       # the tables end inside their slot


@pytest.mark.parametrize("b,t", [tuple(s) for s in GOLDEN["refused"]])
def test_refused_shapes_stay_refused(lib, b, t):
    buf = (C.c_size_t * 16)()
    assert lib.sir_model_workspace_bytes(None, b, t, 0) == 0
    assert lib.sir_model_workspace_offsets(None, b, t, 0, buf, 16) == _native.SIR_EINVAL
    assert lib.sir_model_infer_table_offsets(None, b, t, buf, 10) == _native.SIR_EINVAL
