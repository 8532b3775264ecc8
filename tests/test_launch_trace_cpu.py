"""ppt_amd.engine launches what tests/golden/launch_traces.json.gz recorded: for every case of the grid (shapes, operand precisions,
switch settings -- tests/golden/make_golden_traces.py) the launch sequence of vit_block_forward and of text_tower_forward /
text_tower_backward is recomputed on CPU stand-ins (tests/launch_trace.py) and compared with the recorded text.  No GPU needed."""
import difflib
import gzip
import hashlib
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import launch_trace as LT                     # noqa: E402

with gzip.open(os.path.join(HERE, "golden", "launch_traces.json.gz"), "rt") as _f:
    GOLDEN = json.load(_f)


def _check(fn, row):
    want = GOLDEN["traces"][row["trace"]]
    assert hashlib.sha1(want.encode()).hexdigest() == row["sha1"], "the fixture's own text does not match its SHA-1"
    got = LT.TRACERS[fn](row["case"])
    if got != want:
        diff = "\n".join(difflib.unified_diff(want.splitlines(), got.splitlines(), f"recorded at {GOLDEN['commit'][:12]}", "now", lineterm=""))
        pytest.fail(f"{fn} launches something else for {row['case']}:\n{diff}", pytrace=False)


def _ids(fn):
    return [f"{fn}-{i}" for i in range(len(GOLDEN["cases"][fn]))]


@pytest.mark.parametrize("row", GOLDEN["cases"]["vit_block"], ids=_ids("vit_block"))
def test_vit_block_forward_launches_the_recorded_sequence(row):
    _check("vit_block", row)


@pytest.mark.parametrize("row", GOLDEN["cases"]["text_tower"], ids=_ids("text_tower"))
def test_text_tower_launches_the_recorded_sequence(row):
    _check("text_tower", row)


def test_an_op_without_a_fake_raises():
    rec = LT.Recorder()
    with pytest.raises(AssertionError, match="no fake"):
        rec.fps
    assert rec.HALF is LT.real_ops.HALF and rec.split16_enabled() is False
