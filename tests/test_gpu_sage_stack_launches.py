"""The fused GraphSage stack node issues exactly the launches recorded in tests/golden/sage_stack_launches.json, and the DiffPool and
base encoders' forward + backward exactly those in tests/golden/diffpool_launches.json: per configuration of
scripts/record_stack_launches.py (every switch flipped once; the head, readout, node and pair routes; the shapes that steer the
fallback branches; the encoders' final_dim, pooling, masking and per-graph routes) the same entry points, dispatched kernels and
canonical arguments in the same order, and — where the recorder found them reproducible — the same bits in the outputs and gradients.

What the files are for: a refactor of two_stage_gnn_amd/sage_stack.py or dense_encoders.py (or of the host code around them) must
leave this test AND the golden files untouched.  A change that alters a launch sequence on purpose re-records the goldens from its
own tree (`python scripts/record_stack_launches.py`, twice: the second time with `--previous` of the first) and shows the diff of the
golden files in its description."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import record_stack_launches as rec  # noqa: E402

GOLDEN = {}
for _family, _fname in rec.GOLDENS.items():
    with open(os.path.join(rec.GOLDEN_DIR, _fname)) as _f:
        GOLDEN[_family] = json.load(_f)
CONFIGS = rec.configurations(None)


def test_golden_covers_every_configuration():
    for family in rec.GOLDENS:
        assert list(GOLDEN[family]) == [c["name"] for c in rec.configurations(family)], family


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS, ids=[c["name"] for c in CONFIGS])
def test_launches_equal_the_record(cfg):
    want = GOLDEN[cfg.get("family", "sage_stack")][cfg["name"]]
    got = json.loads(json.dumps(rec.record(cfg)))
    for i, (a, b) in enumerate(zip(got["launches"], want["launches"])):
        if a != b:
            print("first differing launch: #%d\n  now     : %s\n  recorded: %s" % (i, a, b))
            break
    else:
        if len(got["launches"]) != len(want["launches"]):
            i = min(len(got["launches"]), len(want["launches"]))
            side, longer = ("now", got) if len(got["launches"]) > i else ("recorded", want)
            print("first differing launch: #%d, %s only: %s" % (i, side, longer["launches"][i]))
    assert [r[0] for r in got["launches"]] == [r[0] for r in want["launches"]]
    assert got["launches"] == want["launches"]
    if "digest" in want:
        assert got["digest"] == want["digest"], "same launches, other bits in the outputs or gradients"
