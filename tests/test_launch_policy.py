"""The launch policy over a sweep: what the introspection calls (backend_info, lane_segments, lane_starts,
lane_fixed_q, gap_screen) answer for every case of policy_sweep.py equals tests/golden/launch_policy.rec,
recorded by tests/golden/make_policy_golden.py from the build before the policy's code was last
rearranged. A change that is meant to move a rule's outcome re-records the file and says so; a refactor
leaves it alone. No device is needed."""
import json
import os

import numpy as np
import policy_sweep as ps
import pytest
from conftest import GOLDEN

GOLD = np.load(os.path.join(GOLDEN, "launch_policy.rec"))
VARIANTS = json.loads(str(GOLD["variants"]))
RECORD = GOLD["answers"]
KNOB_IDS = ["none"] + [f"{k}={v}" for k, v in ps.KNOBS]


def test_recorded_sweep_is_the_sweep():
    """The file answers exactly the module's cases, and those contain every value the policy's rules
    distinguish, each against the default of the others."""
    assert VARIANTS == ps.variants()
    assert tuple(GOLD["horizons"]) == ps.HORIZONS and tuple(GOLD["batches"]) == ps.BATCHES
    assert RECORD.shape == (len(VARIANTS), len(ps.HORIZONS), len(ps.BATCHES), ps.ANSWERS)
    assert len(str(GOLD["commit"])) >= 7
    base = dict(gap=0, backend=0, warm=0, udes_inside=0, q_unequal=0, knob=None)
    for axis, values in dict(gap=(0, 1), backend=(0, 1, 2), warm=(0, 1), udes_inside=(0, 1), q_unequal=(0, 1)).items():
        for x in values:
            assert {**base, axis: x} in VARIANTS
    for k, v in ps.KNOBS:
        assert {**base, "knob": [k, v]} in VARIANTS


@pytest.mark.parametrize("knob_id", KNOB_IDS)
def test_policy_answers_match_the_record(capi, knob, monkeypatch, knob_id):
    for name in ps.KNOB_NAMES:
        monkeypatch.delenv(name, raising=False)
    want = None if knob_id == "none" else [knob_id.split("=")[0], int(knob_id.split("=")[1])]
    if want:
        knob(*want)
    assert capi.load(test=True).f110qp_test_build() == 1
    n = 0
    for i, v in enumerate(VARIANTS):
        if v["knob"] != want:
            continue
        got = np.array(ps.answers(capi, v), np.int16)
        bad = np.argwhere((got != RECORD[i]).any(axis=2))
        assert bad.size == 0, (v, [(ps.HORIZONS[h], ps.BATCHES[b], got[h, b].tolist(), RECORD[i][h, b].tolist())
                                   for h, b in bad[:5]])
        n += 1
    assert n == (48 if want is None else 4)
