"""The argument refusals that a front-end unit finds only after the device is open (DEVICE_CASES of tests/frontend_refusal_cases.py):
return code, sfmba_last_error() text and whether the outputs stayed untouched, as recorded in tests/golden/frontend_refusals.json."""
import json
import os

import pytest

import frontend_refusal_cases as frc

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = json.load(open(os.path.join(HERE, "golden", "frontend_refusals.json")))["device_cases"]


def test_the_table_names_every_device_case():
    assert [(r[0], r[1]) for r in ROWS] == [(name, defect) for name, defect, _ in frc.DEVICE_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=lambda r: r[0][6:])
def test_device_side_refusal_is_the_recorded_one(row):
    from sfm_toy_library_amd import capi
    name, defect, rc, message, untouched = row
    e = frc.BY_NAME[name]
    overrides = {(n, d): o for n, d, o in frc.DEVICE_CASES}[(name, defect)]
    assert frc.invoke(capi.lib(), e, e.args(overrides)) == (rc, message, untouched)
