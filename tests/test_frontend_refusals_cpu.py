"""Every argument refusal of the front-end entry points (csrc/api_frontend.hip) against the table recorded in
tests/golden/frontend_refusals.json: the same return code and the same sfmba_last_error() text, byte for byte, and no output
array written.  A refusal comes back before the device check, so this runs with and without a GPU; the one valid call per entry
point gets as far as the device (SFMBA_ERR_NO_DEVICE without one, SFMBA_OK with one)."""
import json
import os

import pytest

import frontend_refusal_cases as frc

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = json.load(open(os.path.join(HERE, "golden", "frontend_refusals.json")))
CASES = [dict(zip(TABLE["columns"], row)) for row in TABLE["cases"]]
SFMBA_OK, SFMBA_ERR_NO_DEVICE = 0, 2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_hip()
    from sfm_toy_library_amd import capi
    return capi.lib()


def test_the_table_and_the_case_list_name_the_same_cases():
    assert [(r["entry"], r["defect"]) for r in CASES] == [(e.name, d) for e in frc.ENTRIES for d, _ in e.cases]
    assert len(frc.ENTRIES) == 23 and all(e.cases for e in frc.ENTRIES)


@pytest.mark.parametrize("row", CASES, ids=lambda r: "%s-%s" % (r["entry"][6:], r["defect"].replace(" ", "_")[:48]))
def test_refusal_is_the_recorded_one_and_writes_nothing(lib, row):
    e = frc.BY_NAME[row["entry"]]
    rc, msg, untouched = frc.invoke(lib, e, e.args(dict(e.cases)[row["defect"]]))
    assert (rc, msg) == (row["rc"], row["message"])
    assert untouched


@pytest.mark.parametrize("name", [e.name for e in frc.ENTRIES])
def test_the_valid_call_reaches_the_device(lib, name):
    e = frc.BY_NAME[name]
    rc, msg, _ = frc.invoke(lib, e, e.args())
    want = SFMBA_OK if (lib.sfmba_device_count() > 0 or name in frc.HOST_ONLY) else SFMBA_ERR_NO_DEVICE
    assert rc == want, msg
