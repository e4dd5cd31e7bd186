"""Records tests/golden/frontend_refusals.json: what libsfmba_hip.so answers to every case of tests/frontend_refusal_cases.py.

    python tests/golden/make_frontend_refusals.py [path/to/libsfmba_hip.so]

The table is the record of one commit (the parent of the front-end API refactor): it is replayed against every later library by
tests/test_frontend_refusals_cpu.py and is not regenerated from the code under test.  No GPU is needed: a refusal for the arguments
comes back before the device check.  The script stops if a refused call changed an output array, or if a "valid" call was refused
for its arguments.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import frontend_refusal_cases as frc  # noqa: E402

SFMBA_OK, SFMBA_ERR_INVALID_ARG, SFMBA_ERR_NO_DEVICE = 0, 1, 2

# INVALID_ARG messages of the front-end entry points that no case reaches, and why
NOT_COVERED = [
    {"message": "depth_fuse: more than 65535 images in one call",
     "reason": "the poses of 65536 images are checked first: a 3 MB input array"},
    {"message": "depth_normals: more than 65535 images in one call",
     "reason": "the poses of 65536 images are checked first: a 3 MB input array"},
]


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(HERE)), "sfm-toy-library_amd", "csrc",
                                                              "libsfmba_hip.so")
    lib = ctypes.CDLL(os.path.abspath(path))
    have_gpu = lib.sfmba_device_count() > 0
    rows = []
    for e in frc.ENTRIES:
        rc, msg, _ = frc.invoke(lib, e, e.args())
        want = SFMBA_OK if (have_gpu or e.name in frc.HOST_ONLY) else SFMBA_ERR_NO_DEVICE
        assert rc == want, "%s: the valid call returned %d (%s)" % (e.name, rc, msg)
        for defect, overrides in e.cases:
            rc, msg, untouched = frc.invoke(lib, e, e.args(overrides))
            assert rc == SFMBA_ERR_INVALID_ARG, "%s, %s: rc %d (%s)" % (e.name, defect, rc, msg)
            assert untouched, "%s, %s: a refused call wrote to an output" % (e.name, defect)
            rows.append([e.name, defect, rc, msg])
    table = os.path.join(HERE, "frontend_refusals.json")
    if have_gpu:
        device_rows = []
        for name, defect, overrides in frc.DEVICE_CASES:
            e = frc.BY_NAME[name]
            rc, msg, untouched = frc.invoke(lib, e, e.args(overrides))
            assert rc == SFMBA_ERR_INVALID_ARG, "%s, %s: rc %d (%s)" % (name, defect, rc, msg)
            device_rows.append([name, defect, rc, msg, untouched])
    else:
        device_rows = json.load(open(table)).get("device_cases", []) if os.path.exists(table) else []

    def block(rows):
        return ",\n".join("  " + json.dumps(r) for r in rows)
    with open(table, "w") as f:          # one case per line
        f.write('{\n "columns": ["entry", "defect", "rc", "message"],\n "cases": [\n%s\n ],\n'
                ' "device_columns": ["entry", "defect", "rc", "message", "untouched"],\n "device_cases": [\n%s\n ],\n "not_covered": [\n%s\n ]\n}\n' %
                (block(rows), block(device_rows), block(NOT_COVERED)))
    print("%d cases, %d entry points, %d distinct messages" % (len(rows), len(frc.ENTRIES), len({r[3] for r in rows})))


if __name__ == "__main__":
    main()
