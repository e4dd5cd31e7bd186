"""The "[sfmba <tag>] name value ..." lines the SFMBA_*_TIMING switches put on stderr (tools/*_bench.py parse them): one child
process calls every timed entry point once (tests/timing_lines_run.py); tags and field names, in order, are those recorded in
tests/golden/timing_lines.json, and every time is a finite number that is not negative."""
import json
import math
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "timing_lines.json")))["lines"]
# the units whose event array became a PhaseTimer: their copies in and out are real work on every call
CONVERTED = ("match", "match_l2", "pnp", "homography", "essential")


@pytest.fixture(scope="module")
def lines():
    sys.path.insert(0, HERE)
    import timing_lines_run
    env = dict(os.environ, **{s: "1" for s in timing_lines_run.SWITCHES})
    run = subprocess.run([sys.executable, os.path.join(HERE, "timing_lines_run.py")], env=env, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    out = []
    for line in run.stderr.splitlines():
        m = re.match(r"\[sfmba (\w+)\] (.*)", line)
        if m:
            tok = m.group(2).split()
            out.append((m.group(1), tok[0::2], [float(v) for v in tok[1::2]]))
    return out


@pytest.mark.gpu
def test_tags_and_field_names_are_the_recorded_ones(lines):
    assert [(tag, names) for tag, names, _ in lines] == [(g[0], g[1:]) for g in GOLDEN]


@pytest.mark.gpu
def test_every_time_is_finite_and_not_negative(lines):
    for tag, names, values in lines:
        for name, v in zip(names, values):
            if name.endswith("_ms"):
                assert math.isfinite(v) and v >= 0.0, (tag, name, v)


@pytest.mark.gpu
def test_the_converted_timers_see_the_upload_and_the_download(lines):
    seen = {tag: dict(zip(names, values)) for tag, names, values in lines}
    for tag in CONVERTED:
        assert seen[tag]["upload_ms"] > 0.0 and seen[tag]["download_ms"] > 0.0, (tag, seen[tag])
