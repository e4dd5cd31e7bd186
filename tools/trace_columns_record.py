"""Runs tests/test_gpu_trace_columns.py on the GPU and writes the worst measured / bar per case, column and precision (the test's WORST)
to a file: python tools/trace_columns_record.py [profiles/trace_columns.txt].  The numbers are a record of what was measured; the bars
are derived in tests/trace_row_check.py and are not to be moved on the strength of this file."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "trace_columns.txt")
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_trace_columns.py")])
    worst = sys.modules["test_gpu_trace_columns"].WORST
    lines = ["# tests/test_gpu_trace_columns.py: worst measured / bar per case, column and precision (pytest exit code %d)" % int(rc),
             "# a column marked (not held) is printed by the test, not asserted: its bar is wider than 1e-6 |rho| (fp64) / 1e-3 |rho| (F32J)",
             "%-14s %-5s %-34s %s" % ("case", "prec", "column", "measured / bar")]
    for (case, column, prec), v in sorted(worst.items()):
        lines.append("%-14s %-5s %-34s %.3g" % (case, prec, column, v))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
