"""pytest plugin: record what every tests/_parity.py ``close(..., mag=M)``
comparison of a run measured, quiet or not, without touching the comparison.

    PYTHONPATH=tools DDQ_PARITY_FIGURES=figures.tsv pytest -p parity_record -m gpu
    tools/parity_table.py figures.tsv

It wraps ``_parity.close`` before the test modules import it.  One
tab-separated record per comparison with a non-zero reference: test id,
tensor (close's ``tensor``; without one the label with its numbers replaced by
N), label, pass/FAIL, element count, normwise error, max relative error above
the 1e-2 floor, max absolute error per max|ref| below it, p50 / p99 / p100
relative error.
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import _parity  # noqa: E402

_close = _parity.close


def recording_close(gpu, ref, *args, **kw):
    status = "pass"
    try:
        return _close(gpu, ref, *args, **kw)
    except AssertionError:
        status = "FAIL"
        raise
    finally:
        path = os.environ.get("DDQ_PARITY_FIGURES")
        r = np.asarray(ref, np.float64)
        if path and kw.get("mag") is not None and kw.get("strict", True) and r.size and np.any(r):
            what = kw.get("what", "") or "-"
            tensor = kw.get("tensor") or re.sub(r"\d+", "N", what)
            floor = _parity.OVERRIDES.get(kw.get("tensor"), {}).get("floor", _parity.ELEM_FLOOR)
            nerr, rel_hi, abs_lo, pct = _parity.error_figures(gpu, r, floor)
            with open(path, "a") as f:
                f.write("%s\t%s\t%s\t%s\t%d\t%.4g\t%.4g\t%.4g\t%.4g\t%.4g\t%.4g\n" % (
                    os.environ.get("PYTEST_CURRENT_TEST", "-").split(" ")[0], tensor, what,
                    status, r.size, nerr, rel_hi, abs_lo, *pct))


_parity.close = recording_close
