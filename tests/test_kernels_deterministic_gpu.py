"""Kernel parity in the deterministic mode.  PHX_DETERMINISTIC=1 is read once per process and re-plans the launches of a dozen sites of
libphx (see tests/det_kernels_worker.py for the list and for which check reaches which); tests/test_kernels_gpu.py runs with the
variable unset, and the model-level tests of the mode compare two runs with each other -- a result that is wrong the same way twice
passes them.  Here ONE worker process runs the kernel parity checks against the float64 oracle with the variable set; every check is
a test of its own, and one more test makes sure that the worker ran them all and ended cleanly."""
import os
import subprocess
import sys

import pytest

from tests.det_kernels_worker import CHECKS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER_TIMEOUT_S = 120           # the worker takes about 4 s, imports included (its DONE line): a hang must not cost a model worker's 900 s


@pytest.fixture(scope="module")
def report():
    env = dict(os.environ, PYTHONPATH=ROOT, PHX_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "det_kernels_worker.py")], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=WORKER_TIMEOUT_S)
    checks, done, abort = {}, None, None
    for line in r.stdout.splitlines():
        w = line.split(None, 3)
        if len(w) >= 3 and w[0] == "CHECK":
            checks[w[1]] = (w[2], w[3] if len(w) > 3 else "")
        elif len(w) >= 3 and w[0] == "DONE":
            done = (int(w[1]), float(w[2]))
        elif w and w[0] == "ABORT":
            abort = line
    return dict(rc=r.returncode, checks=checks, done=done, abort=abort, tail=r.stdout[-2000:] + r.stderr[-3000:])


@pytest.mark.parametrize("name", CHECKS)
def test_deterministic_kernel_check(report, name):
    assert name in report["checks"], "the worker did not reach this check: %s" % (report["abort"] or report["tail"])
    verdict, message = report["checks"][name]
    assert verdict == "PASS", message


def test_worker_ran_every_check_and_ended_cleanly(report):
    assert report["rc"] == 0 and report["abort"] is None, report["abort"] or report["tail"]
    assert report["done"] is not None and report["done"][0] == len(CHECKS) == len(report["checks"]), (report["done"], len(CHECKS))
