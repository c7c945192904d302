"""The library's A/B knobs (SPECTAVI_CASCADE_MFMA / MFMA4 / GROUP / QHIST / RU, SPECTAVI_L1K2_Q): each
setting runs in a fresh child process (tests/knob_child.py) with only that knob added to its
environment -- SPECTAVI_L1K2_Q is read once per process -- and the child checks, through the
library's plan, that the knob changed the launch before it compares against the oracle."""
import os
import subprocess
import sys

import pytest

from tests.knob_child import SETTINGS

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "knob_child.py")
CHILD_TIMEOUT_S = 60


def test_static_knobs_in_child_processes():
    """One child per setting, one at a time.  A child that fails, dies on a signal or overruns its
    time limit fails the test with its output, and no further child is started."""
    base = {k: v for k, v in os.environ.items()
            if not k.startswith(("SPECTAVI_CASCADE_", "SPECTAVI_L1K2_", "SPECTAVI_ANN_"))}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [CHILD]
    for setting, (knobs, _, _) in SETTINGS.items():
        env = dict(base, **knobs)
        try:
            r = subprocess.run(cmd + [setting], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                               text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired as e:
            out = e.output.decode(errors="replace") if isinstance(e.output, bytes) else (e.output or "")
            pytest.fail("knob setting %s %s: no result within %d s\n%s" % (setting, knobs, CHILD_TIMEOUT_S, out))
        if r.returncode != 0:
            pytest.fail("knob setting %s %s: child exited with %d\n%s" % (setting, knobs, r.returncode, r.stdout))
        assert ("all ok: %s" % setting) in r.stdout, r.stdout
