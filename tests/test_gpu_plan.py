"""The device facts recorded beside the golden plan images (tests/golden/plan_images.json) are this device's:
without this, tests/test_plan_host.py would pin the planner to the layout of a device nobody has."""
import ctypes as C
import json

import pytest

from sparsematrixvbcs_amd import _lib as L

from .test_plan_host import GOLDEN, facts_dict

pytestmark = pytest.mark.gpu


def test_device_facts_are_the_recorded_ones():
    f = L.vbcx_facts()
    L.check(L.lib().vbcx_device_facts(0, C.byref(f)), "vbcx_device_facts")
    have, want = facts_dict(f), json.loads(GOLDEN.read_text())["facts"]
    assert have == want, f"device facts {have} differ from the recorded {want}"
