"""The device back end of the witness builders (bzk_mpn_set_device: DevBatch, SigBatch) against the host back end on the queues of
tests/mpn_builder_cases.py, builder call by builder call: the same work bytes (withdraw_signed: the same z), the same root, the same
transactions accepted.  The host side is pinned by tests/test_mpn_builder_cpu.py."""
import pytest

import mpn_builder_cases as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(M.CASES))
def test_device_builder_equals_host_builder_call_by_call(bzk, name):
    host, dev = M.run(name), M.run(name, dev=bzk)
    assert len(host) == len(dev)
    for k, (a, b) in enumerate(zip(host, dev)):
        assert (b["accepted"], b["rejected"]) == (a["accepted"], a["rejected"]), f"call {k}"
        assert b["root"] == a["root"], f"call {k}: root"
        assert b["bytes"] == a["bytes"], f"call {k}: work bytes"
