"""The host back end of the witness builders (bazuka_amd/csrc/mpn.hip: one acceptance walk per kind over HostTrees) on the queues of
tests/mpn_builder_cases.py: per builder call the work holds exactly the transactions the hand-written verdicts accept, and its bytes and the
root it leaves are the ones recorded from the host builder before the walks were unified (tests/golden/mpn_builder_cases.json)."""
import pytest

import mpn_builder_cases as M


@pytest.mark.parametrize("name", list(M.CASES))
def test_host_builder_accepts_what_the_rules_accept(name):
    got, want = M.run(name), M.expected_batches(name)
    assert len(got) == len(want)
    for k, (b, (accepted, rejected)) in enumerate(zip(got, want)):
        if isinstance(b["accepted"], list):
            assert b["accepted"] == accepted, f"call {k}"
        else:
            assert (b["accepted"], b["rejected"]) == (len(accepted), rejected), f"call {k}"


@pytest.mark.parametrize("name", list(M.CASES))
def test_host_builder_reproduces_the_recorded_works_and_roots(name):
    assert M.digest(M.run(name)) == M.recorded()[name]


def test_every_queue_outlasts_one_batch_and_names_its_transactions():
    for name, (kind, _, _, queue) in M.CASES.items():
        assert len(M.expected_batches(name)) >= 2, name
        amounts = [args[M.AMOUNT_AT[kind]] for args, _, _ in queue]
        assert len(set(amounts)) == len(amounts), name
