"""The second deferral level ON THE DEVICE: an instance synthesized with BZK_SYNTH_DEFER_SIG leaves the EdDSA gadget's ladders and tail to
witfill.hip's wf_ladder_kernel (the points, one inversion per ladder) and wf_ladder_fill_kernel (the slots).  The device-filled arrays read back must be
the independent restatement's fixtures, and the proofs the oracle prover's bytes.  The CPU side of the same ops: tests/test_defer_sig_cpu.py."""
import hashlib
import json
import os

import pytest

import r1cs_scenarios as S
from bazuka_amd import lib as L
from bazuka_amd import worker as W
from mock_node import MockNode
from test_defer_sig_cpu import _bad_update, hole_masks, poison_holes
from test_gpu_defer import _setup, oracle_prove
from test_gpu_worker import ALICE, _block_of_works, _native
from util import fr_bytes, fr_list

pytestmark = pytest.mark.gpu
FIX = json.load(open(os.path.join(S.G, "r1cs_sha256.json")))


@pytest.mark.parametrize("name", ["update_3_3_1", "withdraw_3_3_1", "update_15_3_2", "withdraw_15_3_3", "update_15_3_4"])
def test_device_filled_sig_arrays_equal_the_independent_restatements_fixtures(bzk, name):
    if name == "update_15_3_4" and os.environ.get("BZK_TEST_PRODUCTION_BYTES", "1") == "0":
        pytest.skip("BZK_TEST_PRODUCTION_BYTES=0")
    from bazuka_amd import Bzk
    dec = L.MpnWork.decode(S.make_work(name))
    d = dec.synthesize(S.PROVER, defer="sig")
    info = d.defer_info()
    assert info["deferred"] == 1 and info["filled"] == 0
    assert (d.n_in, d.n_aux, d.n_constraints) == (FIX[name]["n_in"], FIX[name]["n_aux"], FIX[name]["n_constraints"])
    # the host arrays' holes are overwritten with a value no fill writes (test_defer_sig_cpu.hole_masks): whatever matches below was computed on the device
    poison_holes(d, hole_masks(dec, "sig"))
    for k in ("z", "az", "bz", "cz"):
        assert hashlib.sha256(d.raw(k)).hexdigest() != FIX[name]["sha256"][k], k
    stager = Bzk(bzk.device)
    h = stager.r1cs_stage(d)
    stager.staged_wait(h)              # BZK_E_UNSAT would raise here: every deferred row holds, the signatures included
    for i, k in enumerate(("z", "az", "bz", "cz")):
        got = stager.staged_read(h, i)
        assert len(got) == len(d.raw(k)), k
        assert hashlib.sha256(got).hexdigest() == FIX[name]["sha256"][k], (name, k)
        del got
    assert d.defer_info()["filled"] == 0
    stager.staged_free(h)
    stager.close()
    d.free()


@pytest.mark.parametrize("name", ["update_3_3_1", "update_15_3_2", "withdraw_15_3_3"])
def test_sig_deferred_proof_is_the_oracle_provers_and_the_plain_paths(bzk, co, name):
    dec = L.MpnWork.decode(S.make_work(name))
    r, ph, vkb = _setup(bzk, dec)
    rs = fr_bytes(fr_list(2, 917))
    want = oracle_prove(co, bzk, ph, r, rs)
    assert bzk.groth16_prove(ph, *(r.view(k) for k in ("z", "az", "bz", "cz")), rs[:32], rs[32:]) == want
    d = dec.synthesize(S.PROVER, defer="sig")
    assert d.defer_info()["deferred"] == 1
    assert bzk.groth16_prove_r1cs(ph, d, rs[:32], rs[32:]) == want
    assert d.defer_info()["filled"] == 0
    assert L.groth16_verify(vkb, r.view("z")[32:32 * r.n_in], want)
    bzk.params_free(ph)


@pytest.mark.parametrize("which", ["s", "r"])
def test_a_bad_signature_gives_unsat_from_the_device(bzk, which):
    dec = L.MpnWork.decode(_bad_update(which))
    good = L.MpnWork.decode(S.make_work("update_3_3_1"))
    _, ph, _ = _setup(bzk, good)   # same circuit shape: the CRS of the good work
    d = dec.synthesize(S.PROVER, threads=2, defer="sig")
    assert d.defer_info()["deferred"] == 1
    rs = fr_bytes(fr_list(2, 918))
    with pytest.raises(L.BzkError) as e:
        bzk.groth16_prove_r1cs(ph, d, rs[:32], rs[32:])
    assert e.value.status == L.BZK_E_UNSAT, e.value
    bzk.params_free(ph)


def test_workers_with_the_signature_gadget_deferred(bzk):
    """--defer-sig: both workers synthesize with BZK_SYNTH_DEFER_SIG and prove through bzk_groth16_prove_r1cs - all three kinds of work of a block,
    every proof checked with the work's own key before posting and accepted by the mock node's oracle pairing check"""
    seed = "native-dev"
    keys = W.DevSetup(bzk, {k: W.dev_toxic(seed, k) for k in range(3)})
    vks = [keys.keys(k, 3, 3, 1)[1] for k in range(3)]
    blobs = _block_of_works(vks)
    node = MockNode(blobs)
    try:
        alice = W.Worker(bzk, ALICE, ("127.0.0.1", node.port), keys, self_check=True, defer="sig")
        assert alice.run_once() == len(blobs)
        assert alice.stats["unsat"] == 0 and alice.stats["self_check_failed"] == 0 and node.solved == {k: ALICE for k in blobs}
    finally:
        node.close()
    node = MockNode(blobs)
    try:
        st, err = _native(["--node", f"127.0.0.1:{node.port}", "--address", ALICE.hex(), "--dev-toxic", seed, "--slots-per-device", "2", "--defer-sig",
                           "--self-check", "--rounds", "1", "--poll", "0.05"])
        assert st["proved"] == len(blobs) and st["accepted"] == len(blobs) and st["self_check_failed"] == 0 and st["errors"] == 0, (st, err)
        assert node.solved == {k: ALICE for k in blobs}
    finally:
        node.close()
        keys.close()
