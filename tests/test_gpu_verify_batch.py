"""bzk_groth16_verify_batch / _dev on the GPU (bazuka_amd/csrc/verify.hip: g16v_prepare_kernel, g16v_miller_kernel, g16v_finalexp_kernel, one lane
per proof) against the single host call bzk_groth16_verify, element-wise, on the case tables of tests/verify_cases.py: refused, dead-pair and
verifying lanes share wavefronts."""
import json
import os

import pytest

from bazuka_amd import lib as L
import verify_cases as V

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("key", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_case_table(bzk, key, n):
    vkb, n_inputs, rows, single = V.table(key)
    inputs, proofs, want, names = V.batch(key, n, 100 + n)
    got = bzk.groth16_verify_batch(vkb, inputs, n_inputs, proofs)
    assert got == want, [(i, nm, g, w) for i, (nm, g, w) in enumerate(zip(names, got, want)) if g != w]
    if n >= len(rows):
        assert sum(want) >= 4 and want.count(0) >= 8


def test_dev_form_and_back_to_back_calls(bzk):
    import torch
    from util import to_dev
    n = 65
    for key in (0, 1, 0):   # a second and a third call on one context: the workspace is reused, the key's tables are uploaded again
        vkb, n_inputs, rows, single = V.table(key)
        inputs, proofs, want, names = V.batch(key, n, 7 + key)
        din, dpr = to_dev(inputs), to_dev(proofs)
        ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        bzk.groth16_verify_batch_dev(vkb, din, n_inputs, dpr, n, ok)
        assert bytes(ok.cpu().numpy().tobytes()) == want, key
        assert bzk.groth16_verify_batch(vkb, inputs, n_inputs, proofs) == want, key


def test_key_level_failures_and_arguments(bzk):
    vkb, n_inputs, rows, single = V.table(0)
    n = len(rows)
    inputs, proofs, want, _ = V.batch(0, n, 3)
    assert any(want)
    off_curve = vkb[:387] + bytes([vkb[387] ^ 1]) + vkb[388:]
    assert bzk.groth16_verify_batch(off_curve, inputs, n_inputs, proofs) == bytes(n)
    assert bzk.groth16_verify_batch(vkb + bytes(1), inputs, n_inputs, proofs) == bytes(n)
    lib = L.load_library()
    assert lib.bzk_groth16_verify_batch(bzk.h, None, 0, None, 0, None, 0, None) == 0
    ok = L.C.create_string_buffer(b"\x07" * n, n)
    assert lib.bzk_groth16_verify_batch(bzk.h, vkb, len(vkb), inputs, n_inputs, None, n, ok) == -1 and ok.raw == b"\x07" * n
    assert lib.bzk_groth16_verify_batch(bzk.h, vkb, 877, inputs, n_inputs, proofs, n, ok) == -1 and ok.raw == b"\x07" * n


def test_more_than_sixteen_inputs_take_the_host_threads(bzk):
    import torch
    from util import to_dev
    vkb, n_inputs, inputs, proofs, single = V.wide_key()
    assert bzk.groth16_verify_batch(vkb, inputs, n_inputs, proofs) == single
    ok = torch.full((3,), 7, dtype=torch.uint8, device="cuda")
    din, dpr = to_dev(inputs), to_dev(proofs)
    torch.cuda.synchronize()
    bzk.groth16_verify_batch_dev(vkb, din, n_inputs, dpr, 3, ok)
    assert bytes(ok.cpu().numpy().tobytes()) == single


def test_no_inputs(bzk):
    for vk0, proofs, single in V.no_input_keys():
        assert bzk.groth16_verify_batch(vk0, b"", 0, proofs) == single


def test_production_key(bzk):
    """the five-input production shape mpn_update_empty(3, 3, 1, ...): accepted at its height, refused at another, refused under each of the
    reference's three hard-coded keys"""
    vkb, inputs, other, proof = V.production_fixture()
    assert bzk.groth16_verify_batch(vkb, inputs + other + inputs, 5, proof * 3) == bytes([1, 0, 1])
    G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    for hexvk in json.load(open(os.path.join(G, "reference_vectors.json")))["verifying_keys_bincode_hex"]:
        assert bzk.groth16_verify_batch(bytes.fromhex(hexvk), inputs + other, 5, proof * 2) == bytes(2)


def test_round_crossing(bzk):
    """one call of 2^16 + 65 proofs: a second round reuses the slab; the expected vector comes from the table by index"""
    vkb, n_inputs, rows, single = V.table(0)
    n = (1 << 16) + 65
    inputs, proofs, want, _ = V.batch(0, n, 11)
    got = bzk.groth16_verify_batch(vkb, inputs, n_inputs, proofs)
    assert got[-65:] == want[-65:]
    assert got == want
