"""bzk_groth16_verify_batch without a device (ctx = NULL: the per-proof functions of bazuka_amd/csrc/bzk_pairing28.cuh over the host field, on host
threads) against the single call bzk_groth16_verify, element-wise, on a table of every class of row a verifier must tell apart; the key-level
failures, the argument refusals; and the same functions in their DEVICE-field instantiation, run on the CPU by the stand-alone program
tests/host/_pairing28_check (built by build() with the bound assertions of bzk_fp28.cuh on)."""
import os
import subprocess

import pytest

from bazuka_amd import lib as L
from oracle import pyref as pr
import verify_cases as V

HERE = os.path.dirname(os.path.abspath(__file__))


def test_device_field_instantiation_on_the_cpu():
    exe = os.path.join(HERE, "host", "_pairing28_check")
    assert os.path.exists(exe), "tests/host/_pairing28_check not built (build() compiles it)"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "all checks hold" in p.stdout and "FAIL" not in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    for what in ("e6_mul", "e12_mul", "e12_sqr", "e12_mul_by_014", "e12_inv", "e12_frob", "e12_cyc_sqr", "e12_cyc_exp_x", "final_exp",
                 "miller_one * m == four-pair multi_miller", "prepare_one: X equals double-and-add", "Y = 0 is degenerate", "T = Q is degenerate",
                 "T = -Q is degenerate"):
        assert "ok   " + what in p.stdout, what


@pytest.mark.parametrize("key", [0, 1])
def test_batch_equals_the_single_call_element_wise(key):
    vkb, n_inputs, rows, single = V.table(key)
    for seed in (1, 2):
        inputs, proofs, want, names = V.batch(key, len(rows), seed)
        got = L.host_groth16_verify_batch(vkb, inputs, n_inputs, proofs)
        assert got == want, [(n, g, w) for n, g, w in zip(names, got, want) if g != w]
    # the oracle's verifier agrees on the rows it can read
    vk = pr.vk_from_bytes(vkb)
    for (name, i, p), s in zip(rows, single):
        if name.startswith("valid") or name.startswith("wrong"):
            pub = [int.from_bytes(i[32 * k:32 * k + 32], "little") * pow(1 << 256, -1, pr.R_MOD) % pr.R_MOD for k in range(n_inputs)]
            assert bool(pr.groth16_verify(vk, pub, pr.proof_from_bytes(p))) == bool(s), name


def test_key_level_failures_give_all_zeros():
    vkb, n_inputs, rows, single = V.table(0)
    n = len(rows)
    inputs, proofs, want, _ = V.batch(0, n, 3)
    assert any(want)   # rows that verify under the sound key
    lib = L.load_library()
    zeros = bytes(n)
    # fewer inputs than IC entries (the same proofs, each with one scalar less)
    short = b"".join(inputs[32 * n_inputs * i:32 * n_inputs * (i + 1) - 32] for i in range(n))
    assert L.host_groth16_verify_batch(vkb, short, n_inputs - 1, proofs) == zeros
    assert L.host_groth16_verify_batch(vkb + bytes(1), inputs, n_inputs, proofs) == zeros          # trailing key bytes
    off_curve = vkb[:387] + bytes([vkb[387] ^ 1]) + vkb[388:]                                       # gamma.x tampered
    assert L.host_groth16_verify_batch(off_curve, inputs, n_inputs, proofs) == zeros
    for bad in (vkb + bytes(1), off_curve):
        assert L.groth16_verify(bad, inputs[:32 * n_inputs], proofs[:387]) is False                  # what the single call says there
    ok = L.C.create_string_buffer(b"\x07" * n, n)
    assert lib.bzk_groth16_verify_batch(None, off_curve, len(off_curve), inputs, n_inputs, proofs, n, ok) == 0 and ok.raw == zeros


def test_arguments():
    vkb, n_inputs, rows, single = V.table(0)
    inputs, proofs, want, _ = V.batch(0, 2, 4)
    lib = L.load_library()
    assert lib.bzk_groth16_verify_batch(None, None, 0, None, 0, None, 0, None) == 0                  # n = 0
    assert L.host_groth16_verify_batch(vkb, b"", n_inputs, b"") == b""
    ok = L.C.create_string_buffer(b"\x07" * 2, 2)
    E_ARG = -1
    for args in ((None, len(vkb), inputs, n_inputs, proofs, 2, ok), (vkb, len(vkb), None, n_inputs, proofs, 2, ok),
                 (vkb, len(vkb), inputs, n_inputs, None, 2, ok), (vkb, len(vkb), inputs, n_inputs, proofs, 2, None),
                 (vkb, 877, inputs, n_inputs, proofs, 2, ok)):
        assert lib.bzk_groth16_verify_batch(None, *args) == E_ARG, args[1:4]
    assert ok.raw == b"\x07" * 2                                                                       # nothing written
    assert lib.bzk_groth16_verify_batch_dev(None, vkb, len(vkb), inputs, n_inputs, proofs, 2, ok) == E_ARG   # the device form needs a context


def test_no_inputs():
    """n_inputs = 0 runs with a key whose IC has one entry: X = IC_0, finite or at infinity"""
    for vk0, proofs, single in V.no_input_keys():
        assert L.host_groth16_verify_batch(vk0, b"", 0, proofs) == single


def test_eighteen_inputs():
    vkb, n_inputs, inputs, proofs, single = V.wide_key()
    assert L.host_groth16_verify_batch(vkb, inputs, n_inputs, proofs) == single


def test_production_fixture_is_what_the_oracle_accepts():
    """tests/golden/groth16_production_case.json (the GPU test's production key, made once by the CPU oracle): the oracle's verifier and the single
    call accept the proof at its height and refuse it at another; the batched host path says the same"""
    vkb, inputs, other, proof = V.production_fixture()
    dec = lambda b: [int.from_bytes(b[32 * k:32 * k + 32], "little") * pow(1 << 256, -1, pr.R_MOD) % pr.R_MOD for k in range(5)]
    assert dec(inputs)[:3] == [456, 0, 123] and dec(other)[1] == 1
    vk = pr.vk_from_bytes(vkb)
    assert pr.groth16_verify(vk, dec(inputs), pr.proof_from_bytes(proof)) and not pr.groth16_verify(vk, dec(other), pr.proof_from_bytes(proof))
    assert L.groth16_verify(vkb, inputs, proof) is True and L.groth16_verify(vkb, other, proof) is False
    assert L.host_groth16_verify_batch(vkb, inputs + other, 5, proof * 2) == bytes([1, 0])
