"""The case tables of the batched Groth16 verifier's tests (tests/test_verify_batch_cpu.py, tests/test_gpu_verify_batch.py): per oracle-made key
a list of (name, inputs, proof) rows of every class a verifier must tell apart, and the list of what the SINGLE call bzk_groth16_verify says
about each - the batched call must repeat it element-wise.  Keys, proofs and the single-call verdicts are computed once per session."""
import functools
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # `python tests/verify_cases.py` finds the package as the suite does
from bazuka_amd import lib as L
from oracle import pyref as pr
from util import fr_bytes, fr_list, log2_ceil, r1cs_to_csr, synth_r1cs

KEYS = ((40, 3), (300, 6))   # (multiplications, n_in) of synth_r1cs: n_in - 1 public inputs


def vk_bytes(params):
    return params["vk"] + (len(params["ic"]) // 97).to_bytes(8, "little") + params["ic"]


@functools.lru_cache(maxsize=None)
def _proved(n_mul, n_in):
    from oracle import coracle as co
    co.build()
    co.lib()
    r1 = synth_r1cs(n_mul, n_in=n_in, seed=500 + n_mul)
    A, B, Cm = r1cs_to_csr(co, r1)
    params = co.groth16_setup(A, B, Cm, r1["n_in"], r1["n_aux"], log2_ceil(len(r1["rows"])), fr_bytes(fr_list(5, 77)))
    zb = fr_bytes(r1["z"])
    az, bz, cz = co.r1cs_eval(A, B, Cm, zb)
    proofs = []
    for seed in (9, 10):
        rs = fr_bytes(fr_list(2, seed))
        proofs.append(co.groth16_prove(params, zb, az, bz, cz, rs[:32], rs[32:]))
    return vk_bytes(params), r1["z"][1:n_in], proofs


def _raise(b48: bytes, by: int) -> bytes:
    return (int.from_bytes(b48, "little") + by).to_bytes(len(b48), "little")


@functools.lru_cache(maxsize=None)
def table(key_index):
    """(vk, n_inputs, rows, single): rows = [(name, inputs, proof)], single = [bzk_groth16_verify(vk, inputs, proof) per row]"""
    n_mul, n_in = KEYS[key_index]
    vkb, pub, (proof, proof2) = _proved(n_mul, n_in)
    other_vk, other_pub, (other_proof, _) = _proved(*KEYS[1 - key_index])
    inputs = fr_bytes(pub)
    a, b = pr.g1_from_bytes(proof[:97]), pr.g2_from_bytes(proof[97:290])
    neg = pr.g1_to_bytes((a[0], (-a[1]) % pr.P_MOD)) + pr.g2_to_bytes((b[0], ((-b[1][0]) % pr.P_MOD, (-b[1][1]) % pr.P_MOD))) + proof[290:]
    g1_inf, g2_inf = pr.g1_to_bytes(None), pr.g2_to_bytes(None)
    flip = lambda p, at: p[:at] + bytes([p[at] ^ 1]) + p[at + 1:]
    rows = [
        ("valid", inputs, proof),
        ("valid under other (r, s)", inputs, proof2),
        ("(-A, -B)", inputs, neg),
        ("wrong input", fr_bytes([pub[0] + 1] + pub[1:]), proof),
        ("wrong last input", fr_bytes(pub[:-1] + [pub[-1] + 1]), proof2),
        ("input limbs >= r", _raise(inputs[:32], pr.R_MOD) + inputs[32:], proof),
        ("A and C swapped", inputs, proof[290:387] + proof[97:290] + proof[0:97]),
        ("tampered A.x", inputs, flip(proof, 0)),
        ("tampered B.x.c1", inputs, flip(proof, 97 + 48)),
        ("tampered C.x", inputs, flip(proof, 290)),
        ("A.x limbs >= p", inputs, _raise(proof[:48], pr.P_MOD) + proof[48:]),
        ("B.y.c0 limbs >= p", inputs, proof[:97 + 96] + _raise(proof[97 + 96:97 + 144], pr.P_MOD) + proof[97 + 144:]),
        ("A at infinity", inputs, g1_inf + proof[97:]),
        ("B at infinity", inputs, proof[:97] + g2_inf + proof[290:]),
        ("C at infinity", inputs, proof[:290] + g1_inf),
        ("proof of the other key", inputs, other_proof),
        ("valid again", inputs, proof),
    ]
    single = [1 if L.groth16_verify(vkb, i, p) else 0 for _, i, p in rows]
    assert sum(single) >= 4 and single.count(0) >= 8, single   # a verifier that answers a constant fails what follows
    return vkb, n_in - 1, rows, single


@functools.lru_cache(maxsize=None)
def wide_key():
    """a key of 18 public inputs (above the interface's limit of 16 for the device path: a context routes it to the host threads):
    (vk, n_inputs, inputs of [valid, wrong input, valid], proofs, single-call verdicts)"""
    vkb, pub, (proof, proof2) = _proved(30, 19)
    inputs = fr_bytes(pub) + fr_bytes(pub[:9] + [pub[9] + 1] + pub[10:]) + fr_bytes(pub)
    proofs = proof + proof + proof2
    single = bytes(1 if L.groth16_verify(vkb, inputs[576 * k:576 * k + 576], proofs[387 * k:387 * k + 387]) else 0 for k in range(3))
    assert single == bytes([1, 0, 1])
    return vkb, 18, inputs, proofs, single


@functools.lru_cache(maxsize=None)
def no_input_keys():
    """keys whose IC has one entry (n_inputs = 0): every input of table(0)'s valid row folded into IC_0, and IC_0 at infinity (X at infinity: the
    pair contributes 1, as in the single call).  [(vk, proofs, single-call verdicts)]"""
    vkb, n_inputs, rows, single = table(0)
    _, inputs, proof = rows[0]
    pub = [int.from_bytes(inputs[32 * k:32 * k + 32], "little") * pow(1 << 256, -1, pr.R_MOD) % pr.R_MOD for k in range(n_inputs)]
    ic = [pr.g1_from_bytes(vkb[878 + 97 * i:878 + 97 * (i + 1)]) for i in range(n_inputs + 1)]
    x = ic[0]
    for i in range(n_inputs):
        x = pr.g1_add(x, pr.g1_mul(ic[i + 1], pub[i]))
    proofs = proof + rows[7][2] + rows[1][2] + rows[12][2] + rows[14][2]   # valid, tampered A.x, valid under other (r, s), A at infinity, C at infinity
    out = []
    for ic0 in (pr.g1_to_bytes(x), pr.g1_to_bytes(None)):
        vk0 = vkb[:870] + (1).to_bytes(8, "little") + ic0
        out.append((vk0, proofs, bytes(1 if L.groth16_verify(vk0, b"", proofs[387 * k:387 * k + 387]) else 0 for k in range(5))))
    assert out[0][2] == bytes([1, 0, 1, 0, 0]) and out[1][2][1] == 0
    return out


def batch(key_index, n, seed):
    """n rows taken cyclically from the table in a shuffled order: (inputs, proofs, expected verdict bytes, row names)"""
    vkb, n_inputs, rows, single = table(key_index)
    order = list(range(len(rows)))
    random.Random(seed).shuffle(order)
    pick = [order[i % len(order)] for i in range(n)]
    return (b"".join(rows[k][1] for k in pick), b"".join(rows[k][2] for k in pick), bytes(single[k] for k in pick), [rows[k][0] for k in pick])


@functools.lru_cache(maxsize=None)
def production():
    """The reference's own acceptance case (src/mpn/circuits/test.rs:117-149): MpnCircuit::empty(3, 3, 1) with commitment 456, height 0, state =
    next_state = 123, aux = H2(1, 0); key and proof made by the CPU oracle.  (vk, inputs, inputs at another height, proof)"""
    from oracle import coracle as co
    co.build()
    co.lib()
    F = pr.fr_to_mont_bytes
    aux = pr.poseidon([1, 0])
    r = L.mpn_update_empty(3, 3, 1, F(456), 0, F(123), F(aux), F(123), F(1), record_matrices=True)
    assert r.satisfied
    csr = [co.CsrHolder(r.n_constraints, list(memoryview(r.view("rp" + w)).cast("I")), list(memoryview(r.view("col" + w)).cast("I")), r.view("val" + w))
           for w in "ABC"]
    params = co.groth16_setup(*csr, r.n_in, r.n_aux, 17, fr_bytes(fr_list(5, 123)), nthreads=co.ncpu())
    rs = fr_bytes(fr_list(2, 11))
    proof = co.groth16_prove(params, r.view("z"), r.view("az"), r.view("bz"), r.view("cz"), rs[:32], rs[32:], nthreads=co.ncpu())
    inputs = F(456) + F(0) + F(123) + F(aux) + F(123)
    assert bytes(r.view("z")[32:192]) == inputs
    return vk_bytes(params), inputs, F(456) + F(1) + F(123) + F(aux) + F(123), proof


PRODUCTION_FIXTURE = "groth16_production_case.json"


def production_fixture():
    """production() as recorded under tests/golden (the setup and the proof take half a minute on the CPU; `python tests/verify_cases.py` rewrites
    the file, tests/test_verify_batch_cpu.py checks it with the oracle's verifier)"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", PRODUCTION_FIXTURE)) as f:
        d = json.load(f)
    return tuple(bytes.fromhex(d[k]) for k in ("vk", "inputs", "inputs_other_height", "proof"))


if __name__ == "__main__":
    import json
    import os
    vk, inputs, other, proof = production()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", PRODUCTION_FIXTURE), "w") as f:
        json.dump({"what": "MpnCircuit::empty(3, 3, 1), inputs [456, 0, 123, H2(1, 0), 123]: key and proof by the CPU oracle (tests/verify_cases.py production())",
                   "vk": vk.hex(), "inputs": inputs.hex(), "inputs_other_height": other.hex(), "proof": proof.hex()}, f, indent=1)
        f.write("\n")
