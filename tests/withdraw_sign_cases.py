"""Inputs of the withdrawal-producer tests (tests/test_withdraw_sign_cpu.py, tests/test_gpu_withdraw_sign.py): unsigned MpnWithdraw records in
tests/withdraw_cases.py's record form with junk in mpn_sig and payment.calldata, their keys, and what `TxBuilder::withdraw_mpn` makes of them.
The expected records come from oracle/pyref.py alone - jj_generate_keys, hashlib.sha3_256 through withdraw_cases.fingerprint, poseidon, jj_sign -
never from the code under test.  Keys are 128 bytes pub.x | pub.y | randomness | scalar, scalars 32-byte Montgomery limbs.  Everything is
computed once per process and never changed."""
import copy
import hashlib

import decompress_cases as D
import sign_cases as S
import withdraw_cases as W
from oracle import pyref as pr

F, U = pr.fr_to_mont_bytes, pr.fr_from_mont_bytes
JUNK = (D.ALL_ONES, D.R_LIMBS)  # what the ignored fields of an input hold: neither is a residue's limbs, so a parser that validated would refuse

_keys = {}


def key_of(seed: bytes) -> bytes:
    if seed not in _keys:
        _keys[seed] = S.key_bytes(pr.jj_generate_keys(seed))
    return _keys[seed]


def unsigned(seed: bytes, nonce: int, memo: str, contract_id, atok, amount: int, ftok, fee: int, circuit: int = 0, junk: bytes = D.ALL_ONES):
    """a withdrawal of the key of `seed` before it is signed: every scalar of mpn_sig and payment.calldata is `junk`"""
    x, odd = D.compress(key_of(seed)[:64])
    return {"mpn_address": {"x": x, "odd": bool(odd)}, "mpn_withdraw_nonce": nonce, "mpn_sig": {"r": {"x": junk, "y": junk}, "s": junk},
            "payment": {"memo": memo, "contract_id": contract_id, "withdraw_circuit_id": circuit, "calldata": junk,
                        "dst": hashlib.sha3_256(b"l1 " + seed).digest(), "amount": {"token_id": atok, "amount": amount},
                        "fee": {"token_id": ftok, "amount": fee}}}


def blanked(rec, junk: bytes = D.ALL_ONES):
    """a signed record with its signature and calldata overwritten"""
    m = copy.deepcopy(rec)
    m["mpn_sig"] = {"r": {"x": junk, "y": junk}, "s": junk}
    m["payment"]["calldata"] = junk
    return m


def signed_by_pyref(rec, key: bytes):
    """src/wallet/tx_builder.rs:376-425 by Python integers: sign H2(fingerprint, nonce), then calldata = H6(pub, nonce, signature)"""
    sk = S.key_dict(key)
    nonce = rec["mpn_withdraw_nonce"]
    (rx, ry), s = pr.jj_sign(sk, pr.poseidon([W.fingerprint(rec), nonce]))
    out = copy.deepcopy(rec)
    out["mpn_sig"] = {"r": {"x": F(rx), "y": F(ry)}, "s": F(s)}
    out["payment"]["calldata"] = F(pr.poseidon([sk["pub"][0], sk["pub"][1], nonce, rx, ry, s]))
    return out


_fixed = None


def fixed():
    """[(unsigned record, key, the record as pyref signs it)]: one per memo length of withdraw_cases.MEMO_LENGTHS, payments of
    withdraw_cases.PAYMENT_LENGTHS bytes (the SHA3 rate edges; at 212 the calldata lies across a block edge); the junk alternates"""
    global _fixed
    if _fixed is None:
        out = []
        for k, ml in enumerate(W.MEMO_LENGTHS):
            seed = b"wd sign %d" % k
            rec = unsigned(seed, 1 + k, "m" * ml, W.ZIESHA, W.ZIESHA, 1000 + k, W.ZIESHA, k % 4, junk=JUNK[k % 2])
            out.append((rec, key_of(seed), signed_by_pyref(rec, key_of(seed))))
        assert tuple(len(W.payment_bytes(r)) for r, _, _ in out) == W.PAYMENT_LENGTHS
        _fixed = out
    return _fixed


def refusals():
    """[(class, record, key)] that the producer must leave alone with verdict 0: each is a well-formed record"""
    rec, key, _ = fixed()[1]
    flipped = copy.deepcopy(rec)
    flipped["mpn_address"]["odd"] = not rec["mpn_address"]["odd"]
    out = [("the key of another seed", rec, key_of(b"wd sign someone else")), ("odd flipped in the address", flipped, key)]
    for name, bad in (("r's limbs", D.R_LIMBS), ("all ones", D.ALL_ONES)):
        for f in range(4):
            out.append(("%s = %s" % (S.FIELDS[f], name), rec, key[:32 * f] + bad + key[32 * f + 32:]))
    return out


def batch(rows):
    """(keys, records' bytes, n) of [(record, key, ...)]"""
    return b"".join(r[1] for r in rows), b"".join(W.enc(r[0]) for r in rows), len(rows)


def pool(k: int, seed: int, memo_base: int = 0, spoil: bool = False):
    """k (unsigned record, key) pairs of k different lengths (memos of memo_base + 3 i bytes, token ids of all three forms, so that record and
    payment offsets take every alignment); with spoil the last pair's key has r's limbs for its scalar"""
    toks = (W.ZIESHA, W.NULL, W.custom(4242))
    out = []
    for i in range(k):
        s = b"wd sign pool %d %d" % (seed, i)
        rec = unsigned(s, 7 + i, "p" * (memo_base + 3 * i), W.custom(W.MPN_CONTRACT), toks[i % 3], 10 ** 6 + i, toks[(i + 1) % 3], i % 5, junk=JUNK[i % 2])
        out.append((rec, key_of(s)))
    if spoil:
        rec, key = out[-1]
        out[-1] = (rec, key[:96] + D.R_LIMBS)
    return out
