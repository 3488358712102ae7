"""Inputs of the Ed25519 signing tests (tests/test_ed25519_sign_cpu.py, tests/test_gpu_ed25519_sign.py): the message-length sweep, seeds, rows of
distinct keys and messages, and unsigned wire records with the keys that are to sign them.  Expected values are ed25519_cases' and
l1_tx_cases' (Python integers and hashlib) and the OpenSSL / RFC 8032 fixture tests/golden/ed25519_sign_vectors.json."""
import copy
import hashlib
import json
import os
import random

import ed25519_cases as E
import l1_tx_cases as T

# 32 + len (first hash) or 64 + len (second hash) lands on, one before and one after the points where SHA-512's padding changes the block count
LENGTHS = (0, 1, 47, 48, 63, 64, 65, 79, 80, 95, 96, 97, 111, 112, 127, 128, 129, 175, 176, 191, 192, 193, 207, 208, 223, 224, 225, 300)
SEED_LENGTHS = (0, 1, 135, 136, 137, 272)  # Keccak's rate edges


def fixture():
    with open(os.path.join(E.GOLDEN, "ed25519_sign_vectors.json")) as f:
        return [{k: (bytes.fromhex(v) if k in ("secret", "pk", "msg", "sig") else v) for k, v in row.items()} for row in json.load(f)["vectors"]]


def secret_of(seed: bytes) -> bytes:
    """Ed25519::generate_keys' secret: SHA3-256(seed) with the top bit cleared (src/crypto/ed25519.rs:70-77)"""
    d = bytearray(hashlib.sha3_256(seed).digest())
    d[31] &= 0x7F
    return bytes(d)


def keypair(secret: bytes) -> bytes:
    return secret + E.public_key(secret)


def seeds(n: int):
    """n seeds: the edge lengths, b"ABC", then distinct pseudo-random ones of mixed lengths"""
    rnd = random.Random(8032)
    out = [bytes((7 * k + i) & 0xFF for i in range(k)) for k in SEED_LENGTHS] + [b"ABC"]
    while len(out) < n:
        out.append(b"seed %d " % len(out) + rnd.randbytes(rnd.randrange(0, 300)))
    return out[:n]


def messages(n: int, seed: int, fixed_len=None):
    """n distinct messages, the length sweep cycled over the rows (or all of fixed_len >= 8 bytes); the row number is written into the first
    bytes of every message long enough to hold it, which keeps them distinct"""
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        k = LENGTHS[i % len(LENGTHS)] if fixed_len is None else fixed_len
        m = bytearray(rnd.randbytes(k))
        if k >= 8:
            m[:8] = i.to_bytes(8, "little")
        out.append(bytes(m))
    return out


def key_rows(n: int, seed: int) -> bytes:
    """n x 64 bytes secret | public with distinct secrets, derived by the library's host route (which test_ed25519_sign_cpu pins on E.public_key)"""
    from bazuka_amd import lib as L
    return L.host_ed25519_keys_batch([b"row %d of %d" % (i, seed) for i in range(n)])


# ---- wire records ---------------------------------------------------------------------------------------------------------------------------
ADDRESS = {"x": bytes(31) + b"\0", "odd": False}  # signing does not look at mpn_address


def unsigned_deposit(pk: bytes, memo: str, nonce: int = 1, sig=None):
    return {"mpn_address": ADDRESS,
            "payment": {"memo": memo, "contract_id": E.ZIESHA, "deposit_circuit_id": 0, "calldata": hashlib.sha3_256(pk).digest()[:31] + b"\0",
                        "src": pk, "amount": {"token_id": E.ZIESHA, "amount": 9}, "fee": {"token_id": E.ZIESHA, "amount": 1}, "nonce": nonce, "sig": sig}}


def python_signed_deposit(secret: bytes, rec):
    out = copy.deepcopy(rec)
    out["payment"]["sig"] = E.sign(secret, E.unsigned_bytes(rec))
    return out


def l1_unsigned(tx, pk):
    out = copy.deepcopy(tx)
    out["src"], out["sig"] = pk, ("Unsigned", None)
    return out


def l1_mixed(n: int, pks):
    """n Unsigned transactions cycling the seven TransactionData variants, record i from key i; every ninth has src None"""
    data = T.variant_data()
    return [T.tx_of(copy.deepcopy(data[i % 7]), memo="m" * (i % 40), nonce=i) if i % 9 == 8 else
            l1_unsigned(T.tx_of(data[i % 7], memo="m" * (i % 40), nonce=i), pks[i]) for i in range(n)]
