"""Ed25519 restated in Python integers and hashlib.sha512, and the inputs of the deposit-admission tests (tests/test_ed25519_cpu.py,
tests/test_deposit_admit_cpu.py, tests/test_gpu_deposit_admit.py).  decode / verify follow the rules of `ed25519-dalek = "1"` PublicKey::verify
as bazuka_amd/csrc/bzk_ed25519.cuh states them: cofactorless, no small-order rejection, s < l, A's y taken mod p, x = 0 with the sign bit set
accepted, R compared as bytes.  sign is RFC 8032 section 5.1.6.  tools/make_ed25519_fixtures.py pins verify and sign on OpenSSL; expected values
in the tests come from here and from hashlib, never from the code under test."""
import hashlib
import json
import os
import random

import bincode_ref as B

P = 2 ** 255 - 19
L_ORDER = 2 ** 252 + 27742317777372353535851937790883648493
D = (-121665 * pow(121666, P - 2, P)) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sha512(b: bytes) -> bytes:
    return hashlib.sha512(b).digest()


# ---- the group, extended coordinates (X, Y, Z, T)
def _add(p, q):
    a, b = (p[1] - p[0]) * (q[1] - q[0]) % P, (p[1] + p[0]) * (q[1] + q[0]) % P
    c, d = 2 * D * p[3] * q[3] % P, 2 * p[2] * q[2] % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def mul(k: int, p):
    q = (0, 1, 1, 0)
    while k:
        if k & 1:
            q = _add(q, p)
        p = _add(p, p)
        k >>= 1
    return q


def from_affine(x, y):
    return (x, y, 1, x * y % P)


def encode(p) -> bytes:
    zi = pow(p[2], P - 2, P)
    x, y = p[0] * zi % P, p[1] * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def decode(key: bytes):
    """(x, y) as the verifier sees the key, or None where (y^2 - 1) / (d y^2 + 1) has no root.  y is the low 255 bits mod p (no canonicity
    check); the root is made even and then negated where bit 255 is set (so x = 0 with the bit set stays 0)."""
    v = int.from_bytes(key, "little")
    sign, y = v >> 255, (v & ((1 << 255) - 1)) % P
    u, w = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * pow(w, 3, P) * pow(u * pow(w, 7, P), (P - 5) // 8, P) % P
    if w * x * x % P == u:
        pass
    elif w * x * x % P == (-u) % P:
        x = x * SQRT_M1 % P
    else:
        return None
    if x & 1:
        x = P - x
    if sign:
        x = (P - x) % P
    return x, y


BASE = from_affine(*decode((4 * pow(5, P - 2, P) % P).to_bytes(32, "little")))


def verify(pk: bytes, msg: bytes, sig: bytes) -> bool:
    a = decode(pk)
    s = int.from_bytes(sig[32:], "little")
    if a is None or s >= L_ORDER:
        return False
    k = int.from_bytes(sha512(sig[:32] + pk + msg), "little") % L_ORDER
    minus_a = from_affine((P - a[0]) % P, a[1])
    return encode(_add(mul(s, BASE), mul(k, minus_a))) == sig[:32]


def _expand(seed: bytes):
    h = sha512(seed)
    a = int.from_bytes(h[:32], "little")
    a = (a & ((1 << 254) - 8)) | (1 << 254)
    return a, h[32:]


def public_key(seed: bytes) -> bytes:
    return encode(mul(_expand(seed)[0], BASE))


def sign(seed: bytes, msg: bytes) -> bytes:
    a, prefix = _expand(seed)
    pk = encode(mul(a, BASE))
    r = int.from_bytes(sha512(prefix + msg), "little") % L_ORDER
    rb = encode(mul(r, BASE))
    k = int.from_bytes(sha512(rb + pk + msg), "little") % L_ORDER
    return rb + ((r + k * a) % L_ORDER).to_bytes(32, "little")


# ---- the edge cases the recalled rules decide
def small_order_forgery(msg: bytes):
    """(key, signature): A = (0, -1), of order 2.  With R = [s]B - [k]A and k = H(R | A | msg) the equation holds by construction whenever the
    k that R itself produces gives that same R back: [k]A is A for odd k and the neutral element for even k, so one of the two candidates for R is
    tried with several s until it is consistent.  A strict verifier refuses A; the non-strict one accepts."""
    a_bytes = (P - 1).to_bytes(32, "little")
    a_pt = from_affine(0, P - 1)
    for s in range(1, 200):
        sb = mul(s, BASE)
        for r_pt in (sb, _add(sb, a_pt)):  # -A = A
            rb = encode(r_pt)
            k = int.from_bytes(sha512(rb + a_bytes + msg), "little") % L_ORDER
            if encode(_add(sb, mul(k, a_pt))) == rb:
                return a_bytes, rb + s.to_bytes(32, "little")
    raise AssertionError("no consistent s among 200")


def non_canonical_key_case():
    """(y, key bytes holding y + p): the first small y on the curve; y + p fits 255 bits for y < 19.  Nobody knows such a key's secret, so the case
    checks decoding alone; identity_key_forgery covers verification under a non-canonical key."""
    for y in range(2, 19):
        if decode(y.to_bytes(32, "little")) is not None:
            return y, (y + P).to_bytes(32, "little")
    raise AssertionError("no small y on the curve")


IDENTITY_KEYS = {"canonical": (1).to_bytes(32, "little"), "x = 0 with the sign bit": (1 | (1 << 255)).to_bytes(32, "little"),
                 "y = p + 1": (P + 1).to_bytes(32, "little"), "y = p + 1 with the sign bit": (P + 1 | (1 << 255)).to_bytes(32, "little")}


def identity_key_forgery(s: int = 7) -> bytes:
    """a signature that verifies for every message under any encoding of the neutral element that decodes: [k]A vanishes, so R = [s]B"""
    return encode(mul(s, BASE)) + s.to_bytes(32, "little")


def non_residue_y():
    """a y whose radicand has no root"""
    for y in range(2, 100):
        if decode(y.to_bytes(32, "little")) is None:
            return y.to_bytes(32, "little")
    raise AssertionError


def golden_vectors():
    with open(os.path.join(GOLDEN, "ed25519_vectors.json")) as f:
        return [(bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])) for v in json.load(f)["vectors"]]


def corrupted(pk: bytes, msg: bytes, sig: bytes, rnd):
    """[(what, pk, msg, sig)]: one bit flipped in the message (where it has one), R, s and the key"""
    def flip(b, i):
        return b[:i // 8] + bytes([b[i // 8] ^ (1 << (i % 8))]) + b[i // 8 + 1:]
    out = []
    if msg:
        out.append(("message", pk, flip(msg, rnd.randrange(8 * len(msg))), sig))
    out.append(("R", pk, msg, flip(sig, rnd.randrange(256))))
    out.append(("s", pk, msg, flip(sig, 256 + rnd.randrange(252))))
    out.append(("key", flip(pk, rnd.randrange(256)), msg, sig))
    return out


def genesis_keys():
    with open(os.path.join(GOLDEN, "ed25519_genesis_keys.json")) as f:
        return [bytes.fromhex(k) for k in json.load(f)["keys"]]


# ---- MpnDeposit records
NULL, ZIESHA = ("Null", None), ("Ziesha", None)
MPN_CONTRACT = 0x4D504E  # the ContractId::Custom a synthetic MpnWorld pays to


def mpn_deposit_t(prefixed=False):
    return B.Struct(("mpn_address", B.ZkPublicKey), ("payment", B.contract_deposit(B.L1SignatureLenPrefixed if prefixed else B.L1Signature)))


def enc(rec, prefixed=False) -> bytes:
    return B.encode(mpn_deposit_t(prefixed), rec)


def payment_bytes(rec, prefixed=False) -> bytes:
    return B.encode(B.contract_deposit(B.L1SignatureLenPrefixed if prefixed else B.L1Signature), rec["payment"])


def unsigned_bytes(rec) -> bytes:
    return B.encode(B.ContractDeposit, dict(rec["payment"], sig=None))


def signed_deposit(seed: bytes, address, memo: str, contract_id, atok, amount: int, ftok=ZIESHA, fee: int = 0, nonce: int = 1, circuit: int = 0):
    """address: {"x": 32 Montgomery bytes, "odd": bool}; payment.src = the Ed25519 key of `seed`, which signs the unsigned form"""
    rec = {"mpn_address": address,
           "payment": {"memo": memo, "contract_id": contract_id, "deposit_circuit_id": circuit, "calldata": hashlib.sha3_256(seed).digest()[:31] + b"\0",
                       "src": public_key(seed), "amount": {"token_id": atok, "amount": amount}, "fee": {"token_id": ftok, "amount": fee},
                       "nonce": nonce, "sig": None}}
    rec["payment"]["sig"] = sign(seed, unsigned_bytes(rec))
    return rec


def oracle_signature(rec) -> bool:
    sig = rec["payment"]["sig"]
    return sig is not None and verify(rec["payment"]["src"], unsigned_bytes(rec), sig)


def messages(lengths, seed: int):
    rnd = random.Random(seed)
    return [rnd.randbytes(k) for k in lengths]


# ---- admission: world A queues through bzk_mpn_push_deposit, world B receives the same deposits as signed wire records
N_ACC = 6
DEPOSITS = [(0, 500), (2, 7), (0, 11), (5, 10 ** 6), (3, 1)]  # (account, amount); account 0 twice


def account_address(i: int):
    """the compressed key of account i of withdraw_cases.admission_world (seed b"acct<i>")"""
    import decompress_cases as Dc
    from bazuka_amd import lib as L
    x, odd = Dc.compress(L.host_jubjub_keys(b"acct%d" % i)[:64])
    return {"x": x, "odd": bool(odd)}


def custom(v: int):
    from oracle import pyref as pr
    return ("Custom", pr.fr_to_mont_bytes(v))


def admission_records(which=DEPOSITS, contract_id=None, memo="deposit %d"):
    cid = custom(MPN_CONTRACT) if contract_id is None else contract_id
    return [signed_deposit(b"l1 wallet %d" % k, account_address(acct), memo % k, cid, ZIESHA, amount, ZIESHA, k, nonce=1 + k)
            for k, (acct, amount) in enumerate(which)]


def oracle_admits(rec, world_contract=None) -> bool:
    """mempool.rs:241-258 for a deposit plus the address decompression, by the restatement"""
    import decompress_cases as Dc
    cid = custom(MPN_CONTRACT) if world_contract is None else world_contract
    p = rec["payment"]
    tok = p["amount"]["token_id"]
    return (p["contract_id"] == cid and p["deposit_circuit_id"] == 0 and not (tok[0] == "Custom" and int.from_bytes(tok[1], "little") >= Dc.R)
            and oracle_signature(rec) and Dc.oracle_decompress(rec["mpn_address"]["x"], rec["mpn_address"]["odd"]) is not None)
