"""Inputs and expected values of the wire-form L1 transaction tests (tests/test_l1_admit_cpu.py, tests/test_gpu_l1_admit.py).

The schemas restate the reference's type definitions with the combinators of tests/bincode_ref.py:

  Transaction / TransactionAndDelta / TransactionData / ContractUpdate / ContractUpdateData / RegularSendEntry / Token / Ratio
                                                                                            src/core/transaction.rs:213-363
  Signature<S> { Unsigned, Signed }                                                         src/core/address.rs:34-37
  ZkContract / ZkTokenContract / Zk{Multi,Single}InputVerifierKey / ZkStateModel / ZkDataPairs / ZkDeltaPairs
                                                                                            src/zk/mod.rs:332-345, 427, 471-474, 573-644
  V::Pub (schnorrkel PublicKey): a length-prefixed byte string of 32 [recalled], as the Ed25519 key is

Expected values never come from the code under test and do not splice bytes: a record is decoded by its schema, its signature set to Unsigned and
its state / delta to None, re-encoded, and that goes to hashlib.sha3_256 (Transaction::hash) and to the Ed25519 restatement of
tests/ed25519_cases.py (Transaction::verify_signature).  Merkle roots come from a restatement of src/crypto/merkle.rs that
tests/golden/merkle_vectors.json pins on the reference's own vectors (merkle.rs:131-160)."""
import copy
import functools
import hashlib
import json
import os
import random

import bincode_ref as B
import ed25519_cases as E

FORM_TX, FORM_TX_AND_DELTA = 0, 1
RECORD_MAX = 1 << 20


# ---- schemas
def Pairs(kt, vt):
    """a HashMap whose keys are not hashable in Python (Vec<u64>): a list of (key, value) in wire order"""
    def enc(v):
        return B.U64.enc(len(v)) + b"".join(kt.enc(k) + vt.enc(x) for k, x in v)

    def dec(b, p):
        n, p = B.U64.dec(b, p)
        if n > len(b):
            raise ValueError("map length exceeds input")
        out = []
        for _ in range(n):
            k, p = kt.dec(b, p)
            x, p = vt.dec(b, p)
            out.append((k, x))
        return out, p
    return B.T(enc, dec)


ZkDataPairs = Pairs(B.Vec(B.U64), B.ZkScalar)
ZkDeltaPairs = Pairs(B.Vec(B.U64), B.Option(B.ZkScalar))
VrfPublicKey = B.BYTES  # [recalled]


def _model_enc(v):
    return _MODEL.enc(v)


def _model_dec(b, p):
    return _MODEL.dec(b, p)


_MODEL_REF = B.T(_model_enc, _model_dec)
_MODEL = B.Enum(("Scalar", None), ("Struct", B.Struct(("field_types", B.Vec(_MODEL_REF)))),
                ("List", B.Struct(("log4_size", B.U8), ("item_type", _MODEL_REF))))
ZkStateModel = _MODEL
ZkSingleInputVerifierKey = B.Struct(("verifier_key", B.ZkVerifierKey))
ZkMultiInputVerifierKey = B.Struct(("verifier_key", B.ZkVerifierKey), ("log4_payment_capacity", B.U8))
Token = B.Struct(("name", B.STRING), ("symbol", B.STRING), ("supply", B.U64), ("decimals", B.U8), ("minter", B.Option(B.L1PublicKey)))
ZkTokenContract = B.Struct(("token", Token), ("mint_functions", B.Vec(ZkSingleInputVerifierKey)))
ZkContract = B.Struct(("initial_state", B.ZkCompressedState), ("state_model", ZkStateModel), ("deposit_functions", B.Vec(ZkMultiInputVerifierKey)),
                      ("withdraw_functions", B.Vec(ZkMultiInputVerifierKey)), ("functions", B.Vec(ZkSingleInputVerifierKey)),
                      ("token", B.Option(ZkTokenContract)))
RegularSendEntry = B.Struct(("dst", B.L1PublicKey), ("amount", B.Money))


@functools.lru_cache(maxsize=None)
def schemas(prefixed=False):
    """(Transaction, TransactionAndDelta); prefixed: Ed25519 signatures as length-prefixed byte strings (ed25519 < 1.3)"""
    sig_t = B.L1SignatureLenPrefixed if prefixed else B.L1Signature
    update_data = B.Enum(("Deposit", B.Struct(("deposits", B.Vec(B.contract_deposit(sig_t))))),
                         ("Withdraw", B.Struct(("withdraws", B.Vec(B.ContractWithdraw)))),
                         ("FunctionCall", B.Struct(("fee", B.Money))), ("Mint", B.Struct(("amount", B.U64))))
    update = B.Struct(("circuit_id", B.U32), ("data", update_data), ("next_state", B.ZkCompressedState), ("prover", B.L1PublicKey),
                      ("reward", B.U64), ("proof", B.ZkProof))
    data = B.Enum(("UpdateStaker", B.Struct(("vrf_pub_key", VrfPublicKey), ("commission", B.U8))),
                  ("Delegate", B.Struct(("amount", B.U64), ("to", B.L1PublicKey))),
                  ("Undelegate", B.Struct(("amount", B.U64), ("from", B.L1PublicKey))),
                  ("AutoDelegate", B.Struct(("to", B.L1PublicKey), ("ratio", B.U8))),
                  ("RegularSend", B.Struct(("entries", B.Vec(RegularSendEntry)))),
                  ("CreateContract", B.Struct(("contract", ZkContract), ("money", B.Money), ("state", B.Option(ZkDataPairs)))),
                  ("UpdateContract", B.Struct(("contract_id", B.ContractId), ("updates", B.Vec(update)), ("delta", B.Option(ZkDeltaPairs)))))
    tx = B.Struct(("src", B.Option(B.L1PublicKey)), ("nonce", B.U32), ("data", data), ("fee", B.Money), ("memo", B.STRING),
                  ("sig", B.Enum(("Unsigned", None), ("Signed", sig_t))))
    return tx, B.Struct(("tx", tx), ("state_delta", B.Option(ZkDeltaPairs)))


def schema(form, prefixed=False):
    return schemas(prefixed)[form]


# ---- the reference's rules, by decode / edit / re-encode
def sig_state_excluded(tx):
    clean = copy.deepcopy(tx)
    name, payload = clean["data"]
    if name == "UpdateContract":
        payload["delta"] = None
    elif name == "CreateContract":
        payload["state"] = None
    clean["sig"] = ("Unsigned", None)
    return clean


def signed_bytes(tx, prefixed=False) -> bytes:
    return B.encode(schema(FORM_TX, prefixed), sig_state_excluded(tx))


def expected(record: bytes, form=FORM_TX, prefixed=False):
    """(verify_signature, hash) of one wire record"""
    v = B.decode(schema(form, prefixed), record)
    tx = v["tx"] if form == FORM_TX_AND_DELTA else v
    body = signed_bytes(tx, prefixed)
    h = hashlib.sha3_256(body).digest()
    if tx["src"] is None:
        return True, h
    if tx["sig"][0] == "Unsigned":
        return False, h
    return E.verify(tx["src"], body, tx["sig"][1]), h


def expected_batch(records, form=FORM_TX, prefixed=False):
    out = [expected(r, form, prefixed) for r in records]
    return bytes(1 if ok else 0 for ok, _ in out), b"".join(h for _, h in out)


def sign_tx(seed: bytes, tx, prefixed=False):
    tx["src"] = E.public_key(seed)
    tx["sig"] = ("Signed", E.sign(seed, signed_bytes(tx, prefixed)))
    return tx


def enc(tx, form=FORM_TX, prefixed=False, state_delta=None) -> bytes:
    return B.encode(schema(form, prefixed), {"tx": tx, "state_delta": state_delta} if form == FORM_TX_AND_DELTA else tx)


# ---- values
ZIESHA = ("Ziesha", None)


def _blob(tag: str, n: int) -> bytes:
    return hashlib.shake_128(tag.encode()).digest(n)


def scalar(tag: str) -> bytes:  # 32 bytes below 2^248: limbs of a residue whatever the form
    return _blob("scalar " + tag, 31) + b"\0"


def money(amount: int, token=ZIESHA):
    return {"token_id": token, "amount": amount}


def verifier_key(tag: str, ic: int = 2):
    g1, g2 = (lambda k: _blob(f"{tag} g1 {k}", 97)), (lambda k: _blob(f"{tag} g2 {k}", 193))
    return ("Groth16", {"alpha_g1": g1("a"), "beta_g1": g1("b"), "beta_g2": g2("b"), "gamma_g2": g2("g"), "delta_g1": g1("d"),
                        "delta_g2": g2("d"), "ic": [g1(f"ic{i}") for i in range(ic)]})


def zk_proof(tag: str):
    return ("Groth16", {"a": _blob(tag + " a", 97), "b": _blob(tag + " b", 193), "c": _blob(tag + " c", 97)})


def data_pairs(n: int):
    return [([i, 2 * i + 1][: 1 + i % 2], scalar(f"state {i}")) for i in range(n)]


def delta_pairs(n: int):
    return [([i % 5, i][: 1 + i % 2], None if i % 3 == 2 else scalar(f"delta {i}")) for i in range(n)]


def contract_deposit(seed: bytes, memo: str, prefixed=False):
    d = {"memo": memo, "contract_id": ("Custom", scalar("cid")), "deposit_circuit_id": 0, "calldata": scalar("calldata " + memo),
         "src": E.public_key(seed), "amount": money(5), "fee": money(1), "nonce": 3, "sig": None}
    d["sig"] = _blob("deposit sig " + memo, 64)  # its own signature is not this arm's business: any 64 bytes
    return d


def contract_withdraw(memo: str):
    return {"memo": memo, "contract_id": ("Custom", scalar("cid")), "withdraw_circuit_id": 1, "calldata": scalar("wd " + memo),
            "dst": _blob("dst", 32), "amount": money(9), "fee": money(2)}


def contract_update(kind: str, payload, tag="u"):
    return {"circuit_id": 2, "data": (kind, payload), "next_state": {"state_hash": scalar("next " + tag), "state_size": 12},
            "prover": _blob("prover", 32), "reward": 77, "proof": zk_proof(tag)}


def zk_contract(with_token=True):
    model = ("Struct", {"field_types": [("Scalar", None), ("List", {"log4_size": 3, "item_type": ("Struct", {"field_types": [("Scalar", None), ("Scalar", None)]})})]})
    token = {"token": {"name": "Some Token", "symbol": "STK", "supply": 10 ** 9, "decimals": 9, "minter": _blob("minter", 32)},
             "mint_functions": [{"verifier_key": verifier_key("mint")}]}
    return {"initial_state": {"state_hash": scalar("init"), "state_size": 0}, "state_model": model,
            "deposit_functions": [{"verifier_key": verifier_key("dep"), "log4_payment_capacity": 1}],
            "withdraw_functions": [{"verifier_key": verifier_key("wd", 3), "log4_payment_capacity": 2}],
            "functions": [{"verifier_key": verifier_key("f0")}, {"verifier_key": verifier_key("f1", 1)}], "token": token if with_token else None}


def tx_of(data, memo="memo", nonce=7, fee=3):
    return {"src": None, "nonce": nonce, "data": data, "fee": money(fee), "memo": memo, "sig": ("Unsigned", None)}


def variant_data(prefixed=False):
    """one TransactionData of each of the seven variants; the two with a removable option carry Some"""
    return [
        ("UpdateStaker", {"vrf_pub_key": _blob("vrf", 32), "commission": 25}),
        ("Delegate", {"amount": 1000, "to": _blob("to", 32)}),
        ("Undelegate", {"amount": 10, "from": _blob("from", 32)}),
        ("AutoDelegate", {"to": _blob("to2", 32), "ratio": 128}),
        ("RegularSend", {"entries": [{"dst": _blob("dst0", 32), "amount": money(5)}, {"dst": _blob("dst1", 32), "amount": money(6, ("Custom", scalar("tok")))}]}),
        ("CreateContract", {"contract": zk_contract(), "money": money(50), "state": data_pairs(3)}),
        ("UpdateContract", {"contract_id": ("Custom", scalar("cid")),
                            "updates": [contract_update("Deposit", {"deposits": [contract_deposit(b"d0", "dep memo", prefixed)]}, "u0"),
                                        contract_update("Withdraw", {"withdraws": [contract_withdraw("w"), contract_withdraw("")]}, "u1"),
                                        contract_update("FunctionCall", {"fee": money(4)}, "u2"), contract_update("Mint", {"amount": 3}, "u3")],
                            "delta": delta_pairs(4)}),
    ]


@functools.lru_cache(maxsize=None)
def variant_txs(prefixed=False):
    """the seven variants, each signed by a wallet of its own"""
    return tuple(sign_tx(b"l1 wallet %d" % i, tx_of(d, memo="variant %d" % i, nonce=i), prefixed) for i, d in enumerate(variant_data(prefixed)))


def flip(b: bytes, at: int, bit: int = 0) -> bytes:
    return b[:at] + bytes([b[at] ^ (1 << bit)]) + b[at + 1:]


def layout(tx, prefixed=False):
    """byte offsets inside bincode(tx), from the encoders' lengths: nonce, data tag, the removable option (cut_a, cut_b; None without), fee, the
    memo's last byte, the Signature tag, the signature"""
    t = schemas(prefixed)[0]
    full = B.encode(t, tx)
    src_len = 1 if tx["src"] is None else 41
    sig_len = 4 + (0 if tx["sig"][0] == "Unsigned" else (72 if prefixed else 64))
    sig_tag = len(full) - sig_len
    memo_len = 8 + len(tx["memo"].encode())
    fee = sig_tag - memo_len - len(B.encode(B.Money, tx["fee"]))
    cut = None
    name, payload = tx["data"]
    opt = {"CreateContract": ("state", ZkDataPairs), "UpdateContract": ("delta", ZkDeltaPairs)}.get(name)
    if opt and payload[opt[0]] is not None:
        cut = (fee - 1 - len(B.encode(opt[1], payload[opt[0]])), fee)
    return {"nonce": src_len, "data_tag": src_len + 4, "cut": cut, "fee": fee, "memo_last": sig_tag - 1, "sig_tag": sig_tag, "sig": len(full) - 64,
            "key": 9 if tx["src"] is not None else None, "len": len(full)}


@functools.lru_cache(maxsize=None)
def corpus(form=FORM_TX, prefixed=False):
    """the records of the CPU corpus as wire bytes, with a label each: the seven variants; src None; Unsigned; a wrong signature; a wrong key; a
    bit flipped in each signed region; a bit flipped inside Some(state) / Some(delta) (outside the signature); and, for TransactionAndDelta, in
    the trailing state_delta"""
    out = []
    txs = variant_txs(prefixed)
    sd = delta_pairs(2) if form == FORM_TX_AND_DELTA else None
    e = lambda tx, delta=sd: enc(tx, form, prefixed, delta)  # noqa: E731
    for i, tx in enumerate(txs):
        out.append((f"variant {tx['data'][0]}", e(tx)))
    for i, tx in enumerate(txs):
        lay, rec = layout(tx, prefixed), e(tx)
        name = tx["data"][0]
        out.append((f"{name}: src None", e(dict(tx, src=None))))
        out.append((f"{name}: Unsigned", e(dict(tx, sig=("Unsigned", None)))))
        out.append((f"{name}: wrong signature", flip(rec, lay["sig"] + 5, 3)))
        out.append((f"{name}: wrong key", e(dict(tx, src=E.public_key(b"someone else")))))
        out.append((f"{name}: flip in the first signed region", flip(rec, lay["nonce"])))
        out.append((f"{name}: flip in the last signed region", flip(rec, lay["memo_last"])))
        if lay["cut"]:
            out.append((f"{name}: flip inside the Some(..) the signature leaves out", flip(rec, lay["cut"][1] - 1, 2)))
            out.append((f"{name}: flip in the fee, after the cut", flip(rec, lay["fee"] + 4)))
        if form == FORM_TX_AND_DELTA:
            out.append((f"{name}: flip in the trailing state_delta", flip(rec, len(rec) - 1, 1)))
    out.append(("CreateContract without state and token", e(sign_tx(b"cc", tx_of(("CreateContract", {"contract": zk_contract(False), "money": money(1), "state": None})), prefixed))))
    out.append(("UpdateContract without updates and delta", e(sign_tx(b"uc", tx_of(("UpdateContract", {"contract_id": ZIESHA, "updates": [], "delta": None})), prefixed))))
    if form == FORM_TX_AND_DELTA:
        out.append(("RegularSend, state_delta None", e(txs[4], None)))
    return tuple(out)


def regular_send(seed: bytes, memo: str, entries: int = 1, nonce: int = 1):
    return sign_tx(seed, tx_of(("RegularSend", {"entries": [{"dst": _blob(f"dst {k}", 32), "amount": money(1 + k)} for k in range(entries)]}),
                               memo=memo, nonce=nonce))


@functools.lru_cache(maxsize=None)
def memo_sweep():
    """RegularSend with one entry and memo lengths 0 .. 300: every residue of SHA-512's 128 (with the 64 bytes of R | A in front) and of SHA3's
    136, the zero run of the Unsigned tag crossing a block end included"""
    return tuple(enc(regular_send(b"memo wallet", "m" * k, nonce=k)) for k in range(301))


@functools.lru_cache(maxsize=None)
def cut_sweep():
    """UpdateContract whose first update is a Deposit holding one ContractDeposit with memo lengths 0 .. 15 (every residue of cut_a mod 8: the
    zero byte straddles a word) over delta sizes 0, 1 and 50 (cut_b moves too)"""
    out = []
    for entries in (0, 1, 50):
        for k in range(16):
            data = ("UpdateContract", {"contract_id": ZIESHA, "updates": [contract_update("Deposit", {"deposits": [contract_deposit(b"cs", "x" * k)]})],
                                       "delta": delta_pairs(entries)})
            out.append(enc(sign_tx(b"cut wallet", tx_of(data, memo="cut", nonce=16 * entries + k))))
    return tuple(out)


# ---- MerkleTree<Sha3Hasher> (src/crypto/merkle.rs)
def merkle_nodes(leaves):
    """MerkleTree::new(leaves).data"""
    n = len(leaves)
    if n == 0:
        return [bytes(32)]
    total = 2 * n - 1
    depth = 0 if total == 1 else (1 << (total - 1).bit_length()).bit_length() - 1 - 1  # len.next_power_of_two().trailing_zeros() - 1
    data = [bytes(32)] * total

    def leaf_map(i):
        lower_start = (1 << depth) - 1
        if lower_start + i < total:
            return lower_start + i
        return (1 << (depth - 1)) - 1 - ((total - lower_start) >> 1) + i
    for i, leaf in enumerate(leaves):
        data[leaf_map(i)] = leaf
    for d in range(depth, 0, -1):
        start = (1 << d) - 1
        for k in range(0, 1 << d, 2):
            i = start + k
            if i >= total:
                break
            a, b = data[i], data[i + 1]
            data[(i - 1) >> 1] = hashlib.sha3_256(a + b if a < b else b + a).digest()
    return data


def merkle_root(leaves) -> bytes:
    return merkle_nodes(leaves)[0]


def reference_merkle_vectors():
    """the reference's own vectors (merkle.rs:131-160) as data: leaves sha3([i]) for i in first .. first + count"""
    with open(os.path.join(E.GOLDEN, "merkle_vectors.json")) as f:
        return json.load(f)["vectors"]


MERKLE_COUNTS = (0, 1, 2, 3, 5, 6, 7, 9, 10, 16, 17, 1000)


@functools.lru_cache(maxsize=None)
def merkle_trees():
    """a list of leaves per count of MERKLE_COUNTS"""
    rnd = random.Random(20)
    return tuple(tuple(rnd.randbytes(32) for _ in range(c)) for c in MERKLE_COUNTS)


# ---- block bodies
BODY_COUNTS = (0, 1, 3, 65)
BAD_BODY, BAD_TX = 2, 1  # body 2's second transaction carries a wrong signature


@functools.lru_cache(maxsize=None)
def bodies():
    """(txs bytes, counts, records): bodies of 0, 1, 3 and 65 transactions; one body with one bad signature"""
    records, k = [], 0
    variants = variant_txs()
    for j, c in enumerate(BODY_COUNTS):
        for i in range(c):
            rec = enc(variants[k % 7]) if k % 9 == 4 else enc(regular_send(b"body wallet %d" % (k % 5), "tx %d" % k, 1 + k % 3, nonce=k))
            if (j, i) == (BAD_BODY, BAD_TX):
                rec = flip(rec, len(rec) - 7)
            records.append(rec)
            k += 1
    return b"".join(records), BODY_COUNTS, tuple(records)


@functools.lru_cache(maxsize=None)
def bodies_expected():
    """(sig_ok, roots, tx_ok, hashes) by the restatements"""
    _, counts, records = bodies()
    tx_ok, hashes = expected_batch(records)
    sig_ok, roots, at = bytearray(), b"", 0
    for c in counts:
        sig_ok.append(1 if all(tx_ok[at:at + c]) else 0)
        roots += merkle_root([hashes[32 * i:32 * i + 32] for i in range(at, at + c)])
        at += c
    return bytes(sig_ok), roots, tx_ok, hashes
