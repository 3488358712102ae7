"""Inputs of the wire-form withdrawal tests (tests/test_withdraw_admit_cpu.py, tests/test_gpu_withdraw_admit.py): seeded messages for the SHA3
batch, MpnWithdraw records in the value form tests/bincode_ref.py encodes, the fixed list with its mutations, bulk sets, and the two admission
worlds.  Expected values come from an independent Python route - hashlib.sha3_256, oracle/pyref.py poseidon and jj_verify, and the key
decompression of tests/decompress_cases.py - never from the code under test; scalars are 32-byte Montgomery limbs."""
import copy
import hashlib
import random

import bincode_ref as B
import decompress_cases as D
import r1cs_scenarios as sc
from bazuka_amd import lib as L
from oracle import pyref as pr

F, U = pr.fr_to_mont_bytes, pr.fr_from_mont_bytes
R = pr.R_MOD
NULL, ZIESHA = ("Null", None), ("Ziesha", None)
MPN_CONTRACT = 0x4D504E  # the ContractId::Custom a synthetic MpnWorld pays to


def custom(v: int):
    return ("Custom", F(v))


def messages(lengths, seed: int):
    rnd = random.Random(seed)
    return [rnd.randbytes(k) for k in lengths]


def scalar_new(d: bytes) -> bytes:
    """ZkScalar::new of 32 little-endian bytes, by Python integers"""
    return F(int.from_bytes(d, "little") % R)


# ---- records
def enc(rec) -> bytes:
    return B.encode(B.MpnWithdraw, rec)


def payment_bytes(rec) -> bytes:
    return B.encode(B.ContractWithdraw, rec["payment"])


def calldata_offset(rec) -> int:
    p = rec["payment"]
    return 8 + len(p["memo"].encode()) + len(B.encode(B.ContractId, p["contract_id"])) + 4


def fingerprint(rec) -> int:
    """ContractWithdraw::fingerprint: ZkScalar::new(sha3_256(bincode(payment with calldata := 0)))"""
    blank = copy.deepcopy(rec["payment"])
    blank["calldata"] = bytes(32)
    return int.from_bytes(hashlib.sha3_256(B.encode(B.ContractWithdraw, blank)).digest(), "little") % R


def calldata_of(rec, key_xy, hasher=pr.poseidon) -> bytes:
    s = rec["mpn_sig"]
    return F(hasher([key_xy[0], key_xy[1], rec["mpn_withdraw_nonce"], U(s["r"]["x"]), U(s["r"]["y"]), U(s["s"])]))


def _host_hash(vals):
    return U(L.host_poseidon(b"".join(F(v) for v in vals)))


def signed_withdraw(seed: bytes, nonce: int, memo: str, contract_id, atok, amount: int, ftok, fee: int, circuit: int = 0, hasher=pr.poseidon):
    """as the wallet does (src/wallet/tx_builder.rs:376-425): sign H2(fingerprint, nonce), then calldata = H6(address, nonce, signature)"""
    key = L.host_jubjub_keys(seed)
    x, odd = D.compress(key[:64])
    rec = {"mpn_address": {"x": x, "odd": bool(odd)}, "mpn_withdraw_nonce": nonce, "mpn_sig": None,
           "payment": {"memo": memo, "contract_id": contract_id, "withdraw_circuit_id": circuit, "calldata": bytes(32),
                       "dst": hashlib.sha3_256(b"l1 " + seed).digest(), "amount": {"token_id": atok, "amount": amount},
                       "fee": {"token_id": ftok, "amount": fee}}}
    sig = L.host_jubjub_sign(key, F(hasher([fingerprint(rec), nonce])))
    rec["mpn_sig"] = {"r": {"x": sig[:32], "y": sig[32:64]}, "s": sig[64:]}
    rec["payment"]["calldata"] = calldata_of(rec, (U(key[:32]), U(key[32:64])), hasher)
    return rec


def oracle_withdraw(rec, hasher=pr.poseidon):
    """(verdict bits, fingerprint bytes) by hashlib -> poseidon -> jj_verify; 0 where the key does not decompress or key / signature scalars are
    not residues' limbs"""
    fp = fingerprint(rec)
    s = rec["mpn_sig"]
    key = D.oracle_decompress(rec["mpn_address"]["x"], rec["mpn_address"]["odd"])
    if key is None or any(int.from_bytes(b, "little") >= R for b in (s["r"]["x"], s["r"]["y"], s["s"])):
        return 0, F(fp)
    msg = hasher([fp, rec["mpn_withdraw_nonce"]])
    sig_ok = pr.jj_verify(key, msg, ((U(s["r"]["x"]), U(s["r"]["y"])), U(s["s"])))
    call_ok = rec["payment"]["calldata"] == calldata_of(rec, key, hasher)
    return (1 if sig_ok else 0) | (2 if call_ok else 0), F(fp)


BOTH_FAIL = ("oddity flipped", "key x without a root", "nonce + 1")           # the key or the nonce enters both hashes
SIGNATURE_SIDE = ("memo byte changed", "amount + 1", "bad s", "bad R")        # the calldata check still holds: ok == 2
CALLDATA_ONLY = ("calldata byte changed", "calldata = r's limbs")             # the fingerprint blanks calldata: ok == 1
MUTATIONS = BOTH_FAIL + SIGNATURE_SIDE + CALLDATA_ONLY


def mutate(rec, which: str, rnd, hasher=pr.poseidon):
    m = copy.deepcopy(rec)
    key = D.oracle_decompress(rec["mpn_address"]["x"], rec["mpn_address"]["odd"])
    if which == "oddity flipped":
        m["mpn_address"]["odd"] = not rec["mpn_address"]["odd"]
    elif which == "key x without a root":
        m["mpn_address"]["x"] = D.no_root_x(rnd)
    elif which == "nonce + 1":
        m["mpn_withdraw_nonce"] += 1
    elif which == "memo byte changed":
        memo = rec["payment"]["memo"]
        m["payment"]["memo"] = memo[:-1] + ("Z" if memo[-1] != "Z" else "Y")
    elif which == "amount + 1":
        m["payment"]["amount"]["amount"] += 1
    elif which == "bad s":  # a signature that does not verify, with the calldata that belongs to it
        m["mpn_sig"]["s"] = F((U(rec["mpn_sig"]["s"]) + 1) % R)
        m["payment"]["calldata"] = calldata_of(m, key, hasher)
    elif which == "bad R":
        m["mpn_sig"]["r"]["x"] = F((U(rec["mpn_sig"]["r"]["x"]) + 1) % R)
        m["payment"]["calldata"] = calldata_of(m, key, hasher)
    elif which == "calldata byte changed":
        c = rec["payment"]["calldata"]
        m["payment"]["calldata"] = c[:7] + bytes([c[7] ^ 0x10]) + c[8:]
    elif which == "calldata = r's limbs":
        m["payment"]["calldata"] = D.R_LIMBS
    else:
        raise KeyError(which)
    return m


MEMO_LENGTHS = (0, 23, 24, 25, 100, 159, 160, 161, 5000)
PAYMENT_LENGTHS = (112, 135, 136, 137, 212, 271, 272, 273, 5112)  # with Ziesha ids; 212: the calldata lies across the first block's edge

_fixed = None


def fixed_list():
    """[(class, record, expected verdict bits, expected fingerprint)]: one signed withdrawal per memo length, and every mutation of four of them
    (payments of 135, 136, 212 and 5 112 bytes).  Built once per process."""
    global _fixed
    if _fixed is not None:
        return _fixed
    rnd = random.Random(20240701)
    base = [signed_withdraw(b"wd %d" % k, 1 + k, "m" * ml, ZIESHA, ZIESHA, 1000 + k, ZIESHA, k % 4) for k, ml in enumerate(MEMO_LENGTHS)]
    out = [("valid", r) + oracle_withdraw(r) for r in base]
    for r in (base[1], base[2], base[4], base[8]):
        out += [(w, m) + oracle_withdraw(m) for w in MUTATIONS for m in (mutate(r, w, rnd),)]
    _fixed = out
    return out


def non_residue_variants():
    """(the untouched record, [records with the limbs of r / all ones in place of key.x, r.x, r.y, s])"""
    rec = fixed_list()[0][1]
    out = []
    for bad in (D.R_LIMBS, D.ALL_ONES):
        for path in (("mpn_address", "x"), ("mpn_sig", "r", "x"), ("mpn_sig", "r", "y"), ("mpn_sig", "s")):
            m = copy.deepcopy(rec)
            d = m
            for k in path[:-1]:
                d = d[k]
            d[path[-1]] = bad
            out.append(m)
    return rec, out


_pool = {}


def bulk(n: int, seed: int, memo_len: int = 0, pool: int = 48):
    """n seeded records drawn from `pool` withdrawals signed over bzk_host_poseidon (pinned on pyref by tests/test_host_mpn_cpu.py), all with memos of
    memo_len bytes; of every four records one is as signed (verdict 3), one has its calldata changed (1), one its amount (2), one its nonce (0)"""
    if (seed, memo_len, pool) not in _pool:
        rnd = random.Random(seed)
        signed = [signed_withdraw(b"bulk wd %d %d" % (seed, k), 1 + k, "b" * memo_len, custom(MPN_CONTRACT), ZIESHA, 10 ** 6 + k, ZIESHA, k % 7,
                                  hasher=_host_hash) for k in range(pool)]
        variants = []
        for r in signed:
            variants.append([enc(r)] + [enc(mutate(r, w, rnd, _host_hash)) for w in ("calldata byte changed", "amount + 1", "nonce + 1")])
        _pool[(seed, memo_len, pool)] = variants
    variants = _pool[(seed, memo_len, pool)]
    rnd = random.Random(seed + 1)
    return [variants[rnd.randrange(pool)][i % 4] for i in range(n)]


# ---- admission: world A queues through bzk_mpn_push_withdraw(fingerprint = NULL), world B receives the same withdrawals as wire records
N_ACC = 6
WITHDRAWALS = [(0, 400, 2), (1, 9, 0), (0, 7, 1), (3, 55, 3), (5, 1, 0)]  # (account, amount, fee); account 0 twice: nonces 1 and 2
ZIESHA_ID = F(1)


def admission_world(dev=None):
    w = L.MpnWorld(3, 3)
    if dev is not None:
        w.set_device(dev)
    for i in range(N_ACC):
        w.add_account(i, b"acct%d" % i, ZIESHA_ID, 10 ** 9)
    w.set_height(5)
    return w


def world_a(vks=sc.VKS, reward=10, which=WITHDRAWALS):
    """(the work's bytes, the root after it, the withdrawals cut out of the encoded work as records)"""
    a = admission_world()
    for acct, amount, fee in which:
        a.push_withdraw(acct, ZIESHA_ID, amount, ZIESHA_ID, fee)
    blob = a.make_work(1, vks, reward, log4_batches=(1, 2, 1)).encode()
    work = B.decode(B.MpnWork, blob)
    kind, transitions = work["data"]
    assert kind == "Withdraw"
    recs = [t["tx"] for t in transitions if t["enabled"]]
    assert len(recs) == len(which)
    return blob, a.root(), recs


def bad_withdrawals(good):
    """(class, record) that admission must refuse; each is a well-formed record"""
    rnd = random.Random(5)
    wrong_id = resigned(b"acct1", 1, 9, 0, custom(MPN_CONTRACT + 1), 0)   # both checks hold: refused on the id alone
    circuit1 = resigned(b"acct3", 1, 55, 3, custom(MPN_CONTRACT), 1)
    return [("bad signature", mutate(good[0], "bad s", rnd, _host_hash)), ("bad calldata", mutate(good[2], "calldata byte changed", rnd)),
            ("wrong contract id", wrong_id), ("circuit id 1", circuit1)]


def resigned(seed: bytes, nonce: int, amount: int, fee: int, contract_id, circuit: int):
    """a withdrawal whose signature and calldata are valid for a payment that admission must refuse on its contract id / circuit id alone"""
    return signed_withdraw(seed, nonce, "", contract_id, ZIESHA, amount, ZIESHA, fee, circuit, hasher=_host_hash)


def admit(world, recs):
    return world.push_withdraws(b"".join(enc(r) for r in recs), len(recs))
