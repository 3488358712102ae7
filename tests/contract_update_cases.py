"""Inputs and expected values of the wire-form ContractUpdate tests (tests/test_contract_updates_cpu.py, tests/test_gpu_contract_updates.py).
No tests here.

Keys and proofs come from the CPU oracle (oracle/coracle.py) the way tests/verify_cases.py makes them, over a "free-input" R1CS: the constraint
structure of util.synth_r1cs(40, n_in=6) - it depends on the seed only - with z computed from GIVEN public inputs, because the five inputs of an
update's proof (commit, height, state, aux, next_state) are dictated by its record.  One key per function, distinct seeds: two deposit functions
(capacities 1 and 3), two withdraw functions (0 and 2), two plain functions.

Records are encoded by the schema combinators of tests/bincode_ref.py and the values of tests/l1_tx_cases.py; deposits are signed with the
suite's Python Ed25519 (tests/ed25519_cases.py).  Expected values never come from the code under test:

  aux     tests/pystate.compress on the pairs deposit.rs:16-55, withdraw.rs:16-72 and function_call.rs:28-44 build
  commit  hashlib.sha3_256 of bincode((prover, reward)), as a residue                        update_contract/mod.rs:29-32
  fingerprint  hashlib.sha3_256 of the withdrawal re-encoded with calldata = 0               src/core/transaction.rs:204-211
  PROOF   oracle/pyref.groth16_verify over (commit, height, prev state, aux, next_state)     src/zk/mod.rs:157-193"""
import functools
import hashlib
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bincode_ref as B
import ed25519_cases as E
import l1_tx_cases as X
import pystate
from oracle import pyref as pr
from util import fr_bytes, fr_list, log2_ceil, r1cs_to_csr

PROOF, SIGS, ROUTE, UNSUPPORTED = 1, 2, 4, 0x80
R = pr.R_MOD
F = pr.fr_to_mont_bytes
CID = ("Custom", X.scalar("updates cid"))
CID_BYTES = CID[1]                      # the contract's scalar as the descriptor takes it: Montgomery limbs
OTHER_CID = ("Custom", X.scalar("another cid"))
KIWI = ("Custom", X.scalar("kiwi token"))
DEPOSIT_CAPS, WITHDRAW_CAPS, N_FNS = (1, 3), (0, 2), 2

ContractUpdateData = B.Enum(("Deposit", B.Struct(("deposits", B.Vec(B.ContractDeposit)))), ("Withdraw", B.Struct(("withdraws", B.Vec(B.ContractWithdraw)))),
                            ("FunctionCall", B.Struct(("fee", B.Money))), ("Mint", B.Struct(("amount", B.U64))))
ContractUpdate = B.Struct(("circuit_id", B.U32), ("data", ContractUpdateData), ("next_state", B.ZkCompressedState), ("prover", B.L1PublicKey),
                          ("reward", B.U64), ("proof", B.ZkProof))
FIELD_ORDER = ("circuit_id", "data", "next_state", "prover", "reward", "proof")


# ---- the free-input R1CS
def r1cs_structure(n_mul, n_in, seed, fan=3):
    """util.synth_r1cs's rows for this seed, without its z: [(A, B, C, fresh)] where fresh is None (the new variable is <A,z> <B,z>) or the 0/1
    value of a boolean-style row.  The draws are synth_r1cs's, in its order, so the structure is the one it would build."""
    rnd = random.Random(seed)
    for _ in range(n_in - 1):
        rnd.randrange(R)
    rows, nv = [], n_in
    for k in range(n_mul):
        A = [(rnd.randrange(nv), rnd.randrange(1, R) if rnd.random() < 0.5 else rnd.choice([1, 2, R - 1])) for _ in range(rnd.randint(1, fan))]
        Bm = [(rnd.randrange(nv), rnd.randrange(1, R) if rnd.random() < 0.5 else 1) for _ in range(rnd.randint(1, fan))]
        if k % 7 == 3:
            rows.append(([(nv, 1)], [(0, 1), (nv, R - 1)], [], rnd.randint(0, 1)))
        else:
            rows.append((A, Bm, [(nv, 1)], None))
        nv += 1
    for i in range(n_in):
        rows.append(([(i, 1)], [], [], False))
    return rows


def r1cs_witness(rows, n_in, inputs):
    z = [1] + [x % R for x in inputs]
    assert len(z) == n_in
    for A, Bm, Cm, fresh in rows:
        if fresh is False:
            continue
        if fresh is not None:
            z.append(fresh)
        else:
            z.append(sum(c * z[v] for v, c in A) % R * (sum(c * z[v] for v, c in Bm) % R) % R)
    return z


class Key:
    """one function's circuit: its verifying key (bincode) and a prover for any five inputs"""

    def __init__(self, seed):
        from oracle import coracle as co
        co.build()
        co.lib()
        self.co, self.seed = co, seed
        self.rows = r1cs_structure(40, 6, seed)
        r1 = {"n_in": 6, "rows": [(a, b, c) for a, b, c, _ in self.rows]}
        self.csr = r1cs_to_csr(co, r1)
        n_aux = len(r1cs_witness(self.rows, 6, [0] * 5)) - 6
        self.params = co.groth16_setup(*self.csr, 6, n_aux, log2_ceil(len(self.rows)), fr_bytes(fr_list(5, 1000 + seed)))
        self.vk = self.params["vk"] + (len(self.params["ic"]) // 97).to_bytes(8, "little") + self.params["ic"]
        self.pyvk = pr.vk_from_bytes(self.vk)

    def prove(self, inputs) -> bytes:
        zb = fr_bytes(r1cs_witness(self.rows, 6, inputs))
        az, bz, cz = self.co.r1cs_eval(*self.csr, zb)
        rs = fr_bytes(fr_list(2, int.from_bytes(hashlib.sha3_256(zb).digest()[:6], "little")))   # (r, s) from the assignment: no call order in a proof
        return self.co.groth16_prove(self.params, zb, az, bz, cz, rs[:32], rs[32:])


@functools.lru_cache(maxsize=None)
def key(kind: str, index: int) -> Key:
    # seeds whose structure the oracle's setup accepts (621 draws a row in which one variable's coefficients cancel: a query point at infinity)
    return Key({"Deposit": 610, "Withdraw": 640, "FunctionCall": 630}[kind] + index)


@functools.lru_cache(maxsize=None)
def tables():
    """(deposit_fns, withdraw_fns, fns) as the descriptor takes them"""
    return ([(key("Deposit", i).vk, c) for i, c in enumerate(DEPOSIT_CAPS)], [(key("Withdraw", i).vk, c) for i, c in enumerate(WITHDRAW_CAPS)],
            [key("FunctionCall", i).vk for i in range(N_FNS)])


def desc(L, deposit_fns=None, withdraw_fns=None, fns=None, contract_id=CID_BYTES):
    d, w, f = tables()
    return L.ContractDesc(contract_id, d if deposit_fns is None else deposit_fns, w if withdraw_fns is None else withdraw_fns, f if fns is None else fns)


# ---- values
def token_int(tok) -> int:
    return {"Null": 0, "Ziesha": 1}.get(tok[0]) if tok[0] != "Custom" else pr.fr_from_mont_bytes(tok[1])


def deposit(i: int, circuit_id: int, contract_id=CID, signed=True, seed=None, token=X.ZIESHA):
    seed = seed or b"update wallet %d" % (i % 5)
    d = {"memo": "dep %d" % i if i % 3 else "", "contract_id": contract_id, "deposit_circuit_id": circuit_id, "calldata": X.scalar("dep calldata %d" % i),
         "src": E.public_key(seed), "amount": X.money(100 + i, token), "fee": X.money(i % 4), "nonce": 1 + i, "sig": None}
    if signed:
        d["sig"] = E.sign(seed, B.encode(B.ContractDeposit, d))
    return d


def withdraw(i: int, circuit_id: int, contract_id=CID, token=X.ZIESHA):
    return {"memo": "wd memo %d" % i if i % 2 else "", "contract_id": contract_id, "withdraw_circuit_id": circuit_id,
            "calldata": X.scalar("wd calldata %d" % i), "dst": X._blob("dst %d" % i, 32), "amount": X.money(50 + i, token),
            "fee": X.money(1 + i % 3, KIWI if i % 4 == 1 else X.ZIESHA)}


def fingerprint(w) -> int:
    return int.from_bytes(hashlib.sha3_256(B.encode(B.ContractWithdraw, dict(w, calldata=bytes(32)))).digest(), "little") % R


def aux_of(kind: str, payload, capacity: int) -> int:
    """aux_data.state_hash by the reference's three functions, restated on tests/pystate.compress"""
    sc = ("scalar",)
    if kind == "Deposit":
        pairs = {}
        for i, d in enumerate(payload["deposits"]):
            pairs.update({(i, 0): 1, (i, 1): token_int(d["amount"]["token_id"]), (i, 2): d["amount"]["amount"], (i, 3): pr.fr_from_mont_bytes(d["calldata"])})
        return pystate.compress(("list", capacity, ("struct", [sc] * 4)), pairs)[0]
    if kind == "Withdraw":
        pairs = {}
        for i, w in enumerate(payload["withdraws"]):
            pairs.update({(i, 0): 1, (i, 1): token_int(w["amount"]["token_id"]), (i, 2): w["amount"]["amount"], (i, 3): token_int(w["fee"]["token_id"]),
                          (i, 4): w["fee"]["amount"], (i, 5): fingerprint(w), (i, 6): pr.fr_from_mont_bytes(w["calldata"])})
        return pystate.compress(("list", capacity, ("struct", [sc] * 7)), pairs)[0]
    fee = payload["fee"]
    return pystate.compress(("struct", [sc, sc]), {(0,): token_int(fee["token_id"]), (1,): fee["amount"]})[0]


def commit_of(prover: bytes, reward: int) -> int:
    return int.from_bytes(hashlib.sha3_256(B.encode(B.L1PublicKey, prover) + B.encode(B.U64, reward)).digest(), "little") % R


def capacity_of(kind, circuit_id):
    return {"Deposit": DEPOSIT_CAPS, "Withdraw": WITHDRAW_CAPS}.get(kind, (0,) * N_FNS)[circuit_id]


def make_update(kind, circuit_id, payload, height, prev: bytes, tag: str, prove=True, reward=77, recorded=False, nxt=None):
    """a ContractUpdate (as a value) of function (kind, circuit_id) with a proof for (commit, height, prev, aux, its own next_state); prove False:
    a garbage proof.  recorded: the proof is the one the fixture file holds under `tag` (no oracle is run and aux is not computed).
    -> (value, aux int or None where the payload does not fit the function)"""
    prover = X._blob("prover " + tag, 32)
    nxt = nxt or X.scalar("next state " + tag)
    pf = aux = None
    if recorded:
        pf = recorded_proofs().get(tag) if prove else None
    else:
        try:
            aux = aux_of(kind, payload, capacity_of(kind, circuit_id))
        except ValueError:
            pass
        if prove and aux is not None:
            pf = key(kind, circuit_id).prove([commit_of(prover, reward), height, pr.fr_from_mont_bytes(prev), aux, pr.fr_from_mont_bytes(nxt)])
    if pf is not None:
        proof = ("Groth16", {"a": pf[:97], "b": pf[97:290], "c": pf[290:]})
    else:
        proof = X.zk_proof("garbage " + tag)
    return {"circuit_id": circuit_id, "data": (kind, payload), "next_state": {"state_hash": nxt, "state_size": 9}, "prover": prover, "reward": reward,
            "proof": proof}, aux


def enc(u) -> bytes:
    return B.encode(ContractUpdate, u)


def proof_bytes(u) -> bytes:
    p = u["proof"][1]
    return p["a"] + p["b"] + p["c"]


def expected(updates, counts, height0, state0: bytes, deposit_caps=DEPOSIT_CAPS, withdraw_caps=WITHDRAW_CAPS, n_fns=N_FNS):
    """(ok bytes, aux n x 32, commit n x 32) of update VALUES by the restatements: the semantics of bzk_contract_updates_check written down again"""
    ok, auxs, commits, prev, i = bytearray(), b"", b"", state0, 0
    for j, c in enumerate(counts):
        for u in updates[i:i + c]:
            kind, payload = u["data"]
            commit = commit_of(u["prover"], u["reward"])
            commits += F(commit)
            nxt = u["next_state"]["state_hash"]
            if kind == "Mint":
                ok.append(UNSUPPORTED)
                auxs += bytes(32)
                prev = nxt
                continue
            caps = {"Deposit": deposit_caps, "Withdraw": withdraw_caps, "FunctionCall": (0,) * n_fns}[kind]
            pays = payload.get("deposits", payload.get("withdraws", []))
            cfield = "deposit_circuit_id" if kind == "Deposit" else "withdraw_circuit_id"
            route = u["circuit_id"] < len(caps) and len(pays) <= 4 ** caps[min(u["circuit_id"], len(caps) - 1)] and all(
                p["contract_id"] == CID and p[cfield] == u["circuit_id"] for p in pays)
            sigs = all(p["sig"] is not None and E.verify(p["src"], B.encode(B.ContractDeposit, dict(p, sig=None)), p["sig"]) for p in pays) \
                if kind == "Deposit" else True
            bits = (SIGS if sigs else 0) | (ROUTE if route else 0)
            aux = aux_of(kind, payload, caps[u["circuit_id"]]) if route else 0
            auxs += F(aux)
            if route:
                canon = all(int.from_bytes(b, "little") < R for b in (prev, nxt))  # limbs >= r are no scalar: the wire-form calls answer 0
                a, b2, c2 = proof_bytes(u)[:97], proof_bytes(u)[97:290], proof_bytes(u)[290:]
                try:
                    pf = (pr.g1_from_bytes(a), pr.g2_from_bytes(b2), pr.g1_from_bytes(c2))
                except Exception:
                    pf = None
                if canon and pf is not None and pr.groth16_verify(key(kind, u["circuit_id"]).pyvk, [commit, height0 + j, pr.fr_from_mont_bytes(prev), aux,
                                                                                                  pr.fr_from_mont_bytes(nxt)], pf):
                    bits |= PROOF
            ok.append(bits)
            prev = nxt
        i += c
    return bytes(ok), auxs, commits


# ---- the positive chain: 3 transactions with (2, 3, 1) updates, all three kinds and both functions of each
HEIGHT0 = 41
STATE0 = X.scalar("updates state0")
CHAIN_COUNTS = (2, 3, 1)


@functools.lru_cache(maxsize=None)
def chain(recorded=False):
    """(update values, counts): every update valid given its predecessor's claim, at heights HEIGHT0 + transaction"""
    plan = [("Deposit", 0, {"deposits": [deposit(k, 0) for k in range(3)]}), ("FunctionCall", 1, {"fee": X.money(4)}),
            ("Withdraw", 1, {"withdraws": [withdraw(k, 1, token=KIWI if k == 2 else X.ZIESHA) for k in range(5)]}),
            ("Deposit", 1, {"deposits": [deposit(10 + k, 1, token=KIWI if k == 1 else X.ZIESHA) for k in range(6)]}),
            ("FunctionCall", 0, {"fee": X.money(9, KIWI)}), ("Withdraw", 0, {"withdraws": [withdraw(9, 0)]})]
    out, prev, i = [], STATE0, 0
    for j, c in enumerate(CHAIN_COUNTS):
        for kind, cid, payload in plan[i:i + c]:
            u, _ = make_update(kind, cid, payload, HEIGHT0 + j, prev, "chain %d" % len(out), recorded=recorded)
            out.append(u)
            prev = u["next_state"]["state_hash"]
        i += c
    return tuple(out), CHAIN_COUNTS


# ---- payment counts: one update per row, each its own call's first update (checked against STATE0 at HEIGHT0)
COUNT_ROWS = (("Deposit", 0, 0), ("Deposit", 0, 1), ("Deposit", 0, 3), ("Deposit", 0, 4), ("Deposit", 0, 5),
              ("Deposit", 1, 0), ("Deposit", 1, 1), ("Deposit", 1, 15), ("Deposit", 1, 16), ("Deposit", 1, 17), ("Deposit", 1, 63), ("Deposit", 1, 64),
              ("Deposit", 1, 65), ("Withdraw", 0, 0), ("Withdraw", 0, 1), ("Withdraw", 1, 0), ("Withdraw", 1, 7), ("Withdraw", 1, 16))


@functools.lru_cache(maxsize=None)
def count_rows(recorded=False):
    """[(label, update value)] for COUNT_ROWS; deposits are drawn from a pool of eight signed payments per function"""
    out = []
    for kind, cid, k in COUNT_ROWS:
        if kind == "Deposit":
            payload = {"deposits": [_pool_deposit(cid, q % 8) for q in range(k)]}
        else:
            payload = {"withdraws": [withdraw(q, cid) for q in range(k)]}
        u, _ = make_update(kind, cid, payload, HEIGHT0, STATE0, "count %s %d %d" % (kind, cid, k), recorded=recorded)
        out.append(("%s fn %d x %d" % (kind, cid, k), u))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _pool_deposit(circuit_id, q):
    return deposit(100 + q, circuit_id)


# ---- one fault per row
@functools.lru_cache(maxsize=None)
def fault_rows(recorded=False):
    """[(label, update value, the one bit that must be clear - or UNSUPPORTED for the Mint)]; each is a call's first update"""
    def dep(pays, tag, cid=0, **kw):
        return make_update("Deposit", cid, {"deposits": pays}, HEIGHT0, STATE0, tag, recorded=recorded, **kw)[0]

    def call(cid, fee, tag):
        return make_update("FunctionCall", cid, {"fee": X.money(fee)}, HEIGHT0, STATE0, tag, recorded=recorded)[0]
    good = [deposit(200, 0), deposit(201, 0)]
    bad_sig = dict(good[1], sig=X.flip(good[1]["sig"], 40, 2))
    rows = [("a deposit with a wrong signature", dep([good[0], bad_sig], "f sig"), SIGS),
            ("sig: None", dep([good[0], dict(good[1], sig=None)], "f none"), SIGS),
            ("a payment of another contract", dep([good[0], deposit(202, 0, contract_id=OTHER_CID)], "f cid", prove=False), ROUTE),
            ("a payment of another circuit", dep([good[0], deposit(203, 1)], "f circuit", prove=False), ROUTE),
            ("circuit_id one past the table", dict(call(0, 1, "f past"), circuit_id=N_FNS), ROUTE)]
    u = call(0, 2, "f tamper")
    p = dict(u["proof"][1])
    p["c"] = X.flip(p["c"], 3)
    rows.append(("a tampered proof", dict(u, proof=("Groth16", p)), PROOF))
    u = call(1, 3, "f other key")
    rows.append(("the proof of another function's key", dict(u, circuit_id=0), PROOF))
    u = call(0, 5, "f limbs")
    raised = (int.from_bytes(u["next_state"]["state_hash"], "little") + R).to_bytes(32, "little")
    rows.append(("next_state limbs >= r", dict(u, next_state={"state_hash": raised, "state_size": 9}), PROOF))
    rows.append(("a Mint", X.contract_update("Mint", {"amount": 3}, "f mint"), UNSUPPORTED))
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def repeatable_call(recorded=False):
    """one valid FunctionCall update whose next_state is STATE0: repeated in ONE transaction every copy stays valid"""
    u = make_update("FunctionCall", 0, {"fee": X.money(6)}, HEIGHT0, STATE0, "repeat", reward=5, recorded=recorded, nxt=STATE0)[0]
    return dict(u, next_state={"state_hash": STATE0, "state_size": 1})


def tampered(u):
    p = dict(u["proof"][1])
    p["c"] = X.flip(p["c"], 3)
    return dict(u, proof=("Groth16", p))


# ---- the round-crossing deposit updates: eight signed payments of deposit function 1, 64 per update, rotated by the update's index
def crossing_update(i: int, recorded=False):
    """update i of the payment-round test: 64 deposits (the pool's eight, starting at i mod 8), a garbage proof.  -> (value, aux)"""
    return make_update("Deposit", 1, {"deposits": [_pool_deposit(1, (q + i) % 8) for q in range(64)]}, HEIGHT0, STATE0, "crossing %d" % (i % 8), prove=False,
                       recorded=recorded)


# ---- long records: a Withdraw update of circuit 1 whose k withdrawals carry memos of memo_len bytes (the same withdrawal k times), next_state
# STATE0 so that what follows it in a transaction is still checked against STATE0, a garbage proof
def long_withdraw_update(k: int, memo_len: int):
    w = dict(withdraw(7, 1), memo="m" * memo_len)
    return {"circuit_id": 1, "data": ("Withdraw", {"withdraws": [w] * k}), "next_state": {"state_hash": STATE0, "state_size": 3},
            "prover": X._blob("prover long", 32), "reward": 2, "proof": X.zk_proof("garbage long")}


def long_withdraw_record(k: int, memo_len: int) -> bytes:
    """enc(long_withdraw_update(k, memo_len)) without encoding the withdrawal k times"""
    one = enc(long_withdraw_update(1, memo_len))
    pay = B.encode(B.ContractWithdraw, dict(withdraw(7, 1), memo="m" * memo_len))
    assert one[16:16 + len(pay)] == pay
    return one[:8] + B.encode(B.U64, k) + pay * k + one[16 + len(pay):]


# ---- what is expensive about the cases, as recorded under tests/golden: the six keys, every proof (by the tag its update was made under) and
# the oracles' answers.  With them the generators above rebuild every record without the CPU oracle (recorded=True: signatures and encodings
# are cheap and deterministic), which is what the GPU tests do; tests/test_contract_updates_cpu.py checks the file against a fresh run of
# everything above, `python tests/contract_update_cases.py` rewrites it
FIXTURE = "contract_update_cases.json"      # the oracles' answers, and the order of what the binary file holds
FIXTURE_BIN = "contract_update_cases.bin"    # the six keys (1 460 bytes each: deposit, withdraw, plain functions), then the proofs (387 each)


def build_fixture():
    ups, counts = chain()
    ok, aux, commit = expected(list(ups), counts, HEIGHT0, STATE0)
    d, w, f = tables()
    proofs = {}

    def note(tag, u):
        if u["proof"] != X.zk_proof("garbage " + tag):
            proofs[tag] = proof_bytes(u)

    def row(label, u, extra=None):
        o, a, c = expected([u], (1,), HEIGHT0, STATE0)
        return dict({"label": label, "ok": o[0], "aux": a.hex(), "commit": c.hex()}, **(extra or {}))
    for i, u in enumerate(ups):
        note("chain %d" % i, u)
    for (kind, cid, k), (_, u) in zip(COUNT_ROWS, count_rows()):
        note("count %s %d %d" % (kind, cid, k), u)
    by_label = {label: u for label, u, _ in fault_rows()}
    for tag, label in (("f sig", "a deposit with a wrong signature"), ("f none", "sig: None"), ("f past", "circuit_id one past the table"),
                       ("f other key", "the proof of another function's key"), ("f limbs", "next_state limbs >= r")):
        note(tag, by_label[label])
    proofs["f tamper"] = proof_bytes(tampered(by_label["a tampered proof"]))   # flipping the same bit again gives the proof back
    rep = repeatable_call()
    note("repeat", rep)
    return {"what": "the cases of tests/contract_update_cases.py: keys and proofs by the CPU oracle, expected values by its restatements (build_fixture())",
            "proof_tags": list(proofs), "chain": {"ok": ok.hex(), "aux": aux.hex(), "commit": commit.hex()},
            "count_rows": [row(label, u) for label, u in count_rows()],
            "fault_rows": [row(label, u, {"bit": bit}) for label, u, bit in fault_rows()],
            "repeatable_aux": F(aux_of("FunctionCall", rep["data"][1], 0)).hex(), "repeatable_commit": F(commit_of(rep["prover"], rep["reward"])).hex(),
            "crossing_aux": [F(crossing_update(i)[1]).hex() for i in range(8)]}, \
        b"".join(vk for vk, _ in d + w) + b"".join(f) + b"".join(proofs.values())


@functools.lru_cache(maxsize=None)
def fixture():
    import json
    with open(os.path.join(E.GOLDEN, FIXTURE)) as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=None)
def fixture_bin() -> bytes:
    with open(os.path.join(E.GOLDEN, FIXTURE_BIN), "rb") as fh:
        return fh.read()


@functools.lru_cache(maxsize=None)
def recorded_proofs():
    blob, tags = fixture_bin()[6 * 1460:], fixture()["proof_tags"]
    assert len(blob) == 387 * len(tags)
    return {tag: blob[387 * i:387 * i + 387] for i, tag in enumerate(tags)}


def recorded_tables(deposit_caps=DEPOSIT_CAPS, withdraw_caps=WITHDRAW_CAPS):
    """(deposit_fns, withdraw_fns, fns) as tables() gives them, from the recorded keys"""
    vks = [fixture_bin()[1460 * i:1460 * i + 1460] for i in range(6)]
    return list(zip(vks[0:2], deposit_caps)), list(zip(vks[2:4], withdraw_caps)), vks[4:6]


def fixture_desc(L, **caps):
    return L.ContractDesc(CID_BYTES, *recorded_tables(**caps))


if __name__ == "__main__":
    import json
    answers, binary = build_fixture()
    with open(os.path.join(E.GOLDEN, FIXTURE), "w") as fh:
        json.dump(answers, fh, indent=0)
        fh.write("\n")
    with open(os.path.join(E.GOLDEN, FIXTURE_BIN), "wb") as fh:
        fh.write(binary)
