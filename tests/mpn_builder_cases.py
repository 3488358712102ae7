"""Inputs and hand-written verdicts of the witness-builder tests (tests/test_mpn_builder_cpu.py, tests/test_gpu_mpn_builder.py): per kind a
small deterministic world and ONE queue, pushed up front and longer than the batch capacity, in which accepted transactions are interleaved with
one transaction per acceptance rule of `update::update`, `deposit::deposit`, `withdraw::withdraw` (bazuka_amd/csrc/mpn.hip) that the push calls
of the C ABI can reach.  A case is drained by repeated builder calls; per call the test compares WHICH transactions the work holds (every
transaction of a queue has its own amount, which names it) with the lists written down here from the rules, and the work bytes' sha256 and
the root with tests/golden/mpn_builder_cases.json, recorded from the host builder before it was rewritten (tests/golden/make_mpn_builder_cases.py).

An entry of a queue: (arguments of its push call, verdict, rule).  Key arguments are NAMES resolved by the world (an account's slot, or the
handle a key was registered under); verdict "accept" or "reject"; the rule is the line of the walk that decides it.

Rules the ABI cannot reach, by the walk's own test (none of them is exercised here, or anywhere else in the suite):
  update    a key off the curve (push_tx takes keys from seeds; push_txs admits only records whose keys decompress);
            `src_before.address != tx.src_pub` and `dst_before.address != tx.dst_pub` (the walk finds both slots BY address, or takes an empty one);
            `dst slot holds another token` and `src_token.token_id != tx.amount.token_id` (find_token_index returns the slot OF that token, or a
            free one); `dti < 0`, no free slot at the destination (4^log4_tree slots are searched: at 3 / 2 and 15 / 3 that is more than the
            token tree has leaves, so the rule cannot fire before a write leaves the tree); `!src_after.tokens.count(sfi)` and
            `src_fee_token.token_id != tx.fee.token_id` (sfi is the slot of that token);
  deposit   `tx.mpn_address != acc.address` and `slot holds another token`, for the same reasons; `no free token slot` is out of reach at
            3 / 2 for the reason above, and is reached at 3 / 3, where the 4^3 slots searched are the token tree's own (the case "deposit_full");
  withdraw  `tx.mpn_address != acc.address`, `!acc.tokens.count(ti)`, `tx.amount.token_id != acc_token.token_id`, `!upd.tokens.count(fi)`,
            `tx.fee.token_id != acc_fee.token_id`; and, for a WORK: a bad signature and a stale nonce - push_withdraw signs by itself and numbers
            by queue position (so only a gap, never a stale nonce), and what push_withdraw_signed queues has no payment and so no wire form
            (bzk_mpn_make_work refuses such a queue).  Those two run through bzk_mpn_withdraw_synthesize instead (the case "withdraw_signed"),
            where the instance's z bytes stand in for the work bytes and only the COUNTS of the verdicts can be compared.
"""
import hashlib
import json
import os

import bincode_ref as B
import r1cs_scenarios as sc
from bazuka_amd import lib as L
from oracle import pyref as pr

F = pr.fr_to_mont_bytes
Z, K, UNKNOWN = F(1), F(777), F(999)          # Ziesha, a custom token some accounts hold, a token nobody holds
GOLDEN = os.path.join(sc.G, "mpn_builder_cases.json")
A, R = "accept", "reject"


def _slots(log4_tree, n):
    """n account slots: 0 .. n-1 in the small tree, scattered over the large one (so that the planner's (tree, index) keys differ in both halves)"""
    return list(range(n)) if log4_tree <= 3 else [(i * 7919 + 3) % 4 ** log4_tree for i in range(n)]


# ---- update: 8 funded accounts a0 .. a7 (1000 Ziesha each); a1 also holds 50 of K; "tokonly" holds 30 of K and no Ziesha (both by a deposit
# work before the queue); "newcomer" has a key and no account yet; "ghost" has a key and never gets an account.  Capacity 4.
UPDATE_QUEUE = [
    # (src, dst, token, amount, fee token, fee), verdict, rule
    (("a0", "a1", Z, 101, Z, 1), A, "plain transfer"),
    (("a3", "a3", Z, 102, Z, 2), A, "self-transfer: the destination is read after the sender's write"),
    (("a5", "a2", Z, 103, K, 1), R, "wrong fee token"),
    (("a0", "newcomer", Z, 104, Z, 0), A, "to a slot that does not exist yet"),
    (("a5", "a2", Z, 105, Z, 1), R, "nonce gap: numbered 2 by queue position, a5's first was rejected"),
    (("a2", "a0", UNKNOWN, 106, Z, 1), R, "unknown source token"),
    (("a4", "newcomer", Z, 107, Z, 3), A, "the new account receives a second time"),          # batch 1 is full here
    (("newcomer", "a2", Z, 108, Z, 1), A, "the new account sends"),
    (("a4", "a0", Z, 5000, Z, 1), R, "overspend"),
    (("ghost", "a0", Z, 110, Z, 0), R, "unknown sender"),
    (("tokonly", "a1", K, 11, Z, 0), R, "fee token missing at the sender"),
    (("a1", "a6", K, 12, Z, 4), A, "custom token into a free slot of the destination, fee in Ziesha"),
    (("a3", "a4", Z, 995, Z, 5), R, "fee larger than what is left after the amount (998 - 995 < 5)"),
    (("a7", "tokonly", Z, 114, Z, 0), A, "second token for an existing account"),
    (("a1", "a6", K, 15, Z, 1), A, "the same destination slot again"),                        # batch 2 is full here
    (("a6", "a0", Z, 116, Z, 1), A, "plain transfer"),
    (("a7", "a7", Z, 5, Z, 2000), R, "fee larger than the balance"),
]

# ---- deposit at 3 / 2: 3 funded accounts; two keys without accounts.  No rejection rule is reachable at this shape (module docstring).
DEPOSIT_QUEUE = [
    # (key, token, amount)
    (("a0", Z, 301), A, "existing token of an existing account"),
    (("fresh0", K, 302), A, "new account"),
    (("a1", K, 303), A, "second token for an existing account"),
    (("fresh0", Z, 304), A, "second token for the account this batch created"),                # batch 1 is full here
    (("fresh1", Z, 305), A, "new account after a new account"),
    (("a1", K, 306), A, "the slot the previous batch created"),
]


# ---- deposit at 3 / 3: account a0 (Ziesha in slot 0) receives 63 further tokens, one per slot; then a 65th
def deposit_full_queue():
    q = [(("a0", F(1000 + k), 400 + k), A, "token %d into the next free slot" % k) for k in range(63)]
    q += [(("a0", F(5000), 470), R, "no free token slot"),
          (("a0", Z, 471), A, "existing token of the full account"),
          (("a1", F(5000), 472), A, "the same token into an account that has room")]
    return q


# ---- withdraw: 5 funded accounts; a1 also holds 50 of K; "tokonly" holds 30 of K only; "ghost" has a key and no account.  Capacity 4.
WITHDRAW_QUEUE = [
    # (account, token, amount, fee token, fee)
    (("a0", Z, 201, Z, 1), A, "plain"),
    (("ghost", Z, 202, Z, 0), R, "unknown account"),
    (("a1", K, 20, Z, 3), A, "amount and fee in two slots"),
    (("a2", UNKNOWN, 204, Z, 1), R, "unknown token"),
    (("a0", Z, 205, Z, 2), A, "second withdrawal of an account in one batch"),
    (("a3", Z, 5000, Z, 1), R, "overdraw"),
    (("tokonly", K, 7, Z, 1), R, "fee token missing"),
    (("a4", Z, 208, Z, 0), A, "plain"),                                                        # batch 1 is full here
    (("a3", Z, 209, Z, 1), R, "nonce gap: numbered 2 by queue position, a3's first was rejected"),
    (("a4", Z, 790, Z, 5), R, "fee larger than what is left after the amount (792 - 790 < 5)"),
    (("a1", Z, 211, K, 40), R, "fee larger than the balance of its slot (30 of K left)"),
    (("a0", Z, 212, Z, 0), A, "third withdrawal, on the state of the previous batch"),
    (("a0", Z, 213, Z, 1), A, "and a fourth"),
]

# ---- withdraw with signatures made elsewhere (push_withdraw_signed; bzk_mpn_withdraw_synthesize): (signer seed, nonce, amount, fee, damage)
WITHDRAW_SIGNED_QUEUE = [
    ((b"acct0", 1, 51, 1, None), A, "plain"),
    ((b"acct1", 1, 52, 1, "flip"), R, "bad signature: one byte of s flipped"),
    ((b"acct0", 1, 53, 1, None), R, "stale nonce: well signed, the account's nonce has moved to 1"),
    ((b"stranger", 1, 54, 0, None), R, "unknown account"),
    ((b"acct0", 2, 55, 0, None), A, "the next nonce of the same account"),
    ((b"acct2", 1, 56, 2, None), A, "plain"),
    ((b"acct3", 1, 57, 0, None), A, "plain"),                                                 # batch 1 is full here
    ((b"acct4", 1, 58, 1, None), A, "left for the second call"),
]

# name -> (kind, log4_tree, log4_token_tree, queue)
CASES = {
    "update_3_2": ("update", 3, 2, UPDATE_QUEUE),
    "update_15_3": ("update", 15, 3, UPDATE_QUEUE),
    "deposit_3_2": ("deposit", 3, 2, DEPOSIT_QUEUE),
    "deposit_full_3_3": ("deposit", 3, 3, deposit_full_queue()),
    "withdraw_3_2": ("withdraw", 3, 2, WITHDRAW_QUEUE),
    "withdraw_signed_3_2": ("withdraw_signed", 3, 2, WITHDRAW_SIGNED_QUEUE),
}
LOG4_BATCH = 1
CAP = 4 ** LOG4_BATCH


AMOUNT_AT = {"update": 3, "deposit": 2, "withdraw": 2, "withdraw_signed": 2}   # where an entry's arguments hold the amount that names it


def expected_batches(name):
    """the walk's cut, by hand: a call takes transactions in queue order until CAP are accepted; what it rejected on the way is dropped, the
    rest waits for the next call.  -> [(amounts accepted, number rejected)] per call"""
    kind, _, _, queue = CASES[name]
    out, acc, rej = [], [], 0
    for args, verdict, _ in queue:
        if len(acc) == CAP:
            out.append((acc, rej))
            acc, rej = [], 0
        if verdict == A:
            acc.append(args[AMOUNT_AT[kind]])
        else:
            rej += 1
    out.append((acc, rej))
    return out


def _world(kind, log4_tree, log4_token_tree, dev):
    """-> (world, name -> key handle).  Funded accounts at _slots(); the other keys under handles at the top of the tree, where no account lives
    (push_tx / push_withdraw number a transaction from the account AT the handle)"""
    w = L.MpnWorld(log4_tree, log4_token_tree)
    if dev is not None:
        w.set_device(dev)
    n = 8 if kind == "update" else 5 if kind.startswith("withdraw") else 3
    names = {}
    for i, s in enumerate(_slots(log4_tree, n)):
        w.add_account(s, b"acct%d" % i, Z, 1000)
        names["a%d" % i] = s
    for j, extra in enumerate(("tokonly", "newcomer", "ghost", "fresh0", "fresh1")):
        names[extra] = 4 ** log4_tree - 2 - j
        w.add_key(names[extra], extra.encode())
    w.set_height(7)
    if kind in ("update", "withdraw"):  # the second tokens, by a deposit work of the world's own (not part of what the case compares)
        w.push_deposit(names["a1"], K, 50)
        w.push_deposit(names["tokonly"], K, 30)
        assert w.make_work(0, sc.VKS, 1, log4_batches=(LOG4_BATCH,) * 3).n_transitions == 2
    return w, names


def signed_withdraw(seed, nonce, amount, fee, damage):
    key = L.host_jubjub_keys(seed)
    fingerprint = F(9000 + amount)
    sig = L.host_jubjub_sign(key, L.host_poseidon(fingerprint + F(nonce)))
    if damage == "flip":
        sig = sig[:64] + bytes([sig[64] ^ 1]) + sig[65:]
    return key[:64], nonce, Z, amount, Z, fee, fingerprint, sig


def _push(w, names, kind, args):
    if kind == "update":
        w.push_tx(names[args[0]], names[args[1]], *args[2:])
    elif kind == "deposit":
        w.push_deposit(names[args[0]], *args[1:])
    elif kind == "withdraw":
        w.push_withdraw(names[args[0]], *args[1:])
    else:
        w.push_withdraw_signed(*signed_withdraw(*args))


def accepted_amounts(blob):
    """which transactions a work holds, by tests/bincode_ref.py: the amounts of its enabled transitions, in order"""
    tag, transitions = B.decode(B.MpnWork, blob)["data"]
    assert all(t["enabled"] for t in transitions)
    return [t["tx"]["amount"]["amount"] if tag == "Update" else t["tx"]["payment"]["amount"]["amount"] for t in transitions]


KIND = {"deposit": 0, "withdraw": 1, "update": 2}
_runs = {}


def run(name, dev=None):
    """drains the case's queue: per builder call {"bytes": work bytes (withdraw_signed: the instance's z), "root": root after it, "accepted": amounts
    (withdraw_signed: their number), "rejected": number (a work does not carry it: None)}.  The host run is computed once per process and shared."""
    if dev is None and name in _runs:
        return _runs[name]
    kind, log4_tree, log4_token_tree, queue = CASES[name]
    w, names = _world(kind, log4_tree, log4_token_tree, dev)
    for args, _, _ in queue:
        _push(w, names, kind, args)
    out = []
    for _ in expected_batches(name):
        if kind == "withdraw_signed":
            r = w.withdraw_synthesize(LOG4_BATCH, F(8))
            assert r.satisfied
            out.append({"bytes": bytes(r.view("z")), "root": w.root(), "accepted": r.accepted, "rejected": r.rejected})
            continue
        work = w.make_work(KIND[kind], sc.VKS, 10, log4_batches=(LOG4_BATCH,) * 3)
        blob = work.encode()
        again = L.MpnWork.decode(blob)          # the product's own decoder takes what the builder made
        assert (again.n_transitions, again.state, again.next_state, again.encode()) == (work.n_transitions, work.state, work.next_state, blob)
        assert work.next_state == w.root()
        out.append({"bytes": blob, "root": w.root(), "accepted": accepted_amounts(blob), "rejected": None})
    if dev is None:
        _runs[name] = out
    return out


def recorded():
    return json.load(open(GOLDEN))


def digest(batches):
    """what tests/golden/mpn_builder_cases.json keeps of a run"""
    return [{"sha256": hashlib.sha256(b["bytes"]).hexdigest(), "root": b["root"].hex()} for b in batches]
