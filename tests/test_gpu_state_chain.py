"""GPU parity of bzk_state_update_chain (a chain of deltas through the resident state in one pass, every root checked) against
tests/pystate.py::PyKvState, the pair-at-a-time restatement of the reference's state manager, and against m bzk_state_update calls on a second
handle of the same model: states after every delta, rollbacks, get, prove, keys; claims that hold and claims that do not; refusals inside a
chain; the bincode entry; the height rule."""
import random

import pytest

import pystate as ps
from bazuka_amd import DeviceState
from bazuka_amd.lib import CHAIN_APPLIED as A, CHAIN_MISMATCH as M, CHAIN_NOT_REACHED as N, CHAIN_REFUSED as R
from oracle import pyref as pr

pytestmark = pytest.mark.gpu
S = ("scalar",)
F = pr.fr_to_mont_bytes


def _pairs(delta):
    return [(k, F((v or 0) % pr.R_MOD)) for k, v in delta.items()]


def _c40(h, n):
    return h + n.to_bytes(8, "little")


# the locator generator of test_gpu_state_device.py, restated
def _random_model(rnd, depth):
    k = rnd.random()
    if depth == 0 or k < 0.25:
        return S
    if k < 0.6:
        return ("struct", [_random_model(rnd, depth - 1) for _ in range(rnd.randint(1, 4))])
    return ("list", rnd.randint(0, 3), _random_model(rnd, depth - 1))


def _random_locator(rnd, model, stop=0.0):
    loc = []
    while model[0] != "scalar" and rnd.random() >= stop:
        if model[0] == "struct":
            f = rnd.randrange(len(model[1]))
            loc.append(f)
            model = model[1][f]
        else:
            loc.append(rnd.randrange(min(4 ** model[1], 6)))  # a small index range: the deltas keep meeting
            model = model[2]
    return tuple(loc), model


def _same_handles(a, b, locators, trees=()):
    assert a.root() == b.root()
    assert a.get(locators) == b.get(locators)
    for loc, idx in trees:
        assert a.prove(loc, idx) == b.prove(loc, idx)
    assert a.stats()["keys"] == b.stats()["keys"] and a.stats()["slots"] == b.stats()["slots"]


@pytest.mark.parametrize("seed", range(10))
def test_chains_equal_the_restatement(bzk, seed):
    rnd = random.Random(9100 + seed)
    model = _random_model(rnd, 4)
    dev, ref, height = DeviceState(bzk, ps.model_bincode(model)), ps.PyKvState(model), 0
    for m in (1, 2, 7, 40):
        deltas, want, rollbacks, heights = [], [], [], []
        for _ in range(m):
            delta = {}
            for _ in range(rnd.choice([1, 1, 2, 5, 30] if m < 40 else [1, 1, 1, 2, 3, 30])):  # the long chain: mostly small deltas, the restatement is slow
                delta[_random_locator(rnd, model)[0]] = rnd.choice([None, 0, 1, rnd.randrange(pr.R_MOD), pr.R_MOD - 1])
            height += rnd.randint(1, 3)
            rb = ref.update_contract(delta, height)
            deltas.append(_pairs(delta))
            rollbacks.append([F(rb[k] or 0) for k, _ in deltas[-1]])
            want.append(_c40(F(ref.hash), ref.size))
            heights.append(height)
        applied, verdict, states, prev = dev.update_chain(deltas, heights, claims=want if m != 2 else None, want_rollback=True)
        assert (applied, verdict) == (m, [A] * m)
        assert states == want
        assert prev == rollbacks
        assert dev.root() == (F(ref.hash), ref.size, height)
        locs = [_random_locator(rnd, model, stop=0.3)[0] for _ in range(12)]
        assert dev.get(locs) == [F(ref.get_data(l)) for l in locs]
        for _ in range(3):
            loc, sub = _random_locator(rnd, model, stop=0.4)
            if sub[0] == "list":
                idx = [rnd.randrange(4 ** sub[1]) for _ in range(3)]
                assert dev.prove(loc, idx) == [[[F(x) for x in part] for part in ref.prove(loc, i)] for i in idx]
    assert dev.stats()["keys"] >= len(ref.db)


def _mpn_delta(rnd, L, T, accounts):
    delta = {}
    for idx in rnd.sample(range(4 ** L), accounts):
        delta[(idx, 0)] = rnd.randrange(1, 1 << 60)
        delta[(idx, 4, rnd.randrange(4 ** T), 1)] = rnd.choice([0, rnd.randrange(1, 1 << 40)])
    return _pairs(delta)


def test_chain_equals_the_existing_path_on_the_account_model(bzk):
    """MPN model at L = 8, T = 2, 40 deltas of 300 accounts: the account-struct group holds 12 000 nodes (lane-per-node kernel), the top levels of
    the tree stay below 8 192 (cooperative kernel).  Then seven deltas of 10 .. 700 accounts under round_versions = 5 000: several rounds, the
    700-account delta (more than 5 000 versions on its own) alone in one.  The yardstick is the existing device path, one call per delta."""
    L, T = 8, 2
    rnd = random.Random(31)
    model = ps.model_bincode(ps.mpn_model(L, T))
    chain, seq = DeviceState(bzk, model), DeviceState(bzk, model)
    height = 0
    for sizes, rv in (([300] * 40, 0), ([20, 30, 700, 10, 300, 40, 40], 5000)):
        deltas = [_mpn_delta(rnd, L, T, k) for k in sizes]
        heights = list(range(height + 1, height + 1 + len(deltas)))
        height = heights[-1]
        want, want_prev = [], []
        for d, h in zip(deltas, heights):
            hash_, size, prev = seq.update(d, h, want_rollback=True)
            want.append(_c40(hash_, size))
            want_prev.append(prev)
        applied, verdict, states, prev = chain.update_chain(deltas, heights, claims=want, round_versions=rv, want_rollback=True)
        assert (applied, verdict) == (len(deltas), [A] * len(deltas))
        assert states == want
        assert prev == want_prev
        touched = [loc for d in deltas[-3:] for loc, _ in d[:40]]
        accounts = sorted({loc[0] for loc in touched})[:24]
        _same_handles(chain, seq, touched + [(a,) for a in accounts] + [(a, 4) for a in accounts] + [()],
                      [((), accounts + [0, 4 ** L - 1])] + [((a, 4), [0, 5, 15]) for a in accounts[:6]])


def _small_chain(rnd, model, m):
    deltas, want, ref = [], [], ps.PyKvState(model)
    for j in range(m):
        delta = {}
        for _ in range(rnd.choice([1, 2, 5])):
            delta[_random_locator(rnd, model)[0]] = rnd.choice([0, 1, rnd.randrange(pr.R_MOD)])
        ref.update_contract(delta, j)
        deltas.append(_pairs(delta))
        want.append(_c40(F(ref.hash), ref.size))
    return deltas, want


CLAIM_MODEL = ("list", 2, ("struct", [S, ("list", 1, S), ("struct", [S, S])]))
CLAIM_LOCS = [(i, 0) for i in range(6)] + [(i,) for i in range(6)] + [(i, 1, 2) for i in range(6)] + [()]


@pytest.mark.parametrize("rv", [0, 1, 40])
def test_claims(bzk, rv):
    rnd = random.Random(77)
    m = 7
    deltas, want = _small_chain(rnd, CLAIM_MODEL, m)
    heights = [10 + 2 * j for j in range(m)]
    mb = ps.model_bincode(CLAIM_MODEL)
    full = DeviceState(bzk, mb)
    assert full.update_chain(deltas, heights, claims=want, round_versions=rv) == (m, [A] * m, want)
    for k in (0, m // 2, m - 1):
        for at in (5, 35):  # a byte of the hash, a byte of the size
            claims = list(want)
            claims[k] = claims[k][:at] + bytes([claims[k][at] ^ 1]) + claims[k][at + 1:]
            dev, seq = DeviceState(bzk, mb), DeviceState(bzk, mb)
            applied, verdict, states = dev.update_chain(deltas, heights, claims=claims, round_versions=rv)
            assert applied == k and verdict == [A] * k + [M] + [N] * (m - k - 1)
            assert states == want[:k + 1] + [bytes(40)] * (m - k - 1)  # states_out[k] is the true state
            for d, h in zip(deltas[:k], heights[:k]):
                seq.update(d, h)
            _same_handles(dev, seq, CLAIM_LOCS, [((), [0, 5, 15])])
            # the remaining deltas, with the true claims, land on the full result
            assert dev.update_chain(deltas[k:], heights[k:], claims=want[k:], round_versions=rv) == (m - k, [A] * (m - k), want[k:])
            _same_handles(dev, full, CLAIM_LOCS, [((), [0, 5, 15])])


def test_mismatch_in_the_second_round_commits_the_first(bzk):
    """six deltas of five (i, 0) scalars each: 5 scalars + 5 structs + 2 .. 5 parents + the root = 13 .. 16 versions, so round_versions = 35 puts
    exactly two deltas in a round; a wrong claim at delta 3 stops the second round after its first delta, behind a committed first round"""
    rnd = random.Random(78)
    mb = ps.model_bincode(CLAIM_MODEL)
    dev, seq = DeviceState(bzk, mb), DeviceState(bzk, mb)
    deltas = [[((i, 0), F(rnd.randrange(1, pr.R_MOD))) for i in rnd.sample(range(16), 5)] for _ in range(6)]
    want = [_c40(*seq.update(d, j + 1)) for j, d in enumerate(deltas)]
    claims = want[:3] + [want[3][:-1] + b"\x55"] + want[4:]
    applied, verdict, states = dev.update_chain(deltas, range(1, 7), claims=claims, round_versions=35)
    assert (applied, verdict) == (3, [A] * 3 + [M, N, N]) and states == want[:4] + [bytes(40)] * 2
    seq3 = DeviceState(bzk, mb)
    for j in range(3):
        seq3.update(deltas[j], j + 1)
    _same_handles(dev, seq3, CLAIM_LOCS, [((), [1, 2])])
    assert dev.update_chain(deltas[3:], range(4, 7), claims=want[3:], round_versions=35)[:2] == (3, [A] * 3)
    _same_handles(dev, seq, CLAIM_LOCS, [((), [1, 2])])


def test_refusals_inside_a_chain(bzk):
    m = ("list", 2, ("struct", [S, ("list", 1, S)]))
    mb = ps.model_bincode(m)
    one = F(1)
    good = [[((3, 0), F(9)), ((3, 1, 2), F(4))], [((2, 0), F(5))], [((3, 0), F(6)), ((1, 1, 0), F(7))]]
    INVALID, NON_SCALAR, DUPLICATE, NON_CANONICAL = 1, 2, 4, 5
    bad = [([((16, 0), one)], INVALID), ([((3,), one)], NON_SCALAR), ([((3, 0, 0), one)], INVALID), ([((3, 0), one), ((3, 0), one)], DUPLICATE),
           ([((2, 0), one), ((3, 0), b"\xff" * 32)], NON_CANONICAL)]
    locs = [(3, 0), (2, 0), (1, 1, 0), (3, 1, 2), (3,), ()]
    for n_bad, (delta, code) in enumerate(bad):
        k = n_bad % 4  # the refused delta first, in the middle, last
        chain_in = good[:k] + [delta] + good[k:]
        dev, seq = DeviceState(bzk, mb), DeviceState(bzk, mb)
        applied, verdict, states = dev.update_chain(chain_in, range(1, len(chain_in) + 1))
        assert applied == k and verdict == [A] * k + [R] + [N] * (len(chain_in) - k - 1)
        assert bzk.last_refusal() == code
        assert states[k:] == [bytes(40)] * (len(chain_in) - k)
        for j in range(k):
            assert states[j] == _c40(*seq.update(good[j], j + 1))
        _same_handles(dev, seq, locs, [((), [3, 2])])
        assert dev.update_chain(good[k:], range(10, 10 + 3 - k))[0] == 3 - k  # the handle is usable, and a call that refuses nothing clears the refusal
        assert bzk.last_refusal() == 0
    # the same locator in two deltas of a chain is no duplicate
    dev = DeviceState(bzk, mb)
    assert dev.update_chain([[((3, 0), one)], [((3, 0), F(2))], [((3, 0), one)]], [1, 2, 3])[:2] == (3, [A] * 3)
    assert dev.get([(3, 0)]) == [one]
    # a mismatch in front of a refused delta: the refusal is not reached and not reported
    applied, verdict, _ = DeviceState(bzk, mb).update_chain([good[0], bad[0][0]], [1, 2], claims=[bytes(40), bytes(40)])
    assert (applied, verdict) == (0, [M, N]) and bzk.last_refusal() == 0


def test_bincode_entry_with_mutated_blobs_in_the_middle(bzk):
    """the truncated and bit-flipped blobs of test_gpu_state_device.py's fuzz case as delta 2 of a chain of 5: either the blob still decodes to a
    delta the model accepts - then all five apply as the restatement says - or it is refused and exactly two deltas are part of the state"""
    rnd = random.Random(99)
    model = ("list", 2, ("struct", [S, ("list", 1, S), ("struct", [S, S])]))
    mb = ps.model_bincode(model)

    def rand_delta():
        delta = {}
        for _ in range(rnd.randint(1, 4)):
            i, f = rnd.randrange(16), rnd.randrange(3)
            delta[{0: (i, 0), 1: (i, 1, rnd.randrange(4)), 2: (i, 2, rnd.randrange(2))}[f]] = rnd.choice([None, 0, rnd.randrange(1, pr.R_MOD)])
        return delta
    all_applied = refused = 0
    for case in range(24):
        deltas = [rand_delta() for _ in range(5)]
        blobs = [ps.delta_bincode(d) for d in deltas]
        blob = bytearray(blobs[2])
        if case % 2:
            for _ in range(rnd.randint(1, 3)):
                blob[rnd.randrange(len(blob))] ^= 1 << rnd.randrange(8)
        else:
            blob = blob[:rnd.randrange(len(blob))]
        blobs[2] = bytes(blob)
        try:
            deltas[2] = ps.delta_decode(blobs[2])
            for loc in deltas[2]:
                if ps.model_locate(model, loc)[0] != "scalar":
                    raise ValueError("NonScalarLocatorError")
            k = 5
        except (ValueError, IndexError):
            k = 2
        ref, want = ps.PyKvState(model), []
        for j in range(k):
            ref.update_contract(deltas[j], j + 1)
            want.append(_c40(F(ref.hash), ref.size))
        dev = DeviceState(bzk, mb)
        applied, verdict, states = dev.update_chain_bincode(blobs, range(1, 6), claims=(want + [bytes(40)] * 5)[:5])
        assert applied == k and verdict == ([A] * 5 if k == 5 else [A, A, R, N, N]), (case, verdict)
        assert states == want + [bytes(40)] * (5 - k)
        assert (bzk.last_refusal() != 0) == (k == 2)
        assert dev.root() == (F(ref.hash), ref.size, k)
        all_applied += k == 5
        refused += k == 2
    assert refused >= 8


def test_height_rule_and_empty_deltas(bzk):
    mb = ps.model_bincode(("struct", [S, S]))
    dev = DeviceState(bzk, mb)
    h0 = dev.root()
    assert dev.update_chain([], []) == (0, [], []) and dev.root() == h0
    applied, verdict, states = dev.update_chain([[]], [41])  # an empty delta moves the height only
    assert (applied, verdict, states) == (1, [A], [_c40(h0[0], 0)]) and dev.root() == (h0[0], 0, 41)
    d = [((0,), F(3))]
    applied, verdict, states = dev.update_chain([d, [], [((1,), F(4))], []], [50, 60, 70, 80], claims=None)
    assert applied == 4 and states[0] == states[1] and states[2] == states[3] and dev.root() == (states[3][:32], 2, 80)
    # a mismatch at delta 2: the height is that of delta 1; at delta 0: unchanged
    wrong = [states[3]] * 3
    dev2 = DeviceState(bzk, mb)
    assert dev2.update_chain([d, [], [((1,), F(4))]], [5, 6, 7], claims=[states[0], states[1], bytes(40)])[0] == 2
    assert dev2.root() == (states[0][:32], 1, 6)
    assert dev2.update_chain([[((1,), F(9))]], [99], claims=wrong[:1])[:2] == (0, [M]) and dev2.root()[2] == 6
    assert dev2.update_chain([[((7,), F(9))]], [99])[:2] == (0, [R]) and dev2.root()[2] == 6


def test_wide_structs_take_the_gather_path(bzk):
    """structs of 9 and 16 fields (widths 10 and 17) have no fused kernel: their groups run as a two-source gather and the generic Poseidon launch
    into the arena, between fused levels below (a list of 2-field structs) and above (the 4-ary tree over them)"""
    rnd = random.Random(5)
    wide9, wide16 = ("struct", [S] * 8 + [("list", 1, ("struct", [S, S]))]), ("struct", [S] * 16)
    mb = ps.model_bincode(("struct", [("list", 2, wide9), wide16]))
    chain, seq = DeviceState(bzk, mb), DeviceState(bzk, mb)
    deltas = []
    for _ in range(6):
        d = {}
        for _ in range(8):
            i = rnd.randrange(16)
            d[rnd.choice([(0, i, rnd.randrange(8)), (0, i, 8, rnd.randrange(4), rnd.randrange(2)), (1, rnd.randrange(16))])] = rnd.randrange(pr.R_MOD)
        deltas.append(_pairs(d))
    want = [_c40(*seq.update(d, j + 1)) for j, d in enumerate(deltas)]
    assert chain.update_chain(deltas, range(1, 7), claims=want, round_versions=60) == (6, [A] * 6, want)
    _same_handles(chain, seq, [(0, i) for i in range(16)] + [(0,), (1,), (1, 3), ()], [((0,), [0, 7, 15]), ((0, 3, 8), [1])])
