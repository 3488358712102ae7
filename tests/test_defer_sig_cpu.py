"""The second deferral level, BZK_SYNTH_DEFER_SIG (include/bzk.h, bzk_mpn_set_defer_sig), on the CPU.

Beyond the hash-dependent values of BZK_SYNTH_DEFER, the host generator leaves the EdDSA gadget of every Update and Withdraw transition
(/root/reference/src/zk/groth16/gadgets/eddsa/mod.rs:77-280) to the device: the two 254-step double-and-add ladders, the four additions of the
signature's tail and the two final checks (bzk_witfill.cuh V_LADDER / F_LADDER).  bzk_r1cs_fill_host runs the same __host__ __device__ ops on the
CPU; here instance + host fill == the independent restatement's fixtures (tests/golden/r1cs_sha256.json).  The device run: tests/test_gpu_defer_sig.py."""
import ctypes as C
import hashlib
import json
import os
import random

import numpy as np
import pytest

import bincode_ref as B
import r1cs_scenarios as S
from bazuka_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(S.G, "r1cs_sha256.json")))
ARRAYS = ("z", "az", "bz", "cz", "a_density", "b_density")

# per signature: 254 steps x (add(R, R) 9 + add(D, pk) 9 + two muxes) + 254 x (add(R, R) 9 + add_const(D, base) 3 + two muxes) + the tail's four
# additions x 9 = 8 672 variables and as many constraints; the two final assert_equal_if_enabled move with them (1 variable + 2 constraints each,
# F_ASSERT_EQ_IF) because their operands are now device registers
SIG_SLOTS = 254 * 20 + 254 * 14 + 4 * 9
SIG_HOLE_AUX, SIG_HOLE_CON = SIG_SLOTS + 2, SIG_SLOTS + 4

# A deferred instance leaves its holes untouched, and its arrays come from a pool of pinned blocks: in one process a hole often still holds an earlier
# complete synthesis of the same shape, so the bytes of an unfilled instance say nothing by themselves.  The holes are found instead: a twin instance of
# the same work is overwritten with POISON everywhere and filled on the host - what the fill wrote is a hole.  POISON is above r: no value the generator or
# a fill writes.
POISON = 0xFF
DEFERRED_ARRAYS = ("z", "az", "bz", "cz")


def _elements(r, k):
    return np.frombuffer(r.raw(k), dtype=np.uint8).reshape(-1, 32)  # writable: the instance's own (pinned) array


def hole_masks(dec, defer, threads=0):
    """per array, which 32-byte elements the instance's program writes"""
    twin = dec.synthesize(S.PROVER, threads=threads, defer=defer)
    for k in DEFERRED_ARRAYS:
        _elements(twin, k)[:] = POISON
    assert twin.fill_host()["flags"] == 0
    masks = {k: ~np.all(_elements(twin, k) == POISON, axis=1) for k in DEFERRED_ARRAYS}
    twin.free()
    return masks


def poison_holes(r, masks):
    """the instance's holes overwritten with POISON: whatever holds a field element there afterwards was written by a fill"""
    for k in DEFERRED_ARRAYS:
        _elements(r, k)[masks[k]] = POISON


# bzk_r1cs_defer_info of BZK_SYNTH_DEFER, recorded on the tree before the second level existed: the first level must not move
PRE = {
    "update_15_3_2": {"deferred": 1, "n_tx": 16, "n_ops": 1122, "n_regs": 557, "n_inputs": 989, "n_levels": 20, "hole_aux": 46284, "hole_con": 46289},
    "withdraw_15_3_3": {"deferred": 1, "n_tx": 64, "n_ops": 608, "n_regs": 301, "n_inputs": 536, "n_levels": 20, "hole_aux": 25320, "hole_con": 25323},
}


def test_first_level_program_did_not_move():
    for name, want in PRE.items():
        dec = L.MpnWork.decode(S.make_work(name))
        d = dec.synthesize(S.PROVER, defer=True).defer_info()
        assert {k: d[k] for k in want} == want, name


@pytest.mark.parametrize("name,threads", [("update_3_3_1", 1), ("update_15_3_1", 3), ("update_15_3_2", 0), ("withdraw_3_3_1", 2), ("withdraw_15_3_3", 0)])
def test_sig_instance_plus_host_fill_equals_the_independent_restatement(name, threads):
    dec = L.MpnWork.decode(S.make_work(name))
    r = dec.synthesize(S.PROVER, threads=threads, defer="sig")
    d = r.defer_info()
    assert d["deferred"] == 1 and d["filled"] == 0
    assert (r.n_in, r.n_aux, r.n_constraints) == (FIX[name]["n_in"], FIX[name]["n_aux"], FIX[name]["n_constraints"])
    assert r.satisfied  # the rows the host wrote hold
    masks = hole_masks(dec, "sig", threads)
    assert int(masks["z"].sum()) == d["hole_aux"] * d["n_tx"]  # the fill writes every hole the program declares, and nothing else
    for k in DEFERRED_ARRAYS[1:]:
        assert int(masks[k].sum()) == d["hole_con"] * d["n_tx"], k
    poison_holes(r, masks)
    for k in DEFERRED_ARRAYS:
        assert hashlib.sha256(r.view(k)).hexdigest() != FIX[name]["sha256"][k], k
    # what the level adds per transition, exactly
    d1 = dec.synthesize(S.PROVER, threads=threads, defer=True).defer_info()
    assert (d["hole_aux"] - d1["hole_aux"], d["hole_con"] - d1["hole_con"]) == (SIG_HOLE_AUX, SIG_HOLE_CON), (d, d1)
    # two V_LADDER, two F_LADDER, the two checks; registers: the ladders' points, results and scratch (3 x 508 + 2, 3 x 512 + 2)
    assert d["n_ops"] - d1["n_ops"] == 6 and d["n_regs"] - d1["n_regs"] == (3 * 508 + 2) + (3 * 512 + 2)
    assert d["n_inputs"] - d1["n_inputs"] == 4 + 6 + 2 and d["n_levels"] == d1["n_levels"]
    f = r.fill_host()
    assert f["filled"] == 1 and f["flags"] == 0
    for k in ARRAYS[:4]:
        assert hashlib.sha256(r.view(k)).hexdigest() == FIX[name]["sha256"][k], (name, k)
    plain = dec.synthesize(S.PROVER, threads=threads)
    for k in ARRAYS[4:]:
        assert r.view(k) == plain.view(k), k


@pytest.mark.parametrize("name", ["deposit_3_3_1", "deposit_15_3_3"])
def test_deposit_has_no_signature_gadget_its_instance_is_the_first_levels(name):
    dec = L.MpnWork.decode(S.make_work(name))
    a, b = dec.synthesize(S.PROVER, defer=True), dec.synthesize(S.PROVER, defer="sig")
    assert a.defer_info() == b.defer_info()
    assert a.fill_host()["flags"] == b.fill_host()["flags"] == 0  # (the holes of an unfilled instance hold whatever the memory held)
    for k in ARRAYS:
        assert a.view(k) == b.view(k), k


def test_schedule_info_covers_what_it_did_and_leaves_the_ladders_out():
    """bzk_r1cs_defer_schedule_info describes the one-launch schedule; the ladders have launches of their own and are outside it (include/bzk.h):
    the same hash ops, the two checks more among the fill ops, no violation"""
    dec = L.MpnWork.decode(S.make_work("update_15_3_2"))
    a = dec.synthesize(S.PROVER, defer=True).defer_schedule_info()
    b = dec.synthesize(S.PROVER, defer="sig").defer_schedule_info()
    assert b["violations"] == 0 and b["stages"] == a["stages"] and b["hash_ops"] == a["hash_ops"]
    assert b["fill_ops"] == a["fill_ops"] + 2


def _bad_update(which):
    """update_3_3_1 with its first (enabled) transaction's signature broken: "s" a different scalar, "r" a point off the curve"""
    v = B.decode(B.MpnWork, S.make_work("update_3_3_1"))
    tr = v["data"][1][0]
    assert tr["enabled"]
    sig = tr["tx"]["sig"]
    if which == "s":
        sig["s"] = bytes([sig["s"][0] ^ 1]) + sig["s"][1:]
    else:
        sig["r"]["y"] = bytes([sig["r"]["y"][0] ^ 1]) + sig["r"]["y"][1:]
    return B.encode(B.MpnWork, v)


@pytest.mark.parametrize("which", ["s", "r"])
def test_a_bad_signature_is_reported_by_the_fill(which):
    dec = L.MpnWork.decode(_bad_update(which))
    assert not dec.synthesize(S.PROVER, threads=1).satisfied
    r = dec.synthesize(S.PROVER, threads=2, defer="sig")
    assert r.defer_info()["deferred"] == 1
    if which == "s":
        assert r.satisfied  # every row the host judges holds: the failing check is a deferred one
    else:
        # sig_r's own on-curve check (update_circuit.rs: sig_r.assert_on_curve) reads host values and stays the host's to judge
        assert not r.satisfied
    assert r.fill_host()["flags"] & 1


def test_world_side_entry_and_plain_instance_agree():
    """bzk_mpn_set_defer_sig on the validator-side world: same transitions as a world without deferral, the instance fills to the same arrays;
    bzk_mpn_set_defer(w, 1) afterwards is the first level alone again, bzk_mpn_set_defer(w, 0) turns both off"""
    Z = S.ZIESHA

    def world(mode):
        w = L.MpnWorld(15, 3)
        w.set_threads(2)
        if mode == "sig":
            w.set_defer_sig(True)
        elif mode == "sig-then-defer":
            w.set_defer_sig(True)
            w.set_defer(True)
        elif mode == "sig-then-off":
            w.set_defer_sig(True)
            w.set_defer(False)
        for i in range(8):
            w.add_account(i * 1001 + 5, b"a%d" % i, Z, 10 ** 9)
        for i in range(6):
            w.push_tx(i * 1001 + 5, ((i + 1) % 8) * 1001 + 5, Z, 50 + i, Z, i)
        w.push_tx(5, 5 + 1001, Z, 10 ** 10, Z, 1)
        return w.update_synthesize(2, S.F(77), Z)

    a, b = world(None), world("sig")
    assert a.defer_info()["deferred"] == 0 and b.defer_info()["deferred"] == 1
    assert (a.accepted, a.rejected) == (b.accepted, b.rejected) == (6, 1)
    assert b.fill_host()["flags"] == 0
    for k in ARRAYS:
        assert a.view(k) == b.view(k), k
    c = world("sig-then-defer").defer_info()
    assert c["deferred"] == 1 and b.defer_info()["hole_con"] - c["hole_con"] == SIG_HOLE_CON
    assert world("sig-then-off").defer_info()["deferred"] == 0


def test_synthesize_refuses_an_unknown_defer_keyword():
    dec = L.MpnWork.decode(S.make_work("update_3_3_1"))
    with pytest.raises(ValueError):
        dec.synthesize(S.PROVER, defer="ladders")
    h = C.c_void_p()
    assert dec.lib.bzk_mpn_work_synthesize(dec.h, S.PROVER, None, 1, L.BZK_SYNTH_DEFER_SIG, C.byref(h)) == 0 and h.value
    L.R1cs(h).free()


# ---- the device functions on the host, against the oracle's Jubjub (oracle/pyref.py) ----------------------------------------------------------
@pytest.fixture(scope="module")
def wc():
    so = os.path.join(ROOT, "tests", "host", "_witfill_check.so")
    if not os.path.exists(so):
        pytest.skip("tests/host/_witfill_check.so not built (build() compiles it)")
    return C.CDLL(so)


def test_fr29_inversion_on_host_matches_oracle(wc, pr):
    rnd = random.Random(11)
    for a in [1, 2, pr.R_MOD - 1, pr.R_MOD - 2, 2 ** 254] + [rnd.randrange(1, pr.R_MOD) for _ in range(60)]:
        out = C.create_string_buffer(32)
        assert wc.hc_fr29_inv(pr.fr_to_mont_bytes(a), out) == 0
        assert out.raw == pr.fr_to_mont_bytes(pow(a, pr.R_MOD - 2, pr.R_MOD)), a
    out = C.create_string_buffer(32)
    wc.hc_fr29_inv(pr.fr_to_mont_bytes(0), out)
    assert out.raw == bytes(32)


def _ladder(wc, pr, t, base, k, sig_r=(0, 0)):
    m = pr.fr_to_mont_bytes
    np_ = 2 * 254 + (4 if t == 0 else 0)
    out = C.create_string_buffer(64 * (np_ + 1))
    assert wc.hc_ladder(t, m(base[0]) + m(base[1]) + m(k) + m(pr.JJ_D) + m(sig_r[0]) + m(sig_r[1]), out) == np_
    pts = [(pr.fr_from_mont_bytes(out.raw[64 * i:64 * i + 32]), pr.fr_from_mont_bytes(out.raw[64 * i + 32:64 * i + 64])) for i in range(np_ + 1)]
    return pts[:np_], pts[np_]


def _expect(pr, base, k, sig_r=None):
    """the gadget's ladder on the oracle's curve: R_0 = bit_0 ? base : (0, 1), D = R + R, A = D + base, R = bit ? A : D - a sum only where both
    operands are on the curve, (0, 0) otherwise"""
    def add(p, q):
        return pr.jj_add(p, q) if pr.jj_on_curve(p) and pr.jj_on_curve(q) else (0, 0)
    bits = [(k >> (254 - j)) & 1 for j in range(255)]
    r = base if bits[0] else (0, 1)
    pts = []
    for j in range(1, 255):
        d = add(r, r)
        a = add(d, base)
        pts += [d, a]
        r = a if bits[j] else d
    if sig_r is not None:
        q = add(r, sig_r)
        pts.append(q)
        for _ in range(3):
            q = add(q, q)
            pts.append(q)
    return pts, r


def test_one_ladder_on_host_matches_the_oracles_jubjub(wc, pr):
    rnd = random.Random(12)
    pk = pr.jj_mul(pr.JJ_BASE, rnd.randrange(1, pr.JJ_ORDER))
    sig_r = pr.jj_mul(pr.JJ_BASE, rnd.randrange(1, pr.JJ_ORDER))
    base8 = pr.jj_mul(pr.JJ_BASE, 8)
    h, s = rnd.randrange(pr.R_MOD), rnd.randrange(pr.R_MOD)
    got, res = _ladder(wc, pr, 0, pk, h, sig_r)
    want, wres = _expect(pr, pk, h, sig_r)
    assert got == want and res == wres
    assert want[-1] == pr.jj_mul(pr.jj_add(pr.jj_mul(pk, h), sig_r), 8)
    got, res = _ladder(wc, pr, 1, base8, s)
    want, wres = _expect(pr, base8, s)
    assert got == want and res == wres == pr.jj_mul(base8, s)
    # an off-curve base: the identity doubles to the identity until the first set bit, every other sum is (0, 0); an off-curve sig_r: a (0, 0) tail
    bad = (pk[0], (pk[1] + 1) % pr.R_MOD)
    for k in (h, h >> 40, 0):
        got, res = _ladder(wc, pr, 0, bad, k, sig_r)
        want, wres = _expect(pr, bad, k, sig_r)
        assert got == want and res == wres, k
    got, _ = _ladder(wc, pr, 0, pk, h, (sig_r[0], sig_r[1] + 1))
    assert got[-4:] == [(0, 0)] * 4
