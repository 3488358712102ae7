"""The case table of the subgroup checks (tests/golden/subgroup_points.json, written by tools/gen_subgroup_points.py) with the expected verdict of
every record computed here, once, from the record's bytes alone: 2 when a coordinate's limbs are not below p or the point is off its curve,
else 1 when [r] P is the identity and 0 when it is not - [r] P by the C++ oracle's double-and-add (oracle/curve.hpp handles P = Q and P = -Q).
Flagged records are the identity: 1.  Shared by the CPU and the GPU tests."""
import functools
import json
import os

from oracle import coracle as co
from oracle import pyref as pr

HERE = os.path.dirname(os.path.abspath(__file__))
SIZE = {"g1": 96, "g2": 192}
R_BYTES = pr.R_MOD.to_bytes(32, "little")
BY_KIND = {"subgroup": 1, "curve": 0, "torsion": 0, "malformed": 2, "identity": 1}


def oracle_verdict(group: str, rec: bytes) -> int:
    limbs = [int.from_bytes(rec[48 * i:48 * i + 48], "little") for i in range(len(rec) // 48)]
    if any(v >= pr.P_MOD for v in limbs):
        return 2
    f = [pr.fp_from_mont_bytes(rec[48 * i:48 * i + 48]) for i in range(len(rec) // 48)]
    if group == "g1":
        if not pr.g1_on_curve((f[0], f[1])):
            return 2
        return 1 if co.msm_g1(rec, R_BYTES, mont=False, naive=True)[96] == 1 else 0
    if not pr.g2_on_curve(((f[0], f[1]), (f[2], f[3]))):
        return 2
    return 1 if co.msm_g2(rec, R_BYTES, mont=False, naive=True)[192] == 1 else 0


@functools.lru_cache(maxsize=None)
def table(group: str):
    """(records bytes, inf flag bytes, expected verdict bytes, kinds)"""
    with open(os.path.join(HERE, "golden", "subgroup_points.json")) as f:
        rows = json.load(f)[group]
    assert 0 < len(rows) <= 200
    recs = [bytes.fromhex(r["hex"]) for r in rows]
    assert all(len(r) == SIZE[group] for r in recs)
    inf = bytes(r["inf"] for r in rows)
    want = bytes(1 if i else oracle_verdict(group, r) for r, i in zip(recs, inf))
    kinds = [r["kind"] for r in rows]
    assert [BY_KIND[k] for k in kinds] == list(want), [(k, w) for k, w in zip(kinds, want) if BY_KIND[k] != w]   # the fixture is what it says it is
    return b"".join(recs), inf, want, kinds


def finite(group: str):
    """the unflagged records only: (records, expected)"""
    recs, inf, want, _ = table(group)
    sz = SIZE[group]
    keep = [i for i in range(len(inf)) if not inf[i]]
    return b"".join(recs[sz * i:sz * i + sz] for i in keep), bytes(want[i] for i in keep)


def outside_point(group: str) -> bytes:
    """a curve point outside the subgroup (a torsion case)"""
    recs, inf, want, kinds = table(group)
    i = kinds.index("torsion")
    return recs[SIZE[group] * i:SIZE[group] * (i + 1)]


ARRAYS = ("vk", "ic", "h", "l", "a", "b_g1", "b_g2")   # report[0] of bzk_bellman_params_check, in file order


@functools.lru_cache(maxsize=None)
def small_key():
    """a small proving key made by the oracle (40 multiplications, 4 inputs) in bellman's file format, with everything a load and a proof need:
    (blob, parts by array name, r1cs, oracle params, witness bytes z / az / bz / cz)"""
    from bazuka_amd import lib as L
    from util import fr_bytes, fr_list, log2_ceil, r1cs_to_csr, synth_r1cs
    r1 = synth_r1cs(40, n_in=4, seed=2024)
    A, B, Cm = r1cs_to_csr(co, r1)
    params = co.groth16_setup(A, B, Cm, r1["n_in"], r1["n_aux"], log2_ceil(len(r1["rows"])), fr_bytes(fr_list(5, 31)))
    parts = {k: params[k] for k in ARRAYS}
    blob = L.bellman_params_encode(*[parts[k] for k in ARRAYS])
    zb = fr_bytes(r1["z"])
    az, bz, cz = co.r1cs_eval(A, B, Cm, zb)
    return blob, parts, r1, params, (zb, az, bz, cz)


def tampered_key(array: str, index: int):
    """the small key with one point of one array replaced by a curve point outside the subgroup; for "vk", index counts the six points in file
    order (alpha_g1, beta_g1, beta_g2, gamma_g2, delta_g1, delta_g2)"""
    from bazuka_amd import lib as L
    blob, parts, *_ = small_key()
    p = dict(parts)
    if array == "vk":
        off, g2 = ((0, False), (97, False), (194, True), (387, True), (580, False), (677, True))[index]
        bad = outside_point("g2" if g2 else "g1")
        p["vk"] = p["vk"][:off] + bad + b"\0" + p["vk"][off + len(bad) + 1:]
    elif array == "ic":
        p["ic"] = p["ic"][:97 * index] + outside_point("g1") + b"\0" + p["ic"][97 * index + 97:]
    else:
        sz = 192 if array == "b_g2" else 96
        p[array] = p[array][:sz * index] + outside_point("g2" if array == "b_g2" else "g1") + p[array][sz * index + sz:]
    out = L.bellman_params_encode(*[p[k] for k in ARRAYS])
    assert len(out) == len(blob) and out != blob
    return out
