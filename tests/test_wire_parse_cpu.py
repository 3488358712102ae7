"""The wire-form record parsers (bazuka_amd/csrc/host_bincode.h parse_txs, parse_withdraws, parse_deposits, parse_l1_txs) under the address /
undefined-behaviour sanitizers as a stand-alone child process: tests/host/wire_parse_check.hip parses each case record whole, as every prefix and
with every byte raised by one and set to 0xff, each in a heap block of exactly its length, and checks that what a well-formed record hands on
lies inside it.  The records come from the generators the admission tests use: a handful per kind, every record length class among them."""
import os
import struct
import subprocess

import decompress_cases as D
import ed25519_cases as E
import l1_tx_cases as X
import withdraw_cases as W

HERE = os.path.dirname(os.path.abspath(__file__))
TX, WITHDRAW, DEPOSIT, L1 = range(4)


def _cases():
    out = [(TX, 0, 0, D.enc_tx(t)) for _, t, _, _ in D.tx_list()[:8]]  # the eight valid ones: records of 190, 222 and 254 bytes
    out += [(WITHDRAW, 0, 0, W.enc(r)) for w, r, _, _ in W.fixed_list() if w == "valid"]  # one per memo length
    for prefixed in (False, True):
        recs = E.admission_records()[:3]
        unsigned = dict(recs[0], payment=dict(recs[0]["payment"], sig=None))
        out += [(DEPOSIT, int(prefixed), 0, E.enc(r, prefixed)) for r in recs + [unsigned]]
        for form in (X.FORM_TX, X.FORM_TX_AND_DELTA):
            corpus = X.corpus(form, prefixed)
            picked = [rec for label, rec in corpus if label.startswith(("variant ", "RegularSend: src None", "RegularSend: Unsigned", "RegularSend, state_delta"))
                      or "without" in label]  # the seven variants; src None; Unsigned; no state, token, updates or delta; state_delta None
            out += [(L1, int(prefixed), int(form == X.FORM_TX_AND_DELTA), rec) for rec in picked]
    return out


def test_wire_parsers_under_sanitizers(tmp_path):
    exe = os.path.join(HERE, "host", "_wire_parse_check")
    assert os.path.exists(exe), "tests/host/_wire_parse_check not built (build() compiles it)"
    cases = _cases()
    assert {k for k, _, _, _ in cases} == {TX, WITHDRAW, DEPOSIT, L1}
    path = tmp_path / "records.bin"
    path.write_bytes(struct.pack("<I", len(cases)) + b"".join(struct.pack("<BBBI", k, f, d, len(c)) + c for k, f, d, c in cases))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "%d records" % len(cases) in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
