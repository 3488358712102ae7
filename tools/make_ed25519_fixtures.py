#!/usr/bin/env python3
"""Writes tests/golden/ed25519_vectors.json: (public key, message, signature) triples made by the local `openssl` command line, the independent
signer and verifier that pins the Python restatement tests/ed25519_cases.py.  Message lengths 0, 1, 47, 48, 63, 64, 65, 175, 176 and 300: with
the 64 bytes of R | A in front those are SHA-512's padding and block edges (111 / 112 and 127 / 128 / 129 mod 128).

Nothing is written unless OpenSSL and the restatement agree on every triple (OpenSSL's signature verifies under the restatement and equals the
restatement's own signature for the same seed; Ed25519 signing is deterministic) and on every corrupted variant derived from it (one bit flipped
in message, R, s and key: both refuse, or - should a flipped key still verify - both accept).  One exception is recorded in the file itself:
the command line of OpenSSL 3.0 cannot take an empty input with -rawin ("Could not allocate 0 bytes"), so the empty message is signed by the
restatement under the OpenSSL-made key and marked "openssl": false; its hash input is the 64 bytes of R | A alone.

With --initials FILE it also writes tests/golden/ed25519_genesis_keys.json: the first 256 `ed...` public keys found in that file (the node's
src/config/initials.rs).  Their Display form is the key's bytes reversed; the JSON holds wire order.

    python tools/make_ed25519_fixtures.py [--initials path/to/initials.rs]
"""
import argparse
import json
import os
import random
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ed25519_cases as E  # noqa: E402

LENGTHS = (0, 1, 47, 48, 63, 64, 65, 175, 176, 300)
KEYS = 3
SPKI = bytes.fromhex("302a300506032b6570032100")  # SubjectPublicKeyInfo header of a raw Ed25519 key


def run(*args, ok_codes=(0,)):
    r = subprocess.run(["openssl", *args], capture_output=True)
    if r.returncode not in ok_codes:
        raise SystemExit("openssl %s: %s" % (" ".join(args), r.stderr.decode()))
    return r


def openssl_verify(tmp, pk: bytes, msg: bytes, sig: bytes) -> bool:
    paths = {k: os.path.join(tmp, k) for k in ("pub.der", "m", "s")}
    for k, v in zip(paths, (SPKI + pk, msg, sig)):
        with open(paths[k], "wb") as f:
            f.write(v)
    r = run("pkeyutl", "-verify", "-rawin", "-pubin", "-keyform", "DER", "-inkey", paths["pub.der"], "-in", paths["m"], "-sigfile", paths["s"],
            ok_codes=(0, 1))
    return r.returncode == 0  # a key OpenSSL cannot load is a refusal too


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--initials")
    args = ap.parse_args()
    rnd = random.Random(25519)
    vectors, checked = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        key, msgf, sigf = (os.path.join(tmp, n) for n in ("key.pem", "msg", "sig"))
        for k in range(KEYS):
            run("genpkey", "-algorithm", "ed25519", "-out", key)
            seed = run("pkey", "-in", key, "-outform", "DER").stdout[-32:]
            pk = run("pkey", "-in", key, "-pubout", "-outform", "DER").stdout[-32:]
            assert E.public_key(seed) == pk, "the restatement derives another public key"
            for n in LENGTHS:
                msg = rnd.randbytes(n)
                with open(msgf, "wb") as f:
                    f.write(msg)
                if n == 0 and b"allocate 0 bytes" in run("pkeyutl", "-sign", "-rawin", "-inkey", key, "-in", msgf, "-out", sigf, ok_codes=(0, 1)).stderr:
                    sig = E.sign(seed, msg)
                    assert E.verify(pk, msg, sig)
                    vectors.append({"pk": pk.hex(), "msg": "", "sig": sig.hex(), "openssl": False})
                    continue
                run("pkeyutl", "-sign", "-rawin", "-inkey", key, "-in", msgf, "-out", sigf)
                with open(sigf, "rb") as f:
                    sig = f.read()
                assert len(sig) == 64 and E.sign(seed, msg) == sig, "the restatement signs differently"
                assert E.verify(pk, msg, sig) and openssl_verify(tmp, pk, msg, sig)
                for what, cpk, cmsg, csig in E.corrupted(pk, msg, sig, rnd):
                    a, b = E.verify(cpk, cmsg, csig), openssl_verify(tmp, cpk, cmsg, csig)
                    assert a == b, "OpenSSL %s, the restatement %s: %s flipped, key %d, %d bytes" % (b, a, what, k, n)
                    checked += 1
                vectors.append({"pk": pk.hex(), "msg": msg.hex(), "sig": sig.hex(), "openssl": True})
    out = os.path.join(ROOT, "tests", "golden", "ed25519_vectors.json")
    with open(out, "w") as f:
        json.dump({"source": run("version").stdout.decode().strip(), "vectors": vectors}, f, indent=0)
        f.write("\n")
    print("%s: %d triples, %d corrupted variants agreed on" % (out, len(vectors), checked))
    if args.initials:
        with open(args.initials) as f:
            found = re.findall(r'"ed([0-9a-f]{64})"', f.read())
        keys, seen = [], set()
        for h in found:
            if h not in seen:
                seen.add(h)
                keys.append(bytes.fromhex(h)[::-1].hex())
            if len(keys) == 256:
                break
        assert len(keys) == 256, "fewer than 256 keys in %s" % args.initials
        out = os.path.join(ROOT, "tests", "golden", "ed25519_genesis_keys.json")
        with open(out, "w") as f:
            json.dump({"source": "src/config/initials.rs, the first 256 distinct ed... keys, wire order", "keys": keys}, f, indent=0)
            f.write("\n")
        print("%s: %d keys" % (out, len(keys)))


if __name__ == "__main__":
    main()
