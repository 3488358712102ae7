#!/usr/bin/env python3
"""Writes tests/golden/ed25519_sign_vectors.json: (secret, public key, message, signature) rows made by the local `openssl` command line with the
secret kept, which pin every Ed25519 signing route of the library (tests/test_ed25519_sign_cpu.py) and the restatement tests/ed25519_cases.py on an
independent signer.  Message lengths 0, 1, 47, 48, 63, 64, 65, 79, 80, 95, 96, 97, 111, 112, 127, 128, 129, 175, 176, 191, 192, 193, 207, 208,
223, 224, 225 and 300: with the 32 bytes of the prefix (first hash) or the 64 of R | A (second hash) in front, they land on, one before and one
after the points where SHA-512's padding changes the block count.  RFC 8032 7.1 TEST 1 and TEST 2 are added as printed there.

Nothing is written unless OpenSSL and the restatement agree on every row (the same public key for the secret and the same 64 signature bytes:
Ed25519 signing is deterministic) and the restatement reproduces both RFC rows.  As in make_ed25519_fixtures.py, the command line of OpenSSL 3.0
cannot take an empty input with -rawin; the empty message under the OpenSSL-made key is then signed by the restatement and marked
"openssl": false (RFC TEST 1 is the independent empty-message row).

    python tools/make_ed25519_sign_fixtures.py
"""
import json
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ed25519_cases as E  # noqa: E402

LENGTHS = (0, 1, 47, 48, 63, 64, 65, 79, 80, 95, 96, 97, 111, 112, 127, 128, 129, 175, 176, 191, 192, 193, 207, 208, 223, 224, 225, 300)
KEYS = 2
RFC8032 = (
    ("RFC 8032 7.1 TEST 1", "9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60",
     "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a", "",
     "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b"),
    ("RFC 8032 7.1 TEST 2", "4ccd089b28ff96da9db6c346ec114e0f5b8a319f35aba624da8cf6ed4fb8a6fb",
     "3d4017c3e843895a92b70aa74d1b7ebc9c982ccf2ec4968cc0cd55f12af4660c", "72",
     "92a009a9f0d4cab8720e820b5f642540a2b27b5416503f8fb3762223ebdb69da085ac1e43e15996e458f3613d0f11d8c387b2eaeb4302aeeb00d291612bb0c00"),
)


def run(*args, ok_codes=(0,)):
    r = subprocess.run(["openssl", *args], capture_output=True)
    if r.returncode not in ok_codes:
        raise SystemExit("openssl %s: %s" % (" ".join(args), r.stderr.decode()))
    return r


def main():
    rnd = random.Random(8032)
    vectors = []
    with tempfile.TemporaryDirectory() as tmp:
        key, msgf, sigf = (os.path.join(tmp, n) for n in ("key.pem", "msg", "sig"))
        for k in range(KEYS):
            run("genpkey", "-algorithm", "ed25519", "-out", key)
            secret = run("pkey", "-in", key, "-outform", "DER").stdout[-32:]
            pk = run("pkey", "-in", key, "-pubout", "-outform", "DER").stdout[-32:]
            assert E.public_key(secret) == pk, "the restatement derives another public key"
            for n in LENGTHS:
                msg = rnd.randbytes(n)
                with open(msgf, "wb") as f:
                    f.write(msg)
                by_openssl = True
                if n == 0 and b"allocate 0 bytes" in run("pkeyutl", "-sign", "-rawin", "-inkey", key, "-in", msgf, "-out", sigf, ok_codes=(0, 1)).stderr:
                    sig, by_openssl = E.sign(secret, msg), False
                else:
                    run("pkeyutl", "-sign", "-rawin", "-inkey", key, "-in", msgf, "-out", sigf)
                    with open(sigf, "rb") as f:
                        sig = f.read()
                    assert len(sig) == 64 and E.sign(secret, msg) == sig, "the restatement signs differently: key %d, %d bytes" % (k, n)
                assert E.verify(pk, msg, sig)
                vectors.append({"secret": secret.hex(), "pk": pk.hex(), "msg": msg.hex(), "sig": sig.hex(), "openssl": by_openssl})
    for name, secret, pk, msg, sig in RFC8032:
        s, m = bytes.fromhex(secret), bytes.fromhex(msg)
        assert E.public_key(s).hex() == pk and E.sign(s, m).hex() == sig, "the restatement does not reproduce " + name
        vectors.append({"secret": secret, "pk": pk, "msg": msg, "sig": sig, "openssl": False, "rfc": name})
    out = os.path.join(ROOT, "tests", "golden", "ed25519_sign_vectors.json")
    with open(out, "w") as f:
        json.dump({"source": run("version").stdout.decode().strip() + "; RFC 8032 7.1", "vectors": vectors}, f, indent=0)
        f.write("\n")
    print("%s: %d rows, %d signed by OpenSSL" % (out, len(vectors), sum(v["openssl"] for v in vectors)))


if __name__ == "__main__":
    main()
