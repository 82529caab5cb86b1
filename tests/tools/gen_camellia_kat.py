"""Writes tests/golden/camellia_kat.json with the `openssl` command-line tool (3.0.2 when the committed file was made):

    python tests/tools/gen_camellia_kat.py tests/golden/camellia_kat.json

Every answer is openssl's -- `openssl enc -camellia-256-{ecb,ctr,cbc} -K <key> [-iv <iv>]` (ECB with -nopad) -- but the RFC 3713 Appendix A vector and the
reference's own CBC known answer (its unit test of `PNA test vector!` under key 0x11 x 32, IV 0x22 x 16), which are written down and checked against openssl
here.  Keys, blocks, IVs and messages come from a fixed seed, so a second run gives the same file."""
import json
import os
import random
import subprocess
import sys
import tempfile


def openssl(mode, key, data, iv=None):
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "in"), os.path.join(d, "out")
        with open(a, "wb") as f:
            f.write(data)
        cmd = ["openssl", "enc", "-camellia-256-" + mode, "-K", key.hex(), "-in", a, "-out", b]
        if iv is not None:
            cmd += ["-iv", iv.hex()]
        if mode == "ecb":
            cmd.append("-nopad")
        subprocess.run(cmd, check=True)
        with open(b, "rb") as f:
            return f.read()


def main(path):
    rnd = random.Random(3713)
    rb = lambda n: bytes(rnd.getrandbits(8) for _ in range(n))
    cases = []

    def add(kind, note, key, data, out, iv=None):
        c = {"kind": kind, "note": note, "key": key.hex()}
        if iv is not None:
            c["iv"] = iv.hex()
        c["in"] = data.hex()
        c["out"] = out.hex()
        cases.append(c)

    key = bytes.fromhex("0123456789abcdeffedcba987654321000112233445566778899aabbccddeeff")
    pt = bytes.fromhex("0123456789abcdeffedcba9876543210")
    want = bytes.fromhex("9acc237dff16d76c20ef7c919e3a7509")
    assert openssl("ecb", key, pt) == want
    add("ecb", "RFC 3713 Appendix A, 256-bit key", key, pt, want)
    for i in range(64):
        k, p = rb(32), rb(16)
        add("ecb", "random %d" % i, k, p, openssl("ecb", k, p))
    ivs = [("random", rb(16)), ("low word all ones", rb(12) + b"\xff" * 4), ("carry into the high half", b"\x00" * 8 + b"\xff" * 8)]
    for note, iv in ivs:
        k = rb(32)
        for n in (0, 1, 15, 16, 17, 31, 33, 4097):
            p = rb(n)
            add("ctr", "%s IV, %d bytes" % (note, n), k, p, openssl("ctr", k, p, iv), iv)
    for n in (0, 1, 15, 16, 17, 47, 48):
        k, iv, p = rb(32), rb(16), rb(n)
        add("cbc", "%d bytes" % n, k, p, openssl("cbc", k, p, iv), iv)
    k, iv, p = b"\x11" * 32, b"\x22" * 16, b"PNA test vector!"
    want = bytes.fromhex("47d8900ace4556eff9ff32a5b9605329feabcb5593910cb9acfc2fcb86c8a78b")
    assert openssl("cbc", k, p, iv) == want
    add("cbc", "the reference's known answer (PNA test vector!)", k, p, want, iv)
    ver = subprocess.run(["openssl", "version"], capture_output=True, text=True, check=True).stdout.strip()
    with open(path, "w") as f:
        json.dump({"generator": "tests/tools/gen_camellia_kat.py", "openssl": ver, "cases": cases}, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
