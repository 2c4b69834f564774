"""Generates tests/golden/deposits.json from the Python oracle only: deposits as
block/processDeposit.ts:47-66 sees them, with the verdicts the reference reaches.

Each case: a 184-byte SSZ DepositData (pubkey 48 | withdrawal credentials 32 | amount u64 LE |
signature 96), the deposit domain, the DepositMessage signing root, and
  valid  1 when processDeposit goes on to add the validator
  err    0 when PublicKey.fromBytes(pk, affine, true) and Signature.fromBytes(sig, affine, true)
         both pass (whether or not the signature verifies), else the BLST code of the first
         failing step: key, then signature
  unvalidated  (alias and infinity cases) what a verify without KeyValidate says: 1 valid,
         0 invalid, -code when it throws -- the behaviour of an unflagged job

The first case is the reference's only byte-exact known answer (genesisState.test.ts:51-55,
oracle/interop.py GENESIS_KAT) under the minimal preset's deposit domain.

Run: python tests/golden/gen_deposits.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.curves import E1, g1_compress, g2_compress, BlstError  # noqa: E402
from oracle.fields import P, R  # noqa: E402
from oracle import interop as io  # noqa: E402
from oracle import verifier as ov  # noqa: E402
from tests import blsdata as bd  # noqa: E402


def deposit_data(pubkey, wc, amount, sig):
    assert len(pubkey) == 48 and len(wc) == 32 and len(sig) == 96
    return pubkey + wc + amount.to_bytes(8, "little") + sig


def signing_root(data184, domain):
    d = bytes(data184)
    return io.compute_signing_root(
        io.deposit_message_root(d[:48], d[48:80], int.from_bytes(d[80:88], "little")), domain)


def process_deposit(data184, domain):
    """(valid, err) of processDeposit.ts:57-63"""
    d = bytes(data184)
    try:
        pk = ov.public_key_validate(d[:48])
    except BlstError as e:
        return 0, e.code
    try:
        sig = ov.signature_from_bytes(d[88:], True)
    except BlstError as e:
        return 0, e.code
    return int(ov.verify_single(pk, signing_root(d, domain), sig)), 0


def unvalidated(data184, domain):
    """the same deposit verified as an unflagged single-set job: the key only decoded"""
    d = bytes(data184)
    try:
        pk = ov.public_key_from_bytes(d[:48])
        sig = ov.signature_from_bytes(d[88:], True)
        return int(ov.verify_single(pk, signing_root(d, domain), sig))
    except BlstError as e:
        return -e.code


def alias_key(i, seed=0):
    """pk_i + T with T = [r]X != O for a curve point X outside G1: T lies in the cofactor
    torsion, which the reduced pairing cannot see"""
    T = E1.mul(bd.g1_not_in_group(seed), R)
    assert T is not None
    return g1_compress(E1.add(bd.pk_point(i), T))


def main():
    kat = io.GENESIS_KAT
    domain = io.compute_domain(io.DOMAIN_DEPOSIT, io.GENESIS_FORK_VERSION_MINIMAL, bytes(32))
    pk0 = bytes.fromhex(kat["pubkey"])
    assert pk0 == bd.pk_bytes(0, compressed=True)
    wc = bytes.fromhex(kat["withdrawal_credentials"])
    amount = kat["amount"]
    sig0 = bytes.fromhex(kat["signature"])
    inf_sig = bytes([0xC0]) + bytes(95)

    def signed(pubkey, signer, amt=amount):
        """DepositData over `pubkey` signed by interop key `signer`"""
        blank = deposit_data(pubkey, wc, amt, bytes(96))
        return deposit_data(pubkey, wc, amt, g2_compress(ov.sign(bd.sk(signer), signing_root(blank, domain))))

    def with_sig(data, sig):
        return data[:88] + sig

    cases = []

    def add(name, data, both=False):
        valid, err = process_deposit(data, domain)
        c = {"name": name, "data": data.hex(), "domain": domain.hex(), "root": signing_root(data, domain).hex(),
             "valid": valid, "err": err}
        if both:
            c["unvalidated"] = unvalidated(data, domain)
        cases.append(c)

    kat_data = deposit_data(pk0, wc, amount, sig0)
    add("genesis_kat", kat_data)
    add("amount_changed", deposit_data(pk0, wc, amount - 10 ** 9, sig0))
    add("other_signer", signed(pk0, 1))
    add("alias_key", signed(alias_key(0), 0), both=True)
    add("infinity_key_infinity_sig", deposit_data(bytes([0xC0]) + bytes(47), wc, amount, inf_sig), both=True)
    flipped = bytearray(pk0)
    flipped[0] &= 0x7F  # compression bit cleared
    add("key_encoding_bit", with_sig(signed(bytes(flipped), 0), sig0))
    xp = bytearray(P.to_bytes(48, "big"))  # x = p
    xp[0] |= 0x80
    add("key_x_ge_p", with_sig(signed(bytes(xp), 0), sig0))
    not_in_g2 = bd.corrupt_not_in_group(([pk0], signing_root(kat_data, domain), sig0))[2]
    add("sig_not_in_group", with_sig(kat_data, not_in_g2))
    add("sig_bad_encoding", with_sig(kat_data, bytes([0xE0]) + bytes(95)))
    add("bad_key_bad_sig", deposit_data(alias_key(0), wc, amount, bytes([0xE0]) + bytes(95)))

    assert [c["valid"] for c in cases][:3] == [1, 0, 0] and all(c["err"] == 0 for c in cases[:3]), cases[:3]
    assert cases[3]["err"] == 3 and cases[4]["err"] == 6 and cases[9]["err"] == 3
    json.dump({"cases": cases}, open(os.path.join(HERE, "deposits.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
