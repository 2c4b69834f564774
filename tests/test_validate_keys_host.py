"""Objects that carry their own keys, on the CPU: the deposit fixture against the oracle, the
Node host's opts.validatePubkeys / verifyDeposits against a fake addon, and the N-API addon's
optional entry points against the unchanged host-only stub of the C ABI."""
import json
import os
import shutil
import subprocess

import pytest

from oracle import interop as oi
from oracle import verifier as ov
from oracle.curves import BlstError

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NODE_INCLUDE = "/usr/include/node"


def fixture_cases():
    return json.load(open(os.path.join(HERE, "golden", "deposits.json")))["cases"]


def test_deposit_fixture_roots_and_codes_rederived_from_oracle():
    cases = fixture_cases()
    names = [c["name"] for c in cases]
    assert names == ["genesis_kat", "amount_changed", "other_signer", "alias_key", "infinity_key_infinity_sig",
                     "key_encoding_bit", "key_x_ge_p", "sig_not_in_group", "sig_bad_encoding", "bad_key_bad_sig"]
    minimal = oi.compute_domain(oi.DOMAIN_DEPOSIT, oi.GENESIS_FORK_VERSION_MINIMAL, bytes(32))
    for c in cases:
        d, dom = bytes.fromhex(c["data"]), bytes.fromhex(c["domain"])
        assert len(d) == 184 and dom == minimal
        root = oi.compute_signing_root(
            oi.deposit_message_root(d[:48], d[48:80], int.from_bytes(d[80:88], "little")), dom)
        assert root.hex() == c["root"], c["name"]
        # err: the first failing validation step, key then signature (processDeposit.ts:57-63)
        err = 0
        try:
            ov.public_key_validate(d[:48])
            ov.signature_from_bytes(d[88:], True)
        except BlstError as e:
            err = e.code
        assert err == c["err"], c["name"]
        assert c["valid"] in (0, 1) and not (c["valid"] and c["err"])
    kat = cases[0]
    k = oi.GENESIS_KAT
    assert kat["data"] == k["pubkey"] + k["withdrawal_credentials"] + k["amount"].to_bytes(8, "little").hex() + k["signature"]
    assert kat["root"] == oi.genesis_deposit_signing_root(bytes.fromhex(k["pubkey"]))[1].hex()
    assert [c["valid"] for c in cases] == [1] + [0] * 9
    by = {c["name"]: c for c in cases}
    assert (by["alias_key"]["err"], by["infinity_key_infinity_sig"]["err"], by["bad_key_bad_sig"]["err"]) == (3, 6, 3)
    assert by["alias_key"]["unvalidated"] == 1  # the reduced pairing cannot see the cofactor torsion


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_validate_pubkeys_and_deposits_host_logic():
    r = subprocess.run(["node", os.path.join(HERE, "js", "test_validate_host.js")], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1]
    done, total = last.split()[0].split("/")
    assert last.endswith("passed") and done == total and int(total) == 4, r.stdout


def test_addon_loads_without_the_new_entry_points(tmp_path):
    """Linked against tests/native/lsg_stub.c, which has neither lsg_verify_deposits nor
    lsg_pubkey_validate, the addon compiles with -Wall -Werror, loads, and the two calls throw
    an Error saying the library does not support them."""
    if not shutil.which("node") or not shutil.which("gcc") or not os.path.exists(os.path.join(NODE_INCLUDE, "node_api.h")):
        pytest.skip("node, gcc or node's headers are not available")
    inc = os.path.join(ROOT, "include")
    flags = ["-O1", "-Wall", "-Werror", "-shared", "-fPIC"]
    subprocess.check_call(["gcc"] + flags + ["-I", inc, os.path.join(HERE, "native", "lsg_stub.c"), "-o",
                                             str(tmp_path / "liblodestar_bls.so"), "-lpthread"])
    addon = tmp_path / "lsg_napi.node"
    subprocess.check_call(["gcc", "-std=gnu11"] + flags + ["-DNODE_GYP_MODULE_NAME=lsg_napi", "-I", NODE_INCLUDE, "-I", inc,
                                                           os.path.join(ROOT, "lodestar_amd", "napi", "lsg_napi.c"), "-o",
                                                           str(addon), "-L", str(tmp_path), "-llodestar_bls",
                                                           f"-Wl,-rpath,{tmp_path}", "-lpthread"])
    js = ("const a=require(process.argv[1]);const c=a.open(0);let n=0;"
          "for(const f of [()=>a.verifyDeposits(c,new Uint8Array(184),new Uint8Array(32)),"
          "()=>a.pubkeyValidate(c,new Uint8Array(48),48)]){"
          "try{f();console.log('no throw');}catch(e){if(/does not support/.test(e.message))n++;else console.log(e.message);}}"
          "try{a.verifyDeposits(c,new Uint8Array(183),new Uint8Array(32));}catch(e){if(e instanceof TypeError)n++;}"
          "a.close(c);console.log('unsupported',n);")
    r = subprocess.run(["node", "-e", js, str(addon)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "unsupported 3" in r.stdout, r.stdout + r.stderr
