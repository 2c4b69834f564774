"""Committee + bits sets in the bindings, on the CPU: the Node host's packing of
{committee, bits, bitLen} sets and loadCommittees against a fake addon (tests/js/
test_committees_host.js), the N-API addon's new entry points against the unchanged host-only
stub of the C ABI, and the Python binding's PkBits form."""
import ctypes
import os
import shutil
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NODE_INCLUDE = "/usr/include/node"


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_committee_sets_host_logic():
    r = subprocess.run(["node", os.path.join(HERE, "js", "test_committees_host.js")], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    # a test whose promise never settles lets node exit early with status 0: insist on the summary
    last = r.stdout.strip().splitlines()[-1]
    done, total = last.split()[0].split("/")
    assert last.endswith("passed") and done == total and int(total) == 5, r.stdout


def test_addon_loads_without_the_committee_entry_points(tmp_path):
    """Linked against tests/native/lsg_stub.c, which has neither lsg_committees_set nor
    lsg_committees_clear, the addon compiles with -Wall -Werror, loads, and the two calls throw
    an Error saying the library does not support them; malformed arguments are a TypeError."""
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
          "for(const f of [()=>a.committeesSet(c,3,Uint32Array.of(1,2,3),Uint32Array.of(0,2,3)),"
          "()=>a.committeesClear(c,3,2)]){"
          "try{f();console.log('no throw');}catch(e){if(/does not support/.test(e.message))n++;else console.log(e.message);}}"
          "for(const f of [()=>a.committeesSet(c,3,Uint32Array.of(1,2,3),Uint32Array.of(0,2)),"  # offsets do not end at n
          "()=>a.committeesSet(c,3,Uint32Array.of(1,2,3),Uint32Array.of(1,3)),"
          "()=>a.committeesSet(c,3,[1,2,3],Uint32Array.of(0,3)),()=>a.committeesClear(c,'x',2)]){"
          "try{f();console.log('no throw');}catch(e){if(e instanceof TypeError)n++;else console.log(e.message);}}"
          "a.close(c);console.log('unsupported',n);")
    r = subprocess.run(["node", "-e", js, str(addon)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "unsupported 6" in r.stdout, r.stdout + r.stderr


def test_python_pkbits_form():
    """PkBits -> lsg_set: pk_len LSG_PK_BITS, n_pks the bit count, pks = id (host order) + bits"""
    from lodestar_amd import _native as N
    assert (N.LSG_PK_BITS, N.LSG_ERR_BAD_COMMITTEE) == (8, 103)
    assert "committee" in N.error_message(103).lower()
    b = N.SetBuffer([(N.PkBits(0x12345, b"\xff\x01\xee", 9), b"m" * 32, b"s" * 96),
                     (N.PkIndices([7, 8]), b"m" * 32, b"s" * 96),
                     ([b"k" * 8], b"m" * 32, b"s" * 96)])
    s = b.arr[0]
    assert (s.pk_len, s.n_pks) == (8, 9)
    assert ctypes.string_at(s.pks, 6) == struct.pack("=I", 0x12345) + b"\xff\x01"  # (the spare byte is dropped)
    assert (b.arr[1].pk_len, b.arr[1].n_pks) == (4, 2)
    assert (b.arr[2].pk_len, b.arr[2].n_pks) == (0, 1)  # an 8-byte key: an unknown length, never a bits set
    p = N.PreparedJobs([([(N.PkBits(5, b"\x0f", 4), b"m" * 32, b"s" * 96)], 1)])
    assert (p.sets[0].pk_len, p.sets[0].n_pks) == (8, 4)
    assert ctypes.string_at(p.sets[0].pks, 5) == struct.pack("=I", 5) + b"\x0f"
    short = N.PkBits(1, b"", 12)  # missing bytes are absentees
    assert short.tobytes() == struct.pack("=I", 1) + b"\0\0" and len(short) == 12
