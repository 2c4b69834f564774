"""Sets spanning several committees (LSG_PK_BITS_MULTI) in the bindings, on the CPU: the Node
host's packing of {committees, bits, bitLen} sets against a fake addon (tests/js/
test_committees_multi_host.js), the N-API addon's bounds check of a multi set's key blob against
the unchanged host-only stub of the C ABI, and the Python binding's PkBitsMulti form."""
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
def test_js_multi_committee_sets_host_logic():
    r = subprocess.run(["node", os.path.join(HERE, "js", "test_committees_multi_host.js")], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    # a test whose promise never settles lets node exit early with status 0: insist on the summary
    last = r.stdout.strip().splitlines()[-1]
    done, total = last.split()[0].split("/")
    assert last.endswith("passed") and done == total and int(total) == 5, r.stdout


def test_addon_bounds_a_multi_set_by_its_own_leading_count(tmp_path):
    """Linked against tests/native/lsg_stub.c: a descriptor with pk_len 12 whose blob's leading
    count (or the count word itself) runs past the arena is an argument error of the addon, never
    a read outside the arena; one whose blob fits is handed on."""
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
    # arena: [count, id, id][bits 2 B][msg 32 B][sig 96 B]; the descriptor's key offset and the
    # count word vary
    js = ("const a=require(process.argv[1]);const c=a.open(0);"
          "const run=async(count,pkOff,nBits)=>{const arena=new Uint8Array(14+32+96);"
          "new Uint32Array(arena.buffer,0,3).set([count,1,2]);"
          "const sd=Uint32Array.of(pkOff,12,nBits,14,32,46,96);"
          "try{await a.verifyPacked(c,arena,sd,Uint32Array.of(1,1),1,false);return 'accepted';}"
          "catch(e){return 'refused';}};"
          "(async()=>{const out=[];"
          "out.push(await run(2,0,9));"              # fits: 4 + 8 + 2 bytes
          "out.push(await run(40,0,9));"             # the ids run past the arena
          "out.push(await run(0xffffffff,0,9));"     # ... far past it
          "out.push(await run(2,0,8*200));"          # the bits run past the arena
          "out.push(await run(2,140,0));"            # the count word itself straddles the end
          "out.push(await run(2,4000,0));"
          "a.close(c);console.log('bounds',out.join(','));})();")
    r = subprocess.run(["node", "-e", js, str(addon)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "bounds accepted,refused,refused,refused,refused,refused" in r.stdout, r.stdout + r.stderr


def test_python_pkbitsmulti_form():
    """PkBitsMulti -> lsg_set: pk_len LSG_PK_BITS_MULTI, n_pks the bit count, pks = count, ids
    (host order), bits"""
    from lodestar_amd import _native as N
    assert (N.LSG_PK_BITS_MULTI, N.LSG_MAX_SET_COMMITTEES) == (12, 64)
    b = N.SetBuffer([(N.PkBitsMulti([0x12345, 7, 7], b"\xff\x01\xee", 9), b"m" * 32, b"s" * 96),
                     (N.PkBits(3, b"\x01", 2), b"m" * 32, b"s" * 96),
                     ([b"k" * 12], b"m" * 32, b"s" * 96),
                     (N.PkBitsMulti([], b"", 0), b"m" * 32, b"s" * 96)])
    s = b.arr[0]
    assert (s.pk_len, s.n_pks) == (12, 9)
    assert ctypes.string_at(s.pks, 18) == struct.pack("=4I", 3, 0x12345, 7, 7) + b"\xff\x01"  # (the spare byte is dropped)
    assert (b.arr[1].pk_len, b.arr[1].n_pks) == (8, 2)
    assert (b.arr[2].pk_len, b.arr[2].n_pks) == (0, 1)  # a 12-byte key: an unknown length, never a multi set
    assert (b.arr[3].pk_len, b.arr[3].n_pks) == (12, 0) and ctypes.string_at(b.arr[3].pks, 4) == struct.pack("=I", 0)
    p = N.PreparedJobs([([(N.PkBitsMulti([5, 6], b"\x0f", 4), b"m" * 32, b"s" * 96)], 1)])
    assert (p.sets[0].pk_len, p.sets[0].n_pks) == (12, 4)
    assert ctypes.string_at(p.sets[0].pks, 13) == struct.pack("=3I", 2, 5, 6) + b"\x0f"
    short = N.PkBitsMulti([1, 2], b"", 12)  # missing bytes are absentees
    assert short.tobytes() == struct.pack("=3I", 2, 1, 2) + b"\0\0" and len(short) == 12
