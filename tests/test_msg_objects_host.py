"""Sets whose message is an SSZ object + domain (LSG_MSG_OBJECT) in the bindings, on the CPU:
the Node host's packing of {signingObject, domain} sets against a recording fake addon
(tests/js/test_msg_objects_host.js), the N-API addon's objectSigningRoots against the unchanged
host-only stub of the C ABI, and the Python binding's MsgObject form."""
import ctypes
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NODE_INCLUDE = "/usr/include/node"
MARK = 0x80000000


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_msg_object_sets_host_logic():
    r = subprocess.run(["node", os.path.join(HERE, "js", "test_msg_objects_host.js")], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    # a test whose promise never settles lets node exit early with status 0: insist on the summary
    last = r.stdout.strip().splitlines()[-1]
    done, total = last.split()[0].split("/")
    assert last.endswith("passed") and done == total and int(total) == 6, r.stdout


def test_addon_loads_without_the_object_roots_entry_point(tmp_path):
    """Linked against tests/native/lsg_stub.c, which has no lsg_object_signing_roots, the addon
    compiles with -Wall -Werror, loads, and objectSigningRoots throws an Error saying the library
    does not support it; malformed arguments are a TypeError."""
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
    js = ("const a=require(process.argv[1]);const c=a.open(0);let n=0;const d=new Uint8Array(32);"
          "try{a.objectSigningRoots(c,new Uint8Array(256),128,d);console.log('no throw');}"
          "catch(e){if(/does not support/.test(e.message))n++;else console.log(e.message);}"
          "for(const f of [()=>a.objectSigningRoots(c,new Uint8Array(100),128,d),"  # not n x objLen
          "()=>a.objectSigningRoots(c,new Uint8Array(256),128,new Uint8Array(48)),"  # neither 32 nor n x 32
          "()=>a.objectSigningRoots(c,new Uint8Array(256),0,d),()=>a.objectSigningRoots(c,[1],8,d),"
          "()=>a.objectSigningRoots(c,new Uint8Array(256),128)]){"
          "try{f();console.log('no throw');}catch(e){if(e instanceof TypeError)n++;else console.log(e.message);}}"
          "a.close(c);console.log('unsupported',n);")
    r = subprocess.run(["node", "-e", js, str(addon)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "unsupported 6" in r.stdout, r.stdout + r.stderr


def test_python_msgobject_form():
    """MsgObject -> lsg_set: msg = object || domain, msg_len = LSG_MSG_OBJECT | its length"""
    from lodestar_amd import _native as N
    assert N.LSG_MSG_OBJECT == MARK and "lsg_object_signing_roots" in N.EXPORTS
    obj, dom = bytes(range(128)), bytes(range(100, 132))
    b = N.SetBuffer([([b"k" * 48], N.MsgObject(obj, dom), b"s" * 96),
                     ([b"k" * 48], b"m" * 32, b"s" * 96),
                     (N.PkBits(3, b"\x0f", 4), N.MsgObject(obj[:8], dom), b"s" * 96),
                     ([b"k" * 48], N.MsgObject(b"", b""), b"s" * 96)])
    assert b.arr[0].msg_len == MARK | 160 and ctypes.string_at(b.arr[0].msg, 160) == obj + dom
    assert b.arr[1].msg_len == 32 and ctypes.string_at(b.arr[1].msg, 32) == b"m" * 32
    assert (b.arr[2].msg_len, b.arr[2].pk_len) == (MARK | 40, 8) and ctypes.string_at(b.arr[2].msg, 40) == obj[:8] + dom
    assert b.arr[3].msg_len == MARK and not b.arr[3].msg  # (an argument error the library reports)
    p = N.PreparedJobs([([([b"k" * 48], N.MsgObject(obj[:76], dom), b"s" * 96), ([b"k" * 48], b"m" * 5, b"s" * 96)], 1),
                        ([(N.PkIndices([1, 2]), N.MsgObject(obj[:32], dom), b"s" * 96)], 0)])
    assert [p.sets[i].msg_len for i in range(3)] == [MARK | 108, 5, MARK | 64]
    assert ctypes.string_at(p.sets[0].msg, 108) == obj[:76] + dom
    assert ctypes.string_at(p.sets[1].msg, 5) == b"m" * 5
    assert ctypes.string_at(p.sets[2].msg, 64) == obj[:32] + dom
    assert len(N.MsgObject(obj, dom)) == 160


def test_library_rejects_marked_lengths_where_messages_are_plain():
    """lsg_hash_to_g2 and lsg_sign take plain messages: a marked length is an argument error,
    answered before the context is touched (no device needed)"""
    from lodestar_amd import _native as N
    lib = N.load_library()
    h = ctypes.c_void_p(1)  # never dereferenced: the argument check comes first
    out = ctypes.create_string_buffer(192)
    assert lib.lsg_hash_to_g2(h, b"m" * 64, MARK | 64, 1, b"dst", 3, out) == N.LSG_ERR_INVALID_ARG
    assert lib.lsg_sign(h, b"k" * 32, b"m" * 64, MARK | 64, 1, out) == N.LSG_ERR_INVALID_ARG
