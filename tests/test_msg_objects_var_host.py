"""The kind tag of LSG_MSG_OBJECT sets in the bindings, on the CPU: the Node host's packing of
{signingObject, domain, signingObjectKind} sets against a recording fake addon
(tests/js/test_msg_objects_var_host.js), the N-API addon's objectSigningRootsVar against the
unchanged host-only stub of the C ABI, and the Python binding: MsgObject(..., kind=) produces the
length word MARK | tag << 24 | (object + domain bytes), SetBuffer and PreparedJobs carry it, and
the new entry point is in the ABI list and answers argument errors before the context is
touched."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

from tests import msgobjects_var as mv

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NODE_INCLUDE = "/usr/include/node"
MARK = 0x80000000


def test_python_msgobject_kind_tag():
    from lodestar_amd import _native as N
    assert (N.LSG_MSG_KIND_SHIFT, N.LSG_MSG_KIND_MASK) == (24, 0x7f000000)
    assert (N.LSG_MSG_KIND_AGG_PROOF, N.LSG_MSG_KIND_AGG_PROOF_ELECTRA) == (mv.AGG_PROOF, mv.AGG_PROOF_ELECTRA) == (1, 2)
    assert "lsg_object_signing_roots_var" in N.EXPORTS
    import random
    rng = random.Random(9)
    dom = bytes(range(32))
    a1, _ = mv.make_agg_proof(1, mv.bits_of(450, "random", rng), rng)
    a2, _ = mv.make_agg_proof(2, mv.bits_of(28800, "random", rng), rng)
    assert (len(a1), len(a2)) == (336 + 57, 344 + 3601)
    cap = bytes(264)
    b = N.SetBuffer([([b"k" * 48], N.MsgObject(a1, dom, kind=1), b"s" * 96),
                     ([b"k" * 48], N.MsgObject(a2, dom, kind=N.LSG_MSG_KIND_AGG_PROOF_ELECTRA), b"s" * 96),
                     ([b"k" * 48], N.MsgObject(cap, dom), b"s" * 96),
                     ([b"k" * 48], b"m" * 32, b"s" * 96)])
    assert b.arr[0].msg_len == MARK | 1 << 24 | (len(a1) + 32) == mv.length_word(1, a1)
    assert b.arr[1].msg_len == MARK | 2 << 24 | (len(a2) + 32) == mv.length_word(2, a2)
    assert b.arr[2].msg_len == MARK | 296 and b.arr[3].msg_len == 32
    assert ctypes.string_at(b.arr[0].msg, len(a1) + 32) == a1 + dom
    assert ctypes.string_at(b.arr[1].msg, len(a2) + 32) == a2 + dom
    p = N.PreparedJobs([([([b"k" * 48], N.MsgObject(a2, dom, 2), b"s" * 96), ([b"k" * 48], b"m" * 5, b"s" * 96)], 1),
                        ([(N.PkIndices([1, 2]), N.MsgObject(a1, dom, 1), b"s" * 96)], 0)])
    assert [p.sets[i].msg_len for i in range(3)] == [mv.length_word(2, a2), 5, mv.length_word(1, a1)]
    assert ctypes.string_at(p.sets[0].msg, len(a2) + 32) == a2 + dom
    assert ctypes.string_at(p.sets[2].msg, len(a1) + 32) == a1 + dom
    assert len(N.MsgObject(a1, dom, 1)) == len(a1) + 32 and N.MsgObject(a1, dom).kind == 0
    with pytest.raises(ValueError):
        N.MsgObject(a1, dom, kind=128)
    with pytest.raises(ValueError):
        N.SetBuffer([([b"k" * 48], N.MsgObject(bytes(1 << 24), dom, 1), b"s" * 96)])  # the length leaves bits 0..23


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_tagged_object_sets_host_logic():
    r = subprocess.run(["node", os.path.join(HERE, "js", "test_msg_objects_var_host.js")], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    # a test whose promise never settles lets node exit early with status 0: insist on the summary
    last = r.stdout.strip().splitlines()[-1]
    done, total = last.split()[0].split("/")
    assert last.endswith("passed") and done == total and int(total) == 3, r.stdout


def test_addon_loads_without_the_var_roots_entry_point(tmp_path):
    """Linked against tests/native/lsg_stub.c, which has no lsg_object_signing_roots_var, the addon
    compiles with -Wall -Werror, loads, and objectSigningRootsVar throws an Error saying the
    library does not support it; malformed arguments are a TypeError."""
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
          "const o=new Uint8Array(400),f=Uint32Array.of(0,400);"
          "try{a.objectSigningRootsVar(c,1,o,f,d);console.log('no throw');}"
          "catch(e){if(/does not support/.test(e.message))n++;else console.log(e.message);}"
          "for(const g of [()=>a.objectSigningRootsVar(c,1,o,Uint32Array.of(0,399),d),"  # offsets do not end at the bytes' end
          "()=>a.objectSigningRootsVar(c,1,o,Uint32Array.of(1,400),d),"  # nor start at 0
          "()=>a.objectSigningRootsVar(c,1,o,[0,400],d),()=>a.objectSigningRootsVar(c,1,o,new Uint32Array(0),d),"
          "()=>a.objectSigningRootsVar(c,1,o,f,new Uint8Array(48)),()=>a.objectSigningRootsVar(c,1,o,f)]){"
          "try{g();console.log('no throw');}catch(e){if(e instanceof TypeError)n++;else console.log(e.message);}}"
          "a.close(c);console.log('unsupported',n);")
    r = subprocess.run(["node", "-e", js, str(addon)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "unsupported 7" in r.stdout, r.stdout + r.stderr


ARG_CHECKS = r"""
import ctypes, random, sys
from lodestar_amd import _native as N
from tests import msgobjects_var as mv
lib = N.load_library()
h = ctypes.c_void_p(1)  # never dereferenced: the argument check comes first
rng = random.Random(4)
obj, _ = mv.make_agg_proof(1, mv.bits_of(300, "random", rng), rng)
out, dom = ctypes.create_string_buffer(32), bytes(32)
def call(kind, o, offs=None, stride=0):
    offsets = (ctypes.c_uint32 * 2)(*(offs or (0, len(o))))
    return lib.lsg_object_signing_roots_var(h, kind, o, offsets, 1, dom, stride, out)
bad = N.LSG_ERR_INVALID_ARG
for kind in (0, 2, 3, 127, 128):  # (2: the Electra layout's inner offset differs)
    assert call(kind, obj) == bad, kind
assert call(1, obj[:8] + bytes([109]) + obj[9:]) == bad
assert call(1, obj[:-1] + bytes(1)) == bad
assert call(1, obj[:336]) == bad
assert call(1, obj, offs=(1, len(obj))) == bad
assert call(1, obj, offs=(0, 0)) == bad
assert call(1, obj, stride=16) == bad
assert lib.lsg_object_signing_roots(h, bytes(263), 263, 1, dom, 0, out) == bad
print("argument checks ok")
"""


def test_var_roots_entry_point_checks_its_arguments_first():
    """kind 0, an unknown kind, a malformed object and bad offsets are answered before the
    context is touched (no device needed).  The context passed is a fake pointer, so the calls
    run in a child process: a check that moved behind a dereference fails this assertion
    instead of taking the test run down."""
    r = subprocess.run([sys.executable, "-c", ARG_CHECKS], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "argument checks ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
