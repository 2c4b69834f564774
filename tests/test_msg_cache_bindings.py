"""The message cache in the bindings, on the CPU: the Node host's msgCacheEntries option and
getMsgCacheStats against a fake addon (tests/js/test_msg_cache_host.js), the N-API addon's two
new entry points against the unchanged host-only stub of the C ABI, and the Python binding's
prototypes."""
import ctypes
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NODE_INCLUDE = "/usr/include/node"


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_msg_cache_host_logic():
    r = subprocess.run(["node", os.path.join(HERE, "js", "test_msg_cache_host.js")], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    # a test whose promise never settles lets node exit early with status 0: insist on the summary
    last = r.stdout.strip().splitlines()[-1]
    done, total = last.split()[0].split("/")
    assert last.endswith("passed") and done == total and int(total) == 8, r.stdout


def test_addon_loads_without_the_msg_cache_entry_points(tmp_path):
    """Linked against tests/native/lsg_stub.c, which has neither lsg_msg_cache_set nor
    lsg_msg_cache_get_stats, the addon compiles with -Wall -Werror, loads, and the two calls
    throw an Error saying the library does not support them; malformed arguments are a TypeError."""
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
          "for(const f of [()=>a.msgCacheSet(c,4096),()=>a.msgCacheSet(c,0),()=>a.msgCacheStats(c)]){"
          "try{f();console.log('no throw');}catch(e){if(/does not support/.test(e.message))n++;else console.log(e.message);}}"
          "for(const f of [()=>a.msgCacheSet(c,-1),()=>a.msgCacheSet(c,'x'),()=>a.msgCacheSet(c),()=>a.msgCacheSet(c,2**31)]){"
          "try{f();console.log('no throw');}catch(e){if(e instanceof TypeError)n++;else console.log(e.message);}}"
          "a.close(c);console.log('unsupported',n);")
    r = subprocess.run(["node", "-e", js, str(addon)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "unsupported 7" in r.stdout, r.stdout + r.stderr


def test_python_stats_struct_matches_the_header():
    """lsg_msg_cache_stats: seven uint64 counters, then entries and capacity as uint32"""
    from lodestar_amd import _native as N
    names = [k for k, _ in N.LsgMsgCacheStats._fields_]
    assert names == ["lookups", "hits", "pending", "inserts", "evictions", "bypassed", "full", "entries", "capacity"]
    assert ctypes.sizeof(N.LsgMsgCacheStats) == 7 * 8 + 2 * 4
    src = open(os.path.join(ROOT, "include", "lodestar_bls.h")).read()
    decl = src[src.index("typedef struct {\n  uint64_t lookups"):src.index("} lsg_msg_cache_stats;")]
    assert "".join(decl.split()) == "typedefstruct{uint64_tlookups,hits,pending,inserts,evictions,bypassed,full;uint32_tentries,capacity;"
    for name in ("msg_cache_set", "msg_cache_clear", "msg_cache_stats"):
        assert callable(getattr(N.Context, name))
