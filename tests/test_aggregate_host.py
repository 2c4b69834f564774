"""Per-group signature aggregates in the bindings, on the CPU: the Node host's onAggregates
option against a fake addon (tests/js/test_aggregate_host.js), the N-API addon's grouped
verifyPacked against the unchanged host-only stub of the C ABI (which lacks the two new entry
points), and the Python binding's declarations."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NODE_INCLUDE = "/usr/include/node"


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_aggregate_host_logic():
    r = subprocess.run(["node", os.path.join(HERE, "js", "test_aggregate_host.js")], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    # a test whose promise never settles lets node exit early with status 0: insist on the summary
    last = r.stdout.strip().splitlines()[-1]
    done, total = last.split()[0].split("/")
    assert last.endswith("passed") and done == total and int(total) == 5, r.stdout


def test_addon_loads_without_the_grouped_entry_points(tmp_path):
    """Linked against tests/native/lsg_stub.c, which has neither lsg_submit_jobs_grouped nor
    lsg_wait_jobs_grouped, the addon compiles with -Wall -Werror and loads; a grouped
    verifyPacked throws an Error saying the library does not support groups, a malformed groups
    argument is a TypeError, and nGroups = 0 or no groups is the plain call."""
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
          "const ar=new Uint8Array(256),sd=Uint32Array.of(0,48,1,48,32,80,96),jd=Uint32Array.of(1,1);"
          "try{a.verifyPacked(c,ar,sd,jd,1,false,Uint32Array.of(0),1);console.log('no throw');}"
          "catch(e){if(/does not support groups/.test(e.message))n++;else console.log(e.message);}"
          "for(const f of [()=>a.verifyPacked(c,ar,sd,jd,1,false,Uint32Array.of(0,0),1),"  # one word per set
          "()=>a.verifyPacked(c,ar,sd,jd,1,false,[0],1)]){"
          "try{f();console.log('no throw');}catch(e){if(e instanceof TypeError)n++;else console.log(e.message);}}"
          "Promise.all([a.verifyPacked(c,ar,sd,jd,1,false,Uint32Array.of(0),0),a.verifyPacked(c,ar,sd,jd,1,false,undefined,3),"
          "a.verifyPacked(c,ar,sd,jd,1,false,null,3)])"
          ".then((r)=>{for(const x of r)if(x.agg===undefined&&x.aggCount===undefined&&x.status.length===1)n++;"
          "a.close(c);console.log('checked',n);},(e)=>{console.log(e.message);a.close(c);});")
    r = subprocess.run(["node", "-e", js, str(addon)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "checked 6" in r.stdout, r.stdout + r.stderr


def test_python_binding_declares_the_grouped_calls():
    from lodestar_amd import _native as N
    assert N.LSG_NO_GROUP == 0xFFFFFFFF
    assert {"lsg_submit_jobs_grouped", "lsg_wait_jobs_grouped"} <= set(N.EXPORTS)
    lib = N.load_library()
    assert len(lib.lsg_submit_jobs_grouped.argtypes) == 7 and len(lib.lsg_wait_jobs_grouped.argtypes) == 6
    t = N.GroupedTicket((5, 2))
    t.n_groups = 3
    ticket, n_jobs = t  # a grouped ticket unpacks like a plain one (wait_jobs takes it)
    assert (ticket, n_jobs, t.n_groups) == (5, 2, 3)
    for name in ("wait_jobs_grouped", "verify_jobs_grouped"):
        assert callable(getattr(N.Context, name))
