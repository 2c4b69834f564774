"""Host (x86) builds of the kernel math headers (tests/native/hostcheck.hip) over two Fp
backends: "elem" (12 x 32-bit limbs, fully reduced, lsg_fp_elem.hpp) and "pair" (the pair
backend's lazy signed 14 x 29-bit limbs, lsg_fp_pair.hpp with all limbs in one lane).  Shared by
the host test modules.  Test infrastructure only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "hostcheck.hip")
LIBS = {"elem": (os.path.join(HERE, "native", "libhostcheck.so"), []),
        "pair": (os.path.join(HERE, "native", "libhostcheck_pair.so"), ["-DLSG_HOSTCHECK_PAIR"])}


def build(backend):
    """Path of the backend's library, compiled when older than the headers or the source.  A
    missing compiler or a failed compile raises."""
    lib, defs = LIBS[backend]
    csrc = os.path.join(ROOT, "lodestar_amd", "csrc")
    hdrs = [os.path.join(csrc, f) for f in os.listdir(csrc)]
    newest = max(os.path.getmtime(p) for p in hdrs + [SRC])
    if os.path.exists(lib) and os.path.getmtime(lib) >= newest:
        return lib
    from lodestar_amd.build import hipcc  # (as build(): PATH, else the ROCm install's own)
    subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared"] + defs +
                          ["-I", csrc, SRC, "-o", lib])
    return lib
