"""The variable-size LSG_MSG_OBJECT kinds and altair.ContributionAndProof: serialized objects
and their expected signing roots, composed from oracle/interop.py's helpers (shared by
tests/test_ssz_var_roots_host.py and tests/test_gpu_msg_objects_var.py).

The bitlist is merkleized the naive way -- its chunks padded with zero chunks to the full limit
(8 or 512), then interop._merkleize -- so nothing here shares the zero-subtree shortcut of
lodestar_amd/csrc/lsg_ssz.hpp.

Unpinned beyond the SSZ spec: the reference's tests hold no serialized AggregateAndProof or
ContributionAndProof with a known root, and its snapshot predates Electra (kind 2 follows the
consensus spec's EIP-7549 containers)."""
import random

from oracle import interop as io

AGG_PROOF, AGG_PROOF_ELECTRA = 1, 2  # LSG_MSG_KIND_*
MARK, KIND_SHIFT = 0x80000000, 24
LIMIT_BITS = {AGG_PROOF: 2048, AGG_PROOF_ELECTRA: 131072}
BITS_OFF = {AGG_PROOF: 336, AGG_PROOF_ELECTRA: 344}
# the issue's bit counts: one chunk, the chunk borders, the first level that needs a second
# round of 64 lanes, the full list
BIT_COUNTS = {
    AGG_PROOF: (0, 1, 7, 8, 255, 256, 257, 511, 512, 513, 2047, 2048),
    AGG_PROOF_ELECTRA: (0, 1, 255, 256, 257, 16383, 16384, 16385, 32767, 32768, 32769, 28800, 131071, 131072),
}
CONTRIBUTION_AND_PROOF = 264


def u64(b):
    return io.htr_uint64(int.from_bytes(b, "little"))


def bitlist_bytes(bits):
    """SSZ serialization of a bitlist: bit k = bit k & 7 of byte k >> 3, then the delimiter bit"""
    n = len(bits)
    raw = bytearray(n // 8 + 1)
    for k, b in enumerate(bits):
        raw[k >> 3] |= (b & 1) << (k & 7)
    raw[n >> 3] |= 1 << (n & 7)
    return bytes(raw)


def bitlist_root(bits, limit_bits):
    n = len(bits)
    raw = bytearray((n + 7) // 8)
    for k, b in enumerate(bits):
        raw[k >> 3] |= (b & 1) << (k & 7)
    chunks = [bytes(raw[i:i + 32]).ljust(32, b"\0") for i in range(0, len(raw), 32)]
    chunks += [bytes(32)] * (limit_bits // 256 - len(chunks))  # every padding chunk, hashed
    return io.sha256(io._merkleize(chunks) + n.to_bytes(32, "little"))


def make_agg_proof(kind, bits, rng):
    """(serialized AggregateAndProof of the kind, its hash_tree_root) over random fields"""
    idx, sel, data, sig, cb = rng.randbytes(8), rng.randbytes(96), rng.randbytes(128), rng.randbytes(96), rng.randbytes(8)
    electra = kind == AGG_PROOF_ELECTRA
    inner = (236 if electra else 228).to_bytes(4, "little") + data + sig + (cb if electra else b"") + bitlist_bytes(bits)
    obj = idx + (108).to_bytes(4, "little") + sel + inner
    att = io._merkleize([bitlist_root(bits, LIMIT_BITS[kind]), io.attestation_data_root(data), io.htr_bytes_vector(sig),
                         cb + bytes(24) if electra else bytes(32)])
    root = io._merkleize([u64(idx), att, io.htr_bytes_vector(sel), bytes(32)])
    assert len(obj) == BITS_OFF[kind] + len(bits) // 8 + 1
    return obj, root


def bits_of(n, fill, rng):
    if fill == "zero":
        return [0] * n
    if fill == "one":
        return [1] * n
    v = rng.getrandbits(n) if n else 0
    return [(v >> k) & 1 for k in range(n)]


def contribution_and_proof_root(obj):
    """altair.ContributionAndProof.hashTreeRoot over its 264-byte serialization"""
    assert len(obj) == CONTRIBUTION_AND_PROOF
    c = obj[8:168]
    contribution = io._merkleize([u64(c[:8]), c[8:40], u64(c[40:48]), c[48:64] + bytes(16), io.htr_bytes_vector(c[64:160])])
    return io._merkleize([u64(obj[:8]), contribution, io.htr_bytes_vector(obj[168:264])])


def signing_root(root, domain):
    return io.compute_signing_root(root, domain)


def length_word(kind, obj):
    return MARK | (kind << KIND_SHIFT) | (len(obj) + 32)


_cases = {}


def cases(kind):
    """[(n_bits, fill, object, domain, signing root, object root)] over the kind's bit counts, with zero,
    one and random bits: computed once per run and shared (the full Electra list costs 511
    hashes per object the naive way)"""
    if kind not in _cases:
        rng = random.Random(1000 + kind)
        out = []
        for n in BIT_COUNTS[kind]:
            for fill in ("zero", "one", "random"):
                obj, root = make_agg_proof(kind, bits_of(n, fill, rng), rng)
                dom = rng.randbytes(32)
                out.append((n, fill, obj, dom, signing_root(root, dom), root))
        _cases[kind] = out
    return _cases[kind]
