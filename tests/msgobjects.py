"""SSZ objects of the seven LSG_MSG_OBJECT kinds and their expected signing roots, composed from
oracle/interop.py's helpers (shared by tests/test_ssz_roots_host.py and
tests/test_gpu_msg_objects.py).  The object's serialized length selects its kind."""
from oracle import interop as io

KINDS = (8, 16, 32, 76, 88, 112, 128)  # object bytes; the staged payload is the object + 32


def object_root(obj):
    """hash_tree_root of the object that an SSZ serialization of len(obj) bytes is taken for"""
    n = len(obj)
    u64 = lambda b: io.htr_uint64(int.from_bytes(b, "little"))  # noqa: E731
    if n == 8:  # uint64 (Slot, Epoch)
        return u64(obj)
    if n == 16:  # two uint64 fields (VoluntaryExit, SyncAggregatorSelectionData)
        return io._merkleize([u64(obj[:8]), u64(obj[8:])])
    if n == 32:  # Root
        return bytes(obj)
    if n == 76:  # capella.BLSToExecutionChange: validatorIndex, fromBlsPubkey, toExecutionAddress
        return io._merkleize([u64(obj[:8]), io.htr_bytes_vector(obj[8:56]), obj[56:76] + bytes(12)])
    if n == 88:  # phase0.DepositMessage
        return io.deposit_message_root(obj[:48], obj[48:80], int.from_bytes(obj[80:88], "little"))
    if n == 112:  # phase0.BeaconBlockHeader: slot, proposerIndex, parentRoot, stateRoot, bodyRoot
        return io._merkleize([u64(obj[:8]), u64(obj[8:16]), obj[16:48], obj[48:80], obj[80:112]])
    if n == 128:  # phase0.AttestationData
        return io.attestation_data_root(obj)
    raise ValueError(f"no object kind of {n} bytes")


def signing_root(obj, domain):
    if len(obj) == 128:
        return io.attestation_signing_root(obj, domain)
    return io.compute_signing_root(object_root(obj), domain)


def genesis_kat():
    """(DepositMessage bytes, domain, expected signing root) of the genesis known answer"""
    k = io.GENESIS_KAT
    pk = bytes.fromhex(k["pubkey"])
    wc, root = io.genesis_deposit_signing_root(pk)
    assert wc == bytes.fromhex(k["withdrawal_credentials"])
    obj = pk + wc + int(k["amount"]).to_bytes(8, "little")
    return obj, io.compute_domain(io.DOMAIN_DEPOSIT, io.GENESIS_FORK_VERSION_MINIMAL, bytes(32)), root
