"""Message and DST lengths for hash_to_G2's expand_message_xmd (RFC 9380 5.3.1), derived from the
SHA-256 block arithmetic so that every way a hash can end is reached: k_expand_msg
(lodestar_amd/csrc/lsg_k_hash.hip) runs its own SHA-256 (ShaLds), and which branch of its
padding runs depends only on how many bytes the last block holds.
Plain Python: lengths, contents and the arithmetic; no device, no expected values.
tests/test_msg_lengths_host.py pins the references at these cases on the CPU,
tests/test_gpu_msg_lengths.py runs them through the device.  Test infrastructure only.

With a DST of D bytes and a message of L bytes
  b_0 = H(Z_pad(64) || msg(L) || l_i_b_str(2) || 0(1) || DST(D) || D(1))   68 + L + D bytes
  b_i = H(b_0 ^ b_(i-1) (32) || i(1) || DST(D) || D(1))                     34 + D bytes
and the tail of a hash is its length mod 64: the bytes in the last block before the padding."""
import hashlib

DST_POP = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"
POP = len(DST_POP)

# the tails at which the padding changes shape, and their neighbours
TAILS = tuple(range(52, 64)) + (0, 1, 2, 3)
NAMED = {
    55: "len-fits",      # 0x80 at byte 55: the length field fits exactly
    56: "extra-block",   # the first tail that needs a block of padding alone
    59: "align-to-60",   # 0x80 at byte 59: the alignment padding stops at 60, past the length field
    60: "align-to-64",   # 0x80 at byte 60: the alignment padding itself completes the block
    63: "0x80-flushes",  # the 0x80 byte completes the block
    0: "empty-block",    # the data ended on a block border: 0x80 opens an empty block
}


def b0_bytes(L, D=POP):
    return 68 + L + D


def bi_bytes(D=POP):
    return 34 + D


def b0_tail(L, D=POP):
    return b0_bytes(L, D) % 64


def bi_tail(D=POP):
    return bi_bytes(D) % 64


def tail_name(t):
    return "%d:%s" % (t, NAMED[t]) if t in NAMED else str(t)


# every L in 0..130 under the POP DST: two cycles of b_0's tail, the 16-byte chunk loop of
# shal_bytes at 15/16/17 and 31/32/33; then the message cache's limit (192), the DST limit's
# neighbours as message lengths, and messages of many blocks
MSG_LENS = tuple(range(131)) + (191, 192, 193, 255, 256, 1000, 4099)
# every D the ABI admits with a 32-byte message: four cycles of b_i's tail, and b_0's with it
DST_LENS = tuple(range(256))
DST_MSG_LEN = 32


def _cross():
    """(L, D) for every pair (b_0 tail, b_i tail) out of 55, 56, 63 and 0: D from b_i's tail
    (in a different 64-cycle from pair to pair), then L from b_0's"""
    out = []
    for k, (t0, ti) in enumerate((a, b) for a in (55, 56, 63, 0) for b in (55, 56, 63, 0)):
        D = (ti - 34) % 64 + 64 * (k % 4)  # at most 30 + 192
        L = (t0 - 68 - D) % 64 + 64 * (k % 3)
        out.append((L, D))
    return tuple(out)


CROSS = _cross()


def named_msg_lens():
    """the L of MSG_LENS at which b_0 ends on a named tail (POP DST)"""
    return tuple(L for L in MSG_LENS if b0_tail(L) in NAMED)


def named_dst_lens():
    """the D of DST_LENS at which b_0 (32-byte message) or b_i ends on a named tail"""
    return tuple(D for D in DST_LENS if b0_tail(DST_MSG_LEN, D) in NAMED or bi_tail(D) in NAMED)


def _stream(tag, n):
    out, k = b"", 0
    while len(out) < n:
        out += hashlib.sha256(tag + k.to_bytes(4, "little")).digest()
        k += 1
    return out[:n]


def rnd_msg(L, salt=0):
    """L pseudo-random bytes (a SHA-256 counter stream keyed by L and salt)"""
    return _stream(b"lodestar-mi355x msglens msg %d %d " % (L, salt), L)


def dst_of(D):
    """D pseudo-random bytes"""
    return _stream(b"lodestar-mi355x msglens dst %d " % D, D)


def contents(L):
    """the messages of L bytes: all zero, all 0xFF, pseudo-random (L = 0: the one empty message)"""
    if L == 0:
        return [b""]
    return [bytes(L), b"\xff" * L, rnd_msg(L)]


def m32():
    """the DST sweep's one 32-byte message"""
    return rnd_msg(DST_MSG_LEN, salt=2)


def cross_msg(L):
    return rnd_msg(L, salt=1)


def all_cases():
    """[(msg, dst)]: the message sweep (three contents per length, POP DST), the DST sweep, CROSS"""
    out = [(m, DST_POP) for L in MSG_LENS for m in contents(L)]
    out += [(m32(), dst_of(D)) for D in DST_LENS]
    out += [(cross_msg(L), dst_of(D)) for L, D in CROSS]
    return out


def named_cases():
    """the part of all_cases() at which b_0 or b_i ends on a named tail, and all of CROSS: few
    enough for the pure-Python oracle"""
    out = [(m, DST_POP) for L in named_msg_lens() for m in contents(L)]
    out += [(m32(), dst_of(D)) for D in named_dst_lens()]
    out += [(cross_msg(L), dst_of(D)) for L, D in CROSS]
    return out


def chunks(seq, n):
    """seq in n nearly equal runs (the parametrised sweeps: a few ids, not one per length)"""
    seq = list(seq)
    per = -(-len(seq) // n)
    return [seq[i:i + per] for i in range(0, len(seq), per)]


def chunk_id(run):
    return "%d-%d" % (run[0], run[-1])
