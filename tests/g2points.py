"""E2 points for the tests of the group law that are no valid signatures: the point behind a
compressed encoding whatever subgroup it lies in, and points of small prime order.  Plain Python
on the oracle; test infrastructure only."""
from oracle.curves import B2, E2
from oracle.fields import P, R, f2_add, f2_mul, f2_sqr, f2_sqrt

# the cofactor of E2(Fp2): |E2| = H2 r; 13^2 and 23^2 divide H2
H2 = 0x5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5


def decode_on_curve(sig_hex):
    """the E2 point of a compressed encoding whatever subgroup it lies in; None: not on the curve"""
    b = bytes.fromhex(sig_hex)
    if len(b) != 96 or not b[0] & 0x80 or b[0] & 0x40:
        return None
    x1 = int.from_bytes(bytes([b[0] & 0x1f]) + b[1:48], "big")
    x0 = int.from_bytes(b[48:], "big")
    if x0 >= P or x1 >= P:
        return None
    x = (x0, x1)
    y = f2_sqrt(f2_add(f2_mul(f2_sqr(x), x), B2))
    return None if y is None else (x, y)


def of_order(q, seeds):
    """a point of prime order q (q^2 divides |E2| and the q-part has exponent q) from the first of
    the E2 points `seeds` that gives one: [|E2| / q^2] S has order 1 or q"""
    n = H2 * R
    assert n % (q * q) == 0
    pt = next(p for p in (E2.mul(s, n // (q * q)) for s in seeds) if p is not None)
    assert E2.mul(pt, q) is None
    return pt
