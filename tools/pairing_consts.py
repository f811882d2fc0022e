"""Derives the BN254 tower constants csrc/pairing.hpp carries as data (Montgomery form, eight 32-bit limbs, R = 2^256):
the Frobenius coefficients of Fq6 / Fq12 for the powers 1, 2 and 3, the twist's q-power Frobenius factors of ark-ec
`bn::g2::mul_by_char`, the twist coefficient b' = 3 / (9 + u) and 1/2.  Prints the C++ block; tests/test_pairing_host.py
checks frob_k(x) == x^(q^k) with the constants as compiled.

    python tools/pairing_consts.py
"""
Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
XI = (9, 1)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2_pow(a, e):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = f2_mul(r, r)
        if bit == "1":
            r = f2_mul(r, a)
    return r


def f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], Q - 2, Q)
    return (a[0] * n % Q, (-a[1]) * n % Q)


def limbs(x):
    m = x * (1 << 256) % Q
    return "{" + ", ".join("0x%08xu" % ((m >> (32 * i)) & 0xFFFFFFFF) for i in range(8)) + "}"


def fq2(name, a):
    return "static constexpr uint32_t %s[2][8] = {%s, %s};" % (name, limbs(a[0]), limbs(a[1]))


def constants():
    out = {}
    for k in (1, 2, 3):
        qk = Q ** k
        out["FROB6_C1_%d" % k] = f2_pow(XI, (qk - 1) // 3)
        out["FROB6_C2_%d" % k] = f2_pow(XI, 2 * (qk - 1) // 3)
        out["FROB12_C1_%d" % k] = f2_pow(XI, (qk - 1) // 6)
    out["TWIST_MUL_BY_Q_X"] = f2_pow(XI, (Q - 1) // 3)
    out["TWIST_MUL_BY_Q_Y"] = f2_pow(XI, (Q - 1) // 2)
    out["TWIST_B"] = f2_mul((3, 0), f2_inv(XI))
    out["TWO_INV"] = ((Q + 1) // 2, 0)
    return out


if __name__ == "__main__":
    for name, v in constants().items():
        print(fq2(name, v))
