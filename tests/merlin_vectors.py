"""Merlin transcripts in pure Python, the oracle for csrc/merlin.hpp and the entries built on it: Keccak-f[1600], the
subset of STROBE-128 that the `merlin` crate uses (meta-AD, AD, PRF), Merlin's three calls, and the two transcript shapes
of the reference (creds/src/utils.rs:29-37 `add_to_transcript`: every message is the value's ark-serialize compressed bytes;
creds/src/rangeproof.rs:250-274 and creds/src/dlog.rs:56-99).

`self_check()` ties the permutation to hashlib (SHA3-256 and SHAKE128 are sponges over the same permutation) and the rest
to the crate's published conformance vector and to five known answers of the two shapes."""
import hashlib

MASK = (1 << 64) - 1
RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001,
      0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A,
      0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
      0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]


def _rho_offsets():
    r = [0] * 25
    x, y = 1, 0
    for t in range(24):
        r[x + 5 * y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return r


RHO = _rho_offsets()


def rotl(v, n):
    return ((v << n) | (v >> (64 - n))) & MASK if n else v


def keccak_f(state: bytearray):
    """Keccak-f[1600] in place on 200 bytes"""
    a = [int.from_bytes(state[8 * i:8 * i + 8], "little") for i in range(25)]
    for rc in RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        for x in range(5):
            d = c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1)
            for y in range(5):
                a[x + 5 * y] ^= d
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl(a[x + 5 * y], RHO[x + 5 * y])
        for x in range(5):
            for y in range(5):
                a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & MASK & b[(x + 2) % 5 + 5 * y])
        a[0] ^= rc
    for i in range(25):
        state[8 * i:8 * i + 8] = a[i].to_bytes(8, "little")


def sponge(rate, suffix, msg, out_len):
    """the FIPS 202 sponge over keccak_f: SHA3-256 is (136, 0x06), SHAKE128 (168, 0x1f)"""
    st = bytearray(200)
    padded = bytearray(msg) + bytes([suffix]) + bytes(-(len(msg) + 1) % rate)
    padded[-1] ^= 0x80
    for off in range(0, len(padded), rate):
        for i in range(rate):
            st[i] ^= padded[off + i]
        keccak_f(st)
    out = b""
    while len(out) < out_len:
        out += bytes(st[:rate])
        if len(out) < out_len:
            keccak_f(st)
    return out[:out_len]


R = 166
I, A, C, T, M, K = 1, 2, 4, 8, 16, 32


class Strobe:
    def __init__(self):
        self.st = bytearray(200)
        self.st[0:6] = bytes([1, R + 2, 1, 0, 1, 96])
        self.st[6:18] = b"STROBEv1.0.2"
        keccak_f(self.st)
        self.pos = self.pos_begin = self.cur_flags = 0
        self.n_perm = 1
        self.meta_ad(b"Merlin v1.0", False)

    def run_f(self):
        self.st[self.pos] ^= self.pos_begin
        self.st[self.pos + 1] ^= 0x04
        self.st[R + 1] ^= 0x80
        keccak_f(self.st)
        self.n_perm += 1
        self.pos = self.pos_begin = 0

    def absorb(self, data):
        for b in data:
            self.st[self.pos] ^= b
            self.pos += 1
            if self.pos == R:
                self.run_f()

    def squeeze(self, n):
        out = bytearray()
        for _ in range(n):
            out.append(self.st[self.pos])
            self.st[self.pos] = 0
            self.pos += 1
            if self.pos == R:
                self.run_f()
        return bytes(out)

    def begin_op(self, flags, more):
        if more:
            assert flags == self.cur_flags
            return
        assert not flags & T
        old = self.pos_begin
        self.pos_begin = self.pos + 1
        self.cur_flags = flags
        self.absorb(bytes([old, flags]))
        if flags & (C | K) and self.pos != 0:
            self.run_f()

    def meta_ad(self, data, more):
        self.begin_op(M | A, more)
        self.absorb(data)

    def ad(self, data, more):
        self.begin_op(A, more)
        self.absorb(data)

    def prf(self, n, more=False):
        self.begin_op(I | A | C, more)
        return self.squeeze(n)


class Transcript:
    def __init__(self, label):
        self.strobe = Strobe()
        self.append_message(b"dom-sep", label)

    def append_message(self, label, msg):
        self.strobe.meta_ad(label, False)
        self.strobe.meta_ad(len(msg).to_bytes(4, "little"), True)
        self.strobe.ad(msg, False)

    def challenge_bytes(self, label, n):
        self.strobe.meta_ad(label, False)
        self.strobe.meta_ad(n.to_bytes(4, "little"), True)
        return self.strobe.prf(n)


# ---- the reference's use of it -------------------------------------------------------------------------------------------
def new_transcript():
    return Transcript(b"\0")


def challenge(t):
    """31 bytes read little-endian (Fr::from_random_bytes): always below the scalar modulus"""
    return t.challenge_bytes(b"\0", 31)


def usize(v):
    return v.to_bytes(8, "little")


def byte_slice(b):
    """&[u8] as ark-serialize writes it: the length as u64, then the bytes"""
    return usize(len(b)) + bytes(b)


def range_challenges(com_f, com_g, com_q):
    """(c, rho), 31 bytes each, from the three commitments' compressed bytes (rangeproof.rs:250-257, 270-274)"""
    t = new_transcript()
    t.append_message(b"com_f", com_f)
    t.append_message(b"com_g", com_g)
    c = challenge(t)
    t.append_message(b"com_q", com_q)
    return c, challenge(t)


def dlog_challenge(context, statements):
    """DLogPoK's challenge (dlog.rs:77-99): context is bytes or None; a statement is (bases, k, y), compressed points"""
    t = new_transcript()
    t.append_message(b"context string", byte_slice(context or b""))
    for bases, k, y in statements:
        t.append_message(b"num_bases", usize(len(bases)))
        for b in bases:
            t.append_message(b"base", b)
        t.append_message(b"k", k)
        t.append_message(b"y", y)
    return challenge(t)


def range_dleq_challenge(slot_bases, com_f_basis, k0, k1, ped_com, com_f):
    """the DLEQ of a range proof (rangeproof.rs:218-245): all arguments compressed points"""
    assert len(slot_bases) == 2 and len(com_f_basis) == 4
    return dlog_challenge(None, [(slot_bases, k0, ped_com), (com_f_basis, k1, com_f)])


def to_int(ch):
    return int.from_bytes(ch, "little")


def to_scalar_bytes(ch):
    """a challenge as it crosses the C ABI: 32 canonical bytes, the top one 0"""
    return bytes(ch) + b"\0"


# ---- known answers ---------------------------------------------------------------------------------------------------------
KAT0 = "d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615"
KAT_RANGE_IN = (bytes(range(0x00, 0x20)), bytes(range(0x20, 0x40)), bytes(range(0x40, 0x60)))
KAT_RANGE_C = "f6626087b44cd5ee1e8644c59f13f49c218d536ad20580d43eb2c36f843e5f"
KAT_RANGE_RHO = "cbb92f1236f66957cb6feffa0ded75a194d63fc51c91c2d0f3a981c10cfe40"
KAT_DLOG = [(None, [2, 4], "1027fa2a35594a5813a65a499ed4c5f9b82cc79895d9764237e6b169583928"),
            (None, [1], "efbcd5bbd09b78e5b68cbb87faaccd13b8d39d6fb57accd5066fa4c8dd79d1"),
            (b"presentation", [2, 2, 2, 24], "55b8eb6c6d29f3ec41ade18c72ae1dae1732090af919390c0d5696987878e2")]


def kat_statements(shape):
    """base number b (1, 2, ... across the statements) is 32 bytes of b; k_i is 32 bytes of 0xA0 + i, y_i of 0xB0 + i"""
    out, b = [], 1
    for i, nb in enumerate(shape):
        out.append(([bytes([b + j]) * 32 for j in range(nb)], bytes([0xA0 + i]) * 32, bytes([0xB0 + i]) * 32))
        b += nb
    return out


def kat0():
    t = Transcript(b"test protocol")
    t.append_message(b"some label", b"some data")
    return t.challenge_bytes(b"challenge", 32)


def self_check():
    for n in (0, 135, 136, 137, 1000):
        msg = bytes((7 * i + n) & 0xFF for i in range(n))
        assert sponge(136, 0x06, msg, 32) == hashlib.sha3_256(msg).digest(), n
        assert sponge(168, 0x1F, msg, 400) == hashlib.shake_128(msg).digest(400), n
    assert kat0().hex() == KAT0
    c, rho = range_challenges(*KAT_RANGE_IN)
    assert c.hex() == KAT_RANGE_C and rho.hex() == KAT_RANGE_RHO
    for context, shape, want in KAT_DLOG:
        assert dlog_challenge(context, kat_statements(shape)).hex() == want, shape
