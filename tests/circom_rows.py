"""Circom-shaped R1CS instances for the tests (numpy CSR throughout; no Python list at scale).

Circom's linear substitution leaves rows of thousands of terms (an indicator sum over `max_array_len` signals, chains that grow
row by row), the constant wire 0 in a large share of all constraints, the same wire repeated inside one row, and wide
coefficient dictionaries (bigint limbs: 2^i·k).  The synthetic workloads of workloads.py have none of that; the instances
made here mix all of it into each of A, B and C, so that one matrix exercises every level of the sliced sparse product
(csr_host.hpp: pieces of SELL_PIECE = 8 terms, up to 8 levels), both sides of the setup's long-column threshold
(SPMV_LONG_ROW = 4096 terms of a transposed column) and the doubling / cancelling branches of the C fold:

  * rows of exactly ROW_BOUNDARIES terms (every sliced-level boundary) among ordinary rows of 2..12 terms;
  * hot columns: wire 0 and two more wires in more than 4096 terms of every matrix, and two wires with exactly 4096 and
    4097 terms (repeats included) in every matrix;
  * a row that repeats one wire with the literal one (equal points in the C fold) and a row of pairs c, r - c on one wire
    (the pair cancels);
  * coefficients: the literal one, 0, r - 1, powers of two up to 2^253 and dictionary values (optionally a fresh value per
    term: a dictionary of more than 2^20 entries);
  * satisfiable: the witness is drawn first, then every non-empty C row gets a last term on wire 0 (value one) whose
    coefficient makes <A_i,w>·<B_i,w> = <C_i,w>.
"""
import numpy as np

import cpu_ref

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
ROW_BOUNDARIES = (0, 1, 8, 9, 64, 65, 512, 513, 4096, 4097, 32768, 32769, 262145)
EXACT_COLUMNS = (4096, 4097)
SELL_LIMIT = 8 ** 8                     # the longest row the sliced layout accepts (8 levels of 8-term pieces)

# coefficient kinds: the literal one, zero, r - 1, 2^k (k <= 253), a dictionary value
ONE, ZERO, RMAX, POW2, DICT = range(5)
MIX_CIRCOM = (0.55, 0.04, 0.06, 0.12, 0.23)
MIX_DICT_HEAVY = (0.05, 0.01, 0.02, 0.03, 0.89)


def fr_bytes(vals) -> np.ndarray:
    """ints -> (n, 32) canonical little-endian bytes"""
    vals = [int(v) % R for v in vals]
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), np.uint8).reshape(len(vals), 32).copy()


def ints_of(b) -> list:
    raw = np.ascontiguousarray(b, np.uint8).reshape(-1).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _random_fr(rng, n) -> np.ndarray:
    x = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    x[:, 31] &= 0x1F                                   # below 2^253 < r
    return x


class Instance:
    """l inputs, m constraints, M variables; mats = (A, B, C) as cpu_ref.Csr; w = a satisfying assignment (M x 32 bytes).
    rows[name] = the row index of a special row (the same index in all three matrices); wires[name] = a reserved wire."""

    def __init__(self, l, m, M, mats, w, rows, wires):
        self.l, self.m, self.M, self.mats, self.w, self.rows, self.wires = l, m, M, mats, w, rows, wires

    def row_lengths(self, k) -> np.ndarray:
        return np.diff(self.mats[k].row_ptr.astype(np.int64))

    def column_counts(self, k) -> np.ndarray:
        """terms per wire (repeats included): the row lengths of the transposed matrix the setup reads"""
        return np.bincount(self.mats[k].col, minlength=self.M)

    def row_values(self, k, w=None, nthreads=8) -> np.ndarray:
        return cpu_ref.spmv(self.mats[k], self.m, self.M, self.w if w is None else w, nthreads=nthreads)

    def to_rows(self):
        """the Vec<Vec<(coeff, column)>> form the Python oracle takes (small instances only)"""
        out = []
        for mat in self.mats:
            cs, cf = mat.col.tolist(), ints_of(mat.coeff)
            rp = mat.row_ptr.tolist()
            out.append([list(zip(cf[rp[i]:rp[i + 1]], cs[rp[i]:rp[i + 1]])) for i in range(self.m)])
        return tuple(out)


def circom_instance(l, m, M, seed, boundaries=ROW_BOUNDARIES, exact_columns=EXACT_COLUMNS, hot_terms=5000, repeat_len=700,
                    cancel_pairs=300, mixes=(MIX_CIRCOM, MIX_CIRCOM, MIX_CIRCOM), dict_size=(64, 64, 64), nthreads=8) -> Instance:
    """dict_size[k] = the number of distinct dictionary values of matrix k, or None: a fresh value for every DICT term"""
    rng = np.random.default_rng(seed)
    n_special = len(boundaries) + 2
    assert m >= n_special and M >= l + 4 >= 5
    # reserved wires: l and l + 1 carry exactly exact_columns terms; no random term lands on them
    wires = dict(one=0, hot1=l + 2, hot2=l + 3)
    for k, n in enumerate(exact_columns):
        wires["exact%d" % n] = l + k
    special = rng.permutation(m)[:n_special]
    rows = {"len%d" % n: int(r) for n, r in zip(boundaries, special)}
    rows["repeat"], rows["cancel"] = int(special[-2]), int(special[-1])
    w = _random_fr(rng, M)
    w[0] = 0
    w[0, 0] = 1                                        # the constant-one wire
    if not w[wires["hot1"]].any():
        w[wires["hot1"], 0] = 7                        # the repeated wire's points must reach the proof
    mats = []
    for k in range(3):
        lengths = rng.integers(2, 13, size=m).astype(np.int64)
        for n, r in zip(boundaries, special):
            lengths[r] = n
        lengths[rows["repeat"]] = repeat_len + (k == 2)          # C: one more term, the solved one
        lengths[rows["cancel"]] = 2 * cancel_pairs + (k == 2)
        rp = np.zeros(m + 1, np.uint64)
        rp[1:] = np.cumsum(lengths)
        nnz = int(rp[-1])
        # random columns over the wires that are not reserved: [1, M) without l .. l + len(exact_columns) - 1
        ne = len(exact_columns)
        col = rng.integers(1, M - ne, size=nnz, dtype=np.int64)
        col[col >= l] += ne
        kind = rng.choice(5, size=nnz, p=mixes[k])
        fixed = np.zeros(nnz, bool)                             # terms whose column and coefficient are set below
        pivot = None
        if k == 2:
            nonempty = np.flatnonzero(lengths > 0)
            pivot = rp[1:][nonempty].astype(np.int64) - 1       # the last term of every non-empty C row
            fixed[pivot] = True
        rb = int(rp[rows["repeat"]])
        col[rb:rb + repeat_len] = wires["hot1"]                 # one wire, the literal one, repeat_len times
        kind[rb:rb + repeat_len] = ONE
        fixed[rb:rb + repeat_len] = True
        cb = int(rp[rows["cancel"]])
        col[cb:cb + 2 * cancel_pairs] = wires["hot1"]           # c, r - c, c', r - c', ... on one wire
        fixed[cb:cb + 2 * cancel_pairs] = True
        # hot and exact columns at random free positions (mostly inside the long rows: repeats there)
        pool = np.flatnonzero(~fixed)
        want = [(wires["one"], hot_terms), (wires["hot1"], hot_terms), (wires["hot2"], hot_terms)] + \
               [(wires["exact%d" % n], n) for n in exact_columns]
        pick = pool[rng.choice(pool.size, size=sum(c for _, c in want), replace=False)]
        at = 0
        for wire, c in want:
            col[pick[at:at + c]] = wire
            at += c
        # coefficients
        coeff = np.zeros((nnz, 32), np.uint8)
        coeff[kind == ONE, 0] = 1
        coeff[kind == RMAX] = fr_bytes([R - 1])[0]
        p2 = np.flatnonzero(kind == POW2)
        e = rng.integers(0, 254, size=p2.size)
        e[:min(254, e.size)] = np.arange(min(254, e.size))      # every power 2^0 .. 2^253 at least once
        coeff[p2, e // 8] = (1 << (e % 8)).astype(np.uint8)
        dk = np.flatnonzero(kind == DICT)
        if dict_size[k] is None:
            coeff[dk] = _random_fr(rng, dk.size)
        else:
            coeff[dk] = _random_fr(rng, dict_size[k])[rng.integers(0, dict_size[k], size=dk.size)]
        cv = [int(x) for x in rng.integers(2, 2 ** 62, size=cancel_pairs)]
        coeff[cb:cb + 2 * cancel_pairs] = fr_bytes([v for c in cv for v in (c, R - c)])
        if pivot is not None:
            col[pivot] = wires["one"]
            coeff[pivot] = 0
        mats.append(cpu_ref.Csr(rp, col.astype(np.uint32), coeff.reshape(-1)))
    inst = Instance(l, m, M, tuple(mats), w.reshape(-1), rows, wires)
    # solve C's last terms: w_0 = 1, so the coefficient is <A_i,w>·<B_i,w> - (the rest of <C_i,w>)
    a, b, c = (ints_of(inst.row_values(k, nthreads=nthreads)) for k in range(3))
    C = mats[2]
    nonempty = np.flatnonzero(np.diff(C.row_ptr.astype(np.int64)) > 0)
    assert not any(a[i] * b[i] % R for i in np.flatnonzero(np.diff(C.row_ptr.astype(np.int64)) == 0))
    solved = fr_bytes([a[i] * b[i] - c[i] for i in nonempty])
    cf = C.coeff.reshape(-1, 32)
    cf[C.row_ptr[1:][nonempty].astype(np.int64) - 1] = solved
    return inst


def extreme_witness(inst, kind, rng=None, target_row=None, target=0):
    """kind "zeros" / "max": every wire but the constant one 0 / r - 1.  kind "row": a random witness with one wire moved so
    that the row target_row = (matrix k, row i) evaluates to exactly `target` (0 or r - 1) after all sliced levels."""
    M = inst.M
    if kind in ("zeros", "max"):
        w = np.zeros((M, 32), np.uint8)
        if kind == "max":
            w[:] = fr_bytes([R - 1])[0]
        w[0] = 0
        w[0, 0] = 1
        return w.reshape(-1)
    assert kind == "row"
    rng = rng or np.random.default_rng(1)
    w = _random_fr(rng, M)
    w[0] = 0
    w[0, 0] = 1
    k, i = target_row
    mat = inst.mats[k]
    lo, hi = int(mat.row_ptr[i]), int(mat.row_ptr[i + 1])
    cols = mat.col[lo:hi]
    cf = mat.coeff.reshape(-1, 32)[lo:hi]
    # a wire of the row whose summed coefficient in the row is invertible
    for p in np.unique(cols)[::-1]:
        if p == 0:
            continue
        cp = sum(ints_of(cf[cols == p])) % R
        if cp:
            break
    else:
        raise ValueError("row has no adjustable wire")
    v = cpu_ref.fr_inner(cf, w[cols])
    wp = (ints_of(w[p])[0] + (target - v) * pow(cp, R - 2, R)) % R
    w[p] = fr_bytes([wp])[0]
    assert cpu_ref.fr_inner(cf, w[cols]) == target % R
    return w.reshape(-1)


def long_row_matrix(l, m, M, n_terms, seed):
    """A: row 0 has n_terms terms, all with the literal one, over random wires; every other row of A, B and C 1..3 terms.
    Returns (mats, w): cpu_ref.Csr each and a random assignment (not satisfying: the proof is compared byte for byte)."""
    rng = np.random.default_rng(seed)
    mats = []
    for k in range(3):
        lengths = rng.integers(1, 4, size=m).astype(np.int64)
        if k == 0:
            lengths[0] = n_terms
        rp = np.zeros(m + 1, np.uint64)
        rp[1:] = np.cumsum(lengths)
        nnz = int(rp[-1])
        col = rng.integers(0, M, size=nnz, dtype=np.int64).astype(np.uint32)
        coeff = np.zeros((nnz, 32), np.uint8)
        coeff[:, 0] = 1
        if k:
            coeff[:] = _random_fr(rng, nnz)
        mats.append(cpu_ref.Csr(rp, col, coeff.reshape(-1)))
    w = _random_fr(rng, M)
    w[0] = 0
    w[0, 0] = 1
    return tuple(mats), w.reshape(-1)
