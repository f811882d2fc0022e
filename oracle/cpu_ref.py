"""ctypes wrapper of oracle/cpu_ref.c (TEST INFRASTRUCTURE: the checker and the timed CPU baseline;
never imported by the product).  Parity status: see the header of cpu_ref.c ("parity unpinned")."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libcpu_ref.so")


class _Pk(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "a_query", "b_g1_query",
                                          "b_g2_query", "h_query", "l_query")] + \
               [(n, C.c_uint64) for n in ("a_len", "b_g1_len", "b_g2_len", "h_len", "l_len")]


class _Csr(C.Structure):
    _fields_ = [("row_ptr", C.c_void_p), ("col", C.c_void_p), ("coeff", C.c_void_p), ("nnz", C.c_uint64)]


class RefTimings(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("witness_map_s", "msm_h_s", "msm_l_s", "msm_a_s", "msm_b1_s", "msm_b2_s", "load_s", "total_s")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < os.path.getmtime(os.path.join(_HERE, "cpu_ref.c")):
            subprocess.run(["make", "-s", "-C", _HERE], check=True)
        L = C.CDLL(_SO)
        L.ref_num_procs.restype = C.c_int
        L.ref_msm_g1.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
        L.ref_msm_g2.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
        L.ref_ntt.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.ref_witness_map.argtypes = [C.POINTER(_Csr), C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int]
        L.ref_prove.argtypes = [C.POINTER(_Pk), C.POINTER(_Csr), C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int, C.POINTER(RefTimings)]
        L.ref_spmv.argtypes = [C.POINTER(_Csr), C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int]
        L.ref_qap_at.argtypes = [C.POINTER(_Csr), C.c_uint64, C.c_uint64, C.c_uint64] + [C.c_void_p] * 6
        L.ref_fr_inner.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.ref_fr_combine.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 4
        L.ref_fr_powers.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        _lib = L
    return _lib


def num_procs() -> int:
    return lib().ref_num_procs()


def cpu_quota() -> float:
    """CPUs this process may actually use at once: the cgroup's quota / period (cgroup v2 cpu.max, v1 cpu.cfs_*), or
    +inf without one.  The GPU boxes of this pool show 256 hardware threads and a quota of 16 CPUs: more runnable threads
    than that are throttled by the kernel, which is what the 13 s witness map on 256 threads was
    (profiles/r02_cpu_thread_scaling.txt), not a property of the code."""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            return float(q) / float(p)
    except Exception:
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0 and p > 0:
            return q / p
    except Exception:
        pass
    return float("inf")


def best_threads(visible=None) -> int:
    """threads for the timed baseline: every CPU the process is allowed to use (visible threads capped by the cgroup quota)"""
    import math
    visible = visible or num_procs()
    q = cpu_quota()
    return max(1, min(visible, int(math.ceil(q)) if q != float("inf") else visible))


def _u8(a):
    if isinstance(a, (bytes, bytearray)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)


def msm_g1(bases, scalars, nthreads=1) -> bytes:
    b, s = _u8(bases), _u8(scalars)
    n = min(b.size // 64, s.size // 32)
    out = np.zeros(64, np.uint8)
    lib().ref_msm_g1(b.ctypes.data, s.ctypes.data, n, out.ctypes.data, nthreads)
    return out.tobytes()


def msm_g2(bases, scalars, nthreads=1) -> bytes:
    b, s = _u8(bases), _u8(scalars)
    n = min(b.size // 128, s.size // 32)
    out = np.zeros(128, np.uint8)
    lib().ref_msm_g2(b.ctypes.data, s.ctypes.data, n, out.ctypes.data, nthreads)
    return out.tobytes()


def ntt(data, inverse=False, coset=False, nthreads=1) -> np.ndarray:
    a = _u8(data).copy()
    n = a.size // 32
    rc = lib().ref_ntt(a.ctypes.data, n.bit_length() - 1, int(inverse), int(coset), nthreads)
    assert rc == 0
    return a


def _csr3(mats):
    """mats: three objects with row_ptr(uint64)/col(uint32)/coeff(uint8) numpy arrays"""
    arr = (_Csr * 3)()
    keep = []
    for i, m in enumerate(mats):
        col = m.col if m.col.size else np.zeros(1, np.uint32)
        coeff = m.coeff if m.coeff.size else np.zeros(32, np.uint8)
        keep += [col, coeff, m.row_ptr]
        arr[i].row_ptr = m.row_ptr.ctypes.data
        arr[i].col = col.ctypes.data
        arr[i].coeff = coeff.ctypes.data
        arr[i].nnz = int(m.col.size)
    return arr, keep


def witness_map(mats, l, m, M, witness, nthreads=1) -> np.ndarray:
    D = 1
    while D < m + l:
        D <<= 1
    arr, _k = _csr3(mats)
    w = _u8(witness)
    h = np.zeros(D * 32, np.uint8)
    rc = lib().ref_witness_map(arr, l, m, M, w.ctypes.data, h.ctypes.data, nthreads)
    assert rc == 0
    return h


def spmv(mat, rows, M, witness, nthreads=1) -> np.ndarray:
    """<M_i, w> for every row i < rows (evaluate_constraint, r1cs_to_qap.rs:16-45): rows x 32 canonical bytes"""
    arr, _k = _csr3((mat, mat, mat))
    w = _u8(witness)
    out = np.zeros(max(1, rows) * 32, np.uint8)
    rc = lib().ref_spmv(arr, rows, M, w.ctypes.data, out.ctypes.data, nthreads)
    assert rc == 0
    return out[:rows * 32]


def _fr(x: int) -> np.ndarray:
    return np.frombuffer(int(x).to_bytes(32, "little"), np.uint8).copy()


def qap_at(mats, l, m, M, t: int, want_u=False):
    """instance_map_with_evaluation (r1cs_to_qap.rs:103-147) at the point t: (a, b, c) as M x 32 canonical bytes each, zt as
    an int (and u = L_j(t), D x 32, when asked for)."""
    D = 1
    while D < m + l:
        D <<= 1
    arr, _k = _csr3(mats)
    a, b, c = (np.zeros(M * 32, np.uint8) for _ in range(3))
    zt = np.zeros(32, np.uint8)
    u = np.zeros(D * 32, np.uint8) if want_u else None
    tb = _fr(t)
    rc = lib().ref_qap_at(arr, l, m, M, tb.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data, zt.ctypes.data,
                          u.ctypes.data if want_u else None)
    assert rc == 0, rc
    out = (a, b, c, int.from_bytes(zt.tobytes(), "little"))
    return out + (u,) if want_u else out


def fr_inner(a, b) -> int:
    a, b = _u8(a), _u8(b)
    n = min(a.size, b.size) // 32
    out = np.zeros(32, np.uint8)
    lib().ref_fr_inner(a.ctypes.data, b.ctypes.data, n, out.ctypes.data)
    return int.from_bytes(out.tobytes(), "little")


def fr_combine(a, b, c, x: int, y: int, z: int) -> np.ndarray:
    """(x*a_i + y*b_i + c_i) * z"""
    a, b, c = _u8(a), _u8(b), _u8(c)
    n = a.size // 32
    out = np.zeros(n * 32, np.uint8)
    xb, yb, zb = _fr(x), _fr(y), _fr(z)
    lib().ref_fr_combine(a.ctypes.data, b.ctypes.data, c.ctypes.data, n, xb.ctypes.data, yb.ctypes.data, zb.ctypes.data,
                         out.ctypes.data)
    return out


def fr_powers(s: int, t: int, n: int) -> np.ndarray:
    """s * t^i, i < n"""
    out = np.zeros(n * 32, np.uint8)
    sb, tb = _fr(s), _fr(t)
    lib().ref_fr_powers(sb.ctypes.data, tb.ctypes.data, n, out.ctypes.data)
    return out


def prove(pk, mats, l, m, M, witness, r: int, s: int, nthreads=1, timings=False):
    """pk: object with the ProvingKey fields of crescent_credentials_amd.api (canonical packed numpy arrays)."""
    k = _Pk()
    arrs = dict(alpha_g1=pk.vk.alpha_g1, beta_g1=pk.beta_g1, delta_g1=pk.delta_g1, beta_g2=pk.vk.beta_g2, delta_g2=pk.vk.delta_g2,
                a_query=pk.a_query, b_g1_query=pk.b_g1_query, b_g2_query=pk.b_g2_query, h_query=pk.h_query, l_query=pk.l_query)
    keep = {}
    for name, a in arrs.items():
        a = _u8(a)
        if a.size == 0:
            a = np.zeros(64, np.uint8)
        keep[name] = a
        setattr(k, name, a.ctypes.data)
    k.a_len = pk.a_query.size // 64
    k.b_g1_len = pk.b_g1_query.size // 64
    k.b_g2_len = pk.b_g2_query.size // 128
    k.h_len = pk.h_query.size // 64
    k.l_len = pk.l_query.size // 64
    arr, _k = _csr3(mats)
    w = _u8(witness)
    rb = np.frombuffer(int(r).to_bytes(32, "little"), np.uint8).copy()
    sb = np.frombuffer(int(s).to_bytes(32, "little"), np.uint8).copy()
    out = np.zeros(256, np.uint8)
    tm = RefTimings()
    rc = lib().ref_prove(C.byref(k), arr, l, m, M, w.ctypes.data, rb.ctypes.data, sb.ctypes.data, out.ctypes.data, nthreads, C.byref(tm))
    assert rc == 0, rc
    return (out.tobytes(), tm.as_dict()) if timings else out.tobytes()


# ---- the files either side of the prove step at full size (cpu_ref.c, last section) ----------------------------------
class _R1csInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_wires", "n_pub_out", "n_pub_in", "n_prv_in", "n_constraints")] + \
               [("nnz", C.c_uint64 * 3), ("cons_off", C.c_uint64)]


class _PkLayout(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_abc", "off_abc", "off_beta_g1", "off_a", "n_a", "off_b1", "n_b1", "off_b2", "n_b2",
                                          "off_h", "n_h", "off_l", "n_l", "end")]


class Csr:
    """one matrix as the three numpy arrays every caller here passes around"""

    def __init__(self, row_ptr, col, coeff):
        self.row_ptr, self.col, self.coeff = row_ptr, col, coeff
        self.nnz = int(col.size)


def write_r1cs(mats, m, n_wires, n_pub_out, n_pub_in, n_prv_in) -> np.ndarray:
    """main_c.r1cs for three CSR matrices (writer side of r1cs_reader.rs:54-256)"""
    L = lib()
    arr, _k = _csr3(mats)
    L.ref_r1cs_file_size.restype = C.c_uint64
    L.ref_r1cs_file_size.argtypes = [C.POINTER(_Csr), C.c_uint64, C.c_uint64]
    L.ref_r1cs_write.argtypes = [C.POINTER(_Csr), C.c_uint64] + [C.c_uint32] * 4 + [C.c_void_p, C.c_uint64]
    size = L.ref_r1cs_file_size(arr, m, n_wires)
    out = np.empty(size, np.uint8)
    rc = L.ref_r1cs_write(arr, m, n_wires, n_pub_out, n_pub_in, n_prv_in, out.ctypes.data, size)
    assert rc == 0, rc
    return out


def read_r1cs(data):
    """-> (info dict, (A, B, C) as Csr): the sequential reader, timed as the CPU side of a cold start"""
    L = lib()
    d = _u8(data)
    info = _R1csInfo()
    L.ref_r1cs_scan.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(_R1csInfo)]
    rc = L.ref_r1cs_scan(d.ctypes.data, d.size, C.byref(info))
    assert rc == 0, rc
    m = info.n_constraints
    rps = [np.empty(m + 1, np.uint64) for _ in range(3)]
    cols = [np.empty(max(1, info.nnz[k]), np.uint32) for k in range(3)]
    cfs = [np.empty(max(1, info.nnz[k]) * 32, np.uint8) for k in range(3)]
    P = C.c_void_p * 3
    L.ref_r1cs_fill.argtypes = [C.c_void_p, C.POINTER(_R1csInfo), P, P, P]
    rc = L.ref_r1cs_fill(d.ctypes.data, C.byref(info), P(*[a.ctypes.data for a in rps]), P(*[a.ctypes.data for a in cols]),
                         P(*[a.ctypes.data for a in cfs]))
    assert rc == 0, rc
    mats = tuple(Csr(rps[k], cols[k][:info.nnz[k]], cfs[k][:32 * info.nnz[k]]) for k in range(3))
    hdr = dict(n_wires=info.n_wires, n_pub_out=info.n_pub_out, n_pub_in=info.n_pub_in, n_prv_in=info.n_prv_in, n_constraints=m,
               num_inputs=1 + info.n_pub_in + info.n_pub_out, num_variables=info.n_wires)
    return hdr, mats


def _pk_struct(pk):
    k = _Pk()
    arrs = dict(alpha_g1=pk.vk.alpha_g1, beta_g1=pk.beta_g1, delta_g1=pk.delta_g1, beta_g2=pk.vk.beta_g2, delta_g2=pk.vk.delta_g2,
                a_query=pk.a_query, b_g1_query=pk.b_g1_query, b_g2_query=pk.b_g2_query, h_query=pk.h_query, l_query=pk.l_query)
    keep = {}
    for name, a in arrs.items():
        a = _u8(a)
        if a.size == 0:
            a = np.zeros(64, np.uint8)
        keep[name] = a
        setattr(k, name, a.ctypes.data)
    k.a_len, k.b_g1_len, k.b_g2_len = pk.a_query.size // 64, pk.b_g1_query.size // 64, pk.b_g2_query.size // 128
    k.h_len, k.l_len = pk.h_query.size // 64, pk.l_query.size // 64
    return k, keep


def write_pk(pk, nthreads=8) -> np.ndarray:
    """ark-serialize uncompressed ProvingKey (the `groth16_params` that leads prover_params.bin) from packed canonical arrays"""
    L = lib()
    k, _keep = _pk_struct(pk)
    gabc, g2 = _u8(pk.vk.gamma_abc_g1), _u8(pk.vk.gamma_g2)
    L.ref_pk_file_size.restype = C.c_uint64
    L.ref_pk_file_size.argtypes = [C.POINTER(_Pk), C.c_uint64]
    L.ref_pk_write.argtypes = [C.POINTER(_Pk), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int]
    size = L.ref_pk_file_size(C.byref(k), gabc.size // 64)
    out = np.empty(size, np.uint8)
    rc = L.ref_pk_write(C.byref(k), g2.ctypes.data, gabc.ctypes.data, gabc.size // 64, out.ctypes.data, size, nthreads)
    assert rc == 0, rc
    return out


class _Vk:
    pass


class PkArrays:
    """what read_pk returns: the ProvingKey fields cpu_ref.prove takes (packed canonical numpy arrays)"""


def read_pk(data, nthreads=8):
    """-> (PkArrays, bytes consumed): flags stripped, no curve checks (creds/src/utils.rs:186)"""
    L = lib()
    d = _u8(data)
    lay = _PkLayout()
    L.ref_pk_scan.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(_PkLayout)]
    rc = L.ref_pk_scan(d.ctypes.data, d.size, C.byref(lay))
    assert rc == 0, rc
    L.ref_points_strip.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int]

    def pts(off, n, sz):
        out = np.empty(max(1, n) * sz, np.uint8)
        L.ref_points_strip(d.ctypes.data + off, n, sz, out.ctypes.data, nthreads)
        return out[:n * sz]
    pk = PkArrays()
    pk.vk = _Vk()
    pk.vk.alpha_g1, pk.vk.beta_g2, pk.vk.gamma_g2 = pts(0, 1, 64), pts(64, 1, 128), pts(192, 1, 128)
    pk.vk.delta_g1, pk.vk.delta_g2 = pts(320, 1, 64), pts(384, 1, 128)
    pk.vk.gamma_abc_g1 = pts(lay.off_abc, lay.n_abc, 64)
    pk.beta_g1, pk.delta_g1 = pts(lay.off_beta_g1, 1, 64), pts(lay.off_beta_g1 + 64, 1, 64)
    pk.a_query, pk.b_g1_query = pts(lay.off_a, lay.n_a, 64), pts(lay.off_b1, lay.n_b1, 64)
    pk.b_g2_query = pts(lay.off_b2, lay.n_b2, 128)
    pk.h_query, pk.l_query = pts(lay.off_h, lay.n_h, 64), pts(lay.off_l, lay.n_l, 64)
    return pk, int(lay.end)
