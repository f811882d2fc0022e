"""ctypes bindings for libcrescent_gpu.so + a host-side mirror of the reference's Groth16 interface.

Names follow `forks/groth16` (Groth16::create_proof_with_reduction_and_matrices, ProvingKey,
VerifyingKey, Proof, LibsnarkReduction::witness_map_from_matrices, generate_parameters_with_qap) so
the parity tests read like the reference's own tests.  All data crossing into the library are packed
little-endian byte arrays (numpy uint8), exactly the C ABI of include/crescent_gpu.h.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CRESCENT_GPU_LIB (read by this Python harness, not by the library): load another build of the same ABI - the tuning
# build `libcrescent_gpu_tuning.so` of tools/ab_*.sh and of the fault-injection test
_LIB_PATH = os.environ.get("CRESCENT_GPU_LIB") or os.path.join(_HERE, "libcrescent_gpu.so")
TUNING_LIB_PATH = os.path.join(_HERE, "libcrescent_gpu_tuning.so")

FR_MODULUS = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
FQ_MODULUS = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
CG_FORM_CANONICAL, CG_FORM_MONTGOMERY = 0, 1
CG_FLAG_H_COEFFICIENT_BASIS = 1
CG_FLAG_LATENCY_MODE, CG_FLAG_THROUGHPUT_MODE, CG_FLAG_SPIN_WAIT, CG_FLAG_CONTIGUOUS_H_SHARDS, CG_FLAG_H_SCALARS_EXTERNAL = 2, 4, 8, 16, 32
CG_FLAG_STAGED_LOAD = 64
CG_FLAG_NO_LONE_SLOT = 128
CG_FLAG_CHECK_WITNESS = 256
CG_FLAG_SCALARS_MONTGOMERY = 512
CG_ERR_UNSATISFIED = -8
CG_VERIFY_REJECT, CG_VERIFY_ACCEPT, CG_VERIFY_MALFORMED = 0, 1, 2
CG_IO_REVEALED, CG_IO_HIDDEN, CG_IO_COMMITTED = 0, 1, 2      # PublicIOType, creds/src/structs.rs:33-37
CG_SHOW_MADE, CG_SHOW_MALFORMED = 1, 2
CG_P256_BAD_SIGNATURE = 3          # cg_p256_rtu_batch alone: the row is well formed and its signature does not verify
CG_RANGE_N_RAND, CG_RANGE_N_RESP = 18, 6
CG_DEVICE_LINK_N_RAND = 9


class CrescentGpuError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("libcrescent_gpu error %d: %s" % (code, msg))
        self.code = code


class UnsatisfiedWitness(CrescentGpuError):
    """The witness fails a constraint (CG_ERR_UNSATISFIED): the reference's `cs.is_satisfied()` failing in the circom builder
    (builder.rs:82-94) or in the prover's debug assertion (prover.rs:197).  `report` is the WitnessReport when the check
    itself was called (check_witness, Groth16.prove(check_witness=True)); a proving call on a flagged context
    (Prover(check_witness=True)) names the constraint in its message only."""

    def __init__(self, msg: str, report: Optional["WitnessReport"] = None):
        super().__init__(CG_ERR_UNSATISFIED, msg)
        self.report = report


def library_path() -> str:
    return _LIB_PATH


class _CgProvingKey(C.Structure):
    _fields_ = [
        ("coord_form", C.c_uint32),
        ("alpha_g1", C.c_void_p), ("beta_g1", C.c_void_p), ("delta_g1", C.c_void_p),
        ("beta_g2", C.c_void_p), ("delta_g2", C.c_void_p),
        ("a_query", C.c_void_p), ("a_len", C.c_uint64),
        ("b_g1_query", C.c_void_p), ("b_g1_len", C.c_uint64),
        ("b_g2_query", C.c_void_p), ("b_g2_len", C.c_uint64),
        ("h_query", C.c_void_p), ("h_len", C.c_uint64),
        ("l_query", C.c_void_p), ("l_len", C.c_uint64),
    ]


class _CgCsr(C.Structure):
    _fields_ = [("row_ptr", C.c_void_p), ("col", C.c_void_p), ("coeff", C.c_void_p), ("nnz", C.c_uint64)]


class _CgOptions(C.Structure):
    _fields_ = [("device", C.c_int32), ("window_bits", C.c_int32), ("shard_rank", C.c_int32),
                ("shard_count", C.c_int32), ("proof_slots", C.c_int32), ("flags", C.c_int32), ("hw_queues", C.c_int32), ("shard_span", C.c_int32)]


class CgTimings(C.Structure):
    _fields_ = [("upload_ms", C.c_float), ("witness_map_ms", C.c_float), ("msm_h_ms", C.c_float),
                ("msm_l_ms", C.c_float), ("msm_a_ms", C.c_float), ("msm_b1_ms", C.c_float),
                ("msm_b2_ms", C.c_float), ("finish_ms", C.c_float), ("total_ms", C.c_float),
                ("msm_g1_pairs", C.c_uint64), ("msm_g2_pairs", C.c_uint64),
                ("accum_g1_ms", C.c_float), ("accum_g2_ms", C.c_float), ("sort_ms", C.c_float), ("reserved_ms", C.c_float),
                ("entries_g1", C.c_uint64), ("entries_g2", C.c_uint64),
                ("accum_g1_launches", C.c_uint32), ("accum_g2_launches", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CgCtxInfo(C.Structure):
    _fields_ = [("table_bytes", C.c_uint64), ("matrix_bytes", C.c_uint64), ("slot_bytes", C.c_uint64), ("total_bytes", C.c_uint64),
                ("device_free_bytes", C.c_uint64), ("device_total_bytes", C.c_uint64), ("proof_slots", C.c_int32),
                ("window_bits", C.c_int32 * 5), ("tuned", C.c_int32), ("retune_skipped_for_memory", C.c_int32),
                ("retune_attempts", C.c_int32), ("shard_rank", C.c_int32), ("shard_count", C.c_int32), ("latency_mode", C.c_int32),
                ("warmup", C.c_int32), ("lone_slots", C.c_int32), ("reserved", C.c_int32 * 2), ("slot_entry_bytes", C.c_uint64),
                ("slot_piece_bytes", C.c_uint64), ("slot_bucket_bytes", C.c_uint64), ("slot_transform_bytes", C.c_uint64),
                ("slot_upload_bytes", C.c_uint64), ("lone_slot_bytes", C.c_uint64)]


class CgLoadTimings(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("total_ms", "matrices_ms", "domain_ms", "key_copy_ms", "fold_ms", "window_tables_ms", "slots_ms",
                                         "final_slots_ms", "background_ms", "swap_wait_ms", "ready_after_ms")] + \
               [(n, C.c_int32) for n in ("staged", "ready", "windows_from_proof", "warmup_proofs", "background_status")] + \
               [("reserved", C.c_int32 * 3)]


class _CgWitnessReport(C.Structure):
    _fields_ = [("n_unsatisfied", C.c_uint64), ("first_unsatisfied", C.c_uint64), ("a", C.c_uint8 * 32), ("b", C.c_uint8 * 32),
                ("c", C.c_uint8 * 32), ("check_ms", C.c_float), ("reserved", C.c_int32 * 7)]


@dataclass
class WitnessReport:
    """cg_witness_report: how many constraints the assignment fails, the first of them (what `which_is_unsatisfied` names)
    and the three inner products of that row as integers"""
    n_unsatisfied: int
    first_unsatisfied: Optional[int]
    a: Optional[int]
    b: Optional[int]
    c: Optional[int]
    check_ms: float

    @property
    def satisfied(self) -> bool:
        return self.n_unsatisfied == 0


def _check_witness_call(fn, handle, assignment, on_device: bool, num_variables: int) -> WitnessReport:
    rep = _CgWitnessReport()
    if on_device:
        rc = fn(handle, C.c_void_p(assignment), 1, C.byref(rep))
    else:
        w = _u8(assignment, num_variables * 32)
        rc = fn(handle, _ptr(w), 0, C.byref(rep))
    if rc != CG_ERR_UNSATISFIED:
        _check(rc)
    bad = rep.n_unsatisfied != 0
    val = lambda f: int.from_bytes(bytes(f), "little") if bad else None
    return WitnessReport(int(rep.n_unsatisfied), int(rep.first_unsatisfied) if bad else None, val(rep.a), val(rep.b), val(rep.c),
                         float(rep.check_ms))


class _CgProverParamsView(C.Structure):
    _fields_ = [("pk", _CgProvingKey), ("gamma_g2", C.c_void_p), ("gamma_abc_g1", C.c_void_p), ("gamma_abc_len", C.c_uint64),
                ("vk_bytes", C.c_void_p), ("vk_len", C.c_uint64), ("pvk_bytes", C.c_void_p), ("pvk_len", C.c_uint64),
                ("config_str", C.c_void_p), ("config_len", C.c_uint64)]


class _CgClientStateView(C.Structure):
    _fields_ = [("inputs", C.c_void_p), ("n_inputs", C.c_uint64), ("aux", C.c_void_p), ("aux_len", C.c_uint64),
                ("has_aux", C.c_int32), ("has_input_com_randomness", C.c_int32), ("proof", C.c_void_p),
                ("vk_bytes", C.c_void_p), ("vk_len", C.c_uint64), ("pvk_bytes", C.c_void_p), ("pvk_len", C.c_uint64),
                ("input_com_randomness", C.c_void_p),
                ("openings_bytes", C.c_void_p), ("openings_len", C.c_uint64), ("n_openings", C.c_uint64),
                ("credtype", C.c_void_p), ("credtype_len", C.c_uint64), ("config_str", C.c_void_p), ("config_len", C.c_uint64)]


class _CgShowRangeLink(C.Structure):
    _fields_ = [("committed_index", C.c_uint32), ("slot", C.c_uint32)]


class _CgRangeRows(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("com_f", "com_g", "com_q", "evals", "proofs", "randomizers", "pok_c", "pok_s")]


class _CgDeviceLinkRows(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("com1", "comz", "h_q", "m", "pi0_c", "pi0_s", "pi1_c", "pi1_s")]


class _CgDeviceLinkMade(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("com1", "comz", "m", "pi0_c", "pi0_s", "pi1_c", "pi1_s")]


class _CgRangeMade(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("com_f", "com_g", "com_q", "evals", "proofs", "pok_c", "pok_s", "challenges")]


class _CgR1csHeader(C.Structure):
    _fields_ = [("field_size", C.c_uint32), ("n_wires", C.c_uint32), ("n_pub_out", C.c_uint32),
                ("n_pub_in", C.c_uint32), ("n_prv_in", C.c_uint32), ("n_constraints", C.c_uint32),
                ("n_labels", C.c_uint64), ("num_inputs", C.c_uint64), ("num_variables", C.c_uint64)]


# every symbol include/crescent_gpu.h declares, with its signature
_SIGNATURES = {
    "cg_init": (C.c_int, [C.c_int, C.c_void_p]),
    "cg_set_device": (C.c_int, [C.c_int32]),
    "cg_last_error": (C.c_char_p, []),
    "cg_version": (C.c_char_p, []),
    "cg_circuit_load": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(_CgProvingKey), C.POINTER(_CgCsr), C.c_uint64,
                                  C.c_uint64, C.c_uint64, C.POINTER(_CgOptions)]),
    "cg_circuit_free": (None, [C.c_void_p]),
    "cg_prove": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CgTimings)]),
    "cg_prove_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CgTimings)]),
    "cg_prove_partial": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(CgTimings)]),
    "cg_assemble": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cg_witness_map_coset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "cg_h_scalars_slice": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cg_prove_partial_q": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(CgTimings)]),
    "cg_prove_partial_q_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "cg_partial_witness_map_coset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "cg_prove_partial_q_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(CgTimings)]),
    "cg_prove_partial_q_abort": (None, [C.c_void_p]),
    "cg_witness_map_coset_half": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "cg_partial_witness_map_coset_half": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "cg_prove_partial_q_finish2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(CgTimings)]),
    "cg_host_alloc": (C.c_void_p, [C.c_uint64]),
    "cg_host_free": (None, [C.c_void_p]),
    "cg_host_register": (C.c_int, [C.c_void_p, C.c_uint64]),
    "cg_host_unregister": (C.c_int, [C.c_void_p]),
    "cg_ctx_get_info": (C.c_int, [C.c_void_p, C.POINTER(CgCtxInfo)]),
    "cg_ctx_get_load_timings": (C.c_int, [C.c_void_p, C.POINTER(CgLoadTimings)]),
    "cg_ctx_wait_ready": (C.c_int, [C.c_void_p, C.c_int32]),
    "cg_probe_shader_clock": (C.c_int, [C.c_int32, C.c_uint32, C.POINTER(C.c_double)]),
    "cg_witness_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cg_check_witness": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(_CgWitnessReport)]),
    "cg_qap_check_witness": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(_CgWitnessReport)]),
    "cg_domain_size": (C.c_uint64, [C.c_void_p]),
    "cg_qap_load": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(_CgCsr), C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32]),
    "cg_qap_load_form": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(_CgCsr), C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, C.c_uint32]),
    "cg_scalars_convert": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint64]),
    "cg_qap_witness_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "cg_qap_domain_size": (C.c_uint64, [C.c_void_p]),
    "cg_qap_free": (None, [C.c_void_p]),
    "cg_msm_g1": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p]),
    "cg_msm_g2": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p]),
    "cg_ntt": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_int]),
    "cg_msm_load_g1": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(_CgOptions)]),
    "cg_msm_load_g2": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(_CgOptions)]),
    "cg_msm_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.POINTER(CgTimings)]),
    "cg_msm_free": (None, [C.c_void_p]),
    "cg_ntt_load": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_int32]),
    "cg_ntt_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "cg_ntt_free": (None, [C.c_void_p]),
    "cg_fixed_base_g1": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "cg_fixed_base_g2": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "cg_setup": (C.c_int, [C.POINTER(_CgCsr), C.c_uint64, C.c_uint64, C.c_uint64] + [C.c_void_p] * 11),
    "cg_r1cs_parse": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "cg_r1cs_get": (C.c_int, [C.c_void_p, C.POINTER(_CgR1csHeader), C.POINTER(_CgCsr), C.POINTER(C.c_void_p)]),
    "cg_r1cs_free": (None, [C.c_void_p]),
    "cg_pk_parse": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "cg_pk_get": (C.c_int, [C.c_void_p, C.POINTER(_CgProvingKey), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "cg_pk_free": (None, [C.c_void_p]),
    "cg_pk_serialized_size": (C.c_uint64, [C.POINTER(_CgProvingKey), C.c_uint64]),
    "cg_pk_serialize": (C.c_int, [C.POINTER(_CgProvingKey), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "cg_prover_params_parse": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "cg_prover_params_get": (C.c_int, [C.c_void_p, C.POINTER(_CgProverParamsView)]),
    "cg_prover_params_free": (None, [C.c_void_p]),
    "cg_prover_params_serialized_size": (C.c_uint64, [C.POINTER(_CgProvingKey), C.c_uint64, C.c_uint64, C.c_uint64]),
    "cg_prover_params_serialize": (C.c_int, [C.POINTER(_CgProvingKey), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                             C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "cg_client_state_serialized_size": (C.c_uint64, [C.POINTER(_CgClientStateView)]),
    "cg_client_state_serialize": (C.c_int, [C.POINTER(_CgClientStateView), C.c_void_p, C.c_uint64]),
    "cg_client_state_parse": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "cg_client_state_get": (C.c_int, [C.c_void_p, C.POINTER(_CgClientStateView)]),
    "cg_client_state_free": (None, [C.c_void_p]),
    "cg_pvk_load": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64, C.c_int32]),
    "cg_pvk_num_inputs": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cg_pvk_set_latency_mode": (C.c_int, [C.c_void_p, C.c_int32]),
    "cg_pvk_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "cg_verify_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]),
    "cg_verify_show_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "cg_show_rand_count": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cg_show_commit_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cg_show_respond_batch": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                        C.c_void_p]),
    "cg_pvk_free": (None, [C.c_void_p]),
    "cg_range_pk_load": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32]),
    "cg_range_pk_add_bases": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "cg_range_pk_free": (None, [C.c_void_p]),
    "cg_range_pk_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "cg_range_commit_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "cg_range_quotient_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cg_range_open_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "cg_range_respond_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "cg_range_vk_load": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32]),
    "cg_range_vk_add_bases": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "cg_range_vk_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "cg_range_vk_set_latency_mode": (C.c_int, [C.c_void_p, C.c_int32]),
    "cg_range_vk_free": (None, [C.c_void_p]),
    "cg_range_verify_batch": (C.c_int, [C.c_void_p, C.c_uint32] + [C.c_void_p] * 11 + [C.c_uint64, C.c_void_p, C.c_void_p]),
    "cg_range_prove_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 9),
    "cg_range_verify_proofs_batch": (C.c_int, [C.c_void_p, C.c_uint32] + [C.c_void_p] * 9 + [C.c_uint64, C.c_void_p]),
    "cg_dlog_challenge_batch": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "cg_verify_showings_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64] + [C.c_void_p] * 6
                                 + [C.c_uint32, C.POINTER(_CgShowRangeLink), C.c_void_p, C.POINTER(_CgRangeRows), C.c_uint64, C.c_void_p, C.c_void_p]),
    "cg_pvk_set_showings_overlap": (C.c_int, [C.c_void_p, C.c_int32]),
    "cg_create_showings_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64] + [C.c_void_p] * 3
                                 + [C.c_uint32, C.POINTER(_CgShowRangeLink), C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 5
                                 + [C.POINTER(_CgRangeMade), C.c_void_p, C.c_void_p]),
    "cg_show_shift_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cg_device_link_verify_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(_CgDeviceLinkRows),
                                              C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cg_device_link_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "cg_device_link_prove_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(_CgDeviceLinkMade), C.c_void_p, C.c_void_p]),
    "cg_device_link_prove_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "cg_poseidon_p256_permute_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "cg_hq_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "cg_device_link_prove_hq_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_uint64, C.POINTER(_CgDeviceLinkMade), C.c_void_p, C.c_void_p, C.c_void_p]),
    "cg_hq_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "cg_p256_tu_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cg_p256_rtu_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cg_p256_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "cg_t256_gens_load": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)]),
    "cg_t256_gens_free": (None, [C.c_void_p]),
    "cg_t256_gens_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cg_t256_commit_rows_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "cg_hyrax_commit_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "cg_t256_commit_last_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "cg_revealed_digest_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64, C.c_void_p]),
    "cg_prepare_verifying_key": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
}

_lib = None


def _init_torch_runtime_first() -> None:
    """A Python process that uses torch tensors next to this library holds TWO HIP runtimes: the ROCm one
    libcrescent_gpu.so links and the copy bundled in the torch wheel (different SONAMEs, so the loader keeps both).
    Measured on the MI355X pool: with the bundled runtime initialised first both work; the other way round torch then
    reports "No HIP GPUs are available".  So when torch is present its runtime is brought up before the library is
    loaded.  Hosts without torch (the Rust shim) are not affected."""
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass


def lib() -> C.CDLL:
    """The HIP library.  Raises if it has not been built: there is deliberately no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise CrescentGpuError(-2, "%s not found; run `python -c 'import __graft_entry__ as g; g.build()'`" % _LIB_PATH)
        _init_torch_runtime_first()
        L = C.CDLL(_LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc: int) -> None:
    if rc == CG_ERR_UNSATISFIED:
        raise UnsatisfiedWitness(lib().cg_last_error().decode("utf-8", "replace"))
    if rc != 0:
        raise CrescentGpuError(rc, lib().cg_last_error().decode("utf-8", "replace"))


def _u8(a, nbytes: Optional[int] = None) -> np.ndarray:
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    if nbytes is not None and a.size != nbytes:
        raise ValueError("expected %d bytes, got %d" % (nbytes, a.size))
    return a


def fr_to_bytes(x: int) -> bytes:
    return int(x % FR_MODULUS).to_bytes(32, "little")


def scalars_to_array(vals: Sequence[int]) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).copy()


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def _p256_point(xy: np.ndarray):
    """x ‖ y, 64 bytes big-endian -> (x, y), or None for the identity's 64 zero bytes"""
    b = xy.tobytes()
    return (int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")) if any(b) else None


def scalars_convert(a, in_form: int, out_form: int, out: Optional[np.ndarray] = None) -> np.ndarray:
    """cg_scalars_convert: n x 32 B scalars from one form (CG_FORM_CANONICAL / CG_FORM_MONTGOMERY) to the other, on the
    library's host threads; no GPU involved.  out: a writable uint8 array of the same size to convert into (`a` itself
    converts in place); default a new array.  An element >= r raises CrescentGpuError naming its index; `out` is then
    untouched."""
    src = a if isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags.c_contiguous else _u8(a)
    src = src.reshape(-1)
    if src.size % 32:
        raise ValueError("length is not a multiple of 32 bytes")
    if out is None:
        out = np.empty(src.size, dtype=np.uint8)
    if out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable or out.size != src.size:
        raise ValueError("out must be a writable contiguous uint8 array of the input's size")
    _check(lib().cg_scalars_convert(_ptr(src) if src.size else None, in_form, _ptr(out) if out.size else None, out_form, src.size // 32))
    return out


def show_rand_count(io_types) -> int:
    """the scalars one showing of this layout consumes (cg_show_rand_count): 3 + n_committed + n_resp"""
    io = _u8(np.asarray(list(io_types), dtype=np.uint8))
    n = C.c_uint64()
    _check(lib().cg_show_rand_count(_ptr(io) if io.size else None, io.size, C.byref(n)))
    return int(n.value)


# ------------------------------------------------------------------------------------------------
# data structures (forks/groth16/src/data_structures.rs)
# ------------------------------------------------------------------------------------------------
@dataclass
class VerifyingKey:
    """data_structures.rs:31-44 (fork adds delta_g1).  Packed canonical bytes."""
    alpha_g1: np.ndarray
    beta_g2: np.ndarray
    gamma_g2: np.ndarray
    delta_g1: np.ndarray
    delta_g2: np.ndarray
    gamma_abc_g1: np.ndarray      # num_inputs x 64


@dataclass
class ProvingKey:
    """data_structures.rs:101-118.  Queries are packed arrays: G1 64 B, G2 128 B per point, identity = zeros."""
    vk: VerifyingKey
    beta_g1: np.ndarray
    delta_g1: np.ndarray
    a_query: np.ndarray
    b_g1_query: np.ndarray
    b_g2_query: np.ndarray
    h_query: np.ndarray
    l_query: np.ndarray
    coord_form: int = CG_FORM_CANONICAL

    def _c(self) -> _CgProvingKey:
        k = _CgProvingKey()
        k.coord_form = self.coord_form
        k.alpha_g1 = _ptr(self.vk.alpha_g1); k.beta_g1 = _ptr(self.beta_g1); k.delta_g1 = _ptr(self.delta_g1)
        k.beta_g2 = _ptr(self.vk.beta_g2); k.delta_g2 = _ptr(self.vk.delta_g2)
        k.a_query = _ptr(self.a_query); k.a_len = self.a_query.size // 64
        k.b_g1_query = _ptr(self.b_g1_query); k.b_g1_len = self.b_g1_query.size // 64
        k.b_g2_query = _ptr(self.b_g2_query); k.b_g2_len = self.b_g2_query.size // 128
        k.h_query = _ptr(self.h_query); k.h_len = self.h_query.size // 64
        k.l_query = _ptr(self.l_query); k.l_len = self.l_query.size // 64
        return k


@dataclass
class Proof:
    """data_structures.rs:7-14; `data` is the 256-byte ark-serialize uncompressed a ‖ b ‖ c."""
    data: bytes

    def serialize_uncompressed(self) -> bytes:
        return self.data

    @property
    def a(self) -> bytes:
        return self.data[:64]

    @property
    def b(self) -> bytes:
        return self.data[64:192]

    @property
    def c(self) -> bytes:
        return self.data[192:]


@dataclass
class _Csr:
    row_ptr: np.ndarray   # uint64, rows + 1
    col: np.ndarray       # uint32
    coeff: np.ndarray     # uint8, nnz * 32 canonical

    @property
    def nnz(self) -> int:
        return int(self.col.size)


class ConstraintMatrices:
    """ark-relations ConstraintMatrices<F> (fields visible at forks/circom-compat/src/zkey.rs:181-193),
    held as three CSR matrices."""

    def __init__(self, a: _Csr, b: _Csr, c: _Csr, num_instance_variables: int, num_witness_variables: int,
                 num_constraints: int, _keepalive=None):
        self.a, self.b, self.c = a, b, c
        self.num_instance_variables = num_instance_variables
        self.num_witness_variables = num_witness_variables
        self.num_constraints = num_constraints
        self._keepalive = _keepalive

    @staticmethod
    def from_rows(A, B, Cm, num_instance_variables: int, num_variables: int) -> "ConstraintMatrices":
        """rows: list of list of (coeff:int, column:int) — the Vec<Vec<(F, usize)>> form."""
        def conv(rows):
            rp = np.zeros(len(rows) + 1, dtype=np.uint64)
            cols, coefs = [], []
            for i, row in enumerate(rows):
                for coeff, col in row:
                    cols.append(col)
                    coefs.append(int(coeff % FR_MODULUS).to_bytes(32, "little"))
                rp[i + 1] = len(cols)
            return _Csr(rp, np.asarray(cols, dtype=np.uint32), np.frombuffer(b"".join(coefs), dtype=np.uint8).copy()
                        if coefs else np.zeros(0, dtype=np.uint8))
        return ConstraintMatrices(conv(A), conv(B), conv(Cm), num_instance_variables,
                                  num_variables - num_instance_variables, len(A))

    @property
    def num_variables(self) -> int:
        return self.num_instance_variables + self.num_witness_variables

    def _c(self):
        arr = (_CgCsr * 3)()
        keep = []
        for i, m in enumerate((self.a, self.b, self.c)):
            col = m.col if m.col.size else np.zeros(1, dtype=np.uint32)
            coeff = m.coeff if m.coeff.size else np.zeros(32, dtype=np.uint8)
            keep += [col, coeff]
            arr[i].row_ptr = _ptr(m.row_ptr); arr[i].col = _ptr(col); arr[i].coeff = _ptr(coeff); arr[i].nnz = m.nnz
        return arr, keep


# ------------------------------------------------------------------------------------------------
# prover
# ------------------------------------------------------------------------------------------------
class OpenPartial:
    """a sharded proof between cg_prove_partial_q_begin and _finish (cg_partial): it holds one of its context's proof slots"""

    def __init__(self, prover, handle, keep):
        self._prover, self._h, self._keep = prover, handle, keep

    def witness_map_coset(self, out_dev: Optional[int] = None, out_host: Optional[int] = None):
        """cg_partial_witness_map_coset (the rank that runs the witness map): all coset values for this proof's assignment,
        shard-major; -> numpy bytes, or written to the device address out_dev / the host address out_host"""
        if out_dev is not None:
            _check(lib().cg_partial_witness_map_coset(self._h, C.c_void_p(int(out_dev)), 1))
            return None
        if out_host is not None:
            _check(lib().cg_partial_witness_map_coset(self._h, C.c_void_p(int(out_host)), 0))
            return None
        q = np.zeros(self._prover.domain_size * 32, dtype=np.uint8)
        _check(lib().cg_partial_witness_map_coset(self._h, _ptr(q), 0))
        return q

    def witness_map_coset_half(self, which: int, out_dev: Optional[int] = None, out_host: Optional[int] = None):
        """cg_partial_witness_map_coset_half: ONE side of the coset values (which = 0: vinv·a, 1: b) for this proof's assignment"""
        if out_dev is not None:
            _check(lib().cg_partial_witness_map_coset_half(self._h, which, C.c_void_p(int(out_dev)), 1))
            return None
        if out_host is not None:
            _check(lib().cg_partial_witness_map_coset_half(self._h, which, C.c_void_p(int(out_host)), 0))
            return None
        q = np.zeros(self._prover.domain_size * 32, dtype=np.uint8)
        _check(lib().cg_partial_witness_map_coset_half(self._h, which, _ptr(q), 0))
        return q

    def finish2(self, a_slice, b_slice, on_device: bool = False, timings: bool = False):
        """cg_prove_partial_q_finish2: the h share from this shard's slices of BOTH sides (their products are the h scalars)"""
        out = np.zeros(384, dtype=np.uint8)
        if on_device:
            ap, bp = C.c_void_p(int(a_slice)), C.c_void_p(int(b_slice))
        else:
            a, b = _u8(a_slice), _u8(b_slice)
            ap, bp = C.c_void_p(_ptr(a) if a.size else _ptr(out)), C.c_void_p(_ptr(b) if b.size else _ptr(out))
        tm = CgTimings()
        h, self._h = self._h, None
        _check(lib().cg_prove_partial_q_finish2(h, ap, bp, 1 if on_device else 0, _ptr(out), C.byref(tm) if timings else None))
        return (out.tobytes(), tm.as_dict()) if timings else out.tobytes()

    def finish(self, q_slice, q_on_device: bool = False, timings: bool = False):
        """cg_prove_partial_q_finish: the h share with this shard's slice; -> the 384-byte record.  The handle is gone afterwards,
        whether the call succeeded or not."""
        out = np.zeros(384, dtype=np.uint8)
        if q_on_device:
            qptr = C.c_void_p(int(q_slice))
        else:
            q = _u8(q_slice)
            qptr = C.c_void_p(_ptr(q) if q.size else _ptr(out))
        tm = CgTimings()
        h, self._h = self._h, None
        _check(lib().cg_prove_partial_q_finish(h, qptr, 1 if q_on_device else 0, _ptr(out), C.byref(tm) if timings else None))
        return (out.tobytes(), tm.as_dict()) if timings else out.tobytes()

    def abort(self):
        if self._h is not None:
            h, self._h = self._h, None
            lib().cg_prove_partial_q_abort(h)

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass


class Prover:
    """A circuit loaded on one GPU (cg_ctx): proving key tables + matrices resident in HBM."""

    def __init__(self, pk: ProvingKey, matrices: ConstraintMatrices, device: int = -1, window_bits: int = 0,
                 shard_rank: int = 0, shard_count: int = 1, proof_slots: int = 1, h_coefficient_basis: bool = False,
                 mode: Optional[str] = None, spin_wait: bool = False, contiguous_h_shards: bool = False,
                 h_scalars_external: bool = False, flags: int = 0, staged_load: bool = False, shard_span: Optional[Tuple[int, int]] = None,
                 lone_slot: bool = True, check_witness: bool = False, scalars_montgomery: bool = False):
        """scalars_montgomery=True: CG_FLAG_SCALARS_MONTGOMERY - every assignment the context receives is x * 2^256 mod r per
        element (arkworks' in-memory Fr) and witness_map returns its coefficients in that form; r, s, the witness report and
        the vectors passed between shards stay canonical.
        check_witness=True: CG_FLAG_CHECK_WITNESS - every proving / witness-map call on the context first checks that the
        witness satisfies the R1CS and raises UnsatisfiedWitness instead of returning a proof that cannot verify.
        lone_slot=False: CG_FLAG_NO_LONE_SLOT (a throughput context then holds no extra slot for proofs that arrive alone).
        h_coefficient_basis=True keeps the h query as loaded (seven transforms per proof, CG_FLAG_H_COEFFICIENT_BASIS).
        shard_span: (lo, hi) in 1/10000 of every query - this shard's part instead of the shard_rank-th of shard_count equal parts
        (cg_options.shard_span: unequal shares for the ranks that also run the witness map).
        staged_load: CG_FLAG_STAGED_LOAD - the call returns as soon as the context can prove (warm-up arrangement) and a worker
        thread of the library finishes the load behind the first proofs (wait_ready(), load_timings()).
        mode: None (proof_slots decides), "latency" or "throughput" (CG_FLAG_LATENCY_MODE / CG_FLAG_THROUGHPUT_MODE);
        spin_wait: CG_FLAG_SPIN_WAIT; contiguous_h_shards: CG_FLAG_CONTIGUOUS_H_SHARDS; h_scalars_external:
        CG_FLAG_H_SCALARS_EXTERNAL (a shard that never runs the witness map: prove_partial_q only); flags: further raw bits."""
        if mode not in (None, "latency", "throughput"):
            raise ValueError("mode must be None, 'latency' or 'throughput'")
        flags |= (CG_FLAG_H_COEFFICIENT_BASIS if h_coefficient_basis else 0) | (CG_FLAG_LATENCY_MODE if mode == "latency" else 0) | \
                 (CG_FLAG_THROUGHPUT_MODE if mode == "throughput" else 0) | (CG_FLAG_SPIN_WAIT if spin_wait else 0) | \
                 (CG_FLAG_CONTIGUOUS_H_SHARDS if contiguous_h_shards else 0) | (CG_FLAG_H_SCALARS_EXTERNAL if h_scalars_external else 0) | \
                 (CG_FLAG_STAGED_LOAD if staged_load else 0) | (0 if lone_slot else CG_FLAG_NO_LONE_SLOT) | \
                 (CG_FLAG_CHECK_WITNESS if check_witness else 0) | (CG_FLAG_SCALARS_MONTGOMERY if scalars_montgomery else 0)
        L = lib()
        self.num_inputs = matrices.num_instance_variables
        self.num_constraints = matrices.num_constraints
        self.num_variables = matrices.num_variables
        opt = _CgOptions(device=device, window_bits=window_bits, shard_rank=shard_rank, shard_count=shard_count,
                         proof_slots=proof_slots, flags=flags, shard_span=(shard_span[0] | shard_span[1] << 16) if shard_span else 0)
        self.proof_slots = max(1, proof_slots)
        cpk = pk._c()
        abc, _keep = matrices._c()
        h = C.c_void_p()
        _check(L.cg_circuit_load(C.byref(h), C.byref(cpk), abc, self.num_inputs, self.num_constraints,
                                 self.num_variables, C.byref(opt)))
        self._h = h
        self.domain_size = int(L.cg_domain_size(h))
        self._lease_lock = threading.Lock()
        self._leases = 0                 # callers inside a cached prover (Groth16._prover_for); close() is deferred while > 0
        self._close_when_idle = False

    def close(self):
        if getattr(self, "_h", None):
            lib().cg_circuit_free(self._h)
            self._h = None

    def _lease(self) -> "Prover":
        with self._lease_lock:
            self._leases += 1
        return self

    def _unlease(self) -> None:
        with self._lease_lock:
            self._leases -= 1
            retire = self._leases == 0 and self._close_when_idle
        if retire:
            self.close()

    def _retire(self) -> None:
        """evicted from a cache: closed now if nobody is inside it, otherwise by the last caller to leave"""
        with self._lease_lock:
            self._close_when_idle = True
            idle = self._leases == 0
        if idle:
            self.close()

    def info(self) -> dict:
        """cg_ctx_get_info: resident bytes (tables, matrices, per slot), the current window of each MSM, whether the
        one-time re-tune happened or was skipped for lack of memory"""
        ci = CgCtxInfo()
        _check(lib().cg_ctx_get_info(self._h, C.byref(ci)))
        d = {k: getattr(ci, k) for k, _ in ci._fields_ if k not in ("window_bits", "reserved")}
        d["window_bits"] = dict(zip(("h", "l", "a", "b_g1", "b_g2"), list(ci.window_bits)))
        return d

    def load_timings(self) -> dict:
        """cg_ctx_get_load_timings: where the time of cg_circuit_load went; for a staged load also the background part"""
        lt = CgLoadTimings()
        _check(lib().cg_ctx_get_load_timings(self._h, C.byref(lt)))
        return {k: (round(getattr(lt, k), 3) if isinstance(getattr(lt, k), float) else getattr(lt, k)) for k, _ in lt._fields_ if k != "reserved"}

    def wait_ready(self, timeout_ms: int = -1) -> bool:
        """cg_ctx_wait_ready: True once the final arrangement is in force, False when the time ran out first; raises when the
        background part of a staged load failed"""
        rc = lib().cg_ctx_wait_ready(self._h, timeout_ms)
        if rc == 1:
            return False
        _check(rc)
        return True

    def check_witness(self, assignment, on_device: bool = False) -> WitnessReport:
        """cg_check_witness: does the assignment (host scalars, or a device address with on_device) satisfy the R1CS, and
        which constraint fails first (`cs.is_satisfied()` / `which_is_unsatisfied()`, builder.rs:82-94).  Returns the
        report either way; a non-canonical element raises CrescentGpuError as prove() does."""
        return _check_witness_call(lib().cg_check_witness, self._h, assignment, on_device, self.num_variables)

    def prove_host_ptr(self, ptr: int, r: int, s: int, timings: bool = False):
        """cg_prove on a raw host address (num_variables x 32 B canonical): pageable or page-locked (HostBuffer)"""
        out = np.zeros(256, dtype=np.uint8)
        rb, sb = _u8(fr_to_bytes(r)), _u8(fr_to_bytes(s))
        tm = CgTimings()
        _check(lib().cg_prove(self._h, C.c_void_p(ptr), _ptr(rb), _ptr(sb), _ptr(out), C.byref(tm) if timings else None))
        p = Proof(out.tobytes())
        return (p, tm.as_dict()) if timings else p

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prove(self, full_assignment, r: int, s: int, timings: bool = False):
        w = _u8(full_assignment, self.num_variables * 32)
        out = np.zeros(256, dtype=np.uint8)
        rb, sb = _u8(fr_to_bytes(r)), _u8(fr_to_bytes(s))
        tm = CgTimings()
        _check(lib().cg_prove(self._h, _ptr(w), _ptr(rb), _ptr(sb), _ptr(out), C.byref(tm) if timings else None))
        p = Proof(out.tobytes())
        return (p, tm.as_dict()) if timings else p

    def prove_dev(self, d_ptr: int, r: int, s: int, timings: bool = False):
        """assignment already in this GPU's memory (e.g. a torch uint8 tensor's data_ptr())."""
        out = np.zeros(256, dtype=np.uint8)
        rb, sb = _u8(fr_to_bytes(r)), _u8(fr_to_bytes(s))
        tm = CgTimings()
        _check(lib().cg_prove_dev(self._h, C.c_void_p(d_ptr), _ptr(rb), _ptr(sb), _ptr(out), C.byref(tm) if timings else None))
        p = Proof(out.tobytes())
        return (p, tm.as_dict()) if timings else p

    def prove_partial(self, assignment, r: int, on_device: bool = False, timings: bool = False):
        out = np.zeros(384, dtype=np.uint8)
        rb = _u8(fr_to_bytes(r))
        if on_device:
            ptr = C.c_void_p(int(assignment))
        else:
            w = _u8(assignment, self.num_variables * 32)
            ptr = C.c_void_p(_ptr(w))
        tm = CgTimings()
        _check(lib().cg_prove_partial(self._h, ptr, 1 if on_device else 0, _ptr(rb), _ptr(out), C.byref(tm) if timings else None))
        return (out.tobytes(), tm.as_dict()) if timings else out.tobytes()

    def prove_partial_q(self, assignment, q_slice, r: int, on_device: bool = False, q_on_device: bool = False, timings: bool = False):
        """cg_prove_partial_q: this shard's partial sums with its h scalars supplied (its slice of witness_map_coset's
        output: h_scalars_slice); the witness map is skipped.  assignment / q_slice: numpy bytes, or device addresses."""
        out = np.zeros(384, dtype=np.uint8)
        rb = _u8(fr_to_bytes(r))
        if on_device:
            ptr = C.c_void_p(int(assignment))
        else:
            w = _u8(assignment, self.num_variables * 32)
            ptr = C.c_void_p(_ptr(w))
        if q_on_device:
            qptr = C.c_void_p(int(q_slice))
        else:
            q = _u8(q_slice)
            qptr = C.c_void_p(_ptr(q) if q.size else _ptr(rb))
        tm = CgTimings()
        _check(lib().cg_prove_partial_q(self._h, ptr, 1 if on_device else 0, qptr, 1 if q_on_device else 0, _ptr(rb), _ptr(out),
                                        C.byref(tm) if timings else None))
        return (out.tobytes(), tm.as_dict()) if timings else out.tobytes()

    def prove_partial_q_begin(self, assignment, r: int, on_device: bool = False) -> "OpenPartial":
        """cg_prove_partial_q_begin: takes a proof slot, queues this shard's l, a, b1, b2 partial sums and returns while they run;
        the h share follows with OpenPartial.finish(slice) once the slice has arrived"""
        rb = _u8(fr_to_bytes(r))
        keep = None
        if on_device:
            ptr = C.c_void_p(int(assignment))
        else:
            keep = _u8(assignment, self.num_variables * 32)
            ptr = C.c_void_p(_ptr(keep))
        h = C.c_void_p()
        _check(lib().cg_prove_partial_q_begin(self._h, ptr, 1 if on_device else 0, _ptr(rb), C.byref(h)))
        return OpenPartial(self, h, keep)

    def h_scalars_slice(self, shard: int) -> Tuple[int, int]:
        """(offset, count) of shard `shard`'s scalars inside witness_map_coset's output, in elements (cg_h_scalars_slice)"""
        off, cnt = C.c_uint64(), C.c_uint64()
        _check(lib().cg_h_scalars_slice(self._h, shard, C.byref(off), C.byref(cnt)))
        return int(off.value), int(cnt.value)

    def witness_map_coset(self, assignment, on_device: bool = False, out_dev: Optional[int] = None, out_host: Optional[int] = None):
        """cg_witness_map_coset: ALL coset values q_j of the quotient's a·b part (folded key), domain_size x 32 B canonical,
        shard-major for this context's shard count.  -> numpy bytes, or written to the device address out_dev / the host
        address out_host (domain_size x 32 writable bytes)."""
        if on_device:
            ptr = C.c_void_p(int(assignment))
        else:
            w = _u8(assignment, self.num_variables * 32)
            ptr = C.c_void_p(_ptr(w))
        if out_dev is not None:
            _check(lib().cg_witness_map_coset(self._h, ptr, 1 if on_device else 0, C.c_void_p(int(out_dev)), 1))
            return None
        if out_host is not None:
            _check(lib().cg_witness_map_coset(self._h, ptr, 1 if on_device else 0, C.c_void_p(int(out_host)), 0))
            return None
        q = np.zeros(self.domain_size * 32, dtype=np.uint8)
        _check(lib().cg_witness_map_coset(self._h, ptr, 1 if on_device else 0, _ptr(q), 0))
        return q

    def witness_map_coset_half(self, assignment, which: int, on_device: bool = False, out_dev: Optional[int] = None,
                               out_host: Optional[int] = None):
        """cg_witness_map_coset_half: ONE side of the coset values - which = 0: vinv·a(g w^j), 1: b(g w^j) - as plain canonical
        integers, laid out like witness_map_coset's output; q is their product mod r"""
        if on_device:
            ptr = C.c_void_p(int(assignment))
        else:
            w = _u8(assignment, self.num_variables * 32)
            ptr = C.c_void_p(_ptr(w))
        if out_dev is not None:
            _check(lib().cg_witness_map_coset_half(self._h, ptr, 1 if on_device else 0, which, C.c_void_p(int(out_dev)), 1))
            return None
        if out_host is not None:
            _check(lib().cg_witness_map_coset_half(self._h, ptr, 1 if on_device else 0, which, C.c_void_p(int(out_host)), 0))
            return None
        q = np.zeros(self.domain_size * 32, dtype=np.uint8)
        _check(lib().cg_witness_map_coset_half(self._h, ptr, 1 if on_device else 0, which, _ptr(q), 0))
        return q

    def assemble(self, partials: bytes, n_shards: int, r: int, s: int) -> Proof:
        pb = _u8(partials, 384 * n_shards)
        out = np.zeros(256, dtype=np.uint8)
        rb, sb = _u8(fr_to_bytes(r)), _u8(fr_to_bytes(s))
        _check(lib().cg_assemble(self._h, _ptr(pb), n_shards, _ptr(rb), _ptr(sb), _ptr(out)))
        return Proof(out.tobytes())

    def witness_map(self, full_assignment) -> np.ndarray:
        w = _u8(full_assignment, self.num_variables * 32)
        h = np.zeros(self.domain_size * 32, dtype=np.uint8)
        _check(lib().cg_witness_map(self._h, _ptr(w), _ptr(h)))
        return h


class HostBuffer:
    """Page-locked host memory from cg_host_alloc, viewed as a numpy uint8 array (`.array`): where a host lets the
    witness calculator write the full assignment so that cg_prove's upload is one asynchronous DMA."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        self.ptr = lib().cg_host_alloc(self.nbytes)
        if not self.ptr:
            raise CrescentGpuError(-4, lib().cg_last_error().decode("utf-8", "replace"))
        self.array = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_uint8)), shape=(self.nbytes,))

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            lib().cg_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def set_device(device: int) -> None:
    """cg_set_device: the GPU that the entry points without a device of their own (the setup, the one-shot MSM / NTT) use
    from this thread on.  Needed next to torch: the library links its own HIP runtime, which does not see
    torch.cuda.set_device."""
    _check(lib().cg_set_device(device))


def probe_shader_clock(device: int = -1, window_us: int = 20000) -> float:
    """GHz the shader engines hold over the next `window_us` (cg_probe_shader_clock); safe to call from a second thread
    while proofs run"""
    g = C.c_double(0.0)
    _check(lib().cg_probe_shader_clock(device, window_us, C.byref(g)))
    return float(g.value)


def host_register(a: np.ndarray) -> None:
    """pin an existing contiguous numpy buffer in place (cg_host_register); undo with host_unregister before freeing it"""
    _check(lib().cg_host_register(C.c_void_p(a.ctypes.data), a.nbytes))


def host_unregister(a: np.ndarray) -> None:
    _check(lib().cg_host_unregister(C.c_void_p(a.ctypes.data)))


class _Handle:
    """What the classes that own one C handle share.  `_h` is the c_void_p their load call fills and `_free` names the C
    symbol that releases it.  close() is idempotent, `with` closes on exit, and __del__ swallows errors (an interpreter
    that is shutting down may have let go of the library already)."""
    _free = ""

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(lib(), self._free)(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _LatencyMode:
    """The pairing stage's arrangement of the two verifying keys (PreparedVerifyingKey, RangeVerifyingKey);
    `_set_latency_mode` names the C symbol."""

    def set_latency(self, on: bool) -> None:
        """True: one workgroup per proof, for a host that answers one request at a time; False (the default): one lane per
        proof, for batches (cg_pvk_set_latency_mode / cg_range_vk_set_latency_mode).  The verdicts are the same."""
        _check(getattr(lib(), self._set_latency_mode)(self._h, 1 if on else 0))


class _RangeSlots:
    """The slots and the kernel times of the two range keys (RangeProofKey, RangeVerifyingKey); `_add_bases` and
    `_last_kernel_ms` name the C symbols."""

    def add_bases(self, gamma_abc_point, delta_g1) -> int:
        """registers the Pedersen bases of one range-checked input (2 x 64 B ark-serialize uncompressed G1) and returns
        their slot (cg_range_pk_add_bases / cg_range_vk_add_bases)"""
        b = _u8(bytes(gamma_abc_point) + bytes(delta_g1), 128)
        slot = C.c_uint32()
        _check(getattr(lib(), self._add_bases)(self._h, _ptr(b), C.byref(slot)))
        return int(slot.value)

    def last_kernel_ms(self) -> Tuple[float, float]:
        """HIP-event milliseconds of the last GPU call on this key, by stage: (polynomial stage, fixed-base walks) of a
        RangeProofKey, (group stage, pairing) of a RangeVerifyingKey"""
        a, b = C.c_float(), C.c_float()
        _check(getattr(lib(), self._last_kernel_ms)(self._h, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)


class QapContext(_Handle):
    """Three constraint matrices resident on one GPU with their domain tables, no proving key (cg_qap_ctx)."""
    _free = "cg_qap_free"

    def __init__(self, matrices: ConstraintMatrices, device: int = -1, scalar_form: int = CG_FORM_CANONICAL):
        """scalar_form: the form of the assignments witness_map / check_witness take and of the h witness_map returns
        (cg_qap_load_form); CG_FORM_MONTGOMERY = arkworks' in-memory Fr"""
        self.num_inputs = matrices.num_instance_variables
        self.num_constraints = matrices.num_constraints
        self.num_variables = matrices.num_variables
        abc, _keep = matrices._c()
        self._h = C.c_void_p()
        _check(lib().cg_qap_load_form(C.byref(self._h), abc, self.num_inputs, self.num_constraints, self.num_variables, device, scalar_form))
        self.scalar_form = scalar_form
        self.domain_size = int(lib().cg_qap_domain_size(self._h))
        self._lease_lock = threading.Lock()
        self._leases = 0
        self._close_when_idle = False

    _lease = Prover._lease
    _unlease = Prover._unlease
    _retire = Prover._retire

    def witness_map(self, full_assignment) -> np.ndarray:
        w = _u8(full_assignment, self.num_variables * 32)
        h = np.zeros(self.domain_size * 32, dtype=np.uint8)
        _check(lib().cg_qap_witness_map(self._h, _ptr(w), 0, _ptr(h), 0))
        return h

    def check_witness(self, assignment, on_device: bool = False) -> WitnessReport:
        """cg_qap_check_witness: Prover.check_witness without a key (where the reference's check sits: the circom builder)"""
        return _check_witness_call(lib().cg_qap_check_witness, self._h, assignment, on_device, self.num_variables)

    def witness_map_dev(self, d_assignment: int, d_h: int) -> None:
        """assignment (num_variables x 32 B) and h (domain_size x 32 B) both in this GPU's memory"""
        _check(lib().cg_qap_witness_map(self._h, C.c_void_p(d_assignment), 1, C.c_void_p(d_h), 1))


class R1CSToQAP:
    """forks/groth16/src/r1cs_to_qap.rs:49-98: the trait `Groth16<E, QAP>` is generic over (lib.rs:55-57).  The
    prover's half is `witness_map_from_matrices`; the generator's half (`instance_map_with_evaluation`,
    `h_query_scalars`, :52-56,82-97) is what `generate_parameters_with_qap` -> cg_setup evaluates on the GPU."""

    @classmethod
    def witness_map_from_matrices(cls, matrices: ConstraintMatrices, num_inputs: int, num_constraints: int,
                                  full_assignment) -> np.ndarray:
        raise NotImplementedError


def _content_digest(*arrays) -> bytes:
    """128-bit digest of the bytes of the given numpy arrays / bytes objects (xxh3 when present - tens of milliseconds for
    the 0.6 GB of a full-size circuit - else blake2b).  Cache keys only: never part of a proof."""
    try:
        import xxhash
        h = xxhash.xxh3_128()
    except Exception:
        import hashlib
        h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a)
            h.update(np.int64(a.size).tobytes())
            h.update(a.view(np.uint8).reshape(-1).data if a.size else b"")
        else:
            h.update(np.int64(len(a)).tobytes())
            h.update(a)
    return h.digest()


class _Held:
    """The arrays a content digest was computed over, HELD (so that neither their ids nor their addresses can be recycled by
    an array that replaces them: the memo of rounds 3-4 kept (id, address, size) only, and a dropped array's id and address
    are commonly handed to the next one of the same size) and compared by identity."""

    def __init__(self, arrays):
        self.arrays = tuple(arrays)

    def same_as(self, arrays) -> bool:
        return len(arrays) == len(self.arrays) and all(a is b for a, b in zip(arrays, self.arrays))


def _freeze(*arrays) -> "_Held":
    """The digest of an object is remembered on it, so its arrays must not change afterwards: the arrays that were HASHED are
    made read-only, so that an in-place write through them raises instead of silently proving against the old resident copy.
    Only those: an array they are views of stays as the caller left it (round 5 walked `.base` and froze the parents too, which
    changed unrelated views of a buffer the caller owns).  A view whose parent is still writable can be changed behind the
    memo's back, so such a set is marked not `stable` and its digest is NOT remembered: it is recomputed at every use (0.3 s per
    GB) - slower, never stale.  An attribute REPLACED by another array (the supported way to change a key or a matrix) is seen
    - the memo holds the arrays themselves - and hashed again."""
    stable = True
    for a in arrays:
        if isinstance(a, np.ndarray):
            try:
                a.setflags(write=False)
            except ValueError:
                pass
            b = a.base
            while isinstance(b, np.ndarray):
                if b.flags.writeable:
                    stable = False
                b = b.base
    held = _Held(arrays)
    held.stable = stable
    return held


def _matrices_key(m: "ConstraintMatrices") -> tuple:
    """what the three matrices ARE, not where they live: shape + a digest of every index and coefficient (computed once
    per object and remembered on it; the arrays are immutable from then on, see _freeze)"""
    arrays = (m.a.row_ptr, m.a.col, m.a.coeff, m.b.row_ptr, m.b.col, m.b.coeff, m.c.row_ptr, m.c.col, m.c.coeff)
    memo = getattr(m, "_content_key", None)
    if memo is not None and memo[0].same_as(arrays):
        return memo[1]
    k = (m.num_instance_variables, m.num_witness_variables, m.num_constraints, m.a.nnz, m.b.nnz, m.c.nnz, _content_digest(*arrays))
    held = _freeze(*arrays)
    m._content_key = (held, k) if held.stable else None
    return k


def _pk_key(pk: "ProvingKey") -> tuple:
    """a proving key by content: the verifying key's points, the query lengths and a digest of the queries"""
    arrays = (pk.vk.alpha_g1, pk.vk.beta_g2, pk.vk.gamma_g2, pk.vk.delta_g1, pk.vk.delta_g2, pk.vk.gamma_abc_g1,
              pk.beta_g1, pk.delta_g1, pk.a_query, pk.b_g1_query, pk.b_g2_query, pk.h_query, pk.l_query)
    memo = getattr(pk, "_content_key", None)
    if memo is not None and memo[0].same_as(arrays) and memo[2] == pk.coord_form:
        return memo[1]
    k = (pk.coord_form, pk.a_query.size, pk.h_query.size, pk.l_query.size, _content_digest(*arrays))
    held = _freeze(*arrays)
    pk._content_key = (held, k, pk.coord_form) if held.stable else None
    return k


class _ResidentCache:
    """Resident GPU contexts keyed by the CONTENT of what they were loaded from, least recently used first out, safe to
    use from several threads: lookups and evictions happen under one lock, a context handed out is leased (see
    Prover._lease) and an evicted context is closed by the last caller to leave it, never under one."""

    def __init__(self, max_cached: int):
        self.max_cached = max_cached
        self._lock = threading.Lock()
        self._entries = {}          # key -> context; insertion order = recency
        self._loading = {}          # key -> threading.Event: one thread loads, the others wait for it

    def lease(self, key, make):
        while True:
            with self._lock:
                ctx = self._entries.pop(key, None)
                if ctx is not None:
                    self._entries[key] = ctx                  # most recent
                    return ctx._lease()
                ev = self._loading.get(key)
                if ev is None:
                    ev = self._loading[key] = threading.Event()
                    break
            ev.wait()                                         # another thread is loading this very circuit
        try:
            ctx = make()                                      # seconds: outside the lock
        except BaseException:
            with self._lock:
                self._loading.pop(key).set()
            raise
        evicted = []
        with self._lock:
            self._entries[key] = ctx
            ctx._lease()
            while len(self._entries) > self.max_cached:
                evicted.append(self._entries.pop(next(iter(self._entries))))
            self._loading.pop(key).set()
        for old in evicted:
            old._retire()
        return ctx

    def clear(self):
        with self._lock:
            gone = list(self._entries.values())
            self._entries.clear()
        for ctx in gone:
            ctx._retire()

    def __len__(self):
        with self._lock:
            return len(self._entries)

    def __contains__(self, key):
        with self._lock:
            return key in self._entries


class LibsnarkReduction(R1CSToQAP):
    """forks/groth16/src/r1cs_to_qap.rs:100-226, the default QAP type (lib.rs:55), on the GPU.  The reference's call
    is stateless; the matrices' device copy is kept per matrices CONTENT (shape + digest of every term, at most MAX_CACHED
    resident, least recently used first out) so that repeated calls only move the assignment."""
    MAX_CACHED = 4
    _cache = _ResidentCache(MAX_CACHED)

    @classmethod
    def witness_map_from_matrices(cls, matrices: ConstraintMatrices, num_inputs: int, num_constraints: int,
                                  full_assignment) -> np.ndarray:
        """r1cs_to_qap.rs:150-213 -> the coefficients of h, domain_size x 32 B canonical.  Raises CrescentGpuError
        with code CG_ERR_POLY_DEGREE_TOO_LARGE where the reference returns PolynomialDegreeTooLarge (:156-157)."""
        if num_inputs != matrices.num_instance_variables or num_constraints != matrices.num_constraints:
            raise ValueError("num_inputs/num_constraints disagree with the matrices")
        cls._cache.max_cached = cls.MAX_CACHED
        ctx = cls._cache.lease(_matrices_key(matrices), lambda: QapContext(matrices))
        try:
            return ctx.witness_map(full_assignment)
        finally:
            ctx._unlease()

    @classmethod
    def clear_cache(cls):
        cls._cache.clear()


class Groth16:
    """forks/groth16/src/lib.rs:55-57 / prover.rs.  The reference's calls are stateless; here a loaded circuit (key
    tables + matrices in HBM) is kept per (key, matrices) CONTENT, since re-uploading a 0.6 GB key and redoing the 1.6 s
    change of basis for every proof would defeat the point - also when the caller parses fresh objects from the same
    files for every call, as `create_client_state` does (creds/src/lib.rs:258,268).  At most `MAX_CACHED` circuits stay
    resident; the least recently used one is retired first, and closed only once no thread is inside it."""
    MAX_CACHED = 4
    _cache = _ResidentCache(MAX_CACHED)

    @classmethod
    def _prover_for(cls, pk: ProvingKey, matrices: ConstraintMatrices) -> Prover:
        """a LEASED resident prover for this key and these matrices: the caller must `_unlease()` it"""
        cls._cache.max_cached = cls.MAX_CACHED
        # the load is STAGED (CG_FLAG_STAGED_LOAD): `Groth16::prove` is what create_client_state calls once per credential
        # (creds/src/lib.rs:281-283), so the first proof must not wait for tables that only pay off over many
        return cls._cache.lease((_pk_key(pk), _matrices_key(matrices)), lambda: Prover(pk, matrices, staged_load=True))

    @classmethod
    def create_proof_with_reduction_and_matrices(cls, pk: ProvingKey, r: int, s: int, matrices: ConstraintMatrices,
                                                 num_inputs: int, num_constraints: int, full_assignment,
                                                 check_witness: bool = False) -> Proof:
        """prover.rs:26-51.  check_witness: the `debug_assert!(cs.is_satisfied())` of prover.rs:197 - the witness is checked
        on the resident circuit first and UnsatisfiedWitness (with the report) raised instead of proving."""
        if num_inputs != matrices.num_instance_variables or num_constraints != matrices.num_constraints:
            raise ValueError("num_inputs/num_constraints disagree with the matrices")
        prover = cls._prover_for(pk, matrices)
        try:
            if check_witness:
                rep = prover.check_witness(full_assignment)
                if not rep.satisfied:
                    raise UnsatisfiedWitness("constraint %d of %d is not satisfied (%d in all)"
                                             % (rep.first_unsatisfied, matrices.num_constraints, rep.n_unsatisfied), rep)
            return prover.prove(full_assignment, r, s)
        finally:
            prover._unlease()

    @classmethod
    def create_proof_with_reduction(cls, circuit: "CircomCircuit", pk: ProvingKey, r: int, s: int, check_witness: bool = False) -> Proof:
        """prover.rs:177-221.  The reference synthesises the constraint system from the circuit on every call
        (circuit.rs:29-86) and extracts the matrices (r1cs_to_qap.rs:58-80); here the matrices ARE the circuit's
        R1CS (column = wire id, circuit.rs:61-67) and stay resident, so only the witness travels."""
        if circuit.witness is None:
            raise CrescentGpuError(-1, "AssignmentMissing: the circuit has no witness (SynthesisError::AssignmentMissing, circuit.rs:38-45)")
        cm = circuit.r1cs.matrices
        return cls.create_proof_with_reduction_and_matrices(pk, r, s, cm, cm.num_instance_variables, cm.num_constraints,
                                                            circuit.full_assignment(), check_witness=check_witness)

    @classmethod
    def prove(cls, pk: ProvingKey, circuit: "CircomCircuit", rng, check_witness: bool = False) -> Proof:
        """`SNARK::prove` (lib.rs:76-82) -> create_random_proof_with_reduction (prover.rs:142-154): r and s are
        sampled from `rng` (any object with randrange, e.g. random.Random / random.SystemRandom), r first."""
        r = rng.randrange(FR_MODULUS)
        s = rng.randrange(FR_MODULUS)
        return cls.create_proof_with_reduction(circuit, pk, r, s, check_witness=check_witness)

    @classmethod
    def create_proof_no_zk(cls, circuit: "CircomCircuit", pk: ProvingKey) -> Proof:
        """prover.rs:160-173 (r = s = 0)."""
        return cls.create_proof_with_reduction(circuit, pk, 0, 0)

    @staticmethod
    def prepare_verifying_key(vk_bytes) -> bytes:
        """verifier.rs:13-20 on the host: serialized VerifyingKey -> serialized PreparedVerifyingKey"""
        b = _u8(vk_bytes)
        n = C.c_uint64()
        _check(lib().cg_prepare_verifying_key(_ptr(b) if b.size else None, b.size, None, 0, C.byref(n)))
        out = np.zeros(int(n.value), np.uint8)
        _check(lib().cg_prepare_verifying_key(_ptr(b) if b.size else None, b.size, _ptr(out), out.size, C.byref(n)))
        return out.tobytes()

    @staticmethod
    def verify_batch(pvk: "PreparedVerifyingKey", inputs, proofs) -> np.ndarray:
        """verifier.rs:25-65 for n proofs under one key on the GPU.  inputs: n x num_inputs canonical Fr (one flat byte
        array, or one sequence of ints per proof); proofs: n x 256 B (one flat array, or a list of bytes / Proof).
        Returns n verdict bytes (CG_VERIFY_REJECT / ACCEPT / MALFORMED)."""
        if isinstance(proofs, (list, tuple)):
            proofs = b"".join(p.data if isinstance(p, Proof) else bytes(p) for p in proofs)
        pb = _u8(proofs)
        if pb.size % 256:
            raise ValueError("proofs must be n x 256 bytes")
        n = pb.size // 256
        if isinstance(inputs, (list, tuple)):
            ib = np.concatenate([_inputs_array(x) for x in inputs]) if inputs else np.zeros(0, np.uint8)
        else:
            ib = _u8(inputs)
        if n and ib.size % (32 * n):
            raise ValueError("inputs must be n x num_inputs x 32 bytes")
        n_inputs = ib.size // (32 * n) if n else pvk.num_inputs
        out = np.zeros(max(n, 1), np.uint8)
        _check(lib().cg_verify_batch(pvk._h, _ptr(ib) if ib.size else None, n_inputs, _ptr(pb) if pb.size else None, n, _ptr(out)))
        return out[:n]

    @classmethod
    def verify_with_processed_vk(cls, pvk: "PreparedVerifyingKey", public_inputs, proof) -> bool:
        """`Groth16::verify_with_processed_vk` (verifier.rs:25-65, called at creds/src/lib.rs:288-289).  A proof or an
        input that fails checked deserialisation is rejected (False)."""
        data = proof.data if isinstance(proof, Proof) else bytes(proof)
        return int(cls.verify_batch(pvk, [_inputs_array(public_inputs)], data)[0]) == CG_VERIFY_ACCEPT

    NO_TRANSCRIPT = object()      # verify_show_batch's default `context`: the caller runs the transcript, as before

    @staticmethod
    def verify_show_batch(pvk: "PreparedVerifyingKey", io_types, shows, with_pok: bool = True, context=NO_TRANSCRIPT):
        """`ShowGroth16::verify` (creds/src/groth16rand.rs:232-306) for n showings under one key and one io_types layout,
        up to the Merlin transcript.  io_types: one CG_IO_* per public input; shows: a sequence of (ShowGroth16, revealed
        inputs in input order).  Returns (verdicts, k_bytes): n verdict bytes of the Groth16 half, and per showing the
        n_committed + 1 recomputed Schnorr commitments k_i of `DLogPoK::verify` (creds/src/dlog.rs:137-145) as the 32
        compressed bytes each the transcript absorbs under b"k" - an n x (n_committed + 1) x 32 uint8 array, zero for a
        malformed showing, None with with_pok=False.  The caller runs the transcript and compares the challenge with c.
        With context= (bytes, or None as the reference's `None`) the library's Merlin does that
        (cg_dlog_challenge_batch), and the result is one bool per showing: `ShowGroth16::verify` whole."""
        io = np.ascontiguousarray(np.asarray(list(io_types), dtype=np.uint8))
        n = len(shows)
        n_rev, n_hid, n_com = (int((io == t).sum()) for t in (CG_IO_REVEALED, CG_IO_HIDDEN, CG_IO_COMMITTED))
        n_resp = 2 * n_com + n_hid + 1
        shapes = [2] * n_com + [n_hid + 1]
        for sh, x in shows:
            if [len(si) for si in sh.pok_s] != shapes or len(sh.commited_inputs) != n_com or len(_inputs_array(x)) != 32 * n_rev:
                raise ValueError("a showing does not have the shape of io_types")
        cat = lambda parts, width: _u8(b"".join(parts), n * width)
        fr = lambda v: int(v).to_bytes(32, "little")          # as given: a value >= r must reach the range check
        if context is not Groth16.NO_TRANSCRIPT:
            if not with_pok:
                raise ValueError("the challenge comparison needs the DLogPoK: with_pok=True")
            verdicts, k = Groth16.verify_show_batch(pvk, io, shows)
            # only the accepted showings reach the transcript: a malformed one may hold bytes that are no point at all
            ok = [i for i in range(n) if verdicts[i] == CG_VERIFY_ACCEPT]
            out = [False] * n
            if ok:
                cs = Groth16.show_dlog_challenges(pvk, io, k[ok], _u8(b"".join(b"".join(shows[i][0].commited_inputs) for i in ok)),
                                                  _u8(b"".join(shows[i][0].com_hidden_inputs for i in ok)), context)
                for j, i in enumerate(ok):
                    out[i] = cs[j].tobytes() == fr(shows[i][0].pok_c)
            return out
        return Groth16.verify_show_batch_packed(
            pvk, io, cat([_inputs_array(x).tobytes() for _, x in shows], 32 * n_rev), cat([sh.rand_proof for sh, _ in shows], 256),
            cat([sh.com_hidden_inputs for sh, _ in shows], 64), cat([b"".join(sh.commited_inputs) for sh, _ in shows], 64 * n_com),
            cat([fr(sh.pok_c) for sh, _ in shows], 32) if with_pok else None,
            cat([b"".join(fr(s) for si in sh.pok_s for s in si) for sh, _ in shows], 32 * n_resp) if with_pok else None)

    @staticmethod
    def verify_show_batch_packed(pvk: "PreparedVerifyingKey", io_types, revealed, rand_proofs, com_hidden, committed, pok_c=None,
                                 pok_s=None):
        """cg_verify_show_batch on flat byte arrays laid out as include/crescent_gpu.h states (n = rand_proofs / 256);
        pok_c = None asks for the Groth16 half only.  Returns (verdicts, k_bytes or None)."""
        io = _u8(np.asarray(io_types, dtype=np.uint8))
        n_rev, n_hid, n_com = (int((io == t).sum()) for t in (CG_IO_REVEALED, CG_IO_HIDDEN, CG_IO_COMMITTED))
        pb = _u8(rand_proofs)
        if pb.size % 256:
            raise ValueError("rand_proofs must be n x 256 bytes")
        n = pb.size // 256
        rev, comh, comm = _u8(revealed, 32 * n_rev * n), _u8(com_hidden, 64 * n), _u8(committed, 64 * n_com * n)
        ptr = lambda a: _ptr(a) if a.size else None
        verdicts = np.zeros(max(n, 1), np.uint8)
        pc = ps = k = None
        if pok_c is not None:
            pc, ps = _u8(pok_c, 32 * n), _u8(pok_s, 32 * (2 * n_com + n_hid + 1) * n)
            k = np.zeros((max(n, 1), n_com + 1, 32), np.uint8)
        _check(lib().cg_verify_show_batch(pvk._h, ptr(io), io.size, ptr(rev), ptr(pb), ptr(comh), ptr(comm),
                                          None if pc is None else ptr(pc), None if ps is None else ptr(ps), n, _ptr(verdicts),
                                          None if k is None else _ptr(k)))
        return verdicts[:n], (None if k is None else k[:n])

    @staticmethod
    def show_commit_batch_packed(pvk: "PreparedVerifyingKey", io_types, proofs, inputs, rand):
        """cg_show_commit_batch on flat byte arrays laid out as include/crescent_gpu.h states (n = proofs / 256): the GPU
        half of `ClientState::show_groth16` (creds/src/groth16rand.rs:100-187) before the transcript.  Returns
        (rand_proofs n x 256, com_hidden n x 64, committed n x n_committed x 64, k_bytes n x (n_committed + 1) x 32,
        status n) as uint8 arrays; a CG_SHOW_MALFORMED showing has zero bytes everywhere."""
        io = _u8(np.asarray(list(io_types), dtype=np.uint8))
        n_com = int((io == CG_IO_COMMITTED).sum())
        pb = _u8(proofs)
        if pb.size % 256:
            raise ValueError("proofs must be n x 256 bytes")
        n = pb.size // 256
        n_rand = show_rand_count(io)
        ib, rb = _u8(inputs, 32 * io.size * n), _u8(rand, 32 * n_rand * n)
        ptr = lambda a: _ptr(a) if a.size else None
        m = max(n, 1)
        rp, comh, comm = np.zeros((m, 256), np.uint8), np.zeros((m, 64), np.uint8), np.zeros((m, max(n_com, 1), 64), np.uint8)
        k, status = np.zeros((m, n_com + 1, 32), np.uint8), np.zeros(m, np.uint8)
        _check(lib().cg_show_commit_batch(pvk._h, ptr(io), io.size, ptr(pb), ptr(ib), ptr(rb), n, _ptr(rp), _ptr(comh), _ptr(comm),
                                          _ptr(k), _ptr(status)))
        return rp[:n], comh[:n], comm[:n, :n_com], k[:n], status[:n]

    @staticmethod
    def show_respond_batch(io_types, inputs, rand, pok_c, status=None) -> np.ndarray:
        """cg_show_respond_batch (host only): the responses s_ij = rho_ij - c * secret_ij of `DLogPoK::prove`
        (creds/src/dlog.rs:101-109) for the challenges pok_c (n x 32 B, or n ints) the host's transcript produced.  inputs,
        rand, status: as given to / returned by show_commit_batch_packed.  Returns n x n_resp x 32 uint8."""
        io = _u8(np.asarray(list(io_types), dtype=np.uint8))
        n_rand = show_rand_count(io)
        n_resp = n_rand - 3 - int((io == CG_IO_COMMITTED).sum())
        if isinstance(pok_c, (list, tuple)):
            pok_c = b"".join(int(c).to_bytes(32, "little") for c in pok_c)
        cb = _u8(pok_c)
        if cb.size % 32:
            raise ValueError("pok_c must be n x 32 bytes")
        n = cb.size // 32
        ib, rb = _u8(inputs, 32 * io.size * n), _u8(rand, 32 * n_rand * n)
        st = None if status is None else _u8(status, n)
        ptr = lambda a: _ptr(a) if a.size else None
        out = np.zeros((max(n, 1), n_resp, 32), np.uint8)
        _check(lib().cg_show_respond_batch(ptr(io), io.size, ptr(ib), ptr(rb), ptr(cb), None if st is None else ptr(st), n, _ptr(out)))
        return out[:n]

    @staticmethod
    def show_batch(pvk: "PreparedVerifyingKey", io_types, states, challenge=None, rand=None, context=None) -> List["ShowGroth16"]:
        """`ClientState::show_groth16` (creds/src/groth16rand.rs:100-187) for n client states of one layout: commit on the
        GPU, the caller's transcript, respond on the host.  states: a sequence of (proof bytes or Proof, inputs);
        rand: per state its show_rand_count scalars in the header's order (ints); None draws them with
        `secrets.randbelow` (r1, r2 non-zero, as prover.rs:234-237 redraws them) - a host that keeps the openings
        (committed_input_openings = the r_i, input_com_randomness = z) draws them itself and passes them in;
        challenge(i, k_bytes, committed, com_hidden) -> int is the host's Merlin transcript (dlog.rs:56-99): it gets state
        i's (n_committed + 1) x 32 compressed k_i, its n_committed x 64 committed points and its 64-byte com_hidden, and
        returns c.  challenge=None is the library's Merlin (cg_dlog_challenge_batch) over `context` (bytes, or None as the
        reference's `None`).  A malformed state (status CG_SHOW_MALFORMED) raises ValueError."""
        io = [int(t) for t in io_types]
        n = len(states)
        if n == 0:
            return []
        if rand is None:
            import secrets
            n_rand = show_rand_count(io)
            rand = [[1 + secrets.randbelow(FR_MODULUS - 1) for _ in range(2)] + [secrets.randbelow(FR_MODULUS) for _ in range(n_rand - 2)]
                    for _ in range(n)]
        n_com, n_hid = io.count(CG_IO_COMMITTED), io.count(CG_IO_HIDDEN)
        fr = lambda v: int(v).to_bytes(32, "little")
        proofs = b"".join(p.data if isinstance(p, Proof) else bytes(p) for p, _ in states)
        inputs = np.concatenate([_inputs_array(x) for _, x in states])
        rb = _u8(b"".join(fr(v) for row in rand for v in row))
        rp, comh, comm, k, status = Groth16.show_commit_batch_packed(pvk, io, proofs, inputs, rb)
        bad = np.nonzero(status != CG_SHOW_MADE)[0]
        if bad.size:
            raise ValueError("client state %d is malformed (its proof, an input or a random scalar)" % int(bad[0]))
        if challenge is None:
            cb = Groth16.show_dlog_challenges(pvk, io, k, comm, comh, context)
            cs = [int.from_bytes(cb[i].tobytes(), "little") for i in range(n)]
        else:
            cs = [int(challenge(i, k[i], comm[i], comh[i])) for i in range(n)]
        s = Groth16.show_respond_batch(io, inputs, rb, cs)
        out = []
        for i in range(n):
            flat = [int.from_bytes(s[i, j].tobytes(), "little") for j in range(s.shape[1])]
            pok_s = [flat[2 * j:2 * j + 2] for j in range(n_com)] + [flat[2 * n_com:]]
            assert len(pok_s[-1]) == n_hid + 1
            out.append(ShowGroth16(rp[i].tobytes(), comh[i].tobytes(), cs[i], pok_s, [comm[i, j].tobytes() for j in range(n_com)]))
        return out

    @staticmethod
    def _range_rows(openings, rand, *challenges):
        """the flat input arrays of a range proof call, checked against one another: (n, openings, rand, challenges...)"""
        ob = _u8(openings)
        if ob.size % 64:
            raise ValueError("openings must be n x 64 bytes (m, r)")
        n = ob.size // 64
        return (n, ob, _u8(rand, 32 * CG_RANGE_N_RAND * n)) + tuple(_u8(c, 32 * n) for c in challenges)

    @staticmethod
    def range_commit_batch_packed(key: "RangeProofKey", slot: int, openings, rand):
        """cg_range_commit_batch on flat byte arrays laid out as include/crescent_gpu.h states: the commitments of
        `RangeProof::prove_n_bits` (creds/src/rangeproof.rs:114-339) before its first challenge.  Returns (com_f n x 64,
        com_g n x 64, ts_out n x 4 x 32 [com_f, com_g, k_0, k_1 compressed], status n) as uint8 arrays."""
        n, ob, rb = Groth16._range_rows(openings, rand)
        ptr = lambda a: _ptr(a) if a.size else None
        m = max(n, 1)
        com_f, com_g, ts, status = np.zeros((m, 64), np.uint8), np.zeros((m, 64), np.uint8), np.zeros((m, 4, 32), np.uint8), np.zeros(m, np.uint8)
        _check(lib().cg_range_commit_batch(key._h, slot, ptr(ob), ptr(rb), n, _ptr(com_f), _ptr(com_g), _ptr(ts), _ptr(status)))
        return com_f[:n], com_g[:n], ts[:n], status[:n]

    @staticmethod
    def range_quotient_batch_packed(key: "RangeProofKey", openings, rand, c):
        """cg_range_quotient_batch: com_q for the challenges c (n x 32 B).  Returns (com_q n x 64, ts_q n x 32, status n)."""
        n, ob, rb, cb = Groth16._range_rows(openings, rand, c)
        ptr = lambda a: _ptr(a) if a.size else None
        m = max(n, 1)
        com_q, ts_q, status = np.zeros((m, 64), np.uint8), np.zeros((m, 32), np.uint8), np.zeros(m, np.uint8)
        _check(lib().cg_range_quotient_batch(key._h, ptr(ob), ptr(rb), ptr(cb), n, _ptr(com_q), _ptr(ts_q), _ptr(status)))
        return com_q[:n], ts_q[:n], status[:n]

    @staticmethod
    def range_open_batch_packed(key: "RangeProofKey", openings, rand, c, rho):
        """cg_range_open_batch: the evaluations and openings for the challenges c and rho (n x 32 B each).  Returns
        (evals n x 3 x 32, proofs n x 3 x 96 [W uncompressed ‖ random_v], status n)."""
        n, ob, rb, cb, hb = Groth16._range_rows(openings, rand, c, rho)
        ptr = lambda a: _ptr(a) if a.size else None
        m = max(n, 1)
        evals, proofs, status = np.zeros((m, 3, 32), np.uint8), np.zeros((m, 3, 96), np.uint8), np.zeros(m, np.uint8)
        _check(lib().cg_range_open_batch(key._h, ptr(ob), ptr(rb), ptr(cb), ptr(hb), n, _ptr(evals), _ptr(proofs), _ptr(status)))
        return evals[:n], proofs[:n], status[:n]

    @staticmethod
    def range_respond_batch(openings, rand, c_dleq, status=None) -> np.ndarray:
        """cg_range_respond_batch (host only): the DLEQ's responses s = nonce - c_dleq * secret (creds/src/dlog.rs:101-109),
        n x 6 x 32 uint8: s_00, s_01, s_10..s_13.  status: cg_range_commit_batch's bytes, or None for "all made"."""
        n, ob, rb, cb = Groth16._range_rows(openings, rand, c_dleq)
        st = None if status is None else _u8(status, n)
        ptr = lambda a: _ptr(a) if a.size else None
        out = np.zeros((max(n, 1), CG_RANGE_N_RESP, 32), np.uint8)
        _check(lib().cg_range_respond_batch(ptr(ob), ptr(rb), ptr(cb), None if st is None else ptr(st), n, _ptr(out)))
        return out[:n]

    @staticmethod
    def show_range_batch(key: "RangeProofKey", slot: int, openings, challenge, rand=None) -> List["RangeProof"]:
        """`ClientState::show_range` (creds/src/groth16rand.rs:193-229) for n Pedersen openings (m, r) (ints) whose bases are
        registered as `slot`: the three GPU calls with the caller's transcripts between them, then the responses.
        challenge(phase, i, data) -> int is the host's Merlin: phase "dleq" gets showing i's 4 x 32 compressed com_f,
        com_g, k_0, k_1 (creds/src/dlog.rs:56-99; the bases and y are the host's own), "c" the 2 x 32 com_f, com_g
        (rangeproof.rs:250-257), "rho" the 32 bytes of com_q (:270-274).  prove_range_batch is the same proof in one call,
        with the library's Merlin.  rand: per opening
        its 18 scalars in the header's order; None draws them with `secrets.randbelow`.  A malformed opening raises
        ValueError."""
        n = len(openings)
        if n == 0:
            return []
        if rand is None:
            import secrets
            rand = [[secrets.randbelow(FR_MODULUS) for _ in range(CG_RANGE_N_RAND)] for _ in range(n)]
        fr = lambda v: int(v).to_bytes(32, "little")
        ob = _u8(b"".join(fr(m) + fr(r) for m, r in openings))
        rb = _u8(b"".join(fr(v) for row in rand for v in row))

        def made(status, what):
            bad = np.nonzero(status != CG_SHOW_MADE)[0]
            if bad.size:
                raise ValueError("opening %d is malformed (%s)" % (int(bad[0]), what))

        com_f, com_g, ts, status = Groth16.range_commit_batch_packed(key, slot, ob, rb)
        made(status, "m, r or a random scalar")
        c_dleq = [int(challenge("dleq", i, ts[i])) for i in range(n)]
        cs = [int(challenge("c", i, ts[i, :2])) for i in range(n)]
        cb = _u8(b"".join(fr(v) for v in cs))
        com_q, ts_q, status = Groth16.range_quotient_batch_packed(key, ob, rb, cb)
        made(status, "the challenge c")
        rhos = [int(challenge("rho", i, ts_q[i])) for i in range(n)]
        evals, proofs, status = Groth16.range_open_batch_packed(key, ob, rb, cb, _u8(b"".join(fr(v) for v in rhos)))
        made(status, "the challenge rho")
        s = Groth16.range_respond_batch(ob, rb, _u8(b"".join(fr(v) for v in c_dleq)))
        val = lambda a: int.from_bytes(a.tobytes(), "little")
        return [RangeProof(com_f[i].tobytes(), com_g[i].tobytes(), val(evals[i, 0]), proofs[i, 0].tobytes(), val(evals[i, 1]),
                           proofs[i, 1].tobytes(), com_q[i].tobytes(), val(evals[i, 2]), proofs[i, 2].tobytes(), c_dleq[i],
                           [[val(s[i, j]) for j in range(2)], [val(s[i, j]) for j in range(2, 6)]]) for i in range(n)]

    @staticmethod
    def range_verify_batch_packed(vk: "RangeVerifyingKey", slot: int, ped_com, com_f, com_g, com_q, evals, proofs, c, rho, randomizers,
                                  pok_c=None, pok_s=None):
        """cg_range_verify_batch on flat byte arrays laid out as include/crescent_gpu.h states (n = com_f / 64):
        `RangeProof::verify_n_bits` (creds/src/rangeproof.rs:342-424) between its transcripts.  pok_c = None checks the
        openings and the evaluation identity only (ped_com may then be None too).  Returns (verdicts n, k_out n x 2 x 32 or
        None) as uint8 arrays."""
        fb = _u8(com_f)
        if fb.size % 64:
            raise ValueError("com_f must be n x 64 bytes")
        n = fb.size // 64
        gb, qb, eb, pb = _u8(com_g, 64 * n), _u8(com_q, 64 * n), _u8(evals, 96 * n), _u8(proofs, 288 * n)
        cb, hb, zb = _u8(c, 32 * n), _u8(rho, 32 * n), _u8(randomizers, 32 * n)
        ptr = lambda a: _ptr(a) if a is not None and a.size else None
        verdicts = np.zeros(max(n, 1), np.uint8)
        cm = pc = ps = k = None
        if pok_c is not None:
            cm, pc, ps = _u8(ped_com, 64 * n), _u8(pok_c, 32 * n), _u8(pok_s, 32 * CG_RANGE_N_RESP * n)
            k = np.zeros((max(n, 1), 2, 32), np.uint8)
        _check(lib().cg_range_verify_batch(vk._h, slot, ptr(cm), ptr(fb), ptr(gb), ptr(qb), ptr(eb), ptr(pb), ptr(cb), ptr(hb), ptr(zb),
                                           ptr(pc), ptr(ps), n, _ptr(verdicts), None if k is None else _ptr(k)))
        return verdicts[:n], (None if k is None else k[:n])

    @staticmethod
    def verify_range_batch(vk: "RangeVerifyingKey", slot: int, ped_coms, proofs: List["RangeProof"], challenge, randomizers=None) -> List[bool]:
        """`ShowRange::verify` (creds/src/groth16rand.rs) for n range proofs about the Pedersen commitments ped_coms (64 B
        ark-serialize uncompressed G1 each) whose bases are registered as `slot`: the mirror of show_range_batch.
        challenge(phase, i, data) -> int is the host's Merlin, called with the data show_range_batch passes: "c" gets the
        2 x 32 compressed com_f, com_g, "rho" the 32 bytes of com_q, "dleq" the 4 x 32 com_f, com_g and the recomputed
        k_0, k_1.  randomizers: per proof (r_1, r_2) below 2^128; None draws them with `secrets`.  Returns one bool per
        proof: the verdict is CG_VERIFY_ACCEPT and the recomputed DLEQ challenge equals the proof's dleq_c."""
        n = len(proofs)
        if len(ped_coms) != n:
            raise ValueError("one Pedersen commitment per proof")
        if n == 0:
            return []
        if randomizers is None:
            import secrets
            randomizers = [(secrets.randbits(128), secrets.randbits(128)) for _ in range(n)]
        fr = lambda v: int(v).to_bytes(32, "little")
        join = lambda f: _u8(b"".join(f(p) for p in proofs))
        cf, cg, cq = (np.stack([_g1_compress(getattr(p, name)) for p in proofs]) for name in ("com_f", "com_g", "com_q"))
        cs = [int(challenge("c", i, np.stack([cf[i], cg[i]]))) for i in range(n)]
        rhos = [int(challenge("rho", i, cq[i])) for i in range(n)]
        verdicts, k = Groth16.range_verify_batch_packed(
            vk, slot, _u8(b"".join(bytes(y) for y in ped_coms)), join(lambda p: bytes(p.com_f)), join(lambda p: bytes(p.com_g)),
            join(lambda p: bytes(p.com_q)), join(lambda p: fr(p.eval_g) + fr(p.eval_gw) + fr(p.eval_w_hat)),
            join(lambda p: bytes(p.proof_g) + bytes(p.proof_gw) + bytes(p.proof_w_hat)), _u8(b"".join(fr(v) for v in cs)),
            _u8(b"".join(fr(v) for v in rhos)), _u8(b"".join(int(r).to_bytes(16, "little") for row in randomizers for r in row)),
            join(lambda p: fr(p.dleq_c)), join(lambda p: b"".join(fr(x) for si in p.dleq_s for x in si)))
        return [bool(verdicts[i] == CG_VERIFY_ACCEPT) and int(challenge("dleq", i, np.stack([cf[i], cg[i], k[i, 0], k[i, 1]]))) == int(proofs[i].dleq_c)
                for i in range(n)]

    @staticmethod
    def range_prove_batch_packed(key: "RangeProofKey", slot: int, openings, ped_com, rand):
        """cg_range_prove_batch on flat byte arrays laid out as include/crescent_gpu.h states: `RangeProof::prove_n_bits`
        whole, the library's Merlin between the phases.  Returns (com_f n x 64, com_g n x 64, com_q n x 64, evals n x 3 x
        32, proofs n x 3 x 96, pok_c n x 32, pok_s n x 6 x 32, challenges n x 3 x 32 (c_dleq, c, rho), status n) as uint8
        arrays; a CG_SHOW_MALFORMED showing has zero bytes everywhere."""
        n, ob, rb = Groth16._range_rows(openings, rand)
        pb = _u8(ped_com, 64 * n)
        ptr = lambda a: _ptr(a) if a.size else None
        m = max(n, 1)
        com_f, com_g, com_q = (np.zeros((m, 64), np.uint8) for _ in range(3))
        evals, proofs = np.zeros((m, 3, 32), np.uint8), np.zeros((m, 3, 96), np.uint8)
        pok_c, pok_s, chal = np.zeros((m, 32), np.uint8), np.zeros((m, CG_RANGE_N_RESP, 32), np.uint8), np.zeros((m, 3, 32), np.uint8)
        status = np.zeros(m, np.uint8)
        _check(lib().cg_range_prove_batch(key._h, slot, ptr(ob), ptr(pb), ptr(rb), n, _ptr(com_f), _ptr(com_g), _ptr(com_q), _ptr(evals),
                                          _ptr(proofs), _ptr(pok_c), _ptr(pok_s), _ptr(chal), _ptr(status)))
        return com_f[:n], com_g[:n], com_q[:n], evals[:n], proofs[:n], pok_c[:n], pok_s[:n], chal[:n], status[:n]

    @staticmethod
    def prove_range_batch(key: "RangeProofKey", slot: int, openings, ped_coms, rand=None) -> List["RangeProof"]:
        """`ClientState::show_range` (creds/src/groth16rand.rs:193-229) for n Pedersen openings (m, r) (ints) of the
        commitments ped_coms (64 B ark-serialize uncompressed each) whose bases are registered as `slot`, in ONE call: the
        transcripts are the library's Merlin, on the GPU (cg_range_prove_batch).  rand: per opening its 18 scalars in the
        header's order; None draws them with `secrets.randbelow`.  A malformed opening raises ValueError."""
        n = len(openings)
        if len(ped_coms) != n:
            raise ValueError("one Pedersen commitment per opening")
        if n == 0:
            return []
        if rand is None:
            import secrets
            rand = [[secrets.randbelow(FR_MODULUS) for _ in range(CG_RANGE_N_RAND)] for _ in range(n)]
        fr = lambda v: int(v).to_bytes(32, "little")
        com_f, com_g, com_q, evals, proofs, pok_c, s, _, status = Groth16.range_prove_batch_packed(
            key, slot, _u8(b"".join(fr(m) + fr(r) for m, r in openings)), _u8(b"".join(bytes(y) for y in ped_coms)),
            _u8(b"".join(fr(v) for row in rand for v in row)))
        bad = np.nonzero(status != CG_SHOW_MADE)[0]
        if bad.size:
            raise ValueError("opening %d is malformed (m, r, a random scalar or its commitment)" % int(bad[0]))
        val = lambda a: int.from_bytes(a.tobytes(), "little")
        return [RangeProof(com_f[i].tobytes(), com_g[i].tobytes(), val(evals[i, 0]), proofs[i, 0].tobytes(), val(evals[i, 1]),
                           proofs[i, 1].tobytes(), com_q[i].tobytes(), val(evals[i, 2]), proofs[i, 2].tobytes(), val(pok_c[i]),
                           [[val(s[i, j]) for j in range(2)], [val(s[i, j]) for j in range(2, 6)]]) for i in range(n)]

    @staticmethod
    def range_verify_proofs_batch_packed(vk: "RangeVerifyingKey", slot: int, ped_com, com_f, com_g, com_q, evals, proofs, randomizers,
                                         pok_c, pok_s) -> np.ndarray:
        """cg_range_verify_proofs_batch on flat byte arrays laid out as include/crescent_gpu.h states (n = com_f / 64):
        `RangeProof::verify_n_bits` whole.  Returns the n verdict bytes."""
        fb = _u8(com_f)
        if fb.size % 64:
            raise ValueError("com_f must be n x 64 bytes")
        n = fb.size // 64
        arrays = [_u8(ped_com, 64 * n), fb, _u8(com_g, 64 * n), _u8(com_q, 64 * n), _u8(evals, 96 * n), _u8(proofs, 288 * n),
                  _u8(randomizers, 32 * n), _u8(pok_c, 32 * n), _u8(pok_s, 32 * CG_RANGE_N_RESP * n)]
        verdicts = np.zeros(max(n, 1), np.uint8)
        _check(lib().cg_range_verify_proofs_batch(vk._h, slot, *[_ptr(a) if a.size else None for a in arrays], n, _ptr(verdicts)))
        return verdicts[:n]

    @staticmethod
    def verify_range_proofs(vk: "RangeVerifyingKey", slot: int, ped_coms, proofs: List["RangeProof"], randomizers=None) -> List[bool]:
        """`ShowRange::verify` for n range proofs about the Pedersen commitments ped_coms whose bases are registered as
        `slot`, in ONE call: both transcripts and the comparison of the DLEQ's challenge run on the GPU
        (cg_range_verify_proofs_batch).  randomizers: per proof (r_1, r_2) below 2^128; None draws them with `secrets`.
        True exactly where `verify_n_bits` returns true."""
        n = len(proofs)
        if len(ped_coms) != n:
            raise ValueError("one Pedersen commitment per proof")
        if n == 0:
            return []
        if randomizers is None:
            import secrets
            randomizers = [(secrets.randbits(128), secrets.randbits(128)) for _ in range(n)]
        fr = lambda v: int(v).to_bytes(32, "little")
        join = lambda f: _u8(b"".join(f(p) for p in proofs))
        verdicts = Groth16.range_verify_proofs_batch_packed(
            vk, slot, _u8(b"".join(bytes(y) for y in ped_coms)), join(lambda p: bytes(p.com_f)), join(lambda p: bytes(p.com_g)),
            join(lambda p: bytes(p.com_q)), join(lambda p: fr(p.eval_g) + fr(p.eval_gw) + fr(p.eval_w_hat)),
            join(lambda p: bytes(p.proof_g) + bytes(p.proof_gw) + bytes(p.proof_w_hat)),
            _u8(b"".join(int(r).to_bytes(16, "little") for row in randomizers for r in row)), join(lambda p: fr(p.dleq_c)),
            join(lambda p: b"".join(fr(x) for si in p.dleq_s for x in si)))
        return [bool(v == CG_VERIFY_ACCEPT) for v in verdicts]

    @staticmethod
    def verify_showings_batch_packed(pvk: "PreparedVerifyingKey", range_vk, io_types, revealed, rand_proofs, com_hidden, committed, pok_c,
                                     pok_s, links, shifts, ranges, context=None, context_len: Optional[int] = None, context_stride: int = 0):
        """cg_verify_showings_batch on flat byte arrays laid out as include/crescent_gpu.h states (n = rand_proofs / 256):
        the cryptographic checks of `verify_show` (creds/src/lib.rs:630-658, :832-890) in one call.  links: one
        (committed_index, slot) per range proof of a showing; shifts: n x n_ranges x 32 B; ranges: per link the tuple
        (com_f, com_g, com_q, evals, proofs, randomizers, pok_c, pok_s) of n rows each, as range_verify_proofs_batch_packed
        takes them.  context: as dlog_challenge_batch takes it.  range_vk may be None without links.  Returns (verdicts n,
        part_verdicts n x (1 + n_ranges): the Groth16 part, then the range parts)."""
        io = _u8(np.asarray(list(io_types), dtype=np.uint8))
        n_rev, n_hid, n_com = (int((io == t).sum()) for t in (CG_IO_REVEALED, CG_IO_HIDDEN, CG_IO_COMMITTED))
        pb = _u8(rand_proofs)
        if pb.size % 256:
            raise ValueError("rand_proofs must be n x 256 bytes")
        n = pb.size // 256
        links = list(links)
        if len(ranges) != len(links):
            raise ValueError("one set of range proof rows per link")
        n_ranges = len(links)
        rev, comh, comm = _u8(revealed, 32 * n_rev * n), _u8(com_hidden, 64 * n), _u8(committed, 64 * n_com * n)
        pc, ps = _u8(pok_c, 32 * n), _u8(pok_s, 32 * (2 * n_com + n_hid + 1) * n)
        sb = _u8(shifts, 32 * n_ranges * n)
        cb = _u8(context if context is not None else b"")
        if context_len is None:
            context_len = context_stride if context_stride else cb.size
        if cb.size < (context_stride * (n - 1) + context_len if context_stride and n else context_len):
            raise ValueError("context is shorter than its length and stride say")
        ptr = lambda a: _ptr(a) if a.size else None
        widths = (64, 64, 64, 96, 288, 32, 32, 32 * CG_RANGE_N_RESP)
        keep = [[_u8(a, w * n) for a, w in zip(rows, widths)] for rows in ranges]
        c_links = (_CgShowRangeLink * max(n_ranges, 1))(*[_CgShowRangeLink(int(ci), int(slot)) for ci, slot in links])
        c_rows = (_CgRangeRows * max(n_ranges, 1))(*[_CgRangeRows(*[ptr(a) for a in rows]) for rows in keep])
        verdicts, parts = np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 1 + n_ranges), np.uint8)
        _check(lib().cg_verify_showings_batch(pvk._h, None if range_vk is None else range_vk._h, ptr(io), io.size, ptr(cb), context_len,
                                              context_stride, ptr(rev), ptr(pb), ptr(comh), ptr(comm), ptr(pc), ptr(ps), n_ranges,
                                              c_links if n_ranges else None, ptr(sb), c_rows if n_ranges else None, n, _ptr(verdicts),
                                              _ptr(parts)))
        return verdicts[:n], parts[:n]

    @staticmethod
    def verify_showings_batch(pvk: "PreparedVerifyingKey", range_vk, io_types, shows, links, shifts, range_proofs, context,
                              randomizers=None) -> List[bool]:
        """The cryptographic checks of `verify_show` / `verify_show_mdl` (creds/src/lib.rs:630-658, :832-890) for n showings
        of one layout in one call: `ShowGroth16::verify`, per link ped_com = commited_inputs[committed_index] - t *
        gamma_abc_g1[pos] and `ShowRange::verify` about it, all on the GPU (cg_verify_showings_batch).  shows: a sequence of
        (ShowGroth16, revealed inputs); links: (committed_index, slot of range_vk) per range proof of a showing; shifts[i][j]:
        the public value t of showing i's link j (ints); range_proofs[i][j]: its RangeProof; context: bytes, or None as the
        reference's `None`; randomizers[i][j]: (r_1, r_2) below 2^128, None draws them with `secrets`.  True exactly
        where every check of the reference passes."""
        io = [int(t) for t in io_types]
        n, links = len(shows), list(links)
        if n == 0:
            return []
        n_rev, n_hid, n_com = io.count(CG_IO_REVEALED), io.count(CG_IO_HIDDEN), io.count(CG_IO_COMMITTED)
        shapes = [2] * n_com + [n_hid + 1]
        for sh, x in shows:
            if [len(si) for si in sh.pok_s] != shapes or len(sh.commited_inputs) != n_com or len(_inputs_array(x)) != 32 * n_rev:
                raise ValueError("a showing does not have the shape of io_types")
        if len(shifts) != n or len(range_proofs) != n or any(len(a) != len(links) or len(b) != len(links) for a, b in zip(shifts, range_proofs)):
            raise ValueError("one shift and one range proof per showing and link")
        if randomizers is None:
            import secrets
            randomizers = [[(secrets.randbits(128), secrets.randbits(128)) for _ in links] for _ in range(n)]
        fr = lambda v: int(v).to_bytes(32, "little")
        cat = lambda parts: _u8(b"".join(parts))
        ranges = []
        for j in range(len(links)):
            ps = [range_proofs[i][j] for i in range(n)]
            ranges.append((cat(bytes(p.com_f) for p in ps), cat(bytes(p.com_g) for p in ps), cat(bytes(p.com_q) for p in ps),
                           cat(fr(p.eval_g) + fr(p.eval_gw) + fr(p.eval_w_hat) for p in ps),
                           cat(bytes(p.proof_g) + bytes(p.proof_gw) + bytes(p.proof_w_hat) for p in ps),
                           cat(int(r).to_bytes(16, "little") for i in range(n) for r in randomizers[i][j]),
                           cat(fr(p.dleq_c) for p in ps), cat(b"".join(fr(x) for si in p.dleq_s for x in si) for p in ps)))
        verdicts, _ = Groth16.verify_showings_batch_packed(
            pvk, range_vk, io, cat(_inputs_array(x).tobytes() for _, x in shows), cat(sh.rand_proof for sh, _ in shows),
            cat(sh.com_hidden_inputs for sh, _ in shows), cat(b"".join(sh.commited_inputs) for sh, _ in shows),
            cat(fr(sh.pok_c) for sh, _ in shows), cat(b"".join(fr(s) for si in sh.pok_s for s in si) for sh, _ in shows), links,
            cat(fr(t) for row in shifts for t in row), ranges, context)
        return [bool(v == CG_VERIFY_ACCEPT) for v in verdicts]

    @staticmethod
    def create_showings_batch_packed(pvk: "PreparedVerifyingKey", range_key, io_types, proofs, inputs, rand, links, shifts, range_rand,
                                     context=None, context_len: Optional[int] = None, context_stride: int = 0):
        """cg_create_showings_batch on flat byte arrays laid out as include/crescent_gpu.h states (n = proofs / 256):
        `create_show_proof`'s curve arithmetic and transcripts (creds/src/lib.rs:364-373, :468-471, :505-509) in one call.
        proofs, inputs, rand: as show_commit_batch_packed takes them; links: one (committed_index, slot of range_key) per
        range proof of a showing; shifts: n x n_ranges x 32 B; range_rand: n x n_ranges x 18 x 32 B; context: as
        dlog_challenge_batch takes it.  range_key may be None without links.  Returns (rand_proofs n x 256, com_hidden n x
        64, committed n x n_committed x 64, pok_c n x 32, pok_s n x n_resp x 32, ranges: per link the tuple (com_f, com_g,
        com_q, evals, proofs, pok_c, pok_s, challenges) as range_prove_batch_packed returns them, status n, part_status n x
        (1 + n_ranges)) as uint8 arrays; a part that was not made has zero bytes in its rows."""
        io = _u8(np.asarray(list(io_types), dtype=np.uint8))
        n_com = int((io == CG_IO_COMMITTED).sum())
        pb = _u8(proofs)
        if pb.size % 256:
            raise ValueError("proofs must be n x 256 bytes")
        n = pb.size // 256
        links = list(links)
        n_ranges = len(links)
        n_rand = show_rand_count(io)
        n_resp = n_rand - 3 - n_com
        ib, rb = _u8(inputs, 32 * io.size * n), _u8(rand, 32 * n_rand * n)
        sb, rrb = _u8(shifts, 32 * n_ranges * n), _u8(range_rand, 32 * CG_RANGE_N_RAND * n_ranges * n)
        cb = _u8(context if context is not None else b"")
        if context_len is None:
            context_len = context_stride if context_stride else cb.size
        if cb.size < (context_stride * (n - 1) + context_len if context_stride and n else context_len):
            raise ValueError("context is shorter than its length and stride say")
        ptr = lambda a: _ptr(a) if a.size else None
        m = max(n, 1)
        rp, comh, comm = np.zeros((m, 256), np.uint8), np.zeros((m, 64), np.uint8), np.zeros((m, max(n_com, 1), 64), np.uint8)
        pok_c, pok_s = np.zeros((m, 32), np.uint8), np.zeros((m, n_resp, 32), np.uint8)
        status, parts = np.zeros(m, np.uint8), np.zeros((m, 1 + n_ranges), np.uint8)
        shapes = ((64,), (64,), (64,), (3, 32), (3, 96), (32,), (CG_RANGE_N_RESP, 32), (3, 32))
        made = [[np.zeros((m,) + sh, np.uint8) for sh in shapes] for _ in links]
        c_links = (_CgShowRangeLink * max(n_ranges, 1))(*[_CgShowRangeLink(int(ci), int(slot)) for ci, slot in links])
        c_made = (_CgRangeMade * max(n_ranges, 1))(*[_CgRangeMade(*[_ptr(a) for a in rows]) for rows in made])
        _check(lib().cg_create_showings_batch(pvk._h, None if range_key is None else range_key._h, ptr(io), io.size, ptr(cb), context_len,
                                              context_stride, ptr(pb), ptr(ib), ptr(rb), n_ranges, c_links if n_ranges else None, ptr(sb),
                                              ptr(rrb), n, _ptr(rp), _ptr(comh), _ptr(comm), _ptr(pok_c), _ptr(pok_s),
                                              c_made if n_ranges else None, _ptr(status), _ptr(parts)))
        return (rp[:n], comh[:n], comm[:n, :n_com], pok_c[:n], pok_s[:n], [tuple(a[:n] for a in rows) for rows in made], status[:n],
                parts[:n])

    @staticmethod
    def create_showings_batch(pvk: "PreparedVerifyingKey", range_key, io_types, states, links, shifts, rand=None, range_rand=None,
                              context=None):
        """`create_show_proof` / `create_show_proof_mdl`'s `show_groth16` and `show_range` steps (creds/src/lib.rs:364-373,
        :468-471, :505-509) for n client states of one layout in one call (cg_create_showings_batch), the transcripts the
        library's Merlin on the GPU.  states: a sequence of (proof bytes or Proof, inputs); links: (committed_index, slot of
        range_key) per range proof of a showing; shifts[i][j]: the public value t of state i's link j (ints); rand: per
        state its show_rand_count scalars in the header's order and range_rand[i][j]: the 18 scalars of link j (ints) -
        None draws either with `secrets.randbelow` (r1, r2 non-zero), but a host that keeps the openings (the r_i and z) draws
        them itself and passes them in; context: bytes, or None as the reference's `None`.  Returns per state
        (ShowGroth16, [RangeProof per link]), or None for a state any part of which was not made."""
        io = [int(t) for t in io_types]
        n, links = len(states), list(links)
        if n == 0:
            return []
        if len(shifts) != n or any(len(row) != len(links) for row in shifts):
            raise ValueError("one shift per state and link")
        import secrets
        if rand is None:
            n_rand = show_rand_count(io)
            rand = [[1 + secrets.randbelow(FR_MODULUS - 1) for _ in range(2)] + [secrets.randbelow(FR_MODULUS) for _ in range(n_rand - 2)]
                    for _ in range(n)]
        if range_rand is None:
            range_rand = [[[secrets.randbelow(FR_MODULUS) for _ in range(CG_RANGE_N_RAND)] for _ in links] for _ in range(n)]
        n_com, n_hid = io.count(CG_IO_COMMITTED), io.count(CG_IO_HIDDEN)
        fr = lambda v: int(v).to_bytes(32, "little")
        rp, comh, comm, pok_c, s, ranges, status, _ = Groth16.create_showings_batch_packed(
            pvk, range_key, io, b"".join(p.data if isinstance(p, Proof) else bytes(p) for p, _ in states),
            np.concatenate([_inputs_array(x) for _, x in states]), _u8(b"".join(fr(v) for row in rand for v in row)), links,
            _u8(b"".join(fr(t) for row in shifts for t in row)), _u8(b"".join(fr(v) for row in range_rand for link in row for v in link)), context)
        val = lambda a: int.from_bytes(a.tobytes(), "little")
        out = []
        for i in range(n):
            if status[i] != CG_SHOW_MADE:
                out.append(None)
                continue
            flat = [val(s[i, j]) for j in range(s.shape[1])]
            pok_s = [flat[2 * j:2 * j + 2] for j in range(n_com)] + [flat[2 * n_com:]]
            assert len(pok_s[-1]) == n_hid + 1
            show = ShowGroth16(rp[i].tobytes(), comh[i].tobytes(), val(pok_c[i]), pok_s, [comm[i, j].tobytes() for j in range(n_com)])
            proofs = [RangeProof(com_f[i].tobytes(), com_g[i].tobytes(), val(evals[i, 0]), pr[i, 0].tobytes(), val(evals[i, 1]), pr[i, 1].tobytes(),
                                 com_q[i].tobytes(), val(evals[i, 2]), pr[i, 2].tobytes(), val(rc[i]),
                                 [[val(rs[i, j]) for j in range(2)], [val(rs[i, j]) for j in range(2, 6)]])
                      for com_f, com_g, com_q, evals, pr, rc, rs, _ in ranges]
            out.append((show, proofs))
        return out

    @staticmethod
    def show_shift_batch(pvk: "PreparedVerifyingKey", input_index: int, openings, commitments, shifts):
        """cg_show_shift_batch: the creating side's link `com.m -= t; com.c -= bases[0] * t` (creds/src/lib.rs:370-372,
        :468-470, :505-507) for n openings of the committed input `input_index` (an index into io_types).  openings: n x 64
        B (m, r) or a sequence of (m, r) ints; commitments: n x 64 B or a sequence of 64-byte points; shifts: n x 32 B or a
        sequence of ints.  Returns (openings_out n x 2 x 32, ped_com n x 64, status n) as uint8 arrays, in the layouts
        range_prove_batch_packed takes; a CG_SHOW_MALFORMED row is zero bytes."""
        fr = lambda v: int(v).to_bytes(32, "little")
        if isinstance(openings, (list, tuple)):
            openings = b"".join(fr(m) + fr(r) for m, r in openings)
        if isinstance(commitments, (list, tuple)):
            commitments = b"".join(bytes(c) for c in commitments)
        if isinstance(shifts, (list, tuple)):
            shifts = b"".join(fr(t) for t in shifts)
        ob = _u8(openings)
        if ob.size % 64:
            raise ValueError("openings must be n x 64 bytes (m, r)")
        n = ob.size // 64
        cb, sb = _u8(commitments, 64 * n), _u8(shifts, 32 * n)
        ptr = lambda a: _ptr(a) if a.size else None
        m = max(n, 1)
        out, ped, status = np.zeros((m, 2, 32), np.uint8), np.zeros((m, 64), np.uint8), np.zeros(m, np.uint8)
        _check(lib().cg_show_shift_batch(pvk._h, int(input_index), ptr(ob), ptr(cb), ptr(sb), n, _ptr(out), _ptr(ped), _ptr(status)))
        return out[:n], ped[:n], status[:n]

    @staticmethod
    def dlog_challenge_batch(n_bases, bases, k, y_head, y_last, context=None, context_len: Optional[int] = None,
                             context_stride: int = 0) -> np.ndarray:
        """cg_dlog_challenge_batch (host only, no GPU needed): `DLogPoK`'s Merlin transcript (creds/src/dlog.rs:56-99) for n
        showings of one shape.  n_bases: the number of bases per statement; bases: their 64-byte uncompressed points,
        statement by statement, shared by the batch; k: n x n_statements x 32 compressed (the k_bytes the commit and
        verify calls return); y_head: n x (n_statements - 1) x 64 uncompressed, or None with one statement; y_last: n x 64.
        context: bytes or None (`None` and b"" are the same transcript), one for the batch; with context_stride > 0 it
        holds one context of context_len bytes (default: the stride) per showing, context_stride bytes apart.  Returns
        the n x 32 challenge bytes (canonical scalars)."""
        nb = np.ascontiguousarray(np.asarray(list(n_bases), dtype=np.uint32))
        yl = _u8(y_last)
        if yl.size % 64:
            raise ValueError("y_last must be n x 64 bytes")
        n = yl.size // 64
        bb, kb = _u8(bases, 64 * int(nb.sum())), _u8(k, 32 * nb.size * n)
        yh = None if y_head is None or nb.size <= 1 else _u8(y_head, 64 * (nb.size - 1) * n)
        cb = _u8(context if context is not None else b"")
        if context_len is None:
            context_len = context_stride if context_stride else cb.size
        if cb.size < (context_stride * (n - 1) + context_len if context_stride and n else context_len):
            raise ValueError("context is shorter than its length and stride say")
        ptr = lambda a: _ptr(a) if a is not None and a.size else None
        out = np.zeros((max(n, 1), 32), np.uint8)
        _check(lib().cg_dlog_challenge_batch(ptr(cb), context_len, context_stride, nb.size, nb.ctypes.data_as(C.POINTER(C.c_uint32)), ptr(bb),
                                             ptr(kb), ptr(yh), ptr(yl), n, _ptr(out)))
        return out[:n]

    @staticmethod
    def show_dlog_challenges(pvk: "PreparedVerifyingKey", io_types, k, committed, com_hidden, context=None) -> np.ndarray:
        """the DLogPoK challenge of n showings under pvk and one io_types layout, by the library's Merlin
        (cg_dlog_challenge_batch): per committed input the statement (gamma_abc_g1[i + 1], delta_g1), then the hidden
        inputs' gamma_abc_g1[j + 1] ..., delta_g1 (creds/src/groth16rand.rs:133-174, :246-300).  k, committed, com_hidden:
        as show_commit_batch_packed and verify_show_batch return them.  Returns n x 32 bytes."""
        io = [int(t) for t in io_types]
        com = [i for i, t in enumerate(io) if t == CG_IO_COMMITTED]
        hid = [j for j, t in enumerate(io) if t == CG_IO_HIDDEN]
        abc, delta = pvk.gamma_abc_g1, pvk.delta_g1
        bases = [b for i in com for b in (abc[i + 1], delta)] + [abc[j + 1] for j in hid] + [delta]
        return Groth16.dlog_challenge_batch([2] * len(com) + [len(hid) + 1], np.concatenate(bases), k, committed if com else None,
                                            com_hidden, context)

    @staticmethod
    def device_link_verify_batch_packed(pvk: "PreparedVerifyingKey", io_types, pos0: int, pos1: int, committed, com1, comz, h_q, m, pi0_c,
                                        pi0_s, pi1_c, pi1_s, h_len: Optional[int] = None):
        """cg_device_link_verify_batch on flat byte arrays laid out as include/crescent_gpu.h states (n = com1 / 64): the
        BN254 half of `DeviceProof::verify` (creds/src/device.rs:168-213) for n device-bound showings of one layout.
        committed is the showing's own n x n_committed x 64 array, as verify_showings_batch_packed takes it; pos0 and pos1 are
        the input indices of the two device key values.  h_len defaults to len(h_q) / n.  Returns (verdicts n, part_verdicts
        n x 2 for (pi0, pi1), e_out n x 32: the digest e1_bytes ‖ e2_bytes, zeros on a malformed row)."""
        io = _u8(np.asarray(list(io_types), dtype=np.uint8))
        n_com = int((io == CG_IO_COMMITTED).sum())
        c1 = _u8(com1)
        if c1.size % 64:
            raise ValueError("com1 must be n x 64 bytes")
        n = c1.size // 64
        hq = _u8(h_q if h_q is not None else b"")
        if h_len is None:
            h_len = hq.size // n if n else 0
        comm, cz, hq = _u8(committed, 64 * n_com * n), _u8(comz, 64 * n), _u8(hq, h_len * n)
        arrays = [c1, cz, hq, _u8(m, 32 * n), _u8(pi0_c, 32 * n), _u8(pi0_s, 128 * n), _u8(pi1_c, 32 * n), _u8(pi1_s, 96 * n)]
        ptr = lambda a: _ptr(a) if a.size else None
        rows = _CgDeviceLinkRows(*[ptr(a) for a in arrays])
        verdicts, parts, e_out = np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 2), np.uint8), np.zeros((max(n, 1), 32), np.uint8)
        _check(lib().cg_device_link_verify_batch(pvk._h, ptr(io), io.size, int(pos0), int(pos1), ptr(comm), C.byref(rows), int(h_len), n,
                                                 _ptr(verdicts), _ptr(parts), _ptr(e_out)))
        return verdicts[:n], parts[:n], e_out[:n]

    @staticmethod
    def device_link_verify_batch(pvk: "PreparedVerifyingKey", io_types, pos0: int, pos1: int, committed, proofs) -> List[bool]:
        """The BN254 half of `DeviceProof::verify` for a sequence of DeviceLinkProof, one per showing; committed: per showing
        the sequence of its 64-byte committed points.  True where pi0 (with its equal-scalar pair) and pi1 verify: the
        reference's `true` short of pi2.  Every h_Q must have the same length."""
        proofs = list(proofs)
        fr = lambda v: int(v).to_bytes(32, "little")
        join = lambda f: b"".join(f(p) for p in proofs)
        verdicts, _, _ = Groth16.device_link_verify_batch_packed(
            pvk, io_types, pos0, pos1, b"".join(bytes(c) for row in committed for c in row), join(lambda p: bytes(p.com1)),
            join(lambda p: bytes(p.comz)), join(lambda p: bytes(p.h_q)), join(lambda p: fr(p.m)), join(lambda p: fr(p.pi0_c)),
            join(lambda p: b"".join(fr(x) for si in p.pi0_s for x in si)), join(lambda p: fr(p.pi1_c)),
            join(lambda p: b"".join(fr(x) for si in p.pi1_s for x in si)), h_len=len(proofs[0].h_q) if proofs else 0)
        return [bool(v == CG_VERIFY_ACCEPT) for v in verdicts]

    @staticmethod
    def device_link_prove_batch_packed(pvk: "PreparedVerifyingKey", io_types, pos0: int, pos1: int, committed, openings, rand, h_q,
                                       h_len: Optional[int] = None):
        """cg_device_link_prove_batch on flat byte arrays laid out as include/crescent_gpu.h states (n = openings / 128): the
        BN254 half of `DeviceProof::prove` (creds/src/device.rs:104-160) for n device-bound showings of one layout.
        committed is the showing's own n x n_committed x 64 array, as create_showings_batch_packed returns it; openings: n x
        (q0, r0, q1, r1_orig); rand: n x 9 scalars (z, t_z, r1, a, b, d, n0, n1, n2); h_len defaults to len(h_q) / n.
        Returns (com1 n x 64, comz n x 64, m n x 32, pi0_c n x 32, pi0_s n x 4 x 32, pi1_c n x 32, pi1_s n x 3 x 32, e_out n x
        32: the digest e1_bytes ‖ e2_bytes, status n) as uint8 arrays; a CG_SHOW_MALFORMED row is zero bytes throughout."""
        io = _u8(np.asarray(list(io_types), dtype=np.uint8))
        n_com = int((io == CG_IO_COMMITTED).sum())
        ob = _u8(openings)
        if ob.size % 128:
            raise ValueError("openings must be n x 128 bytes (q0, r0, q1, r1_orig)")
        n = ob.size // 128
        hq = _u8(h_q if h_q is not None else b"")
        if h_len is None:
            h_len = hq.size // n if n else 0
        comm, rb, hq = _u8(committed, 64 * n_com * n), _u8(rand, 32 * CG_DEVICE_LINK_N_RAND * n), _u8(hq, h_len * n)
        ptr = lambda a: _ptr(a) if a.size else None
        m = max(n, 1)
        rows = [np.zeros((m,) + sh, np.uint8) for sh in ((64,), (64,), (32,), (32,), (4, 32), (32,), (3, 32))]
        e_out, status = np.zeros((m, 32), np.uint8), np.zeros(m, np.uint8)
        made = _CgDeviceLinkMade(*[_ptr(a) for a in rows])
        _check(lib().cg_device_link_prove_batch(pvk._h, ptr(io), io.size, int(pos0), int(pos1), ptr(comm), ptr(ob), ptr(rb), ptr(hq),
                                                int(h_len), n, C.byref(made), _ptr(e_out), _ptr(status)))
        return tuple(a[:n] for a in rows) + (e_out[:n], status[:n])

    @staticmethod
    def device_link_prove_batch(pvk: "PreparedVerifyingKey", io_types, pos0: int, pos1: int, committed, openings, h_qs, rand=None):
        """The BN254 half of `DeviceProof::prove` for n showings: committed: per showing the sequence of its 64-byte committed
        points; openings: per showing (q0, r0, q1, r1_orig) ints; h_qs: per showing the bytes `compute_hQ` returned, all of
        one length; rand: per showing the nine scalars in the header's order - None draws them with `secrets.randbelow`, but
        a host that goes on to `ECDSAProof::prove` needs its z and draws them itself.  Returns (proofs, digests): per showing
        a DeviceLinkProof, which device_link_verify_batch takes as it is, or None for a showing that was not made; and the n x
        32 digests e1_bytes ‖ e2_bytes (zeros for such a showing)."""
        openings, h_qs = list(openings), [bytes(h) for h in h_qs]
        n = len(openings)
        if n == 0:
            return [], np.zeros((0, 32), np.uint8)
        if rand is None:
            import secrets
            rand = [[secrets.randbelow(FR_MODULUS) for _ in range(CG_DEVICE_LINK_N_RAND)] for _ in range(n)]
        fr = lambda v: int(v).to_bytes(32, "little")
        com1, comz, m, c0, s0, c1, s1, e, status = Groth16.device_link_prove_batch_packed(
            pvk, io_types, pos0, pos1, b"".join(bytes(c) for row in committed for c in row), b"".join(fr(v) for row in openings for v in row),
            b"".join(fr(v) for row in rand for v in row), b"".join(h_qs), h_len=len(h_qs[0]))
        val = lambda a: int.from_bytes(a.tobytes(), "little")
        out = []
        for i in range(n):
            if status[i] != CG_SHOW_MADE:
                out.append(None)
                continue
            out.append(DeviceLinkProof(com1[i].tobytes(), comz[i].tobytes(), h_qs[i], val(m[i]), val(c0[i]),
                                       [[val(s0[i, 0]), val(s0[i, 1])], [val(s0[i, 2]), val(s0[i, 3])]], val(c1[i]),
                                       [[val(s1[i, 0])], [val(s1[i, 1]), val(s1[i, 2])]]))
        return out, e

    @staticmethod
    def poseidon_p256_permute_batch_packed(pvk: "PreparedVerifyingKey", states):
        """cg_poseidon_p256_permute_batch: Poseidon of width 3 over P-256's base field on n states of 3 x 32 bytes, canonical
        little-endian.  Returns (out n x 3 x 32, status n); a row with an element >= p is CG_SHOW_MALFORMED and zero."""
        sb = _u8(states)
        if sb.size % 96:
            raise ValueError("states must be n x 3 x 32 bytes")
        n = sb.size // 96
        out, status = np.zeros((max(n, 1), 3, 32), np.uint8), np.zeros(max(n, 1), np.uint8)
        _check(lib().cg_poseidon_p256_permute_batch(pvk._h, _ptr(sb) if n else None, n, _ptr(out), _ptr(status)))
        return out[:n], status[:n]

    @staticmethod
    def hq_batch_packed(pvk: "PreparedVerifyingKey", q):
        """cg_hq_batch: `compute_hQ` (ecdsa-pop/src/lib.rs:308-320) for n rows of (q0, q1, z), 3 x 32 bytes canonical Fr.
        Returns (h_q n x 32, big-endian as device_link_prove_batch_packed takes them, status n); a row with a scalar >= r is
        CG_SHOW_MALFORMED and zero."""
        qb = _u8(q)
        if qb.size % 96:
            raise ValueError("q must be n x 3 x 32 bytes (q0, q1, z)")
        n = qb.size // 96
        out, status = np.zeros((max(n, 1), 32), np.uint8), np.zeros(max(n, 1), np.uint8)
        _check(lib().cg_hq_batch(pvk._h, _ptr(qb) if n else None, n, _ptr(out), _ptr(status)))
        return out[:n], status[:n]

    @staticmethod
    def device_link_prove_hq_batch_packed(pvk: "PreparedVerifyingKey", io_types, pos0: int, pos1: int, committed, openings, rand):
        """cg_device_link_prove_hq_batch: device_link_prove_batch_packed with h_Q computed on the GPU in the same call, from q0
        and q1 (openings) and z (rand[0]).  Returns that call's nine arrays and h_q n x 32 as a tenth."""
        io = _u8(np.asarray(list(io_types), dtype=np.uint8))
        n_com = int((io == CG_IO_COMMITTED).sum())
        ob = _u8(openings)
        if ob.size % 128:
            raise ValueError("openings must be n x 128 bytes (q0, r0, q1, r1_orig)")
        n = ob.size // 128
        comm, rb = _u8(committed, 64 * n_com * n), _u8(rand, 32 * CG_DEVICE_LINK_N_RAND * n)
        ptr = lambda a: _ptr(a) if a.size else None
        m = max(n, 1)
        rows = [np.zeros((m,) + sh, np.uint8) for sh in ((64,), (64,), (32,), (32,), (4, 32), (32,), (3, 32))]
        e_out, status, h_q = np.zeros((m, 32), np.uint8), np.zeros(m, np.uint8), np.zeros((m, 32), np.uint8)
        made = _CgDeviceLinkMade(*[_ptr(a) for a in rows])
        _check(lib().cg_device_link_prove_hq_batch(pvk._h, ptr(io), io.size, int(pos0), int(pos1), ptr(comm), ptr(ob), ptr(rb), n, C.byref(made),
                                                   _ptr(e_out), _ptr(status), _ptr(h_q)))
        return tuple(a[:n] for a in rows) + (e_out[:n], status[:n], h_q[:n])

    @staticmethod
    def device_link_prove_hq_batch(pvk: "PreparedVerifyingKey", io_types, pos0: int, pos1: int, committed, openings, rand=None):
        """device_link_prove_batch without h_qs: each DeviceLinkProof carries the h_Q the GPU computed for it.  A host that
        goes on to `ECDSAProof::prove` needs z = rand[i][0] and draws rand itself."""
        openings = list(openings)
        n = len(openings)
        if n == 0:
            return [], np.zeros((0, 32), np.uint8)
        if rand is None:
            import secrets
            rand = [[secrets.randbelow(FR_MODULUS) for _ in range(CG_DEVICE_LINK_N_RAND)] for _ in range(n)]
        fr = lambda v: int(v).to_bytes(32, "little")
        com1, comz, m, c0, s0, c1, s1, e, status, h_q = Groth16.device_link_prove_hq_batch_packed(
            pvk, io_types, pos0, pos1, b"".join(bytes(c) for row in committed for c in row), b"".join(fr(v) for row in openings for v in row),
            b"".join(fr(v) for row in rand for v in row))
        val = lambda a: int.from_bytes(a.tobytes(), "little")
        out = []
        for i in range(n):
            if status[i] != CG_SHOW_MADE:
                out.append(None)
                continue
            out.append(DeviceLinkProof(com1[i].tobytes(), comz[i].tobytes(), h_q[i].tobytes(), val(m[i]), val(c0[i]),
                                       [[val(s0[i, 0]), val(s0[i, 1])], [val(s0[i, 2]), val(s0[i, 3])]], val(c1[i]),
                                       [[val(s1[i, 0])], [val(s1[i, 1]), val(s1[i, 2])]]))
        return out, e

    @staticmethod
    def p256_tu_batch(pvk: "PreparedVerifyingKey", r_xy, digest):
        """cg_p256_tu_batch: `compute_TU` (ecdsa-pop/src/lib.rs:217-240) for n rows: r_xy n x 64 B (R as x ‖ y) and digest
        n x 32 B, every quantity 32 bytes big-endian.  Returns (t_xy n x 64, u_xy n x 64, status n); a row whose R has a
        coordinate >= p, is off the curve or has R.x = 0 mod n is CG_SHOW_MALFORMED and zero; the identity is 64 zero bytes."""
        rb, db = _u8(r_xy), _u8(digest)
        if rb.size % 64 or db.size * 2 != rb.size:
            raise ValueError("r_xy must be n x 64 bytes and digest n x 32")
        n = rb.size // 64
        t, u, status = np.zeros((max(n, 1), 64), np.uint8), np.zeros((max(n, 1), 64), np.uint8), np.zeros(max(n, 1), np.uint8)
        _check(lib().cg_p256_tu_batch(pvk._h, _ptr(rb) if n else None, _ptr(db) if n else None, n, _ptr(t), _ptr(u), _ptr(status)))
        return t[:n], u[:n], status[:n]

    @staticmethod
    def p256_rtu_batch(pvk: "PreparedVerifyingKey", q_xy, sig, digest):
        """cg_p256_rtu_batch: `compute_RTU` (ecdsa-pop/src/lib.rs:180-215) for n rows: q_xy n x 64 B (the device's public key),
        sig n x 64 B (r ‖ s), digest n x 32 B.  Returns (r_xy, t_xy, u_xy, each n x 64, status n): CG_SHOW_MADE,
        CG_SHOW_MALFORMED (Q not a canonical point of the curve, r or s outside [1, n - 1]) or CG_P256_BAD_SIGNATURE, every
        output of a row that is not made being zero."""
        qb, sb, db = _u8(q_xy), _u8(sig), _u8(digest)
        if qb.size % 64 or sb.size != qb.size or db.size * 2 != qb.size:
            raise ValueError("q_xy and sig must be n x 64 bytes and digest n x 32")
        n = qb.size // 64
        r, t, u = (np.zeros((max(n, 1), 64), np.uint8) for _ in range(3))
        status = np.zeros(max(n, 1), np.uint8)
        ptr = lambda a: _ptr(a) if n else None
        _check(lib().cg_p256_rtu_batch(pvk._h, ptr(qb), ptr(sb), ptr(db), n, _ptr(r), _ptr(t), _ptr(u), _ptr(status)))
        return r[:n], t[:n], u[:n], status[:n]

    @staticmethod
    def p256_tu(pvk: "PreparedVerifyingKey", rows):
        """p256_tu_batch on Python integers: rows of ((R.x, R.y), digest), the digest an integer below 2^256.  Returns per row
        (T, U), a point being (x, y) and the identity None, or None for a malformed row."""
        rows = list(rows)
        if not rows:
            return []
        be = lambda v: int(v).to_bytes(32, "big")
        t, u, status = Groth16.p256_tu_batch(pvk, b"".join(be(R[0]) + be(R[1]) for R, _ in rows), b"".join(be(d) for _, d in rows))
        return [(_p256_point(t[i]), _p256_point(u[i])) if status[i] == CG_SHOW_MADE else None for i in range(len(rows))]

    @staticmethod
    def p256_rtu(pvk: "PreparedVerifyingKey", rows):
        """p256_rtu_batch on Python integers: rows of ((Q.x, Q.y), r, s, digest).  Returns per row (status, (R, T, U)), the
        points as p256_tu returns them and the triple None unless the status is CG_SHOW_MADE."""
        rows = list(rows)
        if not rows:
            return []
        be = lambda v: int(v).to_bytes(32, "big")
        r, t, u, status = Groth16.p256_rtu_batch(pvk, b"".join(be(Q[0]) + be(Q[1]) for Q, _, _, _ in rows),
                                                 b"".join(be(r_) + be(s_) for _, r_, s_, _ in rows), b"".join(be(d) for _, _, _, d in rows))
        return [(int(status[i]), (_p256_point(r[i]), _p256_point(t[i]), _p256_point(u[i])) if status[i] == CG_SHOW_MADE else None)
                for i in range(len(rows))]

    @staticmethod
    def device_link_openings(io_types, pos0: int, pos1: int, inputs, rand) -> np.ndarray:
        """The openings (q0, r0, q1, r1_orig) of the two device key values, cut out of the arrays create_showings_batch_packed
        took: per showing m = inputs[pos] and r = rand[2 + committed_index] (`committed_input_openings` of
        groth16rand.rs:135-139).  inputs: n x n_io x 32 B; rand: n x show_rand_count x 32 B.  Returns n x 4 x 32 bytes, the
        layout device_link_prove_batch_packed takes."""
        io = [int(t) for t in io_types]
        com = [i for i, t in enumerate(io) if t == CG_IO_COMMITTED]
        if pos0 not in com or pos1 not in com:
            raise ValueError("pos0 and pos1 must be committed inputs")
        n_rand = show_rand_count(io)
        ib = _u8(inputs)
        if not io or ib.size % (32 * len(io)):
            raise ValueError("inputs must be n x n_io x 32 bytes")
        n = ib.size // (32 * len(io))
        ib, rb = ib.reshape(n, len(io), 32), _u8(rand, 32 * n_rand * n).reshape(n, n_rand, 32)
        return np.stack([ib[:, pos0], rb[:, 2 + com.index(pos0)], ib[:, pos1], rb[:, 2 + com.index(pos1)]], axis=1).copy()

    @staticmethod
    def revealed_digest_batch(items) -> np.ndarray:
        """cg_revealed_digest_batch (host only, no GPU needed): per item SHA-256 and the digest's first 31 bytes through
        `bits_to_num` (creds/src/lib.rs:590-603, utils.rs:78-94), the canonical Fr a host places into `revealed`.  items: a
        sequence of bytes.  Returns n x 32 bytes."""
        items = [bytes(b) for b in items]
        offsets = np.zeros(len(items) + 1, np.uint64)
        offsets[1:] = np.cumsum([len(b) for b in items], dtype=np.uint64)
        data = _u8(b"".join(items))
        out = np.zeros((max(len(items), 1), 32), np.uint8)
        _check(lib().cg_revealed_digest_batch(_ptr(data) if data.size else None, offsets.ctypes.data_as(C.POINTER(C.c_uint64)), len(items),
                                              _ptr(out)))
        return out[:len(items)]

    @classmethod
    def clear_cache(cls):
        cls._cache.clear()


@dataclass
class DeviceLinkProof:
    """The BN254 half of a `DeviceProof` (creds/src/device.rs:80-93) as its serialized pieces: com1 and comz 64 B
    ark-serialize uncompressed G1, h_Q bytes, m an int, and the two DLogPoK as c and the responses s[statement][j] ints
    (pi0: [[s00, s01], [s10, s11]], pi1: [[t0], [u0, u1]])."""
    com1: bytes
    comz: bytes
    h_q: bytes
    m: int
    pi0_c: int
    pi0_s: List[List[int]]
    pi1_c: int
    pi1_s: List[List[int]]


class PreparedVerifyingKey(_LatencyMode, _Handle):
    """forks/groth16/src/data_structures.rs:62-71, parsed from its serialized bytes (`deserialize_uncompressed_unchecked`,
    creds/src/utils.rs:186) and resident on a GPU (cg_pvk_load): alpha_g1_beta_g2, the prepared gamma / delta lines and
    fixed-base tables of gamma_abc_g1.  latency=True switches the handle to the one-workgroup-per-proof arrangement
    (set_latency).  Use as a context manager or close()."""
    _free, _set_latency_mode = "cg_pvk_free", "cg_pvk_set_latency_mode"

    def __init__(self, pvk_bytes, device: int = -1, latency: bool = False):
        b = _u8(pvk_bytes)
        self._h = C.c_void_p()
        _check(lib().cg_pvk_load(C.byref(self._h), _ptr(b) if b.size else None, b.size, device))
        # the bases of a showing's DLogPoK as its transcript absorbs them (Groth16.show_dlog_challenges): the key starts with
        # its VerifyingKey: alpha_g1 | beta_g2 | gamma_g2 | delta_g1 | delta_g2 | u64 count | gamma_abc_g1
        n_abc = int.from_bytes(b[512:520].tobytes(), "little")
        self.delta_g1 = b[320:384].copy()
        self.gamma_abc_g1 = b[520:520 + 64 * n_abc].reshape(n_abc, 64).copy()
        if latency:
            self.set_latency(True)

    def set_showings_overlap(self, on: bool) -> None:
        """cg_pvk_set_showings_overlap: whether verify_showings_batch and create_showings_batch start the range half beside
        the Groth16 half (the default) or behind it; the bytes are the same"""
        _check(lib().cg_pvk_set_showings_overlap(self._h, 1 if on else 0))

    def last_kernel_ms(self) -> Tuple[float, float]:
        """HIP-event milliseconds of the last verifying call on this key: (group stage, pairing)"""
        a, b = C.c_float(), C.c_float()
        _check(lib().cg_pvk_last_kernel_ms(self._h, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def device_link_last_kernel_ms(self) -> Tuple[float, float, float, float]:
        """HIP-event milliseconds of the four kernels of the last device_link_verify_batch on this key: the digest and
        scalar stage, the terms, the sums, the two transcripts"""
        ms = (C.c_float * 4)()
        _check(lib().cg_device_link_last_kernel_ms(self._h, ms))
        return tuple(float(x) for x in ms)

    def device_link_prove_last_kernel_ms(self) -> Tuple[float, ...]:
        """HIP-event milliseconds of the six kernels of the last device_link_prove_batch on this key: the checks, the walks,
        the sums, pi0 with the digest, lhs1, pi1"""
        ms = (C.c_float * 6)()
        _check(lib().cg_device_link_prove_last_kernel_ms(self._h, ms))
        return tuple(float(x) for x in ms)

    def hq_last_kernel_ms(self) -> Tuple[float, float, int]:
        """cg_hq_last_kernel_ms: HIP-event milliseconds of the kernel of the last hq_batch or permute call on this key and of
        the h_Q kernel of its last device_link_prove_hq_batch, and how often the Poseidon constants were uploaded (0 or 1)"""
        ms, up = (C.c_float * 2)(), C.c_uint32()
        _check(lib().cg_hq_last_kernel_ms(self._h, ms, C.byref(up)))
        return float(ms[0]), float(ms[1]), int(up.value)

    def p256_last_kernel_ms(self) -> Tuple[float, float, float, int]:
        """cg_p256_last_kernel_ms: HIP-event milliseconds of the three kernels of the last p256_tu_batch or p256_rtu_batch on
        this key - the scalar stage, the terms, the finishing stage - and how often the table of P-256's generator was
        uploaded (0 or 1)"""
        ms, up = (C.c_float * 3)(), C.c_uint32()
        _check(lib().cg_p256_last_kernel_ms(self._h, ms, C.byref(up)))
        return float(ms[0]), float(ms[1]), float(ms[2]), int(up.value)

    @property
    def num_inputs(self) -> int:
        """gamma_abc_g1.len() - 1"""
        n = C.c_uint64()
        _check(lib().cg_pvk_num_inputs(self._h, C.byref(n)))
        return int(n.value)


class RangeProofKey(_RangeSlots, _Handle):
    """`RangeProofPK` (creds/src/rangeproof.rs:26-29) from the bytes of range_pk.bin (creds/src/lib.rs:241), resident on a
    GPU as fixed-base tables for proofs of n_bits bits (cg_range_pk_load).  Use as a context manager or close()."""
    _free, _add_bases, _last_kernel_ms = "cg_range_pk_free", "cg_range_pk_add_bases", "cg_range_pk_last_kernel_ms"

    def __init__(self, range_pk_bytes, n_bits: int, device: int = -1):
        b = _u8(range_pk_bytes)
        self.n_bits = int(n_bits)
        self._h = C.c_void_p()
        _check(lib().cg_range_pk_load(C.byref(self._h), _ptr(b) if b.size else None, b.size, self.n_bits, device))


def _g1_compress(unc) -> np.ndarray:
    """ark-serialize's compressed form of an uncompressed G1 point: x with the SWFlags - a flag bit and no arithmetic
    (the transcripts absorb commitments compressed, creds/src/utils.rs:29-37)"""
    b = bytes(unc)
    if len(b) != 64:
        raise ValueError("an uncompressed G1 point is 64 bytes")
    out = bytearray(b[:32])
    if b[63] & 0x40:
        out[31] |= 0x40
    else:
        y = int.from_bytes(b[32:63] + bytes([b[63] & 0x3F]), "little")
        if y > FQ_MODULUS - y:
            out[31] |= 0x80
    return np.frombuffer(bytes(out), np.uint8)


class RangeVerifyingKey(_LatencyMode, _RangeSlots, _Handle):
    """`RangeProofVK` (creds/src/rangeproof.rs:74-78) from the 640 bytes of range_vk.bin, resident on a GPU with h and
    beta_h prepared and fixed-base tables of g, gamma_g and com_f_basis, for proofs of n_bits bits (cg_range_vk_load).
    latency=True switches the handle to the one-workgroup-per-proof pairing (set_latency).
    Use as a context manager or close()."""
    _free, _add_bases, _last_kernel_ms = "cg_range_vk_free", "cg_range_vk_add_bases", "cg_range_vk_last_kernel_ms"
    _set_latency_mode = "cg_range_vk_set_latency_mode"

    def __init__(self, range_vk_bytes, n_bits: int, device: int = -1, latency: bool = False):
        b = _u8(range_vk_bytes)
        self.n_bits = int(n_bits)
        self._h = C.c_void_p()
        _check(lib().cg_range_vk_load(C.byref(self._h), _ptr(b) if b.size else None, b.size, self.n_bits, device))
        if latency:
            self.set_latency(True)


class T256Gens(_Handle):
    """`MultiCommitGens { G, h }` of spartan_t256 (forks/Spartan-t256/src/commitments.rs) resident on the current GPU as
    fixed-base tables (cg_t256_gens_load): g_xy n_gens x 64 B and h_xy 64 B, uncompressed T-256 points, x ‖ y big-endian.
    The byte forms of T-256 are UNVERIFIED readings of halo2curves (include/crescent_gpu.h).  A coordinate >= p_T, a point
    off the curve or the identity raises CrescentGpuError before the GPU is touched.  Use as a context manager or close()."""
    _free = "cg_t256_gens_free"

    def __init__(self, g_xy, h_xy):
        g, h = _u8(g_xy), _u8(h_xy, 64)
        if g.size % 64:
            raise ValueError("g_xy is n_gens x 64 bytes")
        self._h = C.c_void_p()
        _check(lib().cg_t256_gens_load(_ptr(g) if g.size else None, g.size // 64, _ptr(h), C.byref(self._h)))
        self.n_gens = g.size // 64

    @property
    def table_bytes(self) -> int:
        """what the set's n_gens + 1 tables take on the device (cg_t256_gens_info)"""
        n, b = C.c_uint64(), C.c_uint64()
        _check(lib().cg_t256_gens_info(self._h, C.byref(n), C.byref(b)))
        return int(b.value)

    def commit_rows_batch(self, scalars, blinds):
        """cg_t256_commit_rows_batch: `Vec<Scalar>::commit` (commitments.rs:88-99) for n rows - scalars n x n_gens x 32 B and
        blinds n x 32 B, little-endian, below q.  Returns (out33 (n, 33) compressed points, status (n,)); a row with a scalar
        or blind >= q is CG_SHOW_MALFORMED and zero bytes.  n_gens = 1 is `Scalar::commit`."""
        s, b = _u8(scalars), _u8(blinds)
        if b.size % 32 or s.size != b.size * self.n_gens:
            raise ValueError("blinds are n x 32 bytes and scalars n x n_gens x 32 bytes")
        n = b.size // 32
        out, status = np.zeros((n, 33), np.uint8), np.zeros(n, np.uint8)
        _check(lib().cg_t256_commit_rows_batch(self._h, _ptr(s) if n else None, _ptr(b) if n else None, n, _ptr(out), _ptr(status)))
        return out, status

    def hyrax_commit_batch(self, num_vars: int, vars_, blinds):
        """cg_hyrax_commit_batch: `DensePolynomial::commit` (dense_mlpoly.rs:181-206) for n proofs of 2^num_vars evaluations
        each, as L x R matrices with L = 2^(num_vars // 2) and R = n_gens: vars_ n x 2^num_vars x 32 B, blinds n x L x 32 B.
        Returns (out33 (n, L, 33), status (n,)); a proof with a scalar or blind >= q is CG_SHOW_MALFORMED and all its rows
        zero bytes."""
        v, b = _u8(vars_), _u8(blinds)
        num_vars = int(num_vars)
        if not 0 <= num_vars < 63:
            raise ValueError("num_vars")
        L = 1 << (num_vars // 2)
        if b.size % (32 * L) or v.size != (b.size // L) << num_vars:
            raise ValueError("blinds are n x L x 32 bytes and vars_ n x 2^num_vars x 32 bytes")
        n = b.size // (32 * L)
        out, status = np.zeros((n, L, 33), np.uint8), np.zeros(n, np.uint8)
        _check(lib().cg_hyrax_commit_batch(self._h, num_vars, _ptr(v) if n else None, _ptr(b) if n else None, n, _ptr(out), _ptr(status)))
        return out, status

    def commit_last_kernel_ms(self) -> Tuple[float, float, int]:
        """cg_t256_commit_last_kernel_ms: HIP-event milliseconds of the last call on this set - the check of the scalars, the
        group stage (the rows' sums and their normalisation) - and how many lanes shared a row in its last chunk"""
        ms, w = (C.c_float * 2)(), C.c_uint32()
        _check(lib().cg_t256_commit_last_kernel_ms(self._h, ms, C.byref(w)))
        return float(ms[0]), float(ms[1]), int(w.value)


@dataclass
class RangeProof:
    """creds/src/rangeproof.rs:82-93 as its serialized pieces: the commitments 64 B ark-serialize uncompressed G1, each
    proof 96 B (W uncompressed ‖ random_v, as cg_range_open_batch writes it), the evaluations, dleq_c and the responses
    dleq_s[statement][j] ints."""
    com_f: bytes
    com_g: bytes
    eval_g: int
    proof_g: bytes
    eval_gw: int
    proof_gw: bytes
    com_q: bytes
    eval_w_hat: int
    proof_w_hat: bytes
    dleq_c: int
    dleq_s: List[List[int]]

    def to_bytes(self) -> bytes:
        """`serialize_uncompressed`, fields in the struct's order; kzg10::Proof is w ‖ Option<Fr> (tag 1, then random_v:
        always Some here, include/crescent_gpu.h), DLogPoK is c ‖ s: Vec<Vec<Fr>>"""
        u64 = lambda v: int(v).to_bytes(8, "little")
        fr = lambda v: int(v).to_bytes(32, "little")

        def proof(p):
            p = bytes(p)
            if len(p) != 96:
                raise ValueError("a proof is 96 bytes: W, then random_v")
            return p[:64] + b"\x01" + p[64:]

        s = u64(len(self.dleq_s)) + b"".join(u64(len(si)) + b"".join(fr(x) for x in si) for si in self.dleq_s)
        return (bytes(self.com_f) + bytes(self.com_g) + fr(self.eval_g) + proof(self.proof_g) + fr(self.eval_gw) + proof(self.proof_gw)
                + bytes(self.com_q) + fr(self.eval_w_hat) + proof(self.proof_w_hat) + fr(self.dleq_c) + s)


@dataclass
class ShowGroth16:
    """creds/src/groth16rand.rs:38-45 as its serialized pieces: rand_proof 256 B (cg_prove's layout), com_hidden_inputs and
    every commited_inputs entry 64 B ark-serialize uncompressed G1, pok_c and the responses pok_s[statement][j] ints."""
    rand_proof: bytes
    com_hidden_inputs: bytes
    pok_c: int
    pok_s: List[List[int]]
    commited_inputs: List[bytes]

    def to_ark_bytes(self) -> bytes:
        """`serialize_uncompressed`: rand_proof | com_hidden_inputs | pok_inputs {c, s: Vec<Vec<Fr>>} | commited_inputs: Vec<G1>"""
        u64 = lambda v: int(v).to_bytes(8, "little")
        fr = lambda v: int(v).to_bytes(32, "little")
        s = u64(len(self.pok_s)) + b"".join(u64(len(si)) + b"".join(fr(x) for x in si) for si in self.pok_s)
        return (bytes(self.rand_proof) + bytes(self.com_hidden_inputs) + fr(self.pok_c) + s
                + u64(len(self.commited_inputs)) + b"".join(bytes(p) for p in self.commited_inputs))

    @staticmethod
    def from_ark_bytes(data) -> "ShowGroth16":
        b = bytes(data)
        at = 0

        def take(k):
            nonlocal at
            if k < 0 or at + k > len(b):
                raise ValueError("unexpected end of a serialized ShowGroth16")
            at += k
            return b[at - k:at]

        def count(item):
            k = int.from_bytes(take(8), "little")
            if k > (len(b) - at) // item:
                raise ValueError("vector length exceeds the remaining data")
            return k

        proof, comh = take(256), take(64)
        c = int.from_bytes(take(32), "little")
        s = [[int.from_bytes(take(32), "little") for _ in range(count(32))] for _ in range(count(8))]
        com = [take(64) for _ in range(count(64))]
        if at != len(b):
            raise ValueError("trailing bytes after a serialized ShowGroth16")
        return ShowGroth16(proof, comh, c, s, com)


def _inputs_array(inputs) -> np.ndarray:
    """public inputs of one proof: canonical 32-byte scalars (bytes / uint8 array) or ints"""
    if isinstance(inputs, (np.ndarray, bytes, bytearray, memoryview)):
        return _u8(inputs)
    return scalars_to_array(list(inputs)) if len(inputs) else np.zeros(0, np.uint8)


class CircomCircuit:
    """forks/circom-compat/src/circom/circuit.rs:11-27: an R1CS plus (optionally) the witness the WASM calculator
    produced for it.  `witness` is the full wire assignment in wire order (wire 0 = 1), canonical 32-byte scalars or
    Python ints; instance wires come first (circuit.rs:61-67), so it is also the prover's `full_assignment`."""

    def __init__(self, r1cs: "R1CSFile", witness=None):
        self.r1cs = r1cs
        self.witness = None
        if witness is not None:
            self.set_witness(witness)

    def set_witness(self, witness):
        if isinstance(witness, (list, tuple)):
            witness = scalars_to_array([int(x) % FR_MODULUS for x in witness])
        self.witness = _u8(witness, self.r1cs.num_variables * 32)

    def full_assignment(self) -> np.ndarray:
        return self.witness

    def check_witness(self) -> WitnessReport:
        """the witness against the circuit's R1CS on the GPU, over the resident matrices LibsnarkReduction keeps"""
        if self.witness is None:
            raise CrescentGpuError(-1, "AssignmentMissing: the circuit has no witness (SynthesisError::AssignmentMissing, circuit.rs:38-45)")
        cm = self.r1cs.matrices
        LibsnarkReduction._cache.max_cached = LibsnarkReduction.MAX_CACHED
        ctx = LibsnarkReduction._cache.lease(_matrices_key(cm), lambda: QapContext(cm))
        try:
            return ctx.check_witness(self.witness)
        finally:
            ctx._unlease()

    def is_satisfied(self) -> bool:
        """`cs.is_satisfied()` as the circom builder asks it (builder.rs:82-94)"""
        return self.check_witness().satisfied

    def which_is_unsatisfied(self) -> Optional[int]:
        """`cs.which_is_unsatisfied()`: the index of the first constraint the witness fails, None when it fails none
        (the reference names the constraint by a string; circom constraints have no names, so the index is the name)"""
        return self.check_witness().first_unsatisfied

    def get_public_inputs(self):
        """circuit.rs:18-26: wires 1 .. num_inputs-1 as integers (None without a witness)"""
        if self.witness is None:
            return None
        b = self.witness[32:32 * self.r1cs.num_inputs].tobytes()
        return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def generate_parameters_with_qap(matrices: ConstraintMatrices, alpha: int, beta: int, delta: int, tau: int) -> ProvingKey:
    """forks/groth16/src/generator.rs:50-228 with gamma = 1 and the standard generators (:28,:34-35), on the GPU."""
    l, m, M = matrices.num_instance_variables, matrices.num_constraints, matrices.num_variables
    D = 1
    while D < m + l:
        D <<= 1
    a = np.zeros(M * 64, np.uint8); b1 = np.zeros(M * 64, np.uint8); b2 = np.zeros(M * 128, np.uint8)
    h = np.zeros((D - 1) * 64, np.uint8); lq = np.zeros(max(M - l, 0) * 64, np.uint8) if M > l else np.zeros(0, np.uint8)
    gabc = np.zeros(l * 64, np.uint8); vkp = np.zeros(576, np.uint8)
    abc, _keep = matrices._c()
    tb, ab, bb, db = (_u8(fr_to_bytes(x)) for x in (tau, alpha, beta, delta))
    lq_buf = lq if lq.size else np.zeros(64, np.uint8)
    _check(lib().cg_setup(abc, l, m, M, _ptr(tb), _ptr(ab), _ptr(bb), _ptr(db), _ptr(a), _ptr(b1), _ptr(b2), _ptr(h),
                          _ptr(lq_buf), _ptr(gabc), _ptr(vkp)))
    vk = VerifyingKey(alpha_g1=vkp[0:64].copy(), beta_g2=vkp[192:320].copy(), gamma_g2=vkp[320:448].copy(),
                      delta_g1=vkp[128:192].copy(), delta_g2=vkp[448:576].copy(), gamma_abc_g1=gabc)
    return ProvingKey(vk=vk, beta_g1=vkp[64:128].copy(), delta_g1=vkp[128:192].copy(), a_query=a, b_g1_query=b1,
                      b_g2_query=b2, h_query=h, l_query=lq, coord_form=CG_FORM_CANONICAL)


# ------------------------------------------------------------------------------------------------
# unit-level operators
# ------------------------------------------------------------------------------------------------
def msm_bigint_g1(bases, scalars, coord_form: int = CG_FORM_CANONICAL, window_bits: int = 0) -> bytes:
    """<G1 as VariableBaseMSM>::msm_bigint (call sites prover.rs:66,74,266) -> affine canonical 64 B."""
    b, s = _u8(bases), _u8(scalars)
    out = np.zeros(64, np.uint8)
    _check(lib().cg_msm_g1(_ptr(b) if b.size else None, coord_form, b.size // 64, _ptr(s) if s.size else None,
                           s.size // 32, window_bits, _ptr(out)))
    return out.tobytes()


def msm_bigint_g2(bases, scalars, coord_form: int = CG_FORM_CANONICAL, window_bits: int = 0) -> bytes:
    b, s = _u8(bases), _u8(scalars)
    out = np.zeros(128, np.uint8)
    _check(lib().cg_msm_g2(_ptr(b) if b.size else None, coord_form, b.size // 128, _ptr(s) if s.size else None,
                           s.size // 32, window_bits, _ptr(out)))
    return out.tobytes()


def _ntt(data, inverse: bool, coset: bool) -> np.ndarray:
    a = _u8(data).copy()
    n = a.size // 32
    if n == 0 or n & (n - 1):
        raise ValueError("length must be a power of two")
    _check(lib().cg_ntt(_ptr(a), n.bit_length() - 1, 1 if inverse else 0, 1 if coset else 0))
    return a


def fft_in_place(data, coset: bool = False) -> np.ndarray:
    """EvaluationDomain::fft_in_place (coset=True: the `get_coset(F::GENERATOR)` domain, r1cs_to_qap.rs:182-185)."""
    return _ntt(data, False, coset)


def ifft_in_place(data, coset: bool = False) -> np.ndarray:
    """EvaluationDomain::ifft_in_place (r1cs_to_qap.rs:179-180,210)."""
    return _ntt(data, True, coset)


class MsmContext(_Handle):
    """A fixed set of G1 (group=1) or G2 (group=2) bases resident on the GPU with its window tables; `run` is
    msm_bigint against them (cg_msm_load_* / cg_msm_run)."""
    _free = "cg_msm_free"

    def __init__(self, bases, group: int = 1, coord_form: int = CG_FORM_CANONICAL, window_bits: int = 0, device: int = -1,
                 scalars_montgomery: bool = False):
        """scalars_montgomery=True: CG_FLAG_SCALARS_MONTGOMERY - run / run_dev take x * 2^256 mod r per scalar"""
        if group not in (1, 2):
            raise ValueError("group must be 1 or 2")
        self.group = group
        self.point_bytes = 64 * group
        b = _u8(bases)
        if b.size % self.point_bytes:
            raise ValueError("bases length is not a multiple of %d bytes" % self.point_bytes)
        self.n = b.size // self.point_bytes
        opt = _CgOptions(device=device, window_bits=window_bits, flags=CG_FLAG_SCALARS_MONTGOMERY if scalars_montgomery else 0)
        self._h = C.c_void_p()
        load = lib().cg_msm_load_g1 if group == 1 else lib().cg_msm_load_g2
        _check(load(C.byref(self._h), _ptr(b) if b.size else None, coord_form, self.n, C.byref(opt)))

    def run(self, scalars, timings: bool = False):
        s = _u8(scalars)
        return self._run(_ptr(s) if s.size else None, 0, s.size // 32, timings)

    def run_dev(self, d_ptr: int, n_scalars: int, timings: bool = False):
        """scalars already on this context's GPU (device pointer, n_scalars x 32 B in the handle's form; not written)"""
        return self._run(d_ptr, 1, n_scalars, timings)

    def _run(self, ptr, on_device, n, timings):
        out = np.zeros(self.point_bytes, np.uint8)
        tm = CgTimings()
        _check(lib().cg_msm_run(self._h, ptr, on_device, n, _ptr(out), C.byref(tm) if timings else None))
        return (out.tobytes(), tm.as_dict()) if timings else out.tobytes()


class NttContext(_Handle):
    """A radix-2 domain of size 2^log_n resident on the GPU (cg_ntt_load / cg_ntt_run)."""
    _free = "cg_ntt_free"

    def __init__(self, log_n: int, device: int = -1):
        self.log_n = log_n
        self._h = C.c_void_p()
        _check(lib().cg_ntt_load(C.byref(self._h), log_n, device))

    def run(self, data, inverse: bool = False, coset: bool = False) -> np.ndarray:
        a = _u8(data, 32 << self.log_n).copy()
        _check(lib().cg_ntt_run(self._h, _ptr(a), 0, 1 if inverse else 0, 1 if coset else 0, None))
        return a

    def run_dev(self, d_ptr: int, inverse: bool = False, coset: bool = False) -> float:
        """in place on device memory (2^log_n x 32 B canonical); returns the HIP-event time of the kernels in ms"""
        ms = C.c_float(0)
        _check(lib().cg_ntt_run(self._h, d_ptr, 1, 1 if inverse else 0, 1 if coset else 0, C.byref(ms)))
        return float(ms.value)


def fixed_base_g1(scalars) -> bytes:
    """scalars[i]·G1 (FixedBase::msm, generator.rs:162-194) -> n x 64 B affine canonical"""
    s = _u8(scalars)
    out = np.zeros(s.size * 2, np.uint8)
    _check(lib().cg_fixed_base_g1(_ptr(s) if s.size else None, s.size // 32, _ptr(out) if out.size else None))
    return out.tobytes()


def fixed_base_g2(scalars) -> bytes:
    s = _u8(scalars)
    out = np.zeros(s.size * 4, np.uint8)
    _check(lib().cg_fixed_base_g2(_ptr(s) if s.size else None, s.size // 32, _ptr(out) if out.size else None))
    return out.tobytes()


def proving_key_from_bytes(data) -> Tuple["ProvingKey", int]:
    """`ProvingKey::deserialize_uncompressed_unchecked` (what creds/src/utils.rs:179-189 does to the head of
    prover_params.bin).  Returns (key with canonical packed arrays, bytes consumed)."""
    L = lib()
    buf = _u8(data)
    h = C.c_void_p()
    used = C.c_uint64()
    _check(L.cg_pk_parse(_ptr(buf), buf.size, C.byref(h), C.byref(used)))
    try:
        v = _CgProvingKey()
        g2 = C.c_void_p(); gabc = C.c_void_p(); ngabc = C.c_uint64()
        _check(L.cg_pk_get(h, C.byref(v), C.byref(g2), C.byref(gabc), C.byref(ngabc)))

        pk = _pk_from_view(v, g2, gabc, ngabc.value)
    finally:
        L.cg_pk_free(h)
    return pk, int(used.value)


def _arr(ptr, nbytes) -> np.ndarray:
    if not nbytes:
        return np.zeros(0, np.uint8)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(int(nbytes),)).copy()


def _pk_from_view(v: _CgProvingKey, gamma_g2, gamma_abc, n_gamma_abc) -> "ProvingKey":
    vk = VerifyingKey(alpha_g1=_arr(v.alpha_g1, 64), beta_g2=_arr(v.beta_g2, 128), gamma_g2=_arr(gamma_g2, 128),
                      delta_g1=_arr(v.delta_g1, 64), delta_g2=_arr(v.delta_g2, 128), gamma_abc_g1=_arr(gamma_abc, 64 * n_gamma_abc))
    return ProvingKey(vk=vk, beta_g1=_arr(v.beta_g1, 64), delta_g1=_arr(v.delta_g1, 64), a_query=_arr(v.a_query, 64 * v.a_len),
                      b_g1_query=_arr(v.b_g1_query, 64 * v.b_g1_len), b_g2_query=_arr(v.b_g2_query, 128 * v.b_g2_len),
                      h_query=_arr(v.h_query, 64 * v.h_len), l_query=_arr(v.l_query, 64 * v.l_len))


@dataclass
class ProverParams:
    """creds/src/lib.rs:58-63.  `groth16_pvk` and `vk_bytes` are the serialized PreparedVerifyingKey / VerifyingKey
    exactly as the file holds them: the prover passes them on to the ClientState (creds/src/lib.rs:292-299)."""
    groth16_params: ProvingKey
    groth16_pvk: bytes
    config_str: str
    vk_bytes: bytes = b""

    @staticmethod
    def from_bytes(data) -> "ProverParams":
        """`read_from_file::<ProverParams>` (creds/src/utils.rs:179-189, creds/src/lib.rs:268)"""
        L = lib()
        buf = _u8(data)
        h = C.c_void_p()
        _check(L.cg_prover_params_parse(_ptr(buf), buf.size, C.byref(h)))
        try:
            v = _CgProverParamsView()
            _check(L.cg_prover_params_get(h, C.byref(v)))
            pk = _pk_from_view(v.pk, v.gamma_g2, v.gamma_abc_g1, v.gamma_abc_len)
            return ProverParams(pk, _arr(v.pvk_bytes, v.pvk_len).tobytes(), _arr(v.config_str, v.config_len).tobytes().decode("utf-8"),
                                _arr(v.vk_bytes, v.vk_len).tobytes())
        finally:
            L.cg_prover_params_free(h)

    def to_bytes(self) -> bytes:
        """`write_to_file(&prover_params, ..)` (creds/src/utils.rs:140-152, creds/src/lib.rs:245-248)"""
        L = lib()
        pk = self.groth16_params
        cpk = pk._c()
        n = pk.vk.gamma_abc_g1.size // 64
        pvk = _u8(self.groth16_pvk)
        cfg = _u8(self.config_str.encode("utf-8"))
        size = int(L.cg_prover_params_serialized_size(C.byref(cpk), n, pvk.size, cfg.size))
        out = np.zeros(size, np.uint8)
        gabc = pk.vk.gamma_abc_g1 if n else np.zeros(64, np.uint8)
        _check(L.cg_prover_params_serialize(C.byref(cpk), _ptr(pk.vk.gamma_g2), _ptr(gabc), n, _ptr(pvk), pvk.size,
                                            _ptr(cfg) if cfg.size else None, cfg.size, _ptr(out), size))
        return out.tobytes()


@dataclass
class ClientState:
    """creds/src/groth16rand.rs:23-35.  vk / pvk travel as their serialized bytes (they come out of prover_params.bin);
    `committed_input_openings` as the serialized items (empty for a state fresh out of create_client_state)."""
    inputs: List[int]
    aux: Optional[str]
    proof: Proof
    vk: bytes
    pvk: bytes
    config_str: str
    credtype: str = "jwt"                       # groth16rand.rs:76
    input_com_randomness: Optional[int] = None
    committed_input_openings: bytes = b""
    n_openings: int = 0

    @staticmethod
    def new(inputs, aux, proof: Proof, vk: bytes, pvk: bytes, config_str: str) -> "ClientState":
        """ClientState::new (groth16rand.rs:60-80)"""
        return ClientState(list(inputs), aux, proof, vk, pvk, config_str)

    def to_bytes(self) -> bytes:
        """ClientState::write_to_file (groth16rand.rs:89-98)"""
        L = lib()
        v = _CgClientStateView()
        keep = []

        def put(field, length_field, data):
            a = _u8(data)
            keep.append(a)
            setattr(v, field, _ptr(a) if a.size else None)
            if length_field:
                setattr(v, length_field, a.size)
        put("inputs", None, scalars_to_array(self.inputs) if self.inputs else b"")
        v.n_inputs = len(self.inputs)
        v.has_aux = 0 if self.aux is None else 1
        put("aux", "aux_len", (self.aux or "").encode("utf-8"))
        put("proof", None, self.proof.data)
        put("vk_bytes", "vk_len", self.vk)
        put("pvk_bytes", "pvk_len", self.pvk)
        v.has_input_com_randomness = 0 if self.input_com_randomness is None else 1
        put("input_com_randomness", None, fr_to_bytes(self.input_com_randomness or 0))
        put("openings_bytes", "openings_len", self.committed_input_openings)
        v.n_openings = self.n_openings
        put("credtype", "credtype_len", self.credtype.encode("utf-8"))
        put("config_str", "config_len", self.config_str.encode("utf-8"))
        if len(self.proof.data) != 256:
            raise ValueError("proof must be 256 bytes")
        size = int(L.cg_client_state_serialized_size(C.byref(v)))
        out = np.zeros(size, np.uint8)
        _check(L.cg_client_state_serialize(C.byref(v), _ptr(out), size))
        return out.tobytes()

    @staticmethod
    def from_bytes(data) -> "ClientState":
        """ClientState::new_from_file (groth16rand.rs:82-87)"""
        L = lib()
        buf = _u8(data)
        h = C.c_void_p()
        _check(L.cg_client_state_parse(_ptr(buf), buf.size, C.byref(h)))
        try:
            v = _CgClientStateView()
            _check(L.cg_client_state_get(h, C.byref(v)))
            ib = _arr(v.inputs, 32 * v.n_inputs).tobytes()
            inputs = [int.from_bytes(ib[i:i + 32], "little") for i in range(0, len(ib), 32)]
            aux = _arr(v.aux, v.aux_len).tobytes().decode("utf-8") if v.has_aux else None
            rnd = int.from_bytes(_arr(v.input_com_randomness, 32).tobytes(), "little") if v.has_input_com_randomness else None
            return ClientState(inputs, aux, Proof(_arr(v.proof, 256).tobytes()), _arr(v.vk_bytes, v.vk_len).tobytes(),
                               _arr(v.pvk_bytes, v.pvk_len).tobytes(), _arr(v.config_str, v.config_len).tobytes().decode("utf-8"),
                               _arr(v.credtype, v.credtype_len).tobytes().decode("utf-8"), rnd,
                               _arr(v.openings_bytes, v.openings_len).tobytes(), int(v.n_openings))
        finally:
            L.cg_client_state_free(h)


class IOLocations:
    """creds/src/structs.rs:26-100: `io_locations.sym`, one `name,location` row per public input/output of the
    Groth16 circuit (location = wire index, so public input i of the proof is location - 1; creds/src/lib.rs:305-307)."""

    def __init__(self, io_data: str):
        self.public_io_locations = {}
        for line in io_data.splitlines():                       # new_from_str (structs.rs:48-68)
            parts = line.split(",")
            if len(parts) != 2:
                raise ValueError("Line %s in io_locations.sym is not formatted correctly! Found %d parts." % (line, len(parts)))
            if not parts[1].isdigit():
                raise ValueError("Line %s in io_locations.sym: location is not an unsigned integer" % line)
            self.public_io_locations[parts[0]] = int(parts[1])
        self.public_io_locations = dict(sorted(self.public_io_locations.items()))    # BTreeMap order

    @staticmethod
    def from_file(path: str) -> "IOLocations":
        with open(path) as f:
            return IOLocations(f.read())

    def get_io_location(self, key: str) -> int:
        if key not in self.public_io_locations:
            raise KeyError("Key %s not found in public_io_locations" % key)
        return self.public_io_locations[key]

    def get_public_key_indices(self) -> List[int]:
        """structs.rs:80-90: zero-based input positions of the issuer key limbs"""
        return sorted(v - 1 for k, v in self.public_io_locations.items() if k.startswith("modulus") or k.startswith("pubkey"))

    def get_all_names(self) -> List[str]:
        return list(self.public_io_locations.keys())


class ProofRejected(CrescentGpuError):
    """create_client_state(verify=True): the fresh proof does not verify (the reference's `assert!`, creds/src/lib.rs:290)"""


def create_client_state(r1cs_bytes, prover_params_bytes, witness, rng, prover_aux: Optional[str] = None,
                        credtype: str = "jwt", prover: Optional["Prover"] = None, verify: bool = False,
                        check_witness: bool = False) -> "ClientState":
    """creds/src/lib.rs:255-301 without the witness generator: parse main_c.r1cs and prover_params.bin, prove with
    (r, s) drawn from `rng`, and assemble the ClientState the `show` step starts from.  `witness` is the full wire
    assignment the WASM calculator would have produced (wire 0 = 1).  With verify=True the proof is checked against the
    groth16_pvk of prover_params.bin on the GPU before the state is built, as the reference does (:286-290), and a
    rejected proof raises ProofRejected.  With check_witness=True the witness is checked against the R1CS on the GPU before it
    is proved (the circom builder's check, builder.rs:82-94) and UnsatisfiedWitness names the first failing constraint."""
    r1cs = R1CSFile(r1cs_bytes)
    pp = ProverParams.from_bytes(prover_params_bytes)
    circuit = CircomCircuit(r1cs, witness)
    if prover is not None:
        if check_witness:
            rep = prover.check_witness(circuit.full_assignment())
            if not rep.satisfied:
                raise UnsatisfiedWitness("constraint %d of %d is not satisfied (%d in all)"
                                         % (rep.first_unsatisfied, prover.num_constraints, rep.n_unsatisfied), rep)
        proof = prover.prove(circuit.full_assignment(), rng.randrange(FR_MODULUS), rng.randrange(FR_MODULUS))
    else:
        proof = Groth16.prove(pp.groth16_params, circuit, rng, check_witness=check_witness)
    if verify:
        with PreparedVerifyingKey(pp.groth16_pvk) as pvk:
            if not Groth16.verify_with_processed_vk(pvk, circuit.get_public_inputs(), proof):
                raise ProofRejected(CG_VERIFY_REJECT, "the proof does not verify against the prepared verifying key")
    cs = ClientState.new(circuit.get_public_inputs(), prover_aux, proof, pp.vk_bytes, pp.groth16_pvk, pp.config_str)
    cs.credtype = credtype
    return cs


def proving_key_to_bytes(pk: "ProvingKey") -> bytes:
    """`ProvingKey::serialize_uncompressed` (creds/src/utils.rs:140-152)."""
    L = lib()
    cpk = pk._c()
    n = pk.vk.gamma_abc_g1.size // 64
    size = int(L.cg_pk_serialized_size(C.byref(cpk), n))
    out = np.zeros(size, np.uint8)
    gabc = pk.vk.gamma_abc_g1 if n else np.zeros(64, np.uint8)
    _check(L.cg_pk_serialize(C.byref(cpk), _ptr(pk.vk.gamma_g2), _ptr(gabc), n, _ptr(out), size))
    return out.tobytes()


class R1CSFile:
    """forks/circom-compat/src/circom/r1cs_reader.rs:40-148 + R1CS::from (:26-38)."""

    def __init__(self, data: bytes):
        L = lib()
        buf = _u8(data)
        h = C.c_void_p()
        _check(L.cg_r1cs_parse(_ptr(buf), buf.size, C.byref(h)))
        try:
            hdr = _CgR1csHeader()
            abc = (_CgCsr * 3)()
            wm = C.c_void_p()
            _check(L.cg_r1cs_get(h, C.byref(hdr), abc, C.byref(wm)))
            self.header = {k: getattr(hdr, k) for k, _ in hdr._fields_}
            n_c = hdr.n_constraints
            mats = []
            for k in range(3):
                nnz = abc[k].nnz
                rp = np.ctypeslib.as_array(C.cast(abc[k].row_ptr, C.POINTER(C.c_uint64)), shape=(n_c + 1,)).copy()
                if nnz:
                    col = np.ctypeslib.as_array(C.cast(abc[k].col, C.POINTER(C.c_uint32)), shape=(nnz,)).copy()
                    coeff = np.ctypeslib.as_array(C.cast(abc[k].coeff, C.POINTER(C.c_uint8)), shape=(nnz * 32,)).copy()
                else:
                    col = np.zeros(0, np.uint32); coeff = np.zeros(0, np.uint8)
                mats.append(_Csr(rp, col, coeff))
            self.wire_mapping = np.ctypeslib.as_array(C.cast(wm, C.POINTER(C.c_uint64)), shape=(hdr.n_wires,)).copy()
            self.num_inputs = int(hdr.num_inputs)
            self.num_variables = int(hdr.num_variables)
            self.num_aux = self.num_variables - self.num_inputs
            self.matrices = ConstraintMatrices(mats[0], mats[1], mats[2], self.num_inputs, self.num_aux, n_c)
        finally:
            L.cg_r1cs_free(h)

    def constraint(self, i: int):
        """(A_i, B_i, C_i) as lists of (wire, coeff:int) — the reference's `Constraints<E>` tuple."""
        out = []
        for m in (self.matrices.a, self.matrices.b, self.matrices.c):
            lo, hi = int(m.row_ptr[i]), int(m.row_ptr[i + 1])
            out.append([(int(m.col[t]), int.from_bytes(m.coeff[32 * t:32 * t + 32].tobytes(), "little")) for t in range(lo, hi)])
        return tuple(out)
