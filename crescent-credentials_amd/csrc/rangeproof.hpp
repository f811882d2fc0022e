// The internal entry of rangeproof.hip, for a caller that owns a second handle (cg_create_showings_batch in verify.hip), as
// rangeverify.hpp declares rangeverify.hip's: `prove_n_bits` whole for a piece of showings whose openings and ped_com are
// ALREADY ON THE DEVICE.  The caller holds the range key's lock for the whole call and orders the range key's stream against
// its own with events; nothing here waits on the host.  The public cg_range_prove_batch is a thin caller of the same code.
// For .hip files only.
#pragma once
#include "common.hpp"

namespace cg {

constexpr uint64_t RANGE_PK_PIECE = 1u << 12;      // the most showings one range_pk_enqueue takes (RCHUNK of rangeproof.hip)

// one proof per showing, a row each: where cg_range_prove_batch's outputs go on the host; challenges and status may be null
struct RangePkOut {
    uint8_t *com_f, *com_g, *com_q, *evals, *proofs, *pok_c, *pok_s, *challenges, *status;
};

std::mutex& range_pk_lock(cg_range_pk* k);
int range_pk_device(const cg_range_pk* k);
hipStream_t range_pk_stream(cg_range_pk* k);
// the 128 bytes registered for `slot`, or null for an unknown slot; under the lock
const uint8_t* range_pk_slot_bytes(const cg_range_pk* k, uint32_t slot);
// room for pieces of `piece` showings in every per-call array; under the lock, with the key's device current.  Nothing is
// timed in such a call: cg_range_pk_last_kernel_ms reads zeros after it
void range_pk_reserve(cg_range_pk* k, uint64_t piece);
// The kernels of cg_range_prove_batch for m <= RANGE_PK_PIECE showings, put on the key's stream: the openings (m x 16
// words) and ped_com (m x 16 words) are read from device memory; the m rows of 18 random scalars come up from `rand`, a host
// pointer at the first row, rows rand_pitch bytes apart; output row i goes down to row off + i of each array of `out`, and
// the m status bytes are also left at d_status (device, may be null).  `slot` has been accepted by range_pk_slot_bytes.
void range_pk_enqueue(cg_range_pk* k, uint32_t slot, const uint32_t* d_openings, const uint32_t* d_ped_com, const uint8_t* rand,
                      uint64_t rand_pitch, const RangePkOut& out, uint64_t off, uint64_t m, uint8_t* d_status);

}  // namespace cg
