// The host code that the key handles of the credential entries share (cg_pvk in verify.hip, cg_range_pk in rangeproof.hip,
// cg_range_vk in rangeverify.hip): a handle's device, stream and lock; the event bracket that times a call's two stages;
// the registered Pedersen slots of the two range keys; a per-call device array with its row width; and the DLogPoK
// responses, which are host arithmetic.  Plain structs and free functions.
// For .hip files only.
#pragma once
#include "ark_codec.hpp"
#include "fixed_base.hpp"
#include "merlin.hpp"
#include "show_make.hpp"

namespace cg {
namespace {

// A handle's device, its own non-blocking stream and the lock every entry takes.
// Destruction order: the stream is waited for BEFORE any DevBuf of the handle is freed.  A destructor here would run after
// the derived handle's members are gone, so there is none: every handle derives from KeyHandle and keeps a one-line
// destructor, `~cg_x() { drain(); }`, whose body runs before its members are destroyed.  That was chosen over a KeyHandle
// member declared last (destroyed first) because it stays right when a buffer is added below it.
struct KeyHandle {
    int device = 0;
    hipStream_t st = nullptr;
    std::mutex mu;
    // after all host-only parsing: every parse error is reported before any HIP call
    void open(int32_t dev) {
        device = dev;
        if (device < 0) CG_HIP(hipGetDevice(&device));
        CG_HIP(hipSetDevice(device));
        CG_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    }
    void drain() {
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
        st = nullptr;
    }
};
template <class K>
void free_handle(K* k) {
    if (!k) return;
    (void)hipSetDevice(k->device);
    delete k;                    // the destructor waits for the handle's stream
}

// HIP-event times of a call's two stages, summed over its chunks: mark(0), stage one, mark(1), stage two, mark(2), and
// add() once the stream has been waited for.
struct StageTimer {
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float ms[2] = {0, 0};        // of the last call
    ~StageTimer() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    void create() { for (hipEvent_t& e : ev) CG_HIP(hipEventCreate(&e)); }
    void reset() { ms[0] = ms[1] = 0; }
    void mark(int i, hipStream_t st) { CG_HIP(hipEventRecord(ev[i], st)); }
    void add() {
        float t0 = 0, t1 = 0;
        CG_HIP(hipEventElapsedTime(&t0, ev[0], ev[1]));
        CG_HIP(hipEventElapsedTime(&t1, ev[1], ev[2]));
        ms[0] += t0;
        ms[1] += t1;
    }
    void read(float* first, float* second) const { *first = ms[0]; *second = ms[1]; }
};
// cg_range_pk_last_kernel_ms / cg_range_vk_last_kernel_ms: a handle with a StageTimer `timer`
template <class K>
int last_kernel_ms(K* k, float* first, float* second) {
    if (!k || !first || !second) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(k->mu);
    k->timer.read(first, second);
    return CG_OK;
}

// cg_pvk_set_latency_mode / cg_range_vk_set_latency_mode: a handle with a `latency` flag, taken under its lock
template <class K>
int set_latency_mode(K* k, int32_t on) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    if (on != 0 && on != 1) return fail(CG_ERR_INVALID_ARGUMENT, "latency mode is 0 or 1, not %d", on);
    std::lock_guard<std::mutex> lk(k->mu);
    k->latency = on != 0;
    return CG_OK;
}

// The Pedersen bases registered on a range key: per slot the fixed-base tables of one pair (2 x 1 MB on the device) and
// the pair's 2 x 32 compressed bytes, which the DLEQ's transcript absorbs under b"base"; on the host the pair's 128 bytes
// as registered, which cg_verify_showings_batch compares with the bases of the Groth16 key it is called with.
struct PedersenSlots {
    static constexpr uint32_t MAX_SLOTS = 64;
    std::vector<DevBuf<G1Affine>> tabs;
    std::vector<DevBuf<uint8_t>> cmps;
    std::vector<std::vector<uint8_t>> registered;
    // cg_range_pk_add_bases / cg_range_vk_add_bases after their null check
    int add(KeyHandle& k, const uint8_t ped_bases[128], uint32_t* slot) {
        std::vector<G1Affine> bases(3, G1Affine::inf()), tab;    // build_tables skips the first entry
        for (int i = 0; i < 2; ++i)
            if (!checked_g1(ped_bases + 64 * i, bases[1 + i])) return fail(CG_ERR_INVALID_ARGUMENT, "Pedersen base %d is no valid G1 point", i);
        try {
            std::lock_guard<std::mutex> lk(k.mu);
            if (tabs.size() >= MAX_SLOTS) return fail(CG_ERR_INVALID_ARGUMENT, "all %u slots of this key are taken", MAX_SLOTS);
            build_tables(bases, tab);
            CG_HIP(hipSetDevice(k.device));
            DevBuf<G1Affine> d(tab.size());
            h2d_sync(d.p, tab.data(), tab.size() * sizeof(G1Affine), k.st);
            uint32_t w[16], cmp[16];
            for (int i = 0; i < 2; ++i) {
                memcpy(w, ped_bases + 64 * i, 64);
                ml_compress_g1(w, cmp + 8 * i);
            }
            DevBuf<uint8_t> dc(sizeof(cmp));
            h2d_sync(dc.p, cmp, sizeof(cmp), k.st);
            tabs.reserve(tabs.size() + 1);
            cmps.reserve(cmps.size() + 1);
            registered.reserve(registered.size() + 1);
            registered.emplace_back(ped_bases, ped_bases + 128);
            tabs.push_back(std::move(d));
            cmps.push_back(std::move(dc));
            *slot = (uint32_t)tabs.size() - 1;
            return CG_OK;
        } catch (...) {
            return translate_current_exception();
        }
    }
    // the tables of a slot, under the handle's lock; `entry` is the call that registers one, for the message.  An unknown
    // slot is thrown: call this only inside the entry's try block, which turns it into the code and the message
    const G1Affine* table(uint32_t slot, const char* entry) const {
        if (slot < tabs.size()) return tabs[slot].p;
        char b[128];
        snprintf(b, sizeof(b), "slot %u was not registered on this key (%s)", slot, entry);
        throw HipError(CG_ERR_INVALID_ARGUMENT, b);
    }
    const uint8_t* compressed(uint32_t slot) const { return cmps[slot].p; }      // after table(slot, ..) has accepted the slot
};
// the domain sizes of a range key; `fn` is prove_n_bits or verify_n_bits.  CG_OK, or the failure already recorded
[[maybe_unused]] int check_range_bits(uint32_t n_bits, const char* fn) {
    if (n_bits == 2 || n_bits == 4 || n_bits == 8 || n_bits == 16 || n_bits == 32) return CG_OK;
    return fail(CG_ERR_INVALID_ARGUMENT, "n_bits = %u: %s takes a power of two, and a value has at most 32 bits here", n_bits, fn);
}

// One array of a call on the device: the caller's bytes, `row` of them per item, a chunk of items at a time.  A fixed
// width is given where the handle declares the buffer (RowBuf b{64}) and reserve(chunk) is all a call says.  A buffer
// declared without one has a width that depends on the call's layout and KEEPS the last call's: every entry names it
// again, reserve(chunk, row), before it copies.
struct RowBuf {
    DevBuf<uint8_t> d;
    uint64_t row = 0;
    explicit RowBuf(uint64_t row_bytes = 0) : row(row_bytes) {}
    // room for `chunk` rows: grown, never shrunk, and never empty, so that the pointer of an array the layout leaves
    // empty (row 0) is still one a kernel may be handed
    void reserve(uint64_t chunk) { grow(d, chunk * row ? chunk * row : 64); }
    void reserve(uint64_t chunk, uint64_t row_bytes) { row = row_bytes; reserve(chunk); }
    // rows [off, off + m) of the caller's array to the start of the buffer and back, on the handle's stream; nothing for
    // an array the layout leaves empty (row 0) or the caller may leave out (null)
    void up(hipStream_t st, const uint8_t* h, uint64_t off, uint64_t m) {
        if (h && row) CG_HIP(hipMemcpyAsync(d.p, h + off * row, m * row, hipMemcpyHostToDevice, st));
    }
    void down(hipStream_t st, uint8_t* h, uint64_t off, uint64_t m) const {
        if (h && row) CG_HIP(hipMemcpyAsync(h + off * row, d.p, m * row, hipMemcpyDeviceToHost, st));
    }
    const uint32_t* words() const { return (const uint32_t*)d.p; }
    uint32_t* words_mut() { return (uint32_t*)d.p; }
    uint8_t* bytes() { return d.p; }                               // a status, flag or verdict byte per item
};

// DLogPoK::prove's responses (dlog.rs:101-109), s = nonce - c·secret (show_make.hpp's row), for n showings of n_resp responses each:
// secret(p, t) and nonce(p, t) point at the 32 bytes of showing p's t-th pair, `what` names the secrets' source in the
// message.  Every value is checked first, so an error writes nothing; a showing whose status is not CG_SHOW_MADE gets zeros.
template <class Secret, class Nonce>
int dlog_respond(uint64_t n, uint32_t n_resp, const uint8_t* status, const uint8_t* c, Secret secret, Nonce nonce, uint8_t* out,
                 const char* what) {
    for (uint64_t p = 0; p < n; ++p) {
        if (status && status[p] != CG_SHOW_MADE) continue;
        bool ok = scalar_is_canonical(c + 32 * p);
        for (uint32_t t = 0; t < n_resp; ++t) ok = ok && scalar_is_canonical(secret(p, t)) && scalar_is_canonical(nonce(p, t));
        if (!ok) return fail(CG_ERR_INVALID_ARGUMENT, "showing %llu: %s, a rand scalar or c is not below the scalar modulus", (unsigned long long)p, what);
    }
    for (uint64_t p = 0; p < n; ++p) {
        uint8_t* s = out + 32 * p * n_resp;
        if (status && status[p] != CG_SHOW_MADE) {
            memset(s, 0, 32 * (size_t)n_resp);
            continue;
        }
        uint32_t w[3][8];                                                   // c, then per row the secret and the nonce; the row is s
        memcpy(w[0], c + 32 * p, 32);
        const Fr cm = mk_challenge_mont(w[0]);
        for (uint32_t t = 0; t < n_resp; ++t) {                             // show_make.hpp: the row k_mk_respond computes
            memcpy(w[1], secret(p, t), 32);
            memcpy(w[2], nonce(p, t), 32);
            mk_response_row(cm, w[1], w[2], w[0]);
            memcpy(s + 32 * t, w[0], 32);
        }
    }
    return CG_OK;
}

}  // namespace
}  // namespace cg
