// The public inputs of pi2 on the GPU: `ECDSACircuitPublicInputs::compute_TU` (ecdsa-pop/src/lib.rs:217-240), which a relying
// party runs at the top of `ECDSAProof::verify`, and `compute_RTU` (:180-215), which a prover runs at the top of
// `ECDSAProof::prove` and which is the only place where the device's ECDSA signature is checked - for a batch of rows under
// one cg_pvk.  The arithmetic is csrc/p256.hpp's (the group), csrc/fp256.hpp's and csrc/fq256.hpp's (its two fields).
//
// The calls use the handle's stream, lock and a state slot of their own and nothing of the key, as cg_hq_batch does.  A
// chunk of m rows runs three kernels with nothing coming down in between; terms are laid out TERM-MAJOR within the chunk
// (term t of row p at t·m + p, devicelink.hip's layout), so that a wave runs one kind of term:
//   k_p256_*_scalars  one lane per row: the point's coordinates below p and on the curve, r (and s) in range, the reductions
//                     mod n, ONE inversion in the scalar field (r for compute_TU; r·s for compute_RTU, which serves both)
//                     -> a flag byte, the row's point in Montgomery form, the canonical scalar of every term
//   k_p256_terms      one lane per (term, row): a 4-bit windowed chain on the row's point, its sixteen multiples in a
//                     per-lane table in global memory, entry-major; or a walk through the 8-bit table of G    -> projective partials
//                       compute_TU:   r^-1 · R | (-d/r) · G
//                       compute_RTU:  (r/s) · Q, (1/s) · Q | (d/s) · G, (d/(r s)) · G, (-d/r) · G
//                     T = r^-1 · R is taken apart as (d/(r s)) · G + (1/s) · Q, so that no term waits for another
//   k_p256_*_finish   one lane per row: R = (d/s) G + (r/s) Q and T by the general, complete addition - a signer chooses Q, and
//                     where Q is a small multiple of +-G the two partial sums coincide or cancel -; one inversion in the base
//                     field normalises all of a row's points; R the identity or R.x mod n != r is CG_P256_BAD_SIGNATURE; the
//                     bytes, big-endian; a row that is not made has every output zeroed here
// A malformed row costs nothing after the stage that found it.
//
// What profiles/device_link_hq.md found holds here: a lane runs its few thousand products one after the other and the wave
// is alone on its SIMD, so a kernel's time is ONE LANE'S LATENCY at every batch size up to some tens of thousands of rows -
// a chain is 334 additions of fourteen products.  That is why the terms are lanes of their own and why a call is worth
// making for a batch, not for one row (profiles/p256_tu.md).
//
// The table of G (522 240 bytes) is built on the host once per process and uploaded once per handle, by the first call that
// needs it.  Every kernel keeps its points in registers, reads scalars and digits through pointers into global memory and
// declares no private segment.
#include <memory>

#include "common.hpp"
#include "device_link.hpp"
#include "key_handle.hpp"
#include "p256.hpp"

using namespace cg;

namespace {

constexpr uint64_t P256CHUNK = 1u << 14;   // rows per launch set; 4 KB of device memory per row, most of it the chains' tables
constexpr int P256BLOCK = 64;

// one chunk's working arrays on the device
struct P256Work {
    uint8_t* flags;                        // a byte per row: 0, or CG_SHOW_MALFORMED
    P256Affine* pts;                       // the row's point, R or Q
    uint32_t* scalars;                     // scalar j of row p at 8·(j·m + p)
    uint32_t* r_words;                     // compute_RTU: r as canonical words
    P256Point* part;                       // term t of row p at t·m + p
    P256Point* tabs;                       // entry e of chain c of row p at (16·c + e)·m + p
    uint64_t m;
};

__global__ __launch_bounds__(P256BLOCK) void k_p256_tu_scalars(const uint8_t* __restrict__ r_xy, const uint8_t* __restrict__ digest, P256Work w) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= w.m) return;
    const P256Curve c = p256_curve();
    P256Affine R;
    const bool ok = p256_tu_scalars(r_xy + 64 * p, digest + 32 * p, c, R, w.scalars + 8 * p, w.m);
    w.pts[p] = R;
    w.flags[p] = ok ? 0 : (uint8_t)CG_SHOW_MALFORMED;
}

__global__ __launch_bounds__(P256BLOCK) void k_p256_rtu_scalars(const uint8_t* __restrict__ q_xy, const uint8_t* __restrict__ sig,
                                                               const uint8_t* __restrict__ digest, P256Work w) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= w.m) return;
    const P256Curve c = p256_curve();
    P256Affine Q;
    const bool ok = p256_rtu_scalars(q_xy + 64 * p, sig + 64 * p, digest + 32 * p, c, Q, w.scalars + 8 * p, w.m, w.r_words + 8 * p);
    w.pts[p] = Q;
    w.flags[p] = ok ? 0 : (uint8_t)CG_SHOW_MALFORMED;
}

__global__ __launch_bounds__(P256BLOCK) void k_p256_terms(P256Work w, uint32_t n_chains, uint32_t n_terms, const P256Affine* __restrict__ g_tab) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t m = w.m;
    if (g >= m * n_terms) return;
    const uint32_t t = (uint32_t)(g / m);
    const uint64_t p = g % m;
    if (w.flags[p]) return;
    const P256Curve c = p256_curve();
    // a walk's lane is handed the table room of chain 0, which it does not touch
    P256Point* tab = w.tabs + (uint64_t)P256_CHAIN_TABLE * (t < n_chains ? t : 0) * m + p;
    w.part[g] = p256_term((int)t, (int)n_chains, g_tab, w.pts[p], w.scalars + 8 * g, tab, m, c);
}

__global__ __launch_bounds__(P256BLOCK) void k_p256_tu_finish(P256Work w, uint8_t* __restrict__ t_xy, uint8_t* __restrict__ u_xy,
                                                             uint8_t* __restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= w.m) return;
    if (w.flags[p]) {
        p256_zero_bytes(t_xy + 64 * p, 64);
        p256_zero_bytes(u_xy + 64 * p, 64);
        status[p] = CG_SHOW_MALFORMED;
        return;
    }
    const P256Curve c = p256_curve();
    p256_tu_finish(w.part[p], w.part[w.m + p], c, t_xy + 64 * p, u_xy + 64 * p);
    status[p] = CG_SHOW_MADE;
}

__global__ __launch_bounds__(P256BLOCK) void k_p256_rtu_finish(P256Work w, uint8_t* __restrict__ r_xy, uint8_t* __restrict__ t_xy,
                                                              uint8_t* __restrict__ u_xy, uint8_t* __restrict__ status) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= w.m) return;
    uint8_t st = w.flags[p] ? (uint8_t)CG_SHOW_MALFORMED : (uint8_t)CG_SHOW_MADE;
    if (st == CG_SHOW_MADE) {
        const P256Curve c = p256_curve();
        const uint64_t m = w.m;
        const P256Point* part = w.part;
        st = p256_rtu_finish([=](int t) { return part[(uint64_t)t * m + p]; }, w.r_words + 8 * p, c, r_xy + 64 * p, t_xy + 64 * p, u_xy + 64 * p);
    }
    if (st != CG_SHOW_MADE) {
        p256_zero_bytes(r_xy + 64 * p, 64);
        p256_zero_bytes(t_xy + 64 * p, 64);
        p256_zero_bytes(u_xy + 64 * p, 64);
    }
    status[p] = st;
}

// A handle's table of G on the device, uploaded by the first call that needs it, and the arrays of the two entries.  Its own
// slot of the handle: the verifier's, the maker's and the h_Q entries' arrays stay where they are.
struct P256State {
    DevBuf<P256Affine> g_tab;
    uint32_t uploads = 0;
    RowBuf b_pt{64}, b_sig{64}, b_digest{32};
    RowBuf b_r{64}, b_t{64}, b_u{64}, b_status{1};
    RowBuf b_flags{1}, b_pts{sizeof(P256Affine)}, b_rw{32};
    DevBuf<uint32_t> b_scalars;
    DevBuf<P256Point> b_part, b_tabs;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};       // around the three kernels of a chunk
    float ms[3] = {0, 0, 0};                                        // of the last call, summed over its chunks
    ~P256State() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
};
void p256_state_free(void* s) { delete (P256State*)s; }
static_assert(sizeof(P256Affine) == 64 && sizeof(P256Point) == 96, "the device arrays are sized by these");

// under the handle's lock, after hipSetDevice
P256State& p256_state(PvkLinkView& v) {
    if (!*v.p256_state) {
        std::unique_ptr<P256State> fresh(new P256State());
        for (hipEvent_t& x : fresh->ev) CG_HIP(hipEventCreate(&x));
        *v.p256_state_free = p256_state_free;
        *v.p256_state = fresh.release();
    }
    P256State& h = *(P256State*)*v.p256_state;
    if (!h.uploads) {
        const std::vector<P256Affine>& tab = p256_table();
        grow(h.g_tab, (uint64_t)tab.size());
        h2d_sync(h.g_tab.p, tab.data(), sizeof(P256Affine) * tab.size(), v.st);
        h.uploads = 1;
    }
    return h;
}

// cg_p256_tu_batch (sig and r_xy null) and cg_p256_rtu_batch, in chunks; pt is r_xy of the first and q_xy of the second
int p256_rows(cg_pvk* k, const uint8_t* pt, const uint8_t* sig, const uint8_t* digest, uint64_t n, uint8_t* r_xy, uint8_t* t_xy, uint8_t* u_xy,
              uint8_t* status, bool rtu) {
    if (!k) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return CG_OK;
    if (!pt || !digest || !t_xy || !u_xy || !status || (rtu && (!sig || !r_xy))) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    PvkLinkView v;
    pvk_link_handle(k, v);
    try {
        std::lock_guard<std::mutex> lk(*v.mu);
        CG_HIP(hipSetDevice(v.device));
        P256State& h = p256_state(v);
        const uint64_t chunk = n < P256CHUNK ? n : P256CHUNK;
        const uint32_t n_chains = rtu ? P256_RTU_CHAINS : P256_TU_CHAINS, n_terms = rtu ? P256_RTU_TERMS : P256_TU_TERMS;
        for (RowBuf* b : {&h.b_pt, &h.b_sig, &h.b_digest, &h.b_r, &h.b_t, &h.b_u, &h.b_status, &h.b_flags, &h.b_pts, &h.b_rw}) b->reserve(chunk);
        grow(h.b_scalars, 8 * chunk * n_terms);
        grow(h.b_part, chunk * n_terms);
        grow(h.b_tabs, chunk * n_chains * P256_CHAIN_TABLE);
        h.ms[0] = h.ms[1] = h.ms[2] = 0;
        for (uint64_t off = 0; off < n; off += chunk) {
            const uint64_t m = n - off < chunk ? n - off : chunk;
            h.b_pt.up(v.st, pt, off, m);
            h.b_sig.up(v.st, sig, off, m);
            h.b_digest.up(v.st, digest, off, m);
            const P256Work w{h.b_flags.bytes(), (P256Affine*)h.b_pts.bytes(), h.b_scalars.p, h.b_rw.words_mut(), h.b_part.p, h.b_tabs.p, m};
            const uint32_t rows = ceil_div(m, P256BLOCK);
            CG_HIP(hipEventRecord(h.ev[0], v.st));
            if (rtu) k_p256_rtu_scalars<<<rows, P256BLOCK, 0, v.st>>>(h.b_pt.bytes(), h.b_sig.bytes(), h.b_digest.bytes(), w);
            else k_p256_tu_scalars<<<rows, P256BLOCK, 0, v.st>>>(h.b_pt.bytes(), h.b_digest.bytes(), w);
            CG_KERNEL_CHECK();
            CG_HIP(hipEventRecord(h.ev[1], v.st));
            k_p256_terms<<<ceil_div(m * n_terms, P256BLOCK), P256BLOCK, 0, v.st>>>(w, n_chains, n_terms, h.g_tab.p);
            CG_KERNEL_CHECK();
            CG_HIP(hipEventRecord(h.ev[2], v.st));
            if (rtu) k_p256_rtu_finish<<<rows, P256BLOCK, 0, v.st>>>(w, h.b_r.bytes(), h.b_t.bytes(), h.b_u.bytes(), h.b_status.bytes());
            else k_p256_tu_finish<<<rows, P256BLOCK, 0, v.st>>>(w, h.b_t.bytes(), h.b_u.bytes(), h.b_status.bytes());
            CG_KERNEL_CHECK();
            CG_HIP(hipEventRecord(h.ev[3], v.st));
            h.b_r.down(v.st, r_xy, off, m);
            h.b_t.down(v.st, t_xy, off, m);
            h.b_u.down(v.st, u_xy, off, m);
            h.b_status.down(v.st, status, off, m);
            CG_HIP(hipStreamSynchronize(v.st));
            for (int i = 0; i < 3; ++i) {
                float t = 0;
                CG_HIP(hipEventElapsedTime(&t, h.ev[i], h.ev[i + 1]));
                h.ms[i] += t;
            }
        }
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

}  // namespace

extern "C" int cg_p256_tu_batch(cg_pvk* k, const uint8_t* r_xy, const uint8_t* digest, uint64_t n, uint8_t* t_xy, uint8_t* u_xy,
                                uint8_t* status) {
    return p256_rows(k, r_xy, nullptr, digest, n, nullptr, t_xy, u_xy, status, false);
}

extern "C" int cg_p256_rtu_batch(cg_pvk* k, const uint8_t* q_xy, const uint8_t* sig, const uint8_t* digest, uint64_t n, uint8_t* r_xy,
                                 uint8_t* t_xy, uint8_t* u_xy, uint8_t* status) {
    return p256_rows(k, q_xy, sig, digest, n, r_xy, t_xy, u_xy, status, true);
}

// Diagnostic: the three kernels of the handle's last cg_p256_tu_batch or cg_p256_rtu_batch - the scalar stage, the terms, the
// finishing stage - by HIP events, summed over the chunks; *uploads how often the table of G went up to this handle
extern "C" int cg_p256_last_kernel_ms(cg_pvk* k, float ms[3], uint32_t* uploads) {
    if (!k || !ms || !uploads) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    PvkLinkView v;
    pvk_link_handle(k, v);
    std::lock_guard<std::mutex> lk(*v.mu);
    const P256State* h = (const P256State*)*v.p256_state;
    for (int i = 0; i < 3; ++i) ms[i] = h ? h->ms[i] : 0.0f;
    *uploads = h ? h->uploads : 0u;
    return CG_OK;
}
