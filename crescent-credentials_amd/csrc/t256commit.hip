// pi2's witness commitment on the GPU: Pedersen vector commitments in T-256 (`Vec<Scalar>::commit` and `Scalar::commit`,
// forks/Spartan-t256/src/commitments.rs:81-99) for a batch of rows over ONE set of generators, and on them the Hyrax
// commitment of `DensePolynomial::commit` (dense_mlpoly.rs:181-206, `commit_inner` :151-163), the first step of
// `R1CSProof::prove` (r1csproof.rs:163-173), for a batch of proofs.  The arithmetic is csrc/t256.hpp's (the group and its
// bytes) over csrc/ft256.hpp (its base field); its scalar field is csrc/fp256.hpp's.
//
// cg_t256_gens is a key handle (key_handle.hpp): `MultiCommitGens { G, h }` as n_gens + 1 fixed-base tables of
// fixed_base.hpp's geometry, 522 240 B each, built on the host when the handle is loaded and resident on the device.
// A call is cut into chunks of whole groups - a group is a proof's L rows, or one row of the rows call - so that the caller's
// scalar array is never resident at once: at most T256_CHUNK_ROWS rows and T256_CHUNK_SCALARS scalars (64 MB) go up per
// chunk - and never less than one group: the 2055-generator limit admits num_vars = 22, whose proof is 2^22 scalars, and
// a chunk is then that one proof's 128 MB.  A chunk runs three kernels with nothing coming down in between:
//   k_t256_check   one wave per group: every scalar and blind of the group below q -> a flag byte per group.  A scalar on
//                  the device IS its eight words (32 bytes little-endian), so there is nothing to convert, and the digits are
//                  taken from those words where they are used.
//   k_t256_rows    W lanes per row, 64 / W rows per wave: lane t of a row walks its share of the row's digits through the
//                  tables into a projective partial (t256_walk_share: a mixed addition per non-zero byte, nothing for a zero
//                  wire; the share is cut by digit, of term j the windows (t - j) mod W, + W, ..., so that a wide scalar
//                  spreads over the row's lanes); the W partials meet in a butterfly of COMPLETE additions through LDS -
//                  generators may repeat or be opposite, and partials then coincide or cancel there -; lane 0 keeps the sum.
//                  No partial goes through HBM: the row's sum does, 96 bytes.
//   k_t256_finish  one lane per row: one inversion normalises the sum; the 33 compressed bytes, or 33 zero bytes for a
//                  malformed group, and the group's status.  With the inversion - some 520 products, more than a whole term
//                  of a uniform scalar - inside k_t256_rows, on one lane of W while the others waited, the group stage took
//                  a tenth longer (profiles/t256_commit.md has both figures).
// W is a power of two, at most 64 and at most the next power of two >= n_gens + 1 (for n_gens < 63 several rows SHARE a wave).
// Below that bound the host halves W while the chunk still fills the chip with T256_TARGET_WAVES waves: what a row costs
// beside its walk, the butterfly's log2 W additions, is paid by W lanes, so a large batch is cheaper at a small W and a small
// batch keeps the short latency of a wide one.
//
// Every kernel keeps its points in registers, reads scalars through pointers into global memory and declares no private
// segment; every HIP call is on the handle's stream.  The library draws no randomness: the blinds are the caller's.
#include <memory>

#include "common.hpp"
#include "host_parallel.hpp"
#include "key_handle.hpp"
#include "t256.hpp"

using namespace cg;

namespace {

constexpr uint64_t T256_CHUNK_ROWS = 1u << 14;         // rows per launch set
constexpr uint64_t T256_CHUNK_SCALARS = 1u << 21;      // scalars per launch set: 64 MB of the caller's array
constexpr uint64_t T256_TARGET_WAVES = 2048;           // two waves for each of the chip's 1024 SIMDs
constexpr uint64_t T256_MAX_TABLE_BYTES = 1ull << 30;  // of one handle's tables on the device: 2056 tables
constexpr uint64_t T256_TABLE_BYTES = (uint64_t)T256_TABLE_POINTS * sizeof(T256Affine);
constexpr int T256BLOCK = 64;                          // one wave
constexpr int T256_POINT_WORDS = 24;
static_assert(sizeof(T256Affine) == 64 && sizeof(T256Point) == 4 * T256_POINT_WORDS, "the tables and the LDS exchange are sized by these");

// group g: rows [g L, (g + 1) L), their L n_gens scalars and L blinds
__global__ __launch_bounds__(T256BLOCK) void k_t256_check(const uint32_t* __restrict__ scalars, const uint32_t* __restrict__ blinds, uint32_t n_gens,
                                                         uint32_t L, uint8_t* __restrict__ flags) {
    const uint64_t g = blockIdx.x;
    const uint64_t n_scalars = (uint64_t)L * n_gens, total = n_scalars + L;
    const uint32_t* s = scalars + 8 * g * n_scalars;
    const uint32_t* b = blinds + 8 * g * L;
    bool ok = true;
    for (uint64_t i = threadIdx.x; i < total; i += T256BLOCK) ok = ok && t256_scalar_ok(i < n_scalars ? s + 8 * i : b + 8 * (i - n_scalars));
    const bool bad = __ballot(!ok) != 0;
    if (threadIdx.x == 0) flags[g] = bad ? (uint8_t)CG_SHOW_MALFORMED : 0;
}

__global__ __launch_bounds__(T256BLOCK) void k_t256_rows(const T256Affine* __restrict__ tabs, const uint32_t* __restrict__ scalars,
                                                        const uint32_t* __restrict__ blinds, const uint8_t* __restrict__ flags, uint32_t n_gens,
                                                        uint32_t log_w, uint32_t L, uint64_t m, T256Point* __restrict__ sums) {
    __shared__ uint32_t sh[T256_POINT_WORDS][T256BLOCK];                       // word-major: a lane's column, no bank shared
    const uint32_t lane = threadIdx.x, W = 1u << log_w, t = lane & (W - 1);
    const uint64_t row = (uint64_t)blockIdx.x * (T256BLOCK >> log_w) + (lane >> log_w);
    const bool live = row < m;
    const uint64_t g = live ? row / L : 0;
    const bool bad = live && flags[g] != 0;
    const T256Curve c = t256_curve();
    T256Point acc = t256_identity(c);
    if (live && !bad) acc = t256_walk_share(tabs, scalars + 8 * row * n_gens, blinds + 8 * row, n_gens, t, log_w, c);
    // lanes t and t + s of a row meet, s = W/2, .., 1; a dead row's lanes carry the identity through the same steps
#pragma unroll 1
    for (uint32_t s = W >> 1; s; s >>= 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            sh[i][lane] = acc.x.l[i];
            sh[8 + i][lane] = acc.y.l[i];
            sh[16 + i][lane] = acc.z.l[i];
        }
        __syncthreads();
        if (t < s) {
            T256Point o;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                o.x.l[i] = sh[i][lane + s];
                o.y.l[i] = sh[8 + i][lane + s];
                o.z.l[i] = sh[16 + i][lane + s];
            }
            acc = t256_add(acc, o, c);
        }
        __syncthreads();
    }
    if (t == 0 && live && !bad) sums[row] = acc;
}

// one lane per row: the row's sum normalised with one inversion and written compressed, or 33 zero bytes for a malformed
// group; the first row of a group writes the group's status
__global__ __launch_bounds__(T256BLOCK) void k_t256_finish(const T256Point* __restrict__ sums, const uint8_t* __restrict__ flags, uint32_t L, uint64_t m,
                                                          uint8_t* __restrict__ out33, uint8_t* __restrict__ status) {
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= m) return;
    const uint64_t g = row / L;
    const bool bad = flags[g] != 0;
    uint8_t* o = out33 + T256_COMPRESSED * row;
    if (bad) {
        for (int i = 0; i < T256_COMPRESSED; ++i) o[i] = 0;
    } else {
        const T256Point sum = sums[row];
        t256_write_compressed(sum, ft256_inv(sum.z), o);
    }
    if (row % L == 0) status[g] = bad ? (uint8_t)CG_SHOW_MALFORMED : (uint8_t)CG_SHOW_MADE;
}

// lanes per row, as a power of two: the header has the rule
uint32_t pick_log_w(uint64_t rows, uint64_t n_terms) {
    uint32_t log_w = 0;
    while (log_w < 6 && (1ull << log_w) < n_terms) ++log_w;
    while (log_w > 0 && ((rows << (log_w - 1)) >> 6) >= T256_TARGET_WAVES) --log_w;
    return log_w;
}

}  // namespace

struct cg_t256_gens : KeyHandle {
    uint64_t n_gens = 0;
    StageTimer timer;                      // the check, the group stage
    uint32_t lanes_per_row = 0;            // of the last chunk of the last call
    DevBuf<T256Affine> tabs;               // G_0 .. G_{n_gens - 1}, then h
    RowBuf b_scal, b_blind{32}, b_out{T256_COMPRESSED}, b_status{1}, b_flags{1};
    DevBuf<T256Point> b_sum;               // a row's sum, between the two kernels of the group stage
    ~cg_t256_gens() { drain(); }           // before the buffers above are freed (key_handle.hpp)
};

extern "C" int cg_t256_gens_load(const uint8_t* g_xy, uint64_t n_gens, const uint8_t* h_xy, cg_t256_gens** out) {
    if (!out || !g_xy || !h_xy) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (n_gens < 1 || n_gens > T256_MAX_TABLE_BYTES / T256_TABLE_BYTES - 1)
        return fail(CG_ERR_INVALID_ARGUMENT, "n_gens = %llu: a set has 1 to %llu generators beside h (%llu bytes of tables each, 1 GiB in all)",
                    (unsigned long long)n_gens, (unsigned long long)(T256_MAX_TABLE_BYTES / T256_TABLE_BYTES - 1), (unsigned long long)T256_TABLE_BYTES);
    try {
        // host only: every refusal of the points comes before any HIP call
        std::vector<T256Affine> pts;
        uint64_t which = 0;
        if (const int rc = t256_read_gens(g_xy, n_gens, h_xy, pts, &which)) {
            char name[32];
            if (which < n_gens) snprintf(name, sizeof(name), "G[%llu]", (unsigned long long)which);
            else snprintf(name, sizeof(name), "h");
            return fail(CG_ERR_INVALID_ARGUMENT, "%s %s", name,
                        rc == T256_GENS_IDENTITY ? "is the identity" : rc == T256_GENS_NOT_CANONICAL ? "has a coordinate that is not below the field's prime"
                                                                                                     : "is not on the curve");
        }
        std::vector<T256Affine> tab((n_gens + 1) * (uint64_t)T256_TABLE_POINTS);
        parallel_ranges(n_gens + 1, 1, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t j = lo; j < hi; ++j) t256_make_table(pts[j], &tab[j * T256_TABLE_POINTS]);
        });
        std::unique_ptr<cg_t256_gens> k(new cg_t256_gens());
        k->n_gens = n_gens;
        k->b_scal.row = 32 * n_gens;
        k->open(-1);
        k->timer.create();
        k->tabs.alloc(tab.size());
        h2d_sync(k->tabs.p, tab.data(), tab.size() * sizeof(T256Affine), k->st);
        *out = k.release();
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

extern "C" void cg_t256_gens_free(cg_t256_gens* g) { free_handle(g); }

extern "C" int cg_t256_gens_info(const cg_t256_gens* g, uint64_t* n_gens, uint64_t* table_bytes) {
    if (!g || !n_gens || !table_bytes) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    *n_gens = g->n_gens;
    *table_bytes = (g->n_gens + 1) * T256_TABLE_BYTES;
    return CG_OK;
}

namespace {

// n_groups groups of L rows each, in chunks of whole groups; status has a byte per group
int t256_commit(cg_t256_gens* k, uint32_t L, const uint8_t* scalars, const uint8_t* blinds, uint64_t n_groups, uint8_t* out33, uint8_t* status) {
    try {
        std::lock_guard<std::mutex> lk(k->mu);
        CG_HIP(hipSetDevice(k->device));
        const uint64_t n_gens = k->n_gens;
        uint64_t per_chunk = std::min(T256_CHUNK_ROWS / L, T256_CHUNK_SCALARS / (L * n_gens));
        per_chunk = std::min(std::max<uint64_t>(per_chunk, 1), n_groups);
        const uint64_t chunk_rows = per_chunk * L;
        k->b_scal.reserve(chunk_rows);
        k->b_blind.reserve(chunk_rows);
        k->b_out.reserve(chunk_rows);
        k->b_status.reserve(per_chunk);
        k->b_flags.reserve(per_chunk);
        grow(k->b_sum, chunk_rows);
        k->timer.reset();
        for (uint64_t off = 0; off < n_groups; off += per_chunk) {
            const uint64_t mg = std::min(n_groups - off, per_chunk), m = mg * L;
            k->b_scal.up(k->st, scalars, off * L, m);
            k->b_blind.up(k->st, blinds, off * L, m);
            const uint32_t log_w = pick_log_w(m, n_gens + 1);
            k->lanes_per_row = 1u << log_w;
            k->timer.mark(0, k->st);
            k_t256_check<<<(uint32_t)mg, T256BLOCK, 0, k->st>>>(k->b_scal.words(), k->b_blind.words(), (uint32_t)n_gens, L, k->b_flags.bytes());
            CG_KERNEL_CHECK();
            k->timer.mark(1, k->st);
            k_t256_rows<<<ceil_div(m, T256BLOCK >> log_w), T256BLOCK, 0, k->st>>>(k->tabs.p, k->b_scal.words(), k->b_blind.words(), k->b_flags.bytes(),
                                                                                 (uint32_t)n_gens, log_w, L, m, k->b_sum.p);
            CG_KERNEL_CHECK();
            k_t256_finish<<<ceil_div(m, T256BLOCK), T256BLOCK, 0, k->st>>>(k->b_sum.p, k->b_flags.bytes(), L, m, k->b_out.bytes(), k->b_status.bytes());
            CG_KERNEL_CHECK();
            k->timer.mark(2, k->st);
            k->b_out.down(k->st, out33, off * L, m);
            k->b_status.down(k->st, status, off, mg);
            CG_HIP(hipStreamSynchronize(k->st));
            k->timer.add();
        }
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}

}  // namespace

extern "C" int cg_t256_commit_rows_batch(cg_t256_gens* g, const uint8_t* scalars, const uint8_t* blinds, uint64_t n_rows, uint8_t* out33,
                                         uint8_t* status) {
    if (!g) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    if (n_rows == 0) return CG_OK;
    if (!scalars || !blinds || !out33 || !status) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    return t256_commit(g, 1, scalars, blinds, n_rows, out33, status);
}

extern "C" int cg_hyrax_commit_batch(cg_t256_gens* g, uint32_t num_vars, const uint8_t* vars, const uint8_t* blinds, uint64_t n, uint8_t* out33,
                                     uint8_t* status) {
    if (!g) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    // compute_factored_lens (dense_mlpoly.rs:88-90)
    const uint32_t left = num_vars / 2, right = num_vars - left;
    if (right >= 32 || (1ull << right) != g->n_gens)
        return fail(CG_ERR_INVALID_ARGUMENT, "num_vars = %u: a row has 2^%u scalars, and this set has %llu generators", num_vars, right,
                    (unsigned long long)g->n_gens);
    if (n == 0) return CG_OK;
    if (!vars || !blinds || !out33 || !status) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    return t256_commit(g, 1u << left, vars, blinds, n, out33, status);
}

// Diagnostic: the kernels of the handle's last call - the check; the group stage, k_t256_rows and k_t256_finish - by HIP events,
// summed over the chunks;
// *lanes_per_row: the W of its last chunk
extern "C" int cg_t256_commit_last_kernel_ms(cg_t256_gens* g, float ms[2], uint32_t* lanes_per_row) {
    if (!g || !ms || !lanes_per_row) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    g->timer.read(&ms[0], &ms[1]);
    *lanes_per_row = g->lanes_per_row;
    return CG_OK;
}
