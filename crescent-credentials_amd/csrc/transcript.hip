// `DLogPoK`'s Merlin transcript (creds/src/dlog.rs:56-58, 77-99 and :130-132, 147-169) for hosts that have no Merlin of
// their own: the challenge between cg_show_commit_batch and cg_show_respond_batch, the one compared behind
// cg_verify_show_batch, and the DLEQ's of the three-call range path.  Host only - merlin.hpp on the library's worker
// threads (host_parallel.hpp) - with no handle and no HIP call, so it runs in a process without a GPU.
#include <vector>

#include "common.hpp"
#include "host_parallel.hpp"
#include "merlin.hpp"

using namespace cg;

namespace {

// an uncompressed G1 point as a transcript may absorb it: flags valid, both coordinates below q.  Not the curve equation:
// the verifying calls check that.
bool point_bytes_ok(const uint8_t* b) {
    if ((b[63] & 0xC0) == 0xC0) return false;
    uint8_t y[32];
    memcpy(y, b + 32, 32);
    y[31] &= 0x3F;
    return fp_is_canonical(fp_from_bytes<Fq>(b)) && fp_is_canonical(fp_from_bytes<Fq>(y));
}
void compress(const uint8_t* b, uint8_t* out) {
    uint32_t w[16], c[8];
    memcpy(w, b, 64);
    ml_compress_g1(w, c);
    memcpy(out, c, 32);
}
[[noreturn]] void refuse(const char* what, unsigned long long at) {
    char b[160];
    snprintf(b, sizeof(b), "%s %llu: a coordinate is not below the base field modulus, or the point flags are invalid", what, at);
    throw HipError(CG_ERR_INVALID_ARGUMENT, b);
}

}  // namespace

extern "C" int cg_dlog_challenge_batch(const uint8_t* context, uint64_t context_len, uint64_t context_stride, uint32_t n_statements,
                                       const uint32_t* n_bases, const uint8_t* bases, const uint8_t* k, const uint8_t* y_head,
                                       const uint8_t* y_last, uint64_t n, uint8_t* c_out) {
    if (n_statements == 0) return fail(CG_ERR_INVALID_ARGUMENT, "a DLogPoK has at least one statement");
    if (!n_bases) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    uint64_t total_bases = 0;
    for (uint32_t i = 0; i < n_statements; ++i) total_bases += n_bases[i];
    if ((total_bases && !bases) || (context_len && !context)) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    if (context_stride && context_stride < context_len)
        return fail(CG_ERR_INVALID_ARGUMENT, "a context stride of %llu is shorter than the context's %llu bytes", (unsigned long long)context_stride,
                    (unsigned long long)context_len);
    if (context_len > 0xffffffffull - 8) return fail(CG_ERR_INVALID_ARGUMENT, "a context of %llu bytes is longer than a Merlin message", (unsigned long long)context_len);
    if (n == 0) return CG_OK;
    if (!k || !y_last || !c_out || (n_statements > 1 && !y_head)) return fail(CG_ERR_INVALID_ARGUMENT, "null argument");
    try {
        // every point is looked at before the first challenge is written: a refused batch leaves c_out as it was
        std::vector<uint8_t> bases_c(32 * total_bases);
        for (uint64_t b = 0; b < total_bases; ++b) {
            if (!point_bytes_ok(bases + 64 * b)) refuse("base", b);
            compress(bases + 64 * b, bases_c.data() + 32 * b);
        }
        const uint64_t n_head = n_statements - 1;
        parallel_ranges(n, 8, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t p = lo; p < hi; ++p) {
                bool ok = point_bytes_ok(y_last + 64 * p);
                for (uint64_t i = 0; i < n_head; ++i) ok = ok && point_bytes_ok(y_head + 64 * (p * n_head + i));
                if (!ok) refuse("showing", p);
            }
        });
        parallel_ranges(n, 8, [&](uint64_t lo, uint64_t hi) {
            std::vector<uint8_t> y(32 * (size_t)n_statements);
            for (uint64_t p = lo; p < hi; ++p) {
                for (uint64_t i = 0; i < n_head; ++i) compress(y_head + 64 * (p * n_head + i), y.data() + 32 * i);
                compress(y_last + 64 * p, y.data() + 32 * n_head);
                ml_dlog_challenge(context ? context + p * context_stride : nullptr, context_len, n_statements, n_bases, bases_c.data(),
                                  k + 32 * p * n_statements, [&](uint32_t i) { return y.data() + 32 * (size_t)i; }, c_out + 32 * p);
            }
        });
        return CG_OK;
    } catch (...) {
        return translate_current_exception();
    }
}
