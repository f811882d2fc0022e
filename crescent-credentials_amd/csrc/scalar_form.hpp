// Scalars in arkworks' in-memory form (CG_FLAG_SCALARS_MONTGOMERY, cg_qap_load_form, cg_scalars_convert).
//
// `Fr.0` of ark-ff is x·2^256 mod r as four u64 limbs: the 32 bytes this library calls CG_FORM_MONTGOMERY.  Everything
// downstream of an entry point - the witness map's packing, the digit extraction, the input checks - reads plain integers,
// so a handle loaded for that form converts ONCE, where the assignment reaches the device, and converts the coefficients
// it hands back on their way out.  One pass over 64 B per element (32 in, 32 out) and one Montgomery product by 1 (from)
// or by R^2 (to) per lane (measured: profiles/scalar_form_montgomery.md).
//
// ONE kernel definition for both translation units that launch it (prover.hip, unit.hip); `static`, so each of them
// carries its own copy of the code object entry and no symbol crosses between them.
#pragma once
#include "common.hpp"

namespace cg {

// to_mont = 0: in[i] is x·2^256 mod r -> out[i] = x; an input >= r is no field element: *bad = 1 (the caller's verdict; the
//              value written for it is some integer < r, so nothing downstream meets a non-canonical operand)
// to_mont = 1: in[i] is x < r -> out[i] = x·2^256 mod r (bad is not read)
// in == out is allowed: a lane reads its element whole before it writes it, and no lane touches another's (hence no
// __restrict__).  One element per lane, two 16-byte loads and two 16-byte stores; lane i at byte 32·i, so a wave reads
// and writes 2 KiB of consecutive memory.
static __global__ void __launch_bounds__(256) k_scalar_form(const Fr* in, Fr* out, uint64_t n, int to_mont, uint32_t* bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4* src = reinterpret_cast<const uint4*>(in + i);
    const uint4 lo = src[0], hi = src[1];
    Fr x;
    x.l[0] = lo.x; x.l[1] = lo.y; x.l[2] = lo.z; x.l[3] = lo.w;
    x.l[4] = hi.x; x.l[5] = hi.y; x.l[6] = hi.z; x.l[7] = hi.w;
    Fr k = Fr::zero();
    k.l[0] = 1u;
    if (to_mont) {
        k = Fr::r2();
    } else {
        bool lt = false, decided = false;
#pragma unroll
        for (int j = 7; j >= 0; --j)
            if (!decided && x.l[j] != FrP::N[j]) { lt = x.l[j] < FrP::N[j]; decided = true; }
        if (!lt) *bad = 1u;
    }
    const Fr y = mul(x, k);            // x·1·R^-1 or x·R^2·R^-1 (field.hpp); any 256-bit x against 1 stays inside the product's bounds
    uint4* dst = reinterpret_cast<uint4*>(out + i);
    dst[0] = make_uint4(y.l[0], y.l[1], y.l[2], y.l[3]);
    dst[1] = make_uint4(y.l[4], y.l[5], y.l[6], y.l[7]);
}

// n Montgomery elements at `in` -> their plain values at `out` (in == out: in place), on `st`; *bad (memory a kernel can
// write: device memory, or the device address of page-locked host memory) is set when an element is >= r
inline void scalars_from_mont(const Fr* in, Fr* out, uint64_t n, uint32_t* bad, hipStream_t st) {
    if (!n) return;
    k_scalar_form<<<ceil_div(n, 256), 256, 0, st>>>(in, out, n, 0, bad);
    CG_KERNEL_CHECK();
}
// n plain elements (< r: the library's own results) at `in` -> Montgomery form at `out`, on `st`
inline void scalars_to_mont(const Fr* in, Fr* out, uint64_t n, hipStream_t st) {
    if (!n) return;
    k_scalar_form<<<ceil_div(n, 256), 256, 0, st>>>(in, out, n, 1, nullptr);
    CG_KERNEL_CHECK();
}

inline bool scalar_form_known(uint32_t form) { return form == CG_FORM_CANONICAL || form == CG_FORM_MONTGOMERY; }

}  // namespace cg
