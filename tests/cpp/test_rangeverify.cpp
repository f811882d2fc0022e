// Host build of csrc/rangeverify.hpp (plain g++, one lane), driven by tests/test_range_verify_cpu.py: one showing per
// input line, every scalar as hex of canonical little-endian bytes.  The Python side computes the same values with
// tests/range_verify_vectors.py.
//
//   LOG_N EVALS(3 x 32 B) RANDOM_V(3 x 32 B) C RHO RANDOMIZERS(2 x 16 B) [POK_C POK_S(6 x 32 B)]
//     -> MALFORMED, or "I E" (the identity bit, the eq_pos bit) and the ten merged term scalars
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../crescent-credentials_amd/csrc/rangeverify.hpp"

using namespace cg;

static std::vector<uint32_t> unhex_words(const std::string& s) {
    std::vector<uint8_t> b(s.size() / 2);
    for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    std::vector<uint32_t> w(b.size() / 4);
    if (!w.empty()) memcpy(w.data(), b.data(), w.size() * 4);
    return w;
}
static void put(const uint32_t* w, size_t words) {
    const uint8_t* b = (const uint8_t*)w;
    for (size_t i = 0; i < 4 * words; ++i) printf("%02x", b[i]);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string ev_s, rv_s, c_s, rho_s, rz_s, pc_s, ps_s;
        uint32_t log_n = 0;
        is >> log_n >> ev_s >> rv_s >> c_s >> rho_s >> rz_s >> pc_s >> ps_s;
        const std::vector<uint32_t> ev = unhex_words(ev_s), rv = unhex_words(rv_s), c = unhex_words(c_s), rho = unhex_words(rho_s),
                                    rz = unhex_words(rz_s), pc = unhex_words(pc_s), ps = unhex_words(ps_s);
        const bool pok = !pc.empty();
        if (log_n < 1 || log_n > 5 || ev.size() != 24 || rv.size() != 24 || c.size() != 8 || rho.size() != 8 || rz.size() != 8 ||
            (pok && (pc.size() != 8 || ps.size() != 8 * RP_N_RESP))) {
            puts("ERR");
            fflush(stdout);
            continue;
        }
        std::vector<uint32_t> proofs(72, 0xA5A5A5A5u);                // the points are not read here
        for (int j = 0; j < 3; ++j) memcpy(&proofs[24 * j + 16], &rv[8 * j], 32);
        const RangeConsts k = range_consts(log_n);
        const RvIn in{ev.data(), proofs.data(), c.data(), rho.data(), rz.data(), pok ? pc.data() : nullptr, pok ? ps.data() : nullptr};
        std::vector<uint32_t> out(8 * RV_N_SCALARS);
        const uint32_t flags = rv_scalars(k, in, out.data(), 1);
        if (flags & RV_MALFORMED) {
            puts("MALFORMED");
        } else {
            printf("%d %d ", flags & RV_IDENTITY ? 1 : 0, flags & RV_EQ_POS ? 1 : 0);
            put(out.data(), out.size());
            puts("");
        }
        fflush(stdout);
    }
    return 0;
}
