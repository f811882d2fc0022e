// Host build of csrc/rangepoly.hpp (plain g++, one lane), driven by tests/test_rangepoly_host.py: one showing per input
// line, every scalar as hex of 32 canonical little-endian bytes.  The Python side computes the same vectors with
// tests/range_vectors.py.
//
//   commit   LOG_N OPEN(2) RAND(18)          -> the n + 17 term scalars of com_f | com_g | k_0 | k_1
//   quotient LOG_N OPEN RAND C               -> the 2n + 7 term scalars of com_q
//   open     LOG_N OPEN RAND C RHO           -> the 4n + 15 term scalars of the three W, then 3 evaluations, then 3 random_v
// MALFORMED where the call reports the showing as malformed.  OPEN and RAND are given as one hex string each.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../crescent-credentials_amd/csrc/rangepoly.hpp"

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
    static RangeWork W;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd, open_s, rand_s, c_s, rho_s;
        uint32_t log_n = 0;
        is >> cmd >> log_n >> open_s >> rand_s >> c_s >> rho_s;
        const std::vector<uint32_t> open = unhex_words(open_s), rand = unhex_words(rand_s), c = unhex_words(c_s), rho = unhex_words(rho_s);
        const bool commit = cmd == "commit", quotient = cmd == "quotient", opening = cmd == "open";
        if (log_n < 1 || log_n > 5 || open.size() != 16 || rand.size() != 8 * RP_N_RAND || (!commit && c.size() != 8) ||
            (opening && rho.size() != 8) || !(commit || quotient || opening)) {
            puts("ERR");
            fflush(stdout);
            continue;
        }
        const RangeConsts k = range_consts(log_n);
        const RangeIn in{open.data(), rand.data(), commit ? nullptr : c.data(), opening ? rho.data() : nullptr};
        HostLane ln;
        std::vector<uint32_t> terms(8 * rp_open_terms(k.n)), evals(24), proofs(72);
        bool made;
        size_t n_terms;
        if (commit) made = rp_commit(k, in, W, terms.data(), ln), n_terms = rp_commit_terms(k.n);
        else if (quotient) made = rp_quotient_call(k, in, W, terms.data(), ln), n_terms = rp_quotient_terms(k.n);
        else made = rp_open(k, in, W, terms.data(), evals.data(), proofs.data(), ln), n_terms = rp_open_terms(k.n);
        if (!made) {
            puts("MALFORMED");
        } else {
            put(terms.data(), 8 * n_terms);
            if (opening) {
                put(evals.data(), 24);
                for (int j = 0; j < 3; ++j) put(proofs.data() + 24 * j + 16, 8);
            }
            puts("");
        }
        fflush(stdout);
    }
    return 0;
}
