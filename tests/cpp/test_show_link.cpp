// Host build of csrc/show_link.hpp and of the one-text DLogPoK transcript of csrc/merlin.hpp (plain g++), driven by
// tests/test_show_link_host.py: one request per input line, bytes as hex ("-" for none).  The Python side computes the same
// with tests/merlin_vectors.py and oracle/bn254_oracle.py.  Points are x ‖ y, canonical little-endian, zeros for O.
//
//   dlog1 CONTEXT SHAPE BASES K Y     ml_dlog_shape_challenge, SHAPE = n_bases joined by commas; CONTEXT "none" is a null
//                                     pointer with length 0                                          -> c, 32 bytes
//   dlog0 CONTEXT SHAPE BASES K Y     the host's ml_dlog_challenge over MerlinTranscript, same operands -> c, 32 bytes
//   shift BASE COMMITTED T            build_tables of BASE, then shift_commitment(table, COMMITTED, T)  -> the point
//   open M T                          shift_opening                                                    -> m - t mod r
//   below T                           link_below_r                                                     -> 0 / 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../crescent-credentials_amd/csrc/merlin.hpp"
#include "../../crescent-credentials_amd/csrc/show_link.hpp"

using namespace cg;
typedef std::vector<uint8_t> Bytes;

static Bytes unhex(const std::string& s) {
    if (s == "-" || s == "none") return Bytes();
    Bytes b(s.size() / 2);
    for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return b;
}
static std::string hex(const uint8_t* b, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        s += d[b[i] >> 4];
        s += d[b[i] & 15];
    }
    return s;
}
static Fq fq_in(const uint8_t* b) {
    Fq a;
    memcpy(a.l, b, 32);
    return to_mont(a);
}
static G1Affine g1_in(const Bytes& b) {
    for (uint8_t c : b)
        if (c) return G1Affine{fq_in(b.data()), fq_in(b.data() + 32)};
    return G1Affine::inf();
}
static std::string g1_out(const G1Affine& p) {
    uint8_t o[64] = {0};
    if (!p.is_inf()) {
        const Fq x = from_mont(p.x), y = from_mont(p.y);
        memcpy(o, x.l, 32);
        memcpy(o + 32, y.l, 32);
    }
    return hex(o, 64);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        std::vector<std::string> w;
        for (std::string s; is >> s;) w.push_back(s);
        std::string out = "ERR";
        if ((cmd == "dlog1" || cmd == "dlog0") && w.size() == 5) {
            std::vector<uint32_t> shape;
            std::istringstream ss(w[1]);
            for (std::string s; std::getline(ss, s, ',');) shape.push_back((uint32_t)strtoul(s.c_str(), nullptr, 10));
            const Bytes context = unhex(w[0]), bases = unhex(w[2]), k = unhex(w[3]), y = unhex(w[4]);
            const uint8_t* ctx = w[0] == "none" ? nullptr : context.data();
            uint64_t nb = 0;
            for (uint32_t s : shape) nb += s;
            if (bases.size() == 32 * nb && k.size() == 32 * shape.size() && y.size() == 32 * shape.size()) {
                uint8_t c[32];
                if (cmd == "dlog1") {
                    alignas(8) uint8_t st[ML_STATE];
                    ml_dlog_shape_challenge(st, ctx, context.size(), (uint32_t)shape.size(), [&](uint32_t i) { return shape[i]; }, bases.data(),
                                            k.data(), y.data(), c);
                } else {
                    ml_dlog_challenge(ctx, context.size(), (uint32_t)shape.size(), shape.data(), bases.data(), k.data(),
                                      [&](uint32_t i) { return y.data() + 32 * i; }, c);
                }
                out = hex(c, 32);
            }
        } else if (cmd == "shift" && w.size() == 3) {
            const Bytes base = unhex(w[0]), com = unhex(w[1]), t = unhex(w[2]);
            if (base.size() == 64 && com.size() == 64 && t.size() == 32) {
                std::vector<G1Affine> tab;
                build_tables(std::vector<G1Affine>{G1Affine::inf(), g1_in(base)}, tab);
                uint32_t tw[8];
                memcpy(tw, t.data(), 32);
                out = g1_out(to_affine(shift_commitment(tab.data(), g1_in(com), tw)));
            }
        } else if (cmd == "open" && w.size() == 2) {
            const Bytes m = unhex(w[0]), t = unhex(w[1]);
            if (m.size() == 32 && t.size() == 32) {
                uint32_t mw[8], tw[8], o[8];
                memcpy(mw, m.data(), 32);
                memcpy(tw, t.data(), 32);
                shift_opening(mw, tw, o);
                out = hex((const uint8_t*)o, 32);
            }
        } else if (cmd == "below" && w.size() == 1) {
            const Bytes t = unhex(w[0]);
            if (t.size() == 32) {
                uint32_t tw[8];
                memcpy(tw, t.data(), 32);
                out = link_below_r(tw) ? "1" : "0";
            }
        }
        puts(out.c_str());
        fflush(stdout);
    }
    return 0;
}
