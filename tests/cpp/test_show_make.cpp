// Host build of csrc/show_make.hpp (plain g++), driven by tests/test_show_make_host.py: one request per input line, scalars
// as 64 hex digits (32 bytes, canonical little-endian).  The Python side computes the same with its own integers.
//
//   row C SECRET NONCE               mk_response_row(mk_challenge_mont(C), SECRET, NONCE)           -> s, 32 bytes
//   at P N_IO N_RAND POS CI          mk_link_opening: the scalar indices of (m, r)                  -> "M,R" in decimal
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../crescent-credentials_amd/csrc/show_make.hpp"

using namespace cg;

static bool unhex32(const std::string& s, uint32_t w[8]) {
    if (s.size() != 64) return false;
    uint8_t b[32];
    for (size_t i = 0; i < 32; ++i) b[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    memcpy(w, b, 32);
    return true;
}
static std::string hex32(const uint32_t w[8]) {
    static const char* d = "0123456789abcdef";
    uint8_t b[32];
    memcpy(b, w, 32);
    std::string s;
    for (uint8_t c : b) {
        s += d[c >> 4];
        s += d[c & 15];
    }
    return s;
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
        if (cmd == "row" && w.size() == 3) {
            uint32_t c[8], secret[8], nonce[8], s[8];
            if (unhex32(w[0], c) && unhex32(w[1], secret) && unhex32(w[2], nonce)) {
                mk_response_row(mk_challenge_mont(c), secret, nonce, s);
                out = hex32(s);
            }
        } else if (cmd == "at" && w.size() == 5) {
            const MkOpeningAt at = mk_link_opening(strtoull(w[0].c_str(), nullptr, 10), (uint32_t)strtoul(w[1].c_str(), nullptr, 10),
                                                   (uint32_t)strtoul(w[2].c_str(), nullptr, 10), (uint32_t)strtoul(w[3].c_str(), nullptr, 10),
                                                   (uint32_t)strtoul(w[4].c_str(), nullptr, 10));
            out = std::to_string(at.m) + "," + std::to_string(at.r);
        }
        puts(out.c_str());
        fflush(stdout);
    }
    return 0;
}
