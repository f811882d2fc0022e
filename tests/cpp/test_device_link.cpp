// Host build of csrc/sha256.hpp and csrc/device_link.hpp (plain g++), driven by tests/test_device_link_host.py: one request
// per input line, bytes as hex ("-" for none).  The Python side computes the same with hashlib and
// tests/device_link_vectors.py.
//
//   sha MSG                                   sha256_of                                              -> 32 bytes
//   sha2 A B                                  one digest over two sha_run calls, A then B (finishing) -> 32 bytes
//   dec V                                     dl_dec of the 32 little-endian bytes V                  -> the text as hex
//   digest C0 COM0 COM1 COMZ HQ               dl_challenge_digest; points 64 B ark-uncompressed       -> 32 bytes
//   scalars M C0 S0 C1 S1 E                   dl_scalars (S0 128 B, S1 96 B, E 32 B)  -> flags, then the three merged scalars
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../crescent-credentials_amd/csrc/device_link.hpp"

using namespace cg;
typedef std::vector<uint8_t> Bytes;

static Bytes unhex(const std::string& s) {
    if (s == "-") return Bytes();
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
    return n ? s : std::string("-");
}
// the caller's bytes as words, on their own heap block so that a sanitizer sees every read past them
static std::vector<uint32_t> words(const Bytes& b) {
    std::vector<uint32_t> w(b.size() / 4);
    memcpy(w.data(), b.data(), w.size() * 4);
    return w;
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
        alignas(8) uint8_t blk[SHA_BLOCK];
        uint8_t digits[DL_DIGITS_ROOM], d[32];
        if (cmd == "sha" && w.size() == 1) {
            const Bytes m = unhex(w[0]);
            sha256_of(blk, m.data(), m.size(), d);
            out = hex(d, 32);
        } else if (cmd == "sha2" && w.size() == 2) {
            const Bytes a = unhex(w[0]), b = unhex(w[1]);
            Sha256 s = sha_begin(blk);
            sha_run(s, 1, false, [&](int) { return sha_bytes(a.data(), (uint32_t)a.size()); });
            sha_run(s, 1, true, [&](int) { return sha_bytes(b.data(), (uint32_t)b.size()); });
            sha_digest(s, d);
            out = hex(d, 32);
        } else if (cmd == "dec" && w.size() == 1) {
            const Bytes v = unhex(w[0]);
            if (v.size() == 32) {
                const std::vector<uint32_t> vw = words(v);
                const uint32_t n = dl_dec(vw.data(), 0xffffffffu, digits);
                out = hex(digits + DL_DIGITS - n, n);
            }
        } else if (cmd == "digest" && w.size() == 5) {
            const Bytes c0 = unhex(w[0]), com0 = unhex(w[1]), com1 = unhex(w[2]), comz = unhex(w[3]), hq = unhex(w[4]);
            if (c0.size() == 32 && com0.size() == 64 && com1.size() == 64 && comz.size() == 64 && hq.size() <= DL_H_MAX) {
                const std::vector<uint32_t> a = words(c0), b = words(com0), c = words(com1), e = words(comz);
                dl_challenge_digest(blk, digits, a.data(), b.data(), c.data(), e.data(), hq.data(), (uint32_t)hq.size(), d);
                out = hex(d, 32);
            }
        } else if (cmd == "scalars" && w.size() == 6) {
            const Bytes m = unhex(w[0]), c0 = unhex(w[1]), s0 = unhex(w[2]), c1 = unhex(w[3]), s1 = unhex(w[4]), e = unhex(w[5]);
            if (m.size() == 32 && c0.size() == 32 && s0.size() == 128 && c1.size() == 32 && s1.size() == 96 && e.size() == 32) {
                const std::vector<uint32_t> mw = words(m), c0w = words(c0), s0w = words(s0), c1w = words(c1), s1w = words(s1), ew = words(e);
                uint32_t merged[8 * DL_N_SCALARS] = {0};
                const uint32_t f = dl_scalars(DlIn{mw.data(), c0w.data(), s0w.data(), c1w.data(), s1w.data(), ew.data()}, merged, 1);
                out = std::to_string(f) + ":" + hex((const uint8_t*)merged, sizeof(merged));
            }
        }
        puts(out.c_str());
        fflush(stdout);
    }
    return 0;
}
