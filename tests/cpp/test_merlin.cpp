// Host build of csrc/merlin.hpp (plain g++), driven by tests/test_merlin_host.py: one request per input line, bytes as
// hex ("-" for none).  The Python side computes the same with tests/merlin_vectors.py.
//
//   seq LABEL (a LABEL MSG | c LABEL N)...   Transcript::new(LABEL), then appends and challenges -> the challenges, joined
//   range COM_F COM_G COM_Q                  the range shape            -> c ‖ rho, 32 bytes each
//   dleq SLOT(2) CFB(4) K(2) PED COM_F       the range proof's DLEQ     -> c, 32 bytes
//   dlog CONTEXT SHAPE BASES K Y             DLogPoK in general, SHAPE = n_bases joined by commas -> c, 32 bytes
//   compress POINT(64)                       ml_compress_g1             -> 32 bytes
// With the argument `kat` it reads nothing and checks the six known answers itself (the sanitizer run).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../crescent-credentials_amd/csrc/merlin.hpp"

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
    return s;
}

static std::string dlog(const Bytes& context, const std::vector<uint32_t>& shape, const Bytes& bases, const Bytes& k, const Bytes& y) {
    uint8_t c[32];
    ml_dlog_challenge(context.data(), context.size(), (uint32_t)shape.size(), shape.data(), bases.data(), k.data(),
                      [&](uint32_t i) { return y.data() + 32 * i; }, c);
    return hex(c, 32);
}

static int kat() {
    int bad = 0;
    auto expect = [&](const char* what, const std::string& got, const std::string& want) {
        if (got != want) {
            printf("%s: got %s want %s\n", what, got.c_str(), want.c_str());
            ++bad;
        }
    };
    {
        MerlinTranscript t((const uint8_t*)"test protocol", 13);
        t.append_message((const uint8_t*)"some label", 10, (const uint8_t*)"some data", 9);
        uint8_t out[32];
        t.challenge_bytes((const uint8_t*)"challenge", 9, out, 32);
        expect("kat0", hex(out, 32), "d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615");
    }
    {
        alignas(8) uint8_t st[ML_STATE];
        uint8_t in[96], c[32], rho[32], c_only[32];
        for (int i = 0; i < 96; ++i) in[i] = (uint8_t)i;
        ml_range_challenges(st, in, in + 32, in + 64, c, rho);
        expect("kat1", hex(c, 32), "f6626087b44cd5ee1e8644c59f13f49c218d536ad20580d43eb2c36f843e5f00");
        expect("kat2", hex(rho, 32), "cbb92f1236f66957cb6feffa0ded75a194d63fc51c91c2d0f3a981c10cfe4000");
        ml_range_challenges(st, in, in + 32, nullptr, c_only, nullptr);
        expect("kat1 alone", hex(c_only, 32), hex(c, 32));
        ml_range_challenges(st, in, in + 32, in + 64, nullptr, c_only);
        expect("kat2 replayed", hex(c_only, 32), hex(rho, 32));
    }
    struct { const char* context; std::vector<uint32_t> shape; const char* want; } cases[3] = {
        {"", {2, 4}, "1027fa2a35594a5813a65a499ed4c5f9b82cc79895d9764237e6b16958392800"},
        {"", {1}, "efbcd5bbd09b78e5b68cbb87faaccd13b8d39d6fb57accd5066fa4c8dd79d100"},
        {"presentation", {2, 2, 2, 24}, "55b8eb6c6d29f3ec41ade18c72ae1dae1732090af919390c0d5696987878e200"}};
    for (auto& cs : cases) {
        Bytes bases, k, y;
        uint8_t b = 1;
        for (size_t i = 0; i < cs.shape.size(); ++i) {
            for (uint32_t j = 0; j < cs.shape[i]; ++j, ++b) bases.insert(bases.end(), 32, b);
            k.insert(k.end(), 32, (uint8_t)(0xA0 + i));
            y.insert(y.end(), 32, (uint8_t)(0xB0 + i));
        }
        expect("dlog", dlog(Bytes(cs.context, cs.context + strlen(cs.context)), cs.shape, bases, k, y), cs.want);
        if (cs.shape.size() == 2 && cs.shape[1] == 4) {            // the fixed shape of a range proof's DLEQ is the same transcript
            alignas(8) uint8_t st[ML_STATE];
            uint8_t c[32];
            ml_range_dleq_challenge(st, bases.data(), bases.data() + 64, k.data(), y.data(), y.data() + 32, c);
            expect("dleq", hex(c, 32), cs.want);
        }
    }
    puts(bad ? "FAILED" : "OK");
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "kat")) return kat();
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        std::vector<std::string> w;
        for (std::string s; is >> s;) w.push_back(s);
        std::string out = "ERR";
        alignas(8) uint8_t st[ML_STATE];
        if (cmd == "seq" && !w.empty()) {
            const Bytes label = unhex(w[0]);
            MerlinTranscript t(label.data(), (uint32_t)label.size());
            out = "";
            for (size_t i = 1; i + 3 <= w.size(); i += 3) {
                const Bytes l = unhex(w[i + 1]);
                if (w[i] == "a") {
                    const Bytes m = unhex(w[i + 2]);
                    t.append_message(l.data(), (uint32_t)l.size(), m.data(), (uint32_t)m.size());
                } else {
                    Bytes c(strtoul(w[i + 2].c_str(), nullptr, 10));
                    t.challenge_bytes(l.data(), (uint32_t)l.size(), c.data(), (uint32_t)c.size());
                    out += hex(c.data(), c.size());
                }
            }
        } else if (cmd == "range" && w.size() == 3) {
            const Bytes f = unhex(w[0]), g = unhex(w[1]), q = unhex(w[2]);
            uint8_t c[64];
            if (f.size() == 32 && g.size() == 32 && q.size() == 32) {
                ml_range_challenges(st, f.data(), g.data(), q.data(), c, c + 32);
                out = hex(c, 64);
            }
        } else if (cmd == "dleq" && w.size() == 5) {
            const Bytes slot = unhex(w[0]), cfb = unhex(w[1]), k = unhex(w[2]), ped = unhex(w[3]), f = unhex(w[4]);
            uint8_t c[32];
            if (slot.size() == 64 && cfb.size() == 128 && k.size() == 64 && ped.size() == 32 && f.size() == 32) {
                ml_range_dleq_challenge(st, slot.data(), cfb.data(), k.data(), ped.data(), f.data(), c);
                out = hex(c, 32);
            }
        } else if (cmd == "dlog" && w.size() == 5) {
            std::vector<uint32_t> shape;
            std::istringstream ss(w[1]);
            for (std::string s; std::getline(ss, s, ',');) shape.push_back((uint32_t)strtoul(s.c_str(), nullptr, 10));
            const Bytes context = unhex(w[0]), bases = unhex(w[2]), k = unhex(w[3]), y = unhex(w[4]);
            uint64_t nb = 0;
            for (uint32_t s : shape) nb += s;
            if (bases.size() == 32 * nb && k.size() == 32 * shape.size() && y.size() == 32 * shape.size()) out = dlog(context, shape, bases, k, y);
        } else if (cmd == "compress" && w.size() == 1) {
            const Bytes p = unhex(w[0]);
            if (p.size() == 64) {
                uint32_t in[16], o[8];
                memcpy(in, p.data(), 64);
                ml_compress_g1(in, o);
                out = hex((const uint8_t*)o, 32);
            }
        }
        puts(out.c_str());
        fflush(stdout);
    }
    return 0;
}
