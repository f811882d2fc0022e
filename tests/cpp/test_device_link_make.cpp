// Host build of csrc/device_link_make.hpp (plain g++), driven by tests/test_device_link_make_host.py: one request per input
// line, bytes as hex ("-" for none).  The Python side computes the same with Python integers and tests/device_link_vectors.py.
//
//   range O R                                 dlm_in_range (O 128 B: q0 r0 q1 r1_orig; R 288 B: the nine rand scalars)  -> 0 / 1
//   pi0s C0 O R                               dlm_pi0_responses                                                        -> 128 bytes
//   recombine E O R                           dlm_recombine (E 32 B: e1 ‖ e2)                                          -> m ‖ r, 64 bytes
//   pi1s C1 RR R                              dlm_pi1_responses (RR 32 B: r)                                           -> 96 bytes
//   prove G GP H COM0 COM1O O R HQ            a whole proof on the host, as csrc/devicelinkmake.hip runs it: tables of g, g' and
//                                             h built here, the fifteen walks, the eight sums, the opening checks, pi0, the
//                                             digest, m and r, lhs1 = r h, pi1; points 64 B ark-uncompressed
//                                             -> status:com1:comz:m:pi0_c:pi0_s:pi1_c:pi1_s:e
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../crescent-credentials_amd/csrc/device_link_make.hpp"

using namespace cg;
typedef std::vector<uint8_t> Bytes;

static Bytes unhex(const std::string& s) {
    if (s == "-") return Bytes();
    Bytes b(s.size() / 2);
    for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return b;
}
static std::string hex(const void* p, size_t n) {
    static const char* d = "0123456789abcdef";
    const uint8_t* b = (const uint8_t*)p;
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

// ark-serialize's uncompressed G1 on the host, for this program alone (the kernels use csrc/ark_codec.hpp): checked read
static bool g1_in(const uint32_t* w, G1Affine& p) {
    const uint32_t f = w[15] >> 30;
    if (f == 3u) return false;
    Fq x, y;
    for (int i = 0; i < 8; ++i) {
        x.l[i] = w[i];
        y.l[i] = w[8 + i];
    }
    y.l[7] &= 0x3fffffffu;
    for (const Fq* c : {&x, &y}) {
        bool below = false;
        for (int i = 7; i >= 0; --i) {
            if (c->l[i] != FqP::N[i]) {
                below = c->l[i] < FqP::N[i];
                break;
            }
        }
        if (!below) return false;
    }
    if (f == 1u) {
        p = G1Affine::inf();
        return true;
    }
    p = {to_mont(x), to_mont(y)};
    Fq three = Fq::zero();
    three.l[0] = 3;
    return sqr(p.y) == add(mul(sqr(p.x), p.x), to_mont(three));
}
// and the write, uncompressed (16 words); ml_compress_g1 makes the compressed form of it
static void g1_out(const G1Affine& p, uint32_t* w) {
    for (int i = 0; i < 16; ++i) w[i] = 0;
    if (p.is_inf()) {
        w[15] = 0x40000000u;
        return;
    }
    const Fq x = from_mont(p.x), y = from_mont(p.y), ny = from_mont(neg(p.y));
    for (int i = 0; i < 8; ++i) {
        w[i] = x.l[i];
        w[8 + i] = y.l[i];
    }
    for (int i = 7; i >= 0; --i) {
        if (ny.l[i] != y.l[i]) {
            if (ny.l[i] < y.l[i]) w[15] |= 0x80000000u;
            break;
        }
    }
}

static std::string prove(const std::vector<Bytes>& in) {
    const std::vector<uint32_t> com0 = words(in[3]), com1o = words(in[4]), open = words(in[5]), rnd = words(in[6]);
    const Bytes& hq = in[7];
    G1Affine base[3], c0p, c1p;
    std::vector<G1Affine> tab[3];
    uint8_t base_bytes[3 * 64];                                     // as a key of two inputs holds them: g, g', then h
    for (int i = 0; i < 3; ++i) {
        if (!g1_in(words(in[i]).data(), base[i])) return "ERR";
        build_tables(std::vector<G1Affine>{G1Affine::inf(), base[i]}, tab[i]);
        memcpy(base_bytes + 64 * i, in[i].data(), 64);
    }
    uint32_t com1[16] = {0}, comz[16] = {0}, m[8] = {0}, c0[8] = {0}, s0[32] = {0}, c1[8] = {0}, s1[24] = {0}, e[8] = {0};
    auto answer = [&](bool made) {
        return std::string(made ? "1:" : "2:") + hex(com1, 64) + ":" + hex(comz, 64) + ":" + hex(m, 32) + ":" + hex(c0, 32) + ":" + hex(s0, 128) + ":" +
               hex(c1, 32) + ":" + hex(s1, 96) + ":" + hex(e, 32);
    };
    // k_dlm_check
    if (!dlm_in_range(open.data(), rnd.data()) || !g1_in(com0.data(), c0p) || !g1_in(com1o.data(), c1p)) return answer(false);
    // k_dlm_terms
    G1XYZZ part[DLM_N_TERMS];
    for (uint32_t t = 0; t < DLM_N_TERMS; ++t) {
        const DlmTerm d = dlm_term(t);
        part[t] = fixed_base_mul(tab[d.base].data(), (d.from_rand ? rnd.data() : open.data()) + 8 * d.index);
    }
    // k_dlm_sum
    uint32_t pts[8 * DLM_N_POINTS] = {0};
    bool opened = true;
    for (uint32_t o = 0; o < DLM_N_OUT; ++o) {
        const G1XYZZ sum = dlm_sum(o, [&](uint32_t t) { return part[t]; });
        if (o == DLM_O_OPEN0 || o == DLM_O_OPEN1) {
            opened = opened && dlm_opens(sum, o == DLM_O_OPEN0 ? c0p : c1p);
            continue;
        }
        uint32_t unc[16];
        g1_out(to_affine(sum), unc);
        if (o == DLM_O_COM1) memcpy(com1, unc, 64);
        if (o == DLM_O_COMZ) memcpy(comz, unc, 64);
        ml_compress_g1(unc, pts + 8 * dlm_point_of(o));
    }
    if (!opened) {
        memset(com1, 0, 64);
        memset(comz, 0, 64);
        return answer(false);
    }
    // k_dlm_pi0
    uint8_t consts[DL_CONSTS_LEN];
    dl_link_consts(base_bytes, 2, 0, 1, consts);
    alignas(8) uint8_t lds[ML_STATE];
    uint32_t r[8];
    ml_compress_g1(com1o.data(), pts + 8 * DLM_P_COM1_ORIG);
    dlm_challenge(lds, consts, 0u, pts, (uint8_t*)c0);
    dlm_pi0_responses(c0, open.data(), rnd.data(), s0);
    dl_challenge_digest(lds, lds + SHA_BLOCK, c0, com0.data(), com1, comz, hq.data(), (uint32_t)hq.size(), (uint8_t*)e);
    dlm_recombine(e, open.data(), rnd.data(), m, r);
    // k_dlm_lhs1
    uint32_t unc[16];
    g1_out(to_affine(fixed_base_mul(tab[DLM_BASE_H].data(), r)), unc);
    ml_compress_g1(unc, pts + 8 * DLM_P_LHS1);
    // k_dlm_pi1
    dlm_challenge(lds, consts, 1u, pts, (uint8_t*)c1);
    dlm_pi1_responses(c1, r, rnd.data(), s1);
    return answer(true);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        std::vector<Bytes> w;
        for (std::string s; is >> s;) w.push_back(unhex(s));
        auto sizes = [&](std::initializer_list<size_t> want) {
            if (w.size() != want.size()) return false;
            size_t i = 0;
            for (size_t n : want)
                if (w[i++].size() != n) return false;
            return true;
        };
        std::string out = "ERR";
        if (cmd == "range" && sizes({128, 288})) {
            const std::vector<uint32_t> o = words(w[0]), r = words(w[1]);
            out = dlm_in_range(o.data(), r.data()) ? "1" : "0";
        } else if (cmd == "pi0s" && sizes({32, 128, 288})) {
            const std::vector<uint32_t> c = words(w[0]), o = words(w[1]), r = words(w[2]);
            std::vector<uint32_t> s(32);
            dlm_pi0_responses(c.data(), o.data(), r.data(), s.data());
            out = hex(s.data(), 128);
        } else if (cmd == "recombine" && sizes({32, 128, 288})) {
            const std::vector<uint32_t> e = words(w[0]), o = words(w[1]), r = words(w[2]);
            std::vector<uint32_t> mr(16);
            dlm_recombine(e.data(), o.data(), r.data(), mr.data(), mr.data() + 8);
            out = hex(mr.data(), 64);
        } else if (cmd == "pi1s" && sizes({32, 32, 288})) {
            const std::vector<uint32_t> c = words(w[0]), rr = words(w[1]), r = words(w[2]);
            std::vector<uint32_t> s(24);
            dlm_pi1_responses(c.data(), rr.data(), r.data(), s.data());
            out = hex(s.data(), 96);
        } else if (cmd == "prove" && w.size() == 8 && w[0].size() == 64 && w[1].size() == 64 && w[2].size() == 64 && w[3].size() == 64 &&
                   w[4].size() == 64 && w[5].size() == 128 && w[6].size() == 288 && w[7].size() <= DL_H_MAX) {
            out = prove(w);
        }
        puts(out.c_str());
        fflush(stdout);
    }
    return 0;
}
