// Host build of csrc/pairing.hpp and csrc/fixed_base.hpp (plain g++), driven by tests/test_pairing_host.py: one command per input line, every
// operand and result as hex of canonical little-endian bytes in ark-serialize order (Fq12: 384 B, G1: x ‖ y, G2:
// x.c0 ‖ x.c1 ‖ y.c0 ‖ y.c1, identity = zeros).  The Python side computes the same values with the oracle.
//
//   f12 OP A [B]            OP in mul sqr inv conj cyc frob1 frob2 frob3      -> Fq12
//   prep Q                  G2Prepared coefficients (91 x 3 Fq2)               -> 91 x 192 B
//   miller NF P0 Q0 P1 Q1 P2 Q2   pairs [0, NF) on the fly, the rest through g2_prepare tables; identity P or Q skips
//   fexp F                  final exponentiation                              -> Fq12, or NONE for F = 0
//   check P|Q KIND          KIND in g1 (on curve), g2 (on twist), sub (in G2)  -> 0 / 1
//   inputs N G0..GN X1..XN  prepare_inputs                                    -> G1
//   fb g1|g2 BASE K         csrc/fixed_base.hpp: build_tables of one base, then fixed_base_mul (K: any 32 bytes)  -> G1 / G2
//   mul254 g1|g2 BASE K     its scalar_mul_254_mixed, K < 2^254              -> G1 / G2
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../crescent-credentials_amd/csrc/fixed_base.hpp"
#include "../../crescent-credentials_amd/csrc/pairing.hpp"

using namespace cg;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> b(s.size() / 2);
    for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return b;
}
static std::string hex(const std::vector<uint8_t>& b) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (uint8_t c : b) { s += d[c >> 4]; s += d[c & 15]; }
    return s;
}
static Fq fq_in(const uint8_t* b) { Fq a; memcpy(a.l, b, 32); return to_mont(a); }
static void fq_out(const Fq& a, std::vector<uint8_t>& o) {
    Fq c = from_mont(a);
    const uint8_t* p = (const uint8_t*)c.l;
    o.insert(o.end(), p, p + 32);
}
static Fq2 fq2_in(const uint8_t* b) { return {fq_in(b), fq_in(b + 32)}; }
static void fq2_out(const Fq2& a, std::vector<uint8_t>& o) { fq_out(a.c0, o); fq_out(a.c1, o); }
static Fq12 f12_in(const std::vector<uint8_t>& b) {
    Fq12 f;
    Fq2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
    for (int i = 0; i < 6; ++i) *c[i] = fq2_in(b.data() + 64 * i);
    return f;
}
static std::vector<uint8_t> f12_out(const Fq12& f) {
    std::vector<uint8_t> o;
    const Fq2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
    for (int i = 0; i < 6; ++i) fq2_out(*c[i], o);
    return o;
}
static bool zeros(const std::vector<uint8_t>& b) {
    for (uint8_t c : b) if (c) return false;
    return true;
}
static G1Affine g1_in(const std::vector<uint8_t>& b) { return zeros(b) ? G1Affine::inf() : G1Affine{fq_in(b.data()), fq_in(b.data() + 32)}; }
static G2Affine g2_in(const std::vector<uint8_t>& b) {
    return zeros(b) ? G2Affine::inf() : G2Affine{fq2_in(b.data()), fq2_in(b.data() + 64)};
}
// the table of one base as a key builds it (the first base of build_tables takes no table), walked once
template <class F>
static XYZZ<F> fb_mul(const Affine<F>& base, const uint32_t k[8]) {
    std::vector<Affine<F>> tab;
    build_tables(std::vector<Affine<F>>{Affine<F>::inf(), base}, tab);
    return fixed_base_mul(tab.data(), k);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "f12") {
            std::string op, a, b;
            in >> op >> a >> b;
            Fq12 x = f12_in(unhex(a)), r;
            if (op == "mul") r = mul(x, f12_in(unhex(b)));
            else if (op == "sqr") r = sqr(x);
            else if (op == "inv") r = inv(x);
            else if (op == "conj") r = conj(x);
            else if (op == "cyc") r = cyclotomic_sqr(x);
            else if (op == "frob1") r = frob(x, 1);
            else if (op == "frob2") r = frob(x, 2);
            else if (op == "frob3") r = frob(x, 3);
            else { printf("ERR\n"); continue; }
            printf("%s\n", hex(f12_out(r)).c_str());
        } else if (cmd == "prep") {
            std::string q;
            in >> q;
            std::vector<EllCoeff> c(PairingConsts::N_COEFFS);
            g2_prepare(g2_in(unhex(q)), c.data());
            std::vector<uint8_t> o;
            for (auto& e : c) { fq2_out(e.c0, o); fq2_out(e.c1, o); fq2_out(e.c2, o); }
            printf("%s\n", hex(o).c_str());
        } else if (cmd == "miller") {
            int nf;
            in >> nf;
            MillerPairs mp;
            std::vector<EllCoeff> tabs[3];
            for (int j = 0; j < 3; ++j) {
                std::string p, q;
                in >> p >> q;
                mp.p[j] = g1_in(unhex(p));
                mp.q[j] = g2_in(unhex(q));
                mp.live[j] = !mp.p[j].is_inf() && !mp.q[j].is_inf();
                tabs[j].resize(PairingConsts::N_COEFFS);
                if (!mp.q[j].is_inf()) g2_prepare(mp.q[j], tabs[j].data());
                mp.tab[j] = tabs[j].data();
            }
            Fq12 f = nf == 0 ? multi_miller_loop<0>(mp) : nf == 1 ? multi_miller_loop<1>(mp) : multi_miller_loop<3>(mp);
            printf("%s\n", hex(f12_out(f)).c_str());
        } else if (cmd == "fexp") {
            std::string a;
            in >> a;
            Fq12 r;
            if (!final_exponentiation(f12_in(unhex(a)), r)) printf("NONE\n");
            else printf("%s\n", hex(f12_out(r)).c_str());
        } else if (cmd == "check") {
            std::string pt, kind;
            in >> pt >> kind;
            bool ok;
            if (kind == "g1") ok = g1_on_curve(g1_in(unhex(pt)));
            else if (kind == "g2") ok = g2_on_twist(g2_in(unhex(pt)));
            else ok = g2_in_subgroup(g2_in(unhex(pt)));
            printf("%d\n", ok ? 1 : 0);
        } else if (cmd == "inputs") {
            int n;
            in >> n;
            std::vector<G1Affine> g(n + 1);
            std::vector<Fr> x(n);
            for (int i = 0; i <= n; ++i) { std::string s; in >> s; g[i] = g1_in(unhex(s)); }
            for (int i = 0; i < n; ++i) { std::string s; in >> s; std::vector<uint8_t> b = unhex(s); memcpy(x[i].l, b.data(), 32); }
            G1Affine r = to_affine(prepare_inputs(g.data(), x.data(), n));
            std::vector<uint8_t> o;
            if (!r.is_inf()) { fq_out(r.x, o); fq_out(r.y, o); } else o.assign(64, 0);
            printf("%s\n", hex(o).c_str());
        } else if (cmd == "fb" || cmd == "mul254") {
            std::string grp, base, ks;
            in >> grp >> base >> ks;
            std::vector<uint8_t> kb = unhex(ks), o;
            uint32_t k[8];
            memcpy(k, kb.data(), 32);
            if (grp == "g1") {
                G1Affine r = to_affine(cmd == "fb" ? fb_mul(g1_in(unhex(base)), k) : scalar_mul_254_mixed(g1_in(unhex(base)), k));
                if (!r.is_inf()) { fq_out(r.x, o); fq_out(r.y, o); } else o.assign(64, 0);
            } else {
                G2Affine r = to_affine(cmd == "fb" ? fb_mul(g2_in(unhex(base)), k) : scalar_mul_254_mixed(g2_in(unhex(base)), k));
                if (!r.is_inf()) { fq2_out(r.x, o); fq2_out(r.y, o); } else o.assign(128, 0);
            }
            printf("%s\n", hex(o).c_str());
        } else if (!cmd.empty()) {
            printf("ERR\n");
        }
        fflush(stdout);
    }
    return 0;
}
