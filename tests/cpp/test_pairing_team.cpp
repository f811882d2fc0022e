// Host build of csrc/pairing_team.hpp (plain g++), driven by tests/test_pairing_team_host.py: the team pairing on ONE host
// lane (nl = 1), over a shared array that checks what one lane would otherwise hide - a missing sync().  sync() counts
// phases; every slot remembers the phase and the job of its last write and of its last read; the program aborts on
//   a read of a slot written in the same phase by another job,
//   a write to a slot read or written in the same phase by another job,
//   a read of a slot nobody has written.
// One command per input line, operands and results as in tests/cpp/test_pairing.cpp (hex of canonical little-endian bytes
// in ark-serialize order).  Every result is also compared with pairing.hpp's serial function here; a difference prints
// MISMATCH instead.
//
//   miller NF MASK P0 Q0 P1 Q1 P2 Q2   pair j is live if bit j of MASK is set and neither point is the identity -> Fq12
//   fexp F                             team_final_exponentiation                  -> Fq12, or NONE for F = 0
//   f12 OP A [B]                       OP in mul cyc inv conj frob1 frob2 frob3   -> Fq12
//   eq A B / isone A                   team_equals / team_is_one                  -> 0 / 1
// `test_pairing_team toy` runs a deliberately mis-ordered sequence (a product read in the phase that writes it) and must
// die of the check.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../crescent-credentials_amd/csrc/pairing_team.hpp"

using namespace cg;

struct CheckedMem {
    Fq2 v[tp::SLOTS];
    int phase = 0;
    struct Mark { int wp = -1, wj = -1, rp = -1, rj = -1; } m[tp::SLOTS];      // rj = -2: several jobs read it this phase
    [[noreturn]] void die(const char* what, int job, int slot) const {
        fprintf(stderr, "race: %s of slot %d by job %d in phase %d (last write: phase %d job %d; last read: phase %d job %d)\n", what, slot,
                job, phase, m[slot].wp, m[slot].wj, m[slot].rp, m[slot].rj);
        abort();
    }
    Fq2 ld(int job, int slot) {
        if (slot < 0 || slot >= tp::SLOTS) die("out-of-range read", job, 0);
        Mark& k = m[slot];
        if (k.wp < 0) die("read before any write", job, slot);
        if (k.wp == phase && k.wj != job) die("read after another job's write", job, slot);
        k.rj = (k.rp == phase && k.rj != job) ? -2 : job;
        k.rp = phase;
        return v[slot];
    }
    void st(int job, int slot, const Fq2& x) {
        if (slot < 0 || slot >= tp::SLOTS) die("out-of-range write", job, 0);
        Mark& k = m[slot];
        if (k.rp == phase && k.rj != job) die("write after another job's read", job, slot);
        if (k.wp == phase && k.wj != job) die("write after another job's write", job, slot);
        k.wp = phase;
        k.wj = job;
        v[slot] = x;
    }
};
struct CheckedLane {
    static constexpr int lane = 0, nl = 1;
    CheckedMem* mem;
    void sync() const { ++mem->phase; }
};

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
static Fq12 f12_in(const std::vector<uint8_t>& b) {
    Fq12 f;
    Fq2* c[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
    for (int i = 0; i < 6; ++i) *c[i] = fq2_in(b.data() + 64 * i);
    return f;
}
static std::string f12_hex(const Fq12& f) {
    std::vector<uint8_t> o;
    for (int i = 0; i < 6; ++i) { fq_out(fq12_part(f, i).c0, o); fq_out(fq12_part(f, i).c1, o); }
    return hex(o);
}
static bool zeros(const std::vector<uint8_t>& b) {
    for (uint8_t c : b) if (c) return false;
    return true;
}
static G1Affine g1_in(const std::vector<uint8_t>& b) { return zeros(b) ? G1Affine::inf() : G1Affine{fq_in(b.data()), fq_in(b.data() + 32)}; }
static G2Affine g2_in(const std::vector<uint8_t>& b) { return zeros(b) ? G2Affine::inf() : G2Affine{fq2_in(b.data()), fq2_in(b.data() + 64)}; }

// a value into six slots as one phase of six jobs, as a kernel's lanes would write it
static void put12(CheckedLane& ln, CheckedMem& sh, int at, const Fq12& f) {
    team_phase(ln, 6, [&](int job) { sh.st(job, at + job, fq12_part(f, job)); });
}
static void say(const Fq12& team, const Fq12& serial) { printf("%s\n", team == serial ? f12_hex(team).c_str() : "MISMATCH"); }

// the check must see something: job 1 reads the product that job 0 writes in the same phase
static int toy() {
    CheckedMem sh;
    CheckedLane ln{&sh};
    team_phase(ln, 2, [&](int job) { sh.st(job, tp::T + job, Fq2::one()); });
    team_phase(ln, 2, [&](int job) {
        if (job == 0) sh.st(job, tp::T + 2, mul(sh.ld(job, tp::T), sh.ld(job, tp::T + 1)));
        else sh.st(job, tp::T + 3, dbl(sh.ld(job, tp::T + 2)));          // needs a sync() first
    });
    printf("the race check saw nothing\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "toy") return toy();
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        CheckedMem* shp = new CheckedMem();
        CheckedMem& sh = *shp;
        CheckedLane ln{&sh};
        if (cmd == "miller") {
            int nf, mask;
            in >> nf >> mask;
            MillerPairs mp;
            std::vector<EllCoeff> tabs[3];
            for (int j = 0; j < 3; ++j) {
                std::string p, q;
                in >> p >> q;
                mp.p[j] = g1_in(unhex(p));
                mp.q[j] = g2_in(unhex(q));
                mp.live[j] = ((mask >> j) & 1) && !mp.p[j].is_inf() && !mp.q[j].is_inf();
                tabs[j].resize(PairingConsts::N_COEFFS);
                if (!mp.q[j].is_inf()) g2_prepare(mp.q[j], tabs[j].data());
                mp.tab[j] = tabs[j].data();
            }
            Fq12 want;
            if (nf == 0) { team_multi_miller_loop<0>(ln, sh, mp); want = multi_miller_loop<0>(mp); }
            else if (nf == 1) { team_multi_miller_loop<1>(ln, sh, mp); want = multi_miller_loop<1>(mp); }
            else { team_multi_miller_loop<3>(ln, sh, mp); want = multi_miller_loop<3>(mp); }
            say(team_read12(ln, sh, tp::F), want);
        } else if (cmd == "fexp") {
            std::string a;
            in >> a;
            const Fq12 f = f12_in(unhex(a));
            put12(ln, sh, tp::reg(9), f);
            Fq12 want;
            const bool some = final_exponentiation(f, want);
            if (team_final_exponentiation(ln, sh) != some) printf("MISMATCH\n");
            else if (!some) printf("NONE\n");
            else say(team_read12(ln, sh, tp::reg(0)), want);
        } else if (cmd == "f12") {
            std::string op, a, b;
            in >> op >> a >> b;
            const Fq12 x = f12_in(unhex(a));
            const int ra = tp::reg(1), rb = tp::reg(2), ro = tp::reg(3);
            put12(ln, sh, ra, x);
            if (op == "mul") {
                const Fq12 y = f12_in(unhex(b));
                put12(ln, sh, rb, y);
                team_mul12(ln, sh, ro, ra, rb);
                say(team_read12(ln, sh, ro), mul(x, y));
            } else if (op == "cyc") { team_cyc_sqr(ln, sh, ro, ra); say(team_read12(ln, sh, ro), cyclotomic_sqr(x)); }
            else if (op == "inv") { team_inv12(ln, sh, ro, ra); say(team_read12(ln, sh, ro), inv(x)); }
            else if (op == "conj") { team_conj(ln, sh, ro, ra); say(team_read12(ln, sh, ro), conj(x)); }
            else if (op == "frob1" || op == "frob2" || op == "frob3") {
                const int k = op[4] - '0';
                team_frob(ln, sh, ro, ra, k);
                say(team_read12(ln, sh, ro), frob(x, k));
            } else printf("ERR\n");
        } else if (cmd == "eq") {
            std::string a, b;
            in >> a >> b;
            put12(ln, sh, tp::reg(0), f12_in(unhex(a)));
            printf("%d\n", team_equals(ln, sh, tp::reg(0), f12_in(unhex(b))) ? 1 : 0);
        } else if (cmd == "isone") {
            std::string a;
            in >> a;
            put12(ln, sh, tp::reg(0), f12_in(unhex(a)));
            printf("%d\n", team_is_one(ln, sh, tp::reg(0)) ? 1 : 0);
        } else if (!cmd.empty()) {
            printf("ERR\n");
        }
        delete shp;
        fflush(stdout);
    }
    return 0;
}
