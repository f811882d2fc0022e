// Host build of csrc/fq256.hpp, csrc/p256.hpp and what csrc/fp256.hpp gained for them (plain g++), driven by
// tests/test_p256_host.py: one request per input line, every 256-bit quantity as its 32 bytes BIG-endian in hex, a point as
// x ‖ y (64 bytes, the identity all zero).  The Python side computes the same with Python integers and tests/p256_vectors.py.
//
//   qadd A B | qsub A B | qmul A B        the scalar field's operation on canonical A and B, through Montgomery form -> 32 bytes
//   qinv A                                q256_inv                                                                    -> 32 bytes
//   qbelow A                              q256_below_n on any 32 bytes                                                -> 0 / 1
//   qconsts                               R^2 mod n by 512 doublings of 1 and -n^-1 mod 2^32 by search over the
//                                         defining congruence, bit by bit, equal q256_r2 and q256_ninv                -> 0 / 1
//   pinv A                                f256_inv_hd, which must equal the host-only f256_inv                        -> 32 bytes
//   pneg A                                f256_neg                                                                    -> 32 bytes
//   gadd P Q                              the general addition, P scaled to Z = 3 and Q to Z = 5                      -> 64 bytes
//   gmixed P Q                            the mixed addition, P scaled to Z = 3, Q affine (not the identity)          -> 64 bytes
//   oncurve P                             p256_read_point                                                             -> 0 / 1
//   walk K                                K·G through the table                                                       -> 64 bytes
//   chain K P                             K·P by the windowed chain                                                   -> 64 bytes
//   tabrow W                              row W of the table, canonical                                               -> 255 x 64 bytes
//   tu R D                                p256_tu_row                                                                 -> status T U
//   rtu Q SIG D                           p256_rtu_row                                                                -> status R T U
//   tufile IN OUT N | rtufile IN OUT N    N rows of 96 / 160 bytes from IN -> N x (T U | R T U) and N status bytes in OUT
//   time tu|rtu N                         N rows on one thread                                                        -> nanoseconds per row
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../crescent-credentials_amd/csrc/p256.hpp"

using namespace cg;
typedef std::vector<uint8_t> Bytes;

static Bytes unhex(const std::string& s) {
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
    return s;
}
// 32 bytes big-endian -> eight words, on their own heap block so that a sanitizer sees every read past them
static std::vector<uint32_t> words(const Bytes& b) {
    std::vector<uint32_t> w(8);
    if (b.size() == 32) p256_load_be(b.data(), w.data());
    return w;
}
static std::string be(const uint32_t* w) {
    uint8_t b[32];
    p256_store_be(w, b);
    return hex(b, 32);
}
static std::string q_out(const Q256& a) {
    uint32_t w[8];
    q256_to_words(a, w);
    return be(w);
}
static std::string f_out(const F256& a) {
    uint32_t w[8];
    f256_to_words(a, w);
    return be(w);
}
static std::string pt_out(const P256Point& p) {
    uint32_t x[8], y[8];
    p256_to_affine(p, x, y);
    return be(x) + be(y);
}
// x ‖ y -> a projective point with Z = z (the identity for 64 zero bytes); false if it is neither the identity nor on the curve
static bool pt_in(const Bytes& b, uint32_t z, const P256Curve& c, P256Point& out) {
    if (b.size() != 64) return false;
    bool zero = true;
    for (uint8_t v : b) zero = zero && v == 0;
    if (zero) {
        out = p256_identity(c);
        return true;
    }
    P256Affine a;
    if (!p256_read_point(b.data(), c, a)) return false;
    uint32_t zw[8] = {z};
    const F256 zm = f256_from_words(zw);
    out = P256Point{f256_mul(a.x, zm), f256_mul(a.y, zm), zm};
    return true;
}

int main() {
    const P256Curve c = p256_curve();
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, a, b, d;
        in >> op >> a >> b >> d;
        if (op == "qadd" || op == "qsub" || op == "qmul") {
            const std::vector<uint32_t> x = words(unhex(a)), y = words(unhex(b));
            if (!q256_below_n(x.data()) || !q256_below_n(y.data())) {
                printf("ERR\n");
                continue;
            }
            const Q256 u = q256_from_words_reduced(x.data()), v = q256_from_words_reduced(y.data());
            printf("%s\n", q_out(op == "qadd" ? q256_add(u, v) : op == "qsub" ? q256_sub(u, v) : q256_mul(u, v)).c_str());
        } else if (op == "qinv") {
            const std::vector<uint32_t> x = words(unhex(a));
            printf("%s\n", q_out(q256_inv(q256_from_words_reduced(x.data()))).c_str());
        } else if (op == "qbelow") {
            const std::vector<uint32_t> x = words(unhex(a));
            printf("%d\n", q256_below_n(x.data()) ? 1 : 0);
        } else if (op == "qconsts") {
            Q256 v = q256_zero(), want;
            v.l[0] = 1;
            for (int i = 0; i < 512; ++i) v = q256_add(v, v);          // plain residues: add does not care about the form
            for (int i = 0; i < 8; ++i) want.l[i] = q256_r2(i);
            uint32_t x = 0;                                            // n0·x = -1 mod 2^32, solved a bit at a time from below
            for (int bit = 0; bit < 32; ++bit)
                if (((q256_n(0) * x + 1u) >> bit) & 1u) x |= 1u << bit;
            printf("%d\n", q256_eq(v, want) && x == q256_ninv() && q256_n(0) * x == 0xffffffffu ? 1 : 0);
        } else if (op == "pinv" || op == "pneg") {
            const std::vector<uint32_t> x = words(unhex(a));
            if (!f256_below_p(x.data())) {
                printf("ERR\n");
                continue;
            }
            const F256 u = f256_from_words(x.data());
            if (op == "pneg") printf("%s\n", f_out(f256_neg(u)).c_str());
            else if (f256_is_zero(u)) printf("%s\n", f_out(f256_inv_hd(u)).c_str());
            else printf("%s\n", f256_eq(f256_inv_hd(u), f256_inv(u)) ? f_out(f256_inv_hd(u)).c_str() : "ERR");
        } else if (op == "gadd" || op == "gmixed") {
            P256Point p, q;
            const Bytes qb = unhex(b);
            if (!pt_in(unhex(a), 3, c, p) || !pt_in(qb, 5, c, q)) {
                printf("ERR\n");
                continue;
            }
            if (op == "gadd") {
                printf("%s\n", pt_out(p256_add(p, q, c)).c_str());
            } else {
                P256Affine qa;
                if (!p256_read_point(qb.data(), c, qa)) {
                    printf("ERR\n");
                    continue;
                }
                printf("%s\n", pt_out(p256_add_mixed(p, qa, c)).c_str());
            }
        } else if (op == "oncurve") {
            const Bytes pb = unhex(a);
            P256Affine pa;
            printf("%d\n", pb.size() == 64 && p256_read_point(pb.data(), c, pa) ? 1 : 0);
        } else if (op == "walk") {
            const std::vector<uint32_t> k = words(unhex(a));
            printf("%s\n", pt_out(p256_walk(p256_table().data(), k.data(), c)).c_str());
        } else if (op == "chain") {
            const std::vector<uint32_t> k = words(unhex(a));
            const Bytes pb = unhex(b);
            P256Affine pa;
            if (pb.size() != 64 || !p256_read_point(pb.data(), c, pa)) {
                printf("ERR\n");
                continue;
            }
            std::vector<P256Point> tab(P256_CHAIN_TABLE);
            printf("%s\n", pt_out(p256_chain(pa, k.data(), tab.data(), 1, c)).c_str());
        } else if (op == "tabrow") {
            const int w = atoi(a.c_str());
            std::string s;
            for (int e = 0; w >= 0 && w < P256_WINDOWS && e < P256_ROW; ++e) {
                const P256Affine& t = p256_table()[(size_t)w * P256_ROW + e];
                s += f_out(t.x) + f_out(t.y);
            }
            printf("%s\n", s.empty() ? "ERR" : s.c_str());
        } else if (op == "tu") {
            const Bytes r = unhex(a), dg = unhex(b);
            Bytes t(64), u(64);
            if (r.size() != 64 || dg.size() != 32) {
                printf("ERR\n");
                continue;
            }
            const int st = p256_tu_row(r.data(), dg.data(), t.data(), u.data());
            printf("%d%s%s\n", st, hex(t.data(), 64).c_str(), hex(u.data(), 64).c_str());
        } else if (op == "rtu") {
            const Bytes q = unhex(a), sig = unhex(b), dg = unhex(d);
            Bytes r(64), t(64), u(64);
            if (q.size() != 64 || sig.size() != 64 || dg.size() != 32) {
                printf("ERR\n");
                continue;
            }
            const int st = p256_rtu_row(q.data(), sig.data(), dg.data(), r.data(), t.data(), u.data());
            printf("%d%s%s%s\n", st, hex(r.data(), 64).c_str(), hex(t.data(), 64).c_str(), hex(u.data(), 64).c_str());
        } else if (op == "tufile" || op == "rtufile") {
            const bool rtu = op == "rtufile";
            const size_t n = (size_t)strtoull(d.c_str(), nullptr, 10), in_row = rtu ? 160 : 96, out_row = rtu ? 192 : 128;
            Bytes rows(in_row * n), out(out_row * n), status(n);
            FILE* f = fopen(a.c_str(), "rb");
            if (!f || fread(rows.data(), in_row, n, f) != n) {
                printf("ERR\n");
                continue;
            }
            fclose(f);
            for (size_t p = 0; p < n; ++p) {
                const uint8_t* r = &rows[in_row * p];
                uint8_t* o = &out[out_row * p];
                status[p] = rtu ? p256_rtu_row(r, r + 64, r + 128, o, o + 64, o + 128) : p256_tu_row(r, r + 64, o, o + 64);
            }
            f = fopen(b.c_str(), "wb");
            if (!f || fwrite(out.data(), out_row, n, f) != n || fwrite(status.data(), 1, n, f) != n) {
                printf("ERR\n");
                continue;
            }
            fclose(f);
            printf("%zu\n", n);
        } else if (op == "time") {
            // the NIST example's Q, signature and digest; R of the `tu` rows is what the first `rtu` row returns
            const Bytes q = unhex("b7e08afdfe94bad3f1dc8c734798ba1c62b3a0ad1e9ea2a38201cd0889bc7a193603f747959dbf7a4bb226e41928729063adc7ae43529e61b563bbc606cc5e09");
            const Bytes sig = unhex("2b42f576d07f4165ff65d1f3b1500f81e44c316f1f0b3ef57325b69aca46104fdc42c2122d6392cd3e3a993a89502a8198c1886fe69d262c4b329bdb6b63faf1");
            Bytes dg = unhex("a41a41a12a799548211c410c65d8133afde34d28bdd542e4b680cf2899c8a8c4");
            const size_t n = (size_t)strtoull(b.c_str(), nullptr, 10);
            Bytes r(64), t(64), u(64);
            (void)p256_table();
            if (p256_rtu_row(q.data(), sig.data(), dg.data(), r.data(), t.data(), u.data()) != P256_MADE) {
                printf("ERR\n");
                continue;
            }
            const Bytes r0 = r;
            volatile uint32_t sink = 0;
            const auto t0 = std::chrono::steady_clock::now();
            for (size_t p = 0; p < n; ++p) {
                if (a == "rtu") {
                    sink = sink ^ p256_rtu_row(q.data(), sig.data(), dg.data(), r.data(), t.data(), u.data());
                } else {
                    dg[31] = (uint8_t)p;                               // any digest is a valid row of compute_TU
                    sink = sink ^ p256_tu_row(r0.data(), dg.data(), t.data(), u.data()) ^ u[0];
                }
            }
            const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
            printf("%.0f\n", n ? ns / (double)n : 0.0);
        } else if (!op.empty()) {
            printf("ERR\n");
        }
    }
    return 0;
}
