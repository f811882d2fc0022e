// Host build of csrc/ft256.hpp and csrc/t256.hpp (plain g++), driven by tests/test_t256_host.py: one request per input line.
// A field element is its 32 bytes BIG-endian in hex, a point x ‖ y (64 bytes, the identity all zero), a scalar its 32 bytes
// LITTLE-endian in hex - the forms of include/crescent_gpu.h.  The Python side computes the same with Python integers and
// tests/t256_vectors.py.
//
//   fadd A B | fsub A B | fmul A B        the field's operation on canonical A and B, through Montgomery form   -> 32 bytes
//   fneg A | finv A | fsqr A              ft256_neg, ft256_inv (zero gives zero), ft256_sqr                      -> 32 bytes
//   fbelow A                              ft256_below_p on any 32 bytes                                          -> 0 / 1
//   fconsts                               R^2 mod p_T by 512 doublings of 1 and -p_T^-1 mod 2^32 by search over the defining
//                                         congruence, bit by bit, equal ft256_r2 and ft256_pinv (0x0f646959)     -> 0 / 1
//   gadd P Q                              the general addition, P scaled to Z = 3 and Q to Z = 5                 -> 64 bytes
//   gmixed P Q                            the mixed addition, P scaled to Z = 3, Q affine (not the identity)     -> 64 bytes
//   gdbl P                                t256_double, P scaled to Z = 7                                         -> 64 bytes
//   read P                                t256_read_point's code: 0 on the curve, 1 not canonical, 2 off the curve, 3 identity
//   compress P                            t256_write_compressed, P scaled to Z = 3                               -> 33 bytes
//   walk P K                              K·P through P's table by t256_walk_share (n_gens = 1, a zero blind over the same
//                                         table)                                                                 -> 64 bytes
//   tabrow P W                            row W of P's table, canonical                                          -> 255 x 64 bytes
//   gens N G_XY H_XY                      t256_read_gens on N points and h: "code:which"
//   row N G_XY H_XY SCALARS BLIND         t256_commit_row over the tables of the N + 1 points (kept per distinct set)
//                                                                                                                -> status, 33 bytes
//   time N ROWS uniform|mix               ROWS rows over N generators on one thread, scalars uniform or 56/34/10 % zero / one /
//                                         uniform (bench.py's wire mix)                                          -> nanoseconds per row
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../crescent-credentials_amd/csrc/t256.hpp"

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
    if (b.size() == 32) t256_load_be(b.data(), w.data());
    return w;
}
static std::string be(const uint32_t* w) {
    uint8_t b[32];
    t256_store_be(w, b);
    return hex(b, 32);
}
static std::string f_out(const FT256& a) {
    uint32_t w[8];
    ft256_to_words(a, w);
    return be(w);
}
static std::string pt_out(const T256Point& p) {
    uint8_t b[64];
    t256_write_uncompressed(p, ft256_inv(p.z), b);
    return hex(b, 64);
}
// x ‖ y -> a projective point with Z = z (the identity for 64 zero bytes); false if it is neither the identity nor on the curve
static bool pt_in(const Bytes& b, uint32_t z, const T256Curve& c, T256Point& out) {
    if (b.size() != 64) return false;
    T256Affine a;
    const int rc = t256_read_point(b.data(), c, a);
    if (rc == T256_GENS_IDENTITY) {
        out = t256_identity(c);
        return true;
    }
    if (rc != T256_GENS_OK) return false;
    uint32_t zw[8] = {z};
    const FT256 zm = ft256_from_words(zw);
    out = T256Point{ft256_mul(a.x, zm), ft256_mul(a.y, zm), zm};
    return true;
}
// the tables of a set of points, built once per distinct set
static const std::vector<T256Affine>* tables_of(const Bytes& g_xy, const Bytes& h_xy, uint64_t n) {
    static std::map<std::string, std::vector<T256Affine>> kept;
    const std::string key = hex(g_xy.data(), g_xy.size()) + hex(h_xy.data(), h_xy.size());
    auto it = kept.find(key);
    if (it != kept.end()) return &it->second;
    std::vector<T256Affine> pts;
    uint64_t which = 0;
    if (g_xy.size() != 64 * n || h_xy.size() != 64 || t256_read_gens(g_xy.data(), n, h_xy.data(), pts, &which) != T256_GENS_OK) return nullptr;
    std::vector<T256Affine>& tab = kept[key];
    tab.resize((n + 1) * (size_t)T256_TABLE_POINTS);
    for (uint64_t j = 0; j <= n; ++j) t256_make_table(pts[j], &tab[j * T256_TABLE_POINTS]);
    return &tab;
}

int main() {
    const T256Curve c = t256_curve();
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, a, b, d, e, f;
        in >> op >> a >> b >> d >> e >> f;
        if (op == "fadd" || op == "fsub" || op == "fmul") {
            const std::vector<uint32_t> x = words(unhex(a)), y = words(unhex(b));
            if (!ft256_below_p(x.data()) || !ft256_below_p(y.data())) {
                printf("ERR\n");
                continue;
            }
            const FT256 u = ft256_from_words(x.data()), v = ft256_from_words(y.data());
            printf("%s\n", f_out(op == "fadd" ? ft256_add(u, v) : op == "fsub" ? ft256_sub(u, v) : ft256_mul(u, v)).c_str());
        } else if (op == "fneg" || op == "finv" || op == "fsqr") {
            const std::vector<uint32_t> x = words(unhex(a));
            if (!ft256_below_p(x.data())) {
                printf("ERR\n");
                continue;
            }
            const FT256 u = ft256_from_words(x.data());
            printf("%s\n", f_out(op == "fneg" ? ft256_neg(u) : op == "finv" ? ft256_inv(u) : ft256_sqr(u)).c_str());
        } else if (op == "fbelow") {
            const std::vector<uint32_t> x = words(unhex(a));
            printf("%d\n", ft256_below_p(x.data()) ? 1 : 0);
        } else if (op == "fconsts") {
            FT256 v = ft256_zero(), want;
            v.l[0] = 1;
            for (int i = 0; i < 512; ++i) v = ft256_add(v, v);         // plain residues: add does not care about the form
            for (int i = 0; i < 8; ++i) want.l[i] = ft256_r2(i);
            uint32_t x = 0;                                            // p0·x = -1 mod 2^32, solved a bit at a time from below
            for (int bit = 0; bit < 32; ++bit)
                if (((ft256_p(0) * x + 1u) >> bit) & 1u) x |= 1u << bit;
            printf("%d\n", ft256_eq(v, want) && x == ft256_pinv() && x == 0x0f646959u && ft256_p(0) * x == 0xffffffffu ? 1 : 0);
        } else if (op == "gadd" || op == "gmixed") {
            T256Point p, q;
            const Bytes qb = unhex(b);
            if (!pt_in(unhex(a), 3, c, p) || !pt_in(qb, 5, c, q)) {
                printf("ERR\n");
                continue;
            }
            if (op == "gadd") {
                printf("%s\n", pt_out(t256_add(p, q, c)).c_str());
            } else {
                T256Affine qa;
                if (t256_read_point(qb.data(), c, qa) != T256_GENS_OK) {
                    printf("ERR\n");
                    continue;
                }
                printf("%s\n", pt_out(t256_add_mixed(p, qa, c)).c_str());
            }
        } else if (op == "gdbl") {
            T256Point p;
            if (!pt_in(unhex(a), 7, c, p)) {
                printf("ERR\n");
                continue;
            }
            printf("%s\n", pt_out(t256_double(p, c)).c_str());
        } else if (op == "read") {
            const Bytes pb = unhex(a);
            T256Affine pa;
            if (pb.size() != 64) printf("ERR\n");
            else printf("%d\n", t256_read_point(pb.data(), c, pa));
        } else if (op == "compress") {
            T256Point p;
            uint8_t out[T256_COMPRESSED];
            if (!pt_in(unhex(a), 3, c, p)) {
                printf("ERR\n");
                continue;
            }
            t256_write_compressed(p, ft256_inv(p.z), out);
            printf("%s\n", hex(out, sizeof(out)).c_str());
        } else if (op == "walk" || op == "tabrow") {
            const Bytes pb = unhex(a);
            const std::vector<T256Affine>* tab = tables_of(pb, pb, 1);
            if (!tab) {
                printf("ERR\n");
                continue;
            }
            if (op == "walk") {
                const Bytes kb = unhex(b);
                std::vector<uint32_t> k(8), zero(8);
                if (kb.size() != 32) {
                    printf("ERR\n");
                    continue;
                }
                t256_load_scalar(kb.data(), k.data());
                printf("%s\n", pt_out(t256_walk_share(tab->data(), k.data(), zero.data(), 1, 0, 0, c)).c_str());
            } else {
                const int w = atoi(b.c_str());
                std::string s;
                for (int i = 0; w >= 0 && w < T256_WINDOWS && i < T256_ROW; ++i) {
                    const T256Affine& t = (*tab)[(size_t)w * T256_ROW + i];
                    s += f_out(t.x) + f_out(t.y);
                }
                printf("%s\n", s.empty() ? "ERR" : s.c_str());
            }
        } else if (op == "gens") {
            const uint64_t n = strtoull(a.c_str(), nullptr, 10);
            const Bytes g = unhex(b), h = unhex(d);
            std::vector<T256Affine> pts;
            uint64_t which = 0;
            if (!n || g.size() != 64 * n || h.size() != 64) {
                printf("ERR\n");
                continue;
            }
            const int rc = t256_read_gens(g.data(), n, h.data(), pts, &which);
            printf("%d:%llu\n", rc, (unsigned long long)which);
        } else if (op == "row") {
            const uint64_t n = strtoull(a.c_str(), nullptr, 10);
            const Bytes g = unhex(b), h = unhex(d), s = unhex(e), bl = unhex(f);
            const std::vector<T256Affine>* tab = n ? tables_of(g, h, n) : nullptr;
            if (!tab || s.size() != 32 * n || bl.size() != 32) {
                printf("ERR\n");
                continue;
            }
            Bytes out(T256_COMPRESSED);
            const int st = t256_commit_row(tab->data(), n, s.data(), bl.data(), out.data());
            printf("%d%s\n", st, hex(out.data(), out.size()).c_str());
        } else if (op == "time") {
            const uint64_t n = strtoull(a.c_str(), nullptr, 10), rows = strtoull(b.c_str(), nullptr, 10);
            if (!n || !rows) {
                printf("ERR\n");
                continue;
            }
            // generators: multiples of G by the walk itself; the scalars by a 64-bit LCG, top byte cleared (below q)
            uint64_t lcg = 0x256256256ull;
            auto next = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(lcg >> 32); };
            Bytes gxy(64), g_all(64 * n), h_xy(64);
            const T256Point gp = t256_from_affine(t256_generator(), c);
            t256_write_uncompressed(gp, c.one, gxy.data());
            const std::vector<T256Affine>* gt = tables_of(gxy, gxy, 1);
            std::vector<uint32_t> k(8), zero(8);
            for (uint64_t j = 0; j <= n; ++j) {
                for (int i = 0; i < 8; ++i) k[i] = next();
                k[7] &= 0x00ffffffu;
                k[0] |= 1u;
                const T256Point p = t256_walk_share(gt->data(), k.data(), zero.data(), 1, 0, 0, c);
                t256_write_uncompressed(p, ft256_inv(p.z), j < n ? &g_all[64 * j] : h_xy.data());
            }
            const std::vector<T256Affine>* tab = tables_of(g_all, h_xy, n);
            if (!tab) {
                printf("ERR\n");
                continue;
            }
            Bytes s(32 * n * rows), bl(32 * rows), out(T256_COMPRESSED);
            for (uint64_t i = 0; i < n * rows; ++i) {
                const uint32_t u = next() % 100u;
                const bool uniform = d != "mix" || u >= 90;
                for (int j = 0; j < 31; ++j) s[32 * i + j] = uniform ? (uint8_t)next() : 0;
                if (!uniform) s[32 * i] = u < 56 ? 0 : 1;
            }
            for (uint64_t i = 0; i < rows; ++i)
                for (int j = 0; j < 31; ++j) bl[32 * i + j] = (uint8_t)next();
            volatile uint32_t sink = 0;
            const auto t0 = std::chrono::steady_clock::now();
            for (uint64_t r = 0; r < rows; ++r) sink = sink ^ t256_commit_row(tab->data(), n, &s[32 * n * r], &bl[32 * r], out.data()) ^ out[1];
            const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
            printf("%.0f\n", ns / (double)rows);
        } else if (!op.empty()) {
            printf("ERR\n");
        }
    }
    return 0;
}
