// Host-side driver of the per-row predicate of the witness check (csrc/satcheck.hpp), for tests/test_satcheck_host.py:
// reads rows "a b c" - three packed R' form operands as 64 hex digits each (most significant first), any representative
// below 2^256 - and prints for each row the verdict (1 = a·b = c mod r) and the three plain canonical values the report
// would carry.  Plain g++; the expected answers are Python integers, not this arithmetic.
#include <stdio.h>
#include <string.h>

#include "../../crescent-credentials_amd/csrc/satcheck.hpp"

using namespace cg;

static bool parse_hex(const char* s, uint32_t w[8]) {
    if (strlen(s) != 64) return false;
    for (int i = 0; i < 8; ++i) {
        uint32_t v = 0;
        for (int k = 0; k < 8; ++k) {
            const char ch = s[(7 - i) * 8 + k];
            uint32_t d;
            if (ch >= '0' && ch <= '9') d = (uint32_t)(ch - '0');
            else if (ch >= 'a' && ch <= 'f') d = (uint32_t)(ch - 'a' + 10);
            else return false;
            v = (v << 4) | d;
        }
        w[i] = v;
    }
    return true;
}
static void print_hex(const uint32_t w[8]) {
    for (int i = 7; i >= 0; --i) printf("%08x", w[i]);
}

int main() {
    char sa[80], sb[80], sc[80];
    while (scanf("%79s %79s %79s", sa, sb, sc) == 3) {
        uint32_t a[8], b[8], c[8], o[8];
        if (!parse_hex(sa, a) || !parse_hex(sb, b) || !parse_hex(sc, c)) { printf("BAD INPUT\n"); return 1; }
        printf("%d ", sat_row_ok(a, b, c) ? 1 : 0);
        sat_row_value(a, o); print_hex(o); printf(" ");
        sat_row_value(b, o); print_hex(o); printf(" ");
        sat_row_value(c, o); print_hex(o); printf("\n");
    }
    printf("DONE\n");
    return 0;
}
