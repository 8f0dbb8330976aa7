// The host half of chicdiff_amd/csrc/peaks_decimal.h on its own (tests/test_peaks.py builds and runs this): one decimal token per line
// on stdin -> "<PK_OK | PK_MALFORMED | PK_SLOW> <the double's bits in hex>" per line on stdout.
#include <stdio.h>
#include <string.h>

#include "peaks_decimal.h"

struct LineReader {
    const char *s;
    int64_t n;
    unsigned char at(int64_t p) const { return p >= 0 && p < n ? (unsigned char)s[p] : (unsigned char)'\n'; }
    bool line_end(unsigned char c, int64_t p) const { return c == '\n' || (c == '\r' && at(p + 1) == '\n'); }
};

int main() {
    static char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        int64_t n = (int64_t)strlen(line);
        if (n > 0 && line[n - 1] == '\n') n--;
        const LineReader rd{line, n};
        int64_t p = 0;
        double v;
        const int rc = cd::pk_scan_decimal(rd, p, (unsigned char)'\t', cd::kPow5, &v);
        uint64_t b;
        memcpy(&b, &v, 8);
        printf("%d %016llx\n", rc, (unsigned long long)b);
    }
    return 0;
}
