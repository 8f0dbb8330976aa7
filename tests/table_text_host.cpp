// The host half of chicdiff_amd/csrc/table_text.h on its own (tests/test_table_text.py builds and runs this, once more under the address
// and undefined-behaviour sanitisers): 8-byte words on stdin -> one cell per line on stdout.  argv[1] = "double": the words are bit
// patterns of doubles; "int": they are int64 values.  Every cell is written into the middle of a guarded buffer: a byte outside
// [0, length) or a length that differs from tt_double_len / tt_int_len ends the run with status 2.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "table_text.h"

int main(int argc, char **argv) {
    const bool ints = argc > 1 && strcmp(argv[1], "int") == 0;
    std::vector<uint64_t> in;
    uint64_t chunk[4096];
    size_t got;
    while ((got = fread(chunk, 8, 4096, stdin)) > 0) in.insert(in.end(), chunk, chunk + got);
    std::vector<char> out;
    out.reserve(in.size() * 20);
    constexpr int kGuard = 8;
    unsigned char cell[cd::kTtMaxCell + 2 * kGuard];
    for (uint64_t w : in) {
        memset(cell, 0xee, sizeof cell);
        cd::TtBufferSink sink{cell + kGuard};
        const int want = ints ? cd::tt_int_len((int64_t)w) : cd::tt_double_len(w, cd::kPow10);
        const int len = ints ? cd::tt_put_int((int64_t)w, sink, 0) : cd::tt_put_double(w, cd::kPow10, sink, 0);
        bool ok = len == want && len >= 0 && len <= cd::kTtMaxCell;
        for (int i = 0; ok && i < (int)sizeof cell; i++) {
            const bool inside = i >= kGuard && i < kGuard + len;
            if ((cell[i] != 0xee) != inside) ok = false;
        }
        if (!ok) {
            fprintf(stderr, "table_text_host: word %016llx: length %d, expected %d, or a byte outside the cell\n", (unsigned long long)w, len, want);
            return 2;
        }
        out.insert(out.end(), cell + kGuard, cell + kGuard + len);
        out.push_back('\n');
    }
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
