// peaks.hip — reading a peak matrix (host side): the header, and a single-threaded host statement of the rule that peaks_kernels.hip
// follows on the device (chicdiff.R:218-277 readAndFilterPeakMatrix; the rule stands above chicdiff_hip_peaks_parse_dev in
// include/chicdiff_hip.h).  The host statement serves chicdiff_hip_selftest_peaks — the rule checkable without a GPU — and its
// decimal field function is the one that settles the tokens the device leaves undecided.  It is a test entry, not a product path.
#include <fcntl.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "peaks.h"
#include "peaks_textkey.h"

namespace cd {

static const char *const kPeakKeys[CHICDIFF_PEAKS_KEY_COLUMNS] = {"baitChr", "baitStart", "baitEnd", "baitID", "baitName", "oeChr",
                                                                  "oeStart", "oeEnd",     "oeID",    "oeName", "dist"};

void peaks_close(PeaksFile &f) { chinput_close(f.file); }

std::string peaks_malformed(long long offset) {
    return "malformed peak matrix row at byte offset " + std::to_string(offset) +
           " (the first 11 fields and the score columns must be present; coordinates and IDs integers, IDs not negative; dist and scores decimal, NA or empty)";
}

// the file mapped and its header read; names: every column name in file order
static int peaks_open_impl(const char *path, const char *const *targets, int ntargets, PeaksFile &f, std::vector<std::string> &names) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) { f.error = std::string("cannot open ") + path; return -1; }
    struct stat stt;
    if (fstat(fd, &stt) != 0) { close(fd); f.error = "fstat failed"; return -1; }
    const size_t size = (size_t)stt.st_size;
    if (size == 0) { close(fd); f.error = "empty file"; return -1; }
    const char *base = (const char *)mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (base == MAP_FAILED) { f.error = "mmap failed"; return -1; }
    const char *end = base + size, *p = base;
    auto line_end = [&](const char *s) { const char *q = (const char *)memchr(s, '\n', (size_t)(end - s)); return q ? q : end; };
    while (p < end && *p == '#') {  // comment lines, then the header
        const char *e = line_end(p);
        p = e < end ? e + 1 : end;
    }
    names.clear();
    int sep = ' ';
    if (p < end) {
        const char *e = line_end(p), *he = e;
        if (he > p && he[-1] == '\r') he--;
        sep = memchr(p, '\t', (size_t)(he - p)) ? '\t' : (memchr(p, ',', (size_t)(he - p)) ? ',' : ' ');
        for (const char *fs = p; fs <= he;) {
            const char *q = (const char *)memchr(fs, sep, (size_t)(he - fs));
            if (!q) q = he;
            std::string name(fs, q);
            if (name.size() >= 2 && name.front() == '"' && name.back() == '"') name = name.substr(1, name.size() - 2);
            names.push_back(name);
            if (q >= he) break;
            fs = q + 1;
        }
        p = e < end ? e + 1 : end;
    }
    auto refuse = [&](const std::string &msg) {
        munmap((void *)base, size);
        f.error = msg;
        return -1;
    };
    bool keys = names.size() >= (size_t)CHICDIFF_PEAKS_KEY_COLUMNS;
    for (int k = 0; keys && k < CHICDIFF_PEAKS_KEY_COLUMNS; k++) keys = names[k] == kPeakKeys[k];
    if (!keys)
        return refuse("peak matrix header: the first 11 columns must be baitChr, baitStart, baitEnd, baitID, baitName, oeChr, oeStart, oeEnd, oeID, oeName, dist");
    for (int t = 0; t < ntargets; t++) {
        const std::string name = targets[t];
        for (int u = 0; u < t; u++)
            if (name == targets[u]) return refuse("peak matrix: targetColumn " + name + " is named twice");
        for (int k = 0; k < CHICDIFF_PEAKS_KEY_COLUMNS; k++)
            if (name == kPeakKeys[k]) return refuse("peak matrix: targetColumn " + name + " is one of the 11 key columns");
        int found = 0;
        for (size_t k = CHICDIFF_PEAKS_KEY_COLUMNS; k < names.size(); k++) found += names[k] == name;
        if (found == 0) return refuse("All specified targetColumns must be present in the peak file(s)");
        if (found > 1) return refuse("peak matrix: targetColumn " + name + " is named twice");
    }
    if (ntargets > CHICDIFF_PEAKS_MAX_SCORES)
        return refuse("peak matrix: " + std::to_string(ntargets) + " score columns, the device reader takes " + std::to_string(CHICDIFF_PEAKS_MAX_SCORES));
    f.nscore = 0;
    for (size_t k = CHICDIFF_PEAKS_KEY_COLUMNS; k < names.size(); k++)
        for (int t = 0; t < ntargets; t++)
            if (names[k] == targets[t]) {
                f.score_col[f.nscore] = (int32_t)k;
                f.score_target[f.nscore] = t;
                f.nscore++;
            }
    f.sep = sep;
    f.file.base = base; f.file.size = size; f.file.body = (size_t)(p - base);
    return 0;
}

int peaks_open(const char *path, const char *const *targets, int ntargets, PeaksFile &f) {
    std::vector<std::string> names;
    return peaks_open_impl(path, targets, ntargets, f, names);
}

int peaks_open_names(const char *path, PeaksFile &f, std::vector<std::string> &names) { return peaks_open_impl(path, nullptr, 0, f, names); }

const char *peaks_field_end(const char *p, const char *body_end, int sep) {
    const char *q = p;
    while (q < body_end && *q != (char)sep && *q != '\n') q++;
    if ((q == body_end || *q == '\n') && q > p && q[-1] == '\r') q--;
    return q;
}

bool peaks_decimal_host(const char *p, const char *e, double *out) {
    *out = NAN;
    if (p == e || (e - p == 2 && p[0] == 'N' && p[1] == 'A')) return true;
    auto digit = [](char c) { return c >= '0' && c <= '9'; };
    const char *s = p;
    if (*s == '+' || *s == '-') s++;
    int nd = 0;
    while (s < e && digit(*s)) { s++; nd++; }
    if (s < e && *s == '.') {
        s++;
        while (s < e && digit(*s)) { s++; nd++; }
    }
    if (nd == 0) return false;
    if (s < e && (*s == 'e' || *s == 'E')) {
        s++;
        if (s < e && (*s == '+' || *s == '-')) s++;
        if (s == e || !digit(*s)) return false;
        while (s < e && digit(*s)) s++;
    }
    if (s != e) return false;
    const std::string tok(p, e);
    *out = strtod(tok.c_str(), nullptr);
    return true;
}

static bool int_field(const char *p, const char *e, bool not_negative, int32_t *out) {
    bool neg = false;
    if (p < e && (*p == '-' || *p == '+')) { neg = *p == '-'; p++; }
    if (p == e) return false;
    long long v = 0;
    for (; p < e; p++) {
        if (*p < '0' || *p > '9') return false;
        v = v * 10 + (*p - '0');
        if (v > 2147483647LL) return false;
    }
    if (neg) v = -v;
    if (not_negative && v < 0) return false;
    *out = (int32_t)v;
    return true;
}

// one line [p, e), e its end with the '\r' dropped already
static bool parse_line_host(const char *p, const char *e, int sep, const int32_t *score_col, int nscore, int64_t row, const PeaksOut &o,
                            int32_t iv[6], double *dist) {
    static const int kKind[CHICDIFF_PEAKS_KEY_COLUMNS] = {0, 1, 2, 3, 0, 0, 4, 5, 6, 0, 7};
    const int last = nscore > 0 ? score_col[nscore - 1] : CHICDIFF_PEAKS_KEY_COLUMNS - 1;
    int j = 0;
    for (int col = 0;; col++) {
        const char *q = (const char *)memchr(p, sep, (size_t)(e - p));
        if (!q) q = e;
        const int kind = col < CHICDIFF_PEAKS_KEY_COLUMNS ? kKind[col] : (j < nscore && col == score_col[j] ? 8 : 0);
        if (kind >= 1 && kind <= 6) {
            if (!int_field(p, q, kind == 3 || kind == 6, &iv[kind - 1])) return false;
        } else if (kind >= 7) {
            double v;
            if (!peaks_decimal_host(p, q, &v)) return false;
            if (kind == 7) *dist = v;
            else {
                if (row < o.cap) o.scores[(int64_t)j * o.stride + row] = v;
                j++;
            }
        }
        if (col == last) return true;
        if (q == e) return false;  // the line ends with fields missing
        p = q + 1;
    }
}

int64_t peaks_parse_host(const char *body, size_t nbytes, int sep, const int32_t *score_col, int nscore, const PeaksOut &o, long long *bad,
                         int *quote, int *maxbait) {
    *bad = -1;
    *maxbait = -1;
    *quote = nbytes > 0 && memchr(body, '"', nbytes) != nullptr;
    if (*quote) return 0;
    const char *s = body, *end = body + nbytes;
    int64_t row = 0;
    while (s < end) {
        const char *le = (const char *)memchr(s, '\n', (size_t)(end - s));
        if (!le) le = end;
        const char *ce = le;
        if (ce > s && ce[-1] == '\r') ce--;
        if (ce > s) {  // blank lines are skipped
            int32_t iv[6];
            double dist;
            if (!parse_line_host(s, ce, sep, score_col, nscore, row, o, iv, &dist)) {
                if (*bad < 0) *bad = (long long)(s - body);
            } else if (row < o.cap) {
                for (int k = 0; k < 6; k++) o.ints[(int64_t)k * o.stride + row] = iv[k];
                o.dist[row] = dist;
                o.line_off[row] = (int64_t)(s - body);
                if (iv[2] > *maxbait) *maxbait = iv[2];
            }
            row++;
        }
        s = le + 1;
    }
    return row;
}

int peaks_textkeys_host(const char *body, size_t nbytes, int sep, const int64_t *line_off, int64_t n, int64_t *chr, int64_t *name, int cls[2]) {
    int flags[2] = {0, 0};
    std::vector<int64_t> as_int(2 * (size_t)n), as_text(2 * (size_t)n);
    const char *end = body + nbytes;
    for (int64_t r = 0; r < n; r++) {
        const char *p = body + line_off[r];
        for (int field = 0; field < 10; field++) {
            const char *e = peaks_field_end(p, end, sep);
            if (field == 0 || field == 5) {
                PkChrToken tok;
                for (const char *q = p; q < e; q++) tok.feed((unsigned char)*q);
                const size_t at = (field == 5 ? (size_t)n : 0) + (size_t)r;
                flags[field == 5] |= pk_col_flags(tok);
                as_int[at] = tok.value;
                as_text[at] = pk_text_key(tok.packed);
            } else if (field == 4 || field == 9) {
                uint64_t h = kPkFnvBasis;
                for (const char *q = p; q < e; q++) h = pk_fnv_step(h, (unsigned char)*q);
                name[(field == 9 ? (size_t)n : 0) + (size_t)r] = (int64_t)h;
            }
            p = e < end && *e == (char)sep ? e + 1 : e;
        }
    }
    int status = 0;
    for (int k = 0; k < 2; k++) {
        cls[k] = pk_col_class(flags[k], &status);
        const std::vector<int64_t> &from = cls[k] == CHICDIFF_PEAKS_KEY_INT ? as_int : as_text;
        for (int64_t r = 0; r < n; r++) chr[(size_t)k * (size_t)n + (size_t)r] = from[(size_t)k * (size_t)n + (size_t)r];
    }
    return status;
}

void peaks_filter_host(const int32_t *bait, const int32_t *oe, const double *dist, const double *scores, int64_t stride, int64_t n, int nscore,
                       double score, const int32_t *cond_of_col, int ncond, int replicate_rule, std::vector<int64_t> &kept,
                       std::vector<int32_t> &filtered) {
    kept.clear();
    filtered.clear();
    std::vector<int32_t> order;                  // baits in order of first appearance
    std::unordered_map<int32_t, bool> has_kept;  // per bait seen so far
    for (int64_t r = 0; r < n; r++) {
        bool keep = false;
        for (int j = 0; j < nscore; j++) keep = keep || scores[(int64_t)j * stride + r] > score;
        if (keep && replicate_rule)
            for (int c = 0; c < ncond && keep; c++) {
                int cnt = 0;
                for (int j = 0; j < nscore; j++) cnt += cond_of_col[j] == c && !isnan(scores[(int64_t)j * stride + r]);
                keep = cnt >= 2;
            }
        const int64_t b = bait[r], o = oe[r];
        keep = keep && !isnan(dist[r]) && o != b + 1 && o != b - 1;
        auto it = has_kept.find((int32_t)b);
        if (it == has_kept.end()) {
            it = has_kept.emplace((int32_t)b, false).first;
            order.push_back((int32_t)b);
        }
        if (keep) {
            it->second = true;
            kept.push_back(r);
        }
    }
    for (int32_t b : order)
        if (!has_kept[b]) filtered.push_back(b);
}

}  // namespace cd
