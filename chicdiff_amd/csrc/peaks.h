// peaks.h — the peak-matrix reader: what peaks_kernels.hip (device), peaks.hip (host: header, the host statement of the rule, the
// slow-token patch) and text_api.hip (entry points) share.  The rule: include/chicdiff_hip.h, above chicdiff_hip_peaks_parse_dev.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "chinput.h"
#include "common.h"

namespace cd {

// where a row goes: the int32 columns baitStart, baitEnd, baitID, oeStart, oeEnd, oeID as a (6, stride) matrix, dist, the scores as a
// (nscore, stride) matrix, the body offset of the row's line.  Every store is guarded by row < cap.
struct PeaksOut {
    int32_t *ints;
    double *dist;
    double *scores;
    int64_t *line_off;
    int64_t stride, cap;
};

struct PeaksCounters {
    int maxbait;         // -1: no row
    unsigned int nslow;  // slow tokens met (may exceed the list)
    int quote;           // the body holds a '"'
};

// a decimal token the device did not decide: its cell (col -1 = dist, else the score row) and the body offset of its first byte
struct PeaksSlow {
    int64_t row, col, off;
};

// ---- device (peaks_kernels.hip) ----
size_t peaks_parse_workspace_bytes(int64_t nbytes);
PeaksCounters *peaks_counters(char *ws, int64_t nbytes);
PeaksSlow *peaks_slow_list(char *ws, int64_t nbytes);
int launch_peaks_prepare(const unsigned char *text, int64_t nbytes, const int32_t *score_cols_host, int nscore, char *ws, hipStream_t st);
void launch_peaks_parse(const unsigned char *text, int64_t nbytes, int sep, int nscore, const PeaksOut &o, char *ws, hipStream_t st);
void launch_peaks_patch(const double *d_val, int nslow, const PeaksOut &o, char *ws, int64_t nbytes, hipStream_t st);
size_t peaks_filter_workspace_bytes(int64_t n, int64_t maxbait);
int launch_peaks_filter(const int32_t *bait, const int32_t *oe, const double *dist, const double *scores, int64_t stride, int64_t n, int nscore,
                        double score, const int32_t *cond_of_col_host, int ncond, int replicate_rule, int64_t maxbait, int64_t *kept_idx,
                        int32_t *kept_bait, int32_t *kept_oe, int32_t *filtered, char *ws, hipStream_t st, const int64_t **totals_out);

// ---- host (peaks.hip) ----
// The file mapped and its header read: file.body = the offset of the body; sep = the one separator byte; score_col[j] = the 0-based
// field of score column j (ascending), score_target[j] = which entry of `targets` names it.
struct PeaksFile {
    ChinputFile file;
    int sep = '\t';
    int nscore = 0;
    int32_t score_col[CHICDIFF_PEAKS_MAX_SCORES];
    int32_t score_target[CHICDIFF_PEAKS_MAX_SCORES];
    std::string error;
};
int peaks_open(const char *path, const char *const *targets, int ntargets, PeaksFile &f);  // 0, or -1 with f.error set (nothing stays mapped)
void peaks_close(PeaksFile &f);
std::string peaks_malformed(long long offset);
// one decimal field [p, e): empty or NA -> NaN, else the token of the rule through strtod; false = malformed
bool peaks_decimal_host(const char *p, const char *e, double *out);
// the end of the field that starts at p: the separator, or the line's end (a '\r' before the '\n' / the body's end included)
const char *peaks_field_end(const char *p, const char *body_end, int sep);
// the host statement of the parse rule, single-threaded.  Returns the row count; rows below cap are written.  *bad = the body offset
// of the first malformed line or -1; *quote = the body holds a '"' (then nothing is parsed and 0 returned).
int64_t peaks_parse_host(const char *body, size_t nbytes, int sep, const int32_t *score_col, int nscore, const PeaksOut &o, long long *bad,
                         int *quote, int *maxbait);
// the host statement of the filter: kept row indices in file order, and the baits without a kept row in order of first appearance
void peaks_filter_host(const int32_t *bait, const int32_t *oe, const double *dist, const double *scores, int64_t stride, int64_t n, int nscore,
                       double score, const int32_t *cond_of_col, int ncond, int replicate_rule, std::vector<int64_t> &kept,
                       std::vector<int32_t> &filtered);

}  // namespace cd
