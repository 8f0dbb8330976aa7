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

// ---- device (peaks_merge_kernels.hip): .multimerge ----
// the F files of one merge, rows concatenated file-major: file f holds the rows off[f] .. off[f + 1] - 1 and the score rows
// score_off[f] .. score_off[f + 1] - 1 of the result; its matrices are contiguous with n_f = off[f + 1] - off[f] columns
struct PeaksMergeFiles {
    int nfiles;
    int64_t off[CHICDIFF_PEAKS_MERGE_MAX_FILES + 1];
    int32_t score_off[CHICDIFF_PEAKS_MERGE_MAX_FILES + 1];
    const int32_t *ints[CHICDIFF_PEAKS_MERGE_MAX_FILES];  // (6, n_f)
    const double *dist[CHICDIFF_PEAKS_MERGE_MAX_FILES];   // (n_f)
    const double *scores[CHICDIFF_PEAKS_MERGE_MAX_FILES]; // (T_f, n_f)
    const int64_t *chr[CHICDIFF_PEAKS_MERGE_MAX_FILES];   // (2, n_f): chr(baitChr), chr(oeChr)
    const int64_t *name[CHICDIFF_PEAKS_MERGE_MAX_FILES];  // (2, n_f): the hashes of baitName, oeName
};
struct PeaksMergeWork {
    int *status;         // CHICDIFF_PEAKS_ST_MERGE_* bits
    uint64_t *w, *ka, *kb;
    uint32_t *pa, *pb;   // pa: the permutation once sorted
    int32_t *flags;      // (N + 1): head flags, then their exclusive scan; flags[N] = n_out
    void *tmp;
    size_t tmp_bytes;
};
size_t peaks_textkeys_workspace_bytes(int64_t stride);
int *peaks_textkeys_flags(char *ws);
int64_t *peaks_textkeys_bytes(char *ws);
int launch_peaks_textkeys(const unsigned char *text, int64_t nbytes, int sep, const int64_t *line_off, int64_t n, int64_t stride,
                          int64_t *d_chr, int64_t *d_name, char *ws, hipStream_t st);
size_t peaks_merge_workspace_bytes(int64_t N);
PeaksMergeWork peaks_merge_work(char *ws, int64_t N);
int launch_peaks_merge_sort(const PeaksMergeFiles &F, PeaksMergeWork &k, hipStream_t st);
int launch_peaks_merge_heads(const PeaksMergeFiles &F, const PeaksMergeWork &k, hipStream_t st);
void launch_peaks_merge_write(const PeaksMergeFiles &F, const PeaksMergeWork &k, int64_t cap, int32_t *o_ints, double *o_dist, double *o_scores,
                              int32_t *o_file, int64_t *o_row, hipStream_t st);

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
// the same header rule without targets: the file mapped as above (nscore = 0) and every column name in file order
int peaks_open_names(const char *path, PeaksFile &f, std::vector<std::string> &names);
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

// the host statement of the text keys (peaks_textkey.h) for the rows whose lines start at body + line_off[r]: chr (2, n) in the form of
// each column's class, name (2, n); returns the status bits (CHICDIFF_PEAKS_ST_CHR_*), cls[2] = the columns' classes
int peaks_textkeys_host(const char *body, size_t nbytes, int sep, const int64_t *line_off, int64_t n, int64_t *chr, int64_t *name, int cls[2]);

}  // namespace cd
