// text_api.hip — entry points of the text readers: .chinput files (chinput.hip, chinput_kernels.hip) and the peak matrix (peaks.hip,
// peaks_kernels.hip).
#include "ctx.h"
#include "peaks.h"
#include "peaks_textkey.h"

// host-side self test of the .chinput parser (no device, no context): the three columns of up to `cap` rows
extern "C" int chicdiff_hip_selftest_chinput(const char *path, int32_t nthreads, int64_t cap, int32_t *bait, int32_t *oe, int32_t *N,
                                             int64_t *nrows, char *err, int32_t errcap) {
    if (!path || !nrows) return CHICDIFF_E_INVALID;
    ChinputCols cols;
    const int64_t n = chinput_parse(path, nthreads, cols);
    if (n < 0) {
        if (err && errcap > 0) snprintf(err, (size_t)errcap, "%s", cols.error.c_str());
        return CHICDIFF_E_INVALID;
    }
    *nrows = n;
    const size_t m = (size_t)(n < cap ? n : cap);
    if (bait) memcpy(bait, cols.bait.data(), 4 * m);
    if (oe) memcpy(oe, cols.oe.data(), 4 * m);
    if (N) memcpy(N, cols.N.data(), 4 * m);
    return CHICDIFF_OK;
}

// f2 — the text side: fread(chinput) + column pick (chicdiff.R:828, :849) with host threads (chinput.hip), then the key
// table of the count join on the device
extern "C" int chicdiff_hip_chinput_read(chicdiff_hip_ctx *c, const char *path, int32_t nthreads, int64_t *nrows_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!path || !nrows_host) return fail(c, CHICDIFF_E_INVALID, "chinput_read: bad arguments");
    if (!c->chin) c->chin = new ChinputCols();
    const int64_t n = chinput_parse(path, nthreads > 0 ? nthreads : c->host.host_copy_threads, *c->chin);
    if (n < 0) return fail(c, CHICDIFF_E_INVALID, "chinput_read: %s", c->chin->error.c_str());
    c->chin_dev_rows = -1;
    *nrows_host = n;
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_chinput_caps(int32_t *tile_bytes, int32_t *lane_bytes, int32_t *window_bytes) {
    if (tile_bytes) *tile_bytes = CHICDIFF_CHINPUT_TILE_BYTES;
    if (lane_bytes) *lane_bytes = CHICDIFF_CHINPUT_LANE_BYTES;
    if (window_bytes) *window_bytes = CHICDIFF_CHINPUT_WINDOW_BYTES;
    return CHICDIFF_OK;
}

// f2, text part on the device (chinput_kernels.hip): mark pass, scan, host stop for the row count, parse pass, host stop for the verdict.
// `what` names the entry point in messages; file_offset = the body's place in its file (what a reported offset counts from).
static int chinput_parse_impl(chicdiff_hip_ctx *c, const char *what, const uint8_t *d_text, int64_t nbytes, int ib, int io, int in,
                              int32_t *d_bait, int32_t *d_oe, int32_t *d_N, int64_t cap, bool grow_cols, int64_t file_offset,
                              int64_t *nrows_host, int64_t *bad_offset_host) {
    *nrows_host = 0;
    if (bad_offset_host) *bad_offset_host = -1;
    if (nbytes == 0) return CHICDIFF_OK;
    if (int rc = ensure_aux(c, chinput_workspace_bytes(nbytes))) return rc;
    const int64_t *d_nrows = nullptr;
    const unsigned long long *d_bad = nullptr;
    {
        Scope t(c, "chinput_mark");
        if (launch_chinput_count(d_text, nbytes, c->aux, c->stream, &d_nrows, &d_bad)) return fail(c, CHICDIFF_E_HIP, "%s: memset failed", what);
    }
    {
        Scope t(c, "chinput_scan");
        if (launch_chinput_scan(nbytes, c->aux, c->stream)) return fail(c, CHICDIFF_E_HIP, "%s: scan failed", what);
    }
    int64_t nrows = 0;
    HIPCHK(c, hipMemcpyAsync(&nrows, d_nrows, sizeof nrows, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    *nrows_host = nrows;
    if (grow_cols) {  // the context's columns: room for the rows now that their number is known
        const size_t rows = ((size_t)nrows + 63) & ~(size_t)63;
        if (int rc = grow_dev(c, (void **)&c->chin_cols, &c->chin_cols_rows, rows, 3 * sizeof(int32_t), false, CHICDIFF_E_NOMEM,
                              "%s: device columns of %lld rows for a file of %lld bytes", what, (long long)nrows, (long long)(file_offset + nbytes)))
            return rc;
        d_bait = c->chin_cols; d_oe = d_bait + c->chin_cols_rows; d_N = d_oe + c->chin_cols_rows;
        cap = nrows;
    }
    if (nrows > cap) return fail(c, CHICDIFF_E_INVALID, "%s: the text holds %lld rows, the columns have room for %lld", what, (long long)nrows, (long long)cap);
    if (nrows == 0) return CHICDIFF_OK;  // blank lines only
    {
        Scope t(c, "chinput_parse");
        launch_chinput_parse(d_text, nbytes, ib, io, in, d_bait, d_oe, d_N, cap, c->aux, c->stream);
    }
    unsigned long long bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    if (bad != ~0ull) {
        if (bad_offset_host) *bad_offset_host = (int64_t)bad;
        return fail(c, CHICDIFF_E_INVALID, "%s: %s", what, chinput_malformed((long long)bad + (long long)file_offset).c_str());
    }
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_chinput_parse_dev(chicdiff_hip_ctx *c, const uint8_t *d_text, int64_t nbytes, int32_t ib, int32_t io, int32_t in,
                                              int32_t *d_bait, int32_t *d_oe, int32_t *d_N, int64_t cap, int64_t *nrows_host,
                                              int64_t *bad_offset_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!nrows_host || nbytes < 0 || cap < 0 || (nbytes > 0 && !d_text) || (cap > 0 && (!d_bait || !d_oe || !d_N)))
        return fail(c, CHICDIFF_E_INVALID, "chinput_parse: bad arguments");
    if (ib < 0 || io < 0 || in < 0 || ib == io || ib == in || io == in)
        return fail(c, CHICDIFF_E_INVALID, "chinput_parse: columns (%d, %d, %d) must be distinct and not negative", (int)ib, (int)io, (int)in);
    if ((uintptr_t)d_text & 15) return fail(c, CHICDIFF_E_INVALID, "chinput_parse: d_text must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    const int rc = chinput_parse_impl(c, "chinput_parse", d_text, nbytes, ib, io, in, d_bait, d_oe, d_N, cap, false, 0, nrows_host, bad_offset_host);
    timing_collect(c);
    return rc;
}

// The body of an open file -> c->chin_text through the bounded pinned area (chinput_upload), both grow-only.  `what` names the entry
// point in messages, `scope` the timer.
static int upload_body(chicdiff_hip_ctx *c, const char *what, const char *scope, const ChinputFile &f) {
    const size_t body = f.size - f.body;
    if (body == 0) return CHICDIFF_OK;
    constexpr size_t kHalfMax = (size_t)64 << 20;  // the pinned area is two halves of at most 64 MiB, whatever the file's size
    const size_t half = body < kHalfMax ? ((body + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1)) : kHalfMax;
    hipError_t e = hipSuccess;
    if (int rc = grow_dev(c, (void **)&c->chin_text, &c->chin_text_bytes, align256(body), 1, true, CHICDIFF_E_NOMEM,
                          "%s: device text buffer for a file of %zu bytes", what, f.size))
        return rc;
    if (int rc = grow_pin(c, (void **)&c->chin_pin, &c->chin_pin_half, half, 2, true, CHICDIFF_E_NOMEM,
                          "%s: pinned staging of %zu bytes for a file of %zu bytes", what, 2 * half, f.size))
        return rc;
    for (hipEvent_t &ev : c->chin_ev)
        if (!ev) HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    {
        Scope t(c, scope);
        e = chinput_upload(f, c->chin_text, c->chin_pin, c->chin_pin_half, c->host.host_copy_threads, c->stream, c->chin_ev);
    }
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);  // the staging area may still be read
        timing_collect(c);
        return fail(c, CHICDIFF_E_HIP, "%s: upload: %s", what, hipGetErrorString(e));
    }
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_chinput_read_dev(chicdiff_hip_ctx *c, const char *path, int64_t *nrows_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!path || !nrows_host) return fail(c, CHICDIFF_E_INVALID, "chinput_read: bad arguments");
    ChinputFile f;
    if (chinput_open(path, f) != 0) return fail(c, CHICDIFF_E_INVALID, "chinput_read: %s", f.error.c_str());
    struct Closer { ChinputFile &f; ~Closer() { chinput_close(f); } } closer{f};
    const size_t body = f.size - f.body;
    HIPCHK(c, hipSetDevice(c->device));
    c->chin_dev_rows = -1;  // nothing to serve until this read has succeeded: an earlier read's columns are given up
    c->pk_text_bytes = -1;  // (and the text buffer no longer holds a peak matrix)
    delete c->chin;
    c->chin = nullptr;
    timing_reset(c);
    if (int rc = upload_body(c, "chinput_read", "chinput_upload", f)) return rc;
    const int rc = chinput_parse_impl(c, "chinput_read", (const uint8_t *)c->chin_text, (int64_t)body, f.ib, f.io, f.in, nullptr, nullptr, nullptr, 0,
                                      true, (int64_t)f.body, nrows_host, nullptr);
    if (rc) (void)hipStreamSynchronize(c->stream);
    timing_collect(c);
    if (rc) return rc;
    c->chin_dev_rows = *nrows_host;
    return CHICDIFF_OK;
}
extern "C" int chicdiff_hip_chinput_table_dev(chicdiff_hip_ctx *c, const uint8_t *d_bait_in_RU, int32_t max_id, int64_t *d_keys,
                                              int32_t *d_vals, int64_t *nkeys_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (c->chin_dev_rows >= 0) {  // the read that came last left its columns on the device
        if (!nkeys_host) return fail(c, CHICDIFF_E_INVALID, "chinput_table: bad arguments");
        *nkeys_host = 0;
        if (c->chin_dev_rows == 0) return CHICDIFF_OK;  // as below: a header without data rows
        const int32_t *d_b = c->chin_cols;
        return chicdiff_hip_count_table_dev(c, d_b, d_b + c->chin_cols_rows, d_b + 2 * c->chin_cols_rows, c->chin_dev_rows, d_bait_in_RU, max_id,
                                            d_keys, d_vals, nkeys_host);
    }
    if (!c->chin) return fail(c, CHICDIFF_E_INVALID, "chinput_table: nothing read (call chicdiff_hip_chinput_read first)");
    if (!nkeys_host) return fail(c, CHICDIFF_E_INVALID, "chinput_table: bad arguments");
    if (c->chin->bait.empty()) {  // a header without data rows: fread gives an empty table, merge(all.x = TRUE) then N = 0 for every RU row
        *nkeys_host = 0;
        return CHICDIFF_OK;
    }
    const size_t n = c->chin->bait.size(), col = align256(sizeof(int32_t) * n);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_io(c, 3 * col, 0);
    if (rc) return rc;
    int32_t *d_b = (int32_t *)c->io_dev, *d_o = (int32_t *)(c->io_dev + col), *d_n = (int32_t *)(c->io_dev + 2 * col);
    HIPCHK(c, hipMemcpyAsync(d_b, c->chin->bait.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_o, c->chin->oe.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_n, c->chin->N.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
    return chicdiff_hip_count_table_dev(c, d_b, d_o, d_n, (int64_t)n, d_bait_in_RU, max_id, d_keys, d_vals, nkeys_host);
}

// ---- readAndFilterPeakMatrix on the device (chicdiff.R:218-277; peaks_kernels.hip, peaks.hip) -------------------------------------------
extern "C" int chicdiff_hip_peaks_caps(int32_t *tile_bytes, int32_t *window_bytes, int32_t *max_scores, int32_t *max_slow) {
    if (tile_bytes) *tile_bytes = CHICDIFF_CHINPUT_TILE_BYTES;
    if (window_bytes) *window_bytes = CHICDIFF_CHINPUT_WINDOW_BYTES;
    if (max_scores) *max_scores = CHICDIFF_PEAKS_MAX_SCORES;
    if (max_slow) *max_slow = CHICDIFF_PEAKS_MAX_SLOW;
    return CHICDIFF_OK;
}

static void peaks_info_clear(int64_t *info, int sep, int nscore, int64_t body) {
    for (int k = 0; k < CHICDIFF_PEAKS_INFO_WORDS; k++) info[k] = 0;
    info[CHICDIFF_PEAKS_INFO_MAXBAIT] = -1;
    info[CHICDIFF_PEAKS_INFO_BAD] = -1;
    info[CHICDIFF_PEAKS_INFO_BODY] = body;
    info[CHICDIFF_PEAKS_INFO_SEP] = sep;
    info[CHICDIFF_PEAKS_INFO_NSCORE] = nscore;
}

// the context's columns of `rows` rows and nscore score columns, as one grow-only allocation
static PeaksOut peaks_ctx_out(chicdiff_hip_ctx *c, int64_t rows, int nscore) {
    PeaksOut o;
    const int64_t st = c->pk_stride;
    o.ints = (int32_t *)c->pk_buf;
    o.dist = (double *)(c->pk_buf + align256(sizeof(int32_t) * 6 * (size_t)st));
    o.scores = o.dist + st;
    o.line_off = (int64_t *)(o.scores + (size_t)nscore * (size_t)st);
    o.stride = st;
    o.cap = rows;
    return o;
}

// Mark pass, scan, quote pass; host stop for the row count; parse pass; host stop for the verdict; the slow tokens settled from
// h_body (the body in host memory; NULL: it is copied back from the device when a slow token turns up).  `grow`: the rows go to the
// context's columns, sized once their number is known; otherwise to `out` (nrows > out.cap is refused before anything is written).
static int peaks_parse_impl(chicdiff_hip_ctx *c, const char *what, const uint8_t *d_text, int64_t nbytes, const char *h_body, int sep,
                            const int32_t *score_cols, int nscore, PeaksOut out, bool grow, int64_t file_offset, int64_t *info) {
    if (nbytes == 0) return CHICDIFF_OK;
    if (int rc = ensure_aux(c, peaks_parse_workspace_bytes(nbytes) + align256(sizeof(double) * CHICDIFF_PEAKS_MAX_SLOW))) return rc;
    double *d_slow_val = (double *)(c->aux + peaks_parse_workspace_bytes(nbytes));
    const int64_t *d_nrows = nullptr;
    const unsigned long long *d_bad = nullptr;
    {
        Scope t(c, "peaks_mark");
        if (launch_chinput_count(d_text, nbytes, c->aux, c->stream, &d_nrows, &d_bad)) return fail(c, CHICDIFF_E_HIP, "%s: memset failed", what);
        if (launch_peaks_prepare(d_text, nbytes, score_cols, nscore, c->aux, c->stream)) return fail(c, CHICDIFF_E_HIP, "%s: workspace setup failed", what);
    }
    {
        Scope t(c, "peaks_scan");
        if (launch_chinput_scan(nbytes, c->aux, c->stream)) return fail(c, CHICDIFF_E_HIP, "%s: scan failed", what);
    }
    int64_t nrows = 0;
    PeaksCounters cnt;
    PeaksCounters *d_cnt = peaks_counters(c->aux, nbytes);
    HIPCHK(c, hipMemcpyAsync(&nrows, d_nrows, sizeof nrows, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    info[CHICDIFF_PEAKS_INFO_NROWS] = nrows;
    if (cnt.quote) {
        info[CHICDIFF_PEAKS_INFO_STATUS] |= CHICDIFF_PEAKS_ST_QUOTE;
        return CHICDIFF_OK;
    }
    if (nrows >= ((int64_t)1 << 31)) return fail(c, CHICDIFF_E_INVALID, "%s: %lld rows: the device reader takes fewer than 2^31", what, (long long)nrows);
    if (grow) {
        const size_t rows = ((size_t)nrows + 63) & ~(size_t)63;
        const size_t need = align256(sizeof(int32_t) * 6 * rows) + sizeof(double) * rows * (size_t)(1 + nscore) + sizeof(int64_t) * rows;
        if (int rc = grow_dev(c, (void **)&c->pk_buf, &c->pk_buf_bytes, need, 1, false, CHICDIFF_E_NOMEM,
                              "%s: device columns of %lld rows for a file of %lld bytes", what, (long long)nrows, (long long)(file_offset + nbytes)))
            return rc;
        c->pk_stride = (int64_t)rows;
        out = peaks_ctx_out(c, nrows, nscore);
    }
    if (nrows > out.cap) return fail(c, CHICDIFF_E_INVALID, "%s: the text holds %lld rows, the columns have room for %lld", what, (long long)nrows, (long long)out.cap);
    if (nrows == 0) return CHICDIFF_OK;  // blank lines only
    {
        Scope t(c, "peaks_parse");
        launch_peaks_parse(d_text, nbytes, sep, nscore, out, c->aux, c->stream);
    }
    unsigned long long bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    if (bad != ~0ull) {
        info[CHICDIFF_PEAKS_INFO_BAD] = (int64_t)bad;
        return fail(c, CHICDIFF_E_INVALID, "%s: %s", what, peaks_malformed((long long)bad + (long long)file_offset).c_str());
    }
    info[CHICDIFF_PEAKS_INFO_MAXBAIT] = cnt.maxbait;
    info[CHICDIFF_PEAKS_INFO_NSLOW] = (int64_t)cnt.nslow;
    if (cnt.nslow > (unsigned int)CHICDIFF_PEAKS_MAX_SLOW) {
        info[CHICDIFF_PEAKS_INFO_STATUS] |= CHICDIFF_PEAKS_ST_SLOW_OVERFLOW;
        return CHICDIFF_OK;
    }
    if (cnt.nslow > 0) {  // the tokens the device left undecided: strtod on the host, one kernel writes the cells
        Scope t(c, "peaks_patch");
        const size_t ns = cnt.nslow;
        std::vector<PeaksSlow> list(ns);
        std::vector<double> val(ns);
        std::vector<char> copy;
        HIPCHK(c, hipMemcpyAsync(list.data(), peaks_slow_list(c->aux, nbytes), sizeof(PeaksSlow) * ns, hipMemcpyDeviceToHost, c->stream));
        if (!h_body) {
            copy.resize((size_t)nbytes);
            HIPCHK(c, hipMemcpyAsync(copy.data(), d_text, (size_t)nbytes, hipMemcpyDeviceToHost, c->stream));
            h_body = copy.data();
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < ns; i++) {
            const int64_t off = list[i].off;
            if (off < 0 || off >= nbytes || list[i].row < 0 || list[i].row >= nrows || list[i].col < -1 || list[i].col >= nscore)
                return fail(c, CHICDIFF_E_HIP, "%s: slow-token list entry %zu out of range", what, i);
            const char *p = h_body + off;
            if (!peaks_decimal_host(p, peaks_field_end(p, h_body + nbytes, sep), &val[i]))
                return fail(c, CHICDIFF_E_HIP, "%s: the host refuses a token the device took (body offset %lld)", what, (long long)off);
        }
        HIPCHK(c, hipMemcpyAsync(d_slow_val, val.data(), sizeof(double) * ns, hipMemcpyHostToDevice, c->stream));
        launch_peaks_patch(d_slow_val, (int)ns, out, c->aux, nbytes, c->stream);
        HIPCHK(c, hipStreamSynchronize(c->stream));  // val and list leave scope
        HIPCHK(c, hipGetLastError());
    }
    return CHICDIFF_OK;
}

static int peaks_check_cols(chicdiff_hip_ctx *c, const char *what, int32_t sep, const int32_t *score_cols, int32_t nscore) {
    if (sep != '\t' && sep != ',' && sep != ' ') return fail(c, CHICDIFF_E_INVALID, "%s: the separator is a tab, a comma or a blank", what);
    if (nscore < 0 || nscore > CHICDIFF_PEAKS_MAX_SCORES || (nscore > 0 && !score_cols))
        return fail(c, CHICDIFF_E_INVALID, "%s: 0 .. %d score columns", what, CHICDIFF_PEAKS_MAX_SCORES);
    for (int j = 0; j < nscore; j++)
        if (score_cols[j] < CHICDIFF_PEAKS_KEY_COLUMNS || (j > 0 && score_cols[j] <= score_cols[j - 1]))
            return fail(c, CHICDIFF_E_INVALID, "%s: score columns are fields from %d on, ascending", what, CHICDIFF_PEAKS_KEY_COLUMNS);
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_peaks_parse_dev(chicdiff_hip_ctx *c, const uint8_t *d_text, int64_t nbytes, int32_t sep, const int32_t *score_cols,
                                            int32_t nscore, int32_t *d_ints, double *d_dist, double *d_scores, int64_t *d_line_off, int64_t cap,
                                            int64_t *info) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!info || nbytes < 0 || cap < 0 || (nbytes > 0 && !d_text) || (cap > 0 && (!d_ints || !d_dist || !d_line_off)))
        return fail(c, CHICDIFF_E_INVALID, "peaks_parse: bad arguments");
    if (int rc = peaks_check_cols(c, "peaks_parse", sep, score_cols, nscore)) return rc;
    if (cap > 0 && nscore > 0 && !d_scores) return fail(c, CHICDIFF_E_INVALID, "peaks_parse: bad arguments");
    if ((uintptr_t)d_text & 15) return fail(c, CHICDIFF_E_INVALID, "peaks_parse: d_text must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    peaks_info_clear(info, sep, nscore, 0);
    timing_reset(c);
    const PeaksOut out{d_ints, d_dist, d_scores, d_line_off, cap, cap};
    const int rc = peaks_parse_impl(c, "peaks_parse", d_text, nbytes, nullptr, sep, score_cols, nscore, out, false, 0, info);
    if (rc) (void)hipStreamSynchronize(c->stream);
    timing_collect(c);
    return rc;
}

extern "C" int chicdiff_hip_peaks_read_dev(chicdiff_hip_ctx *c, const char *path, const char *const *targets, int32_t ntargets,
                                           int32_t *score_target, int64_t *info) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!path || !info || ntargets < 0 || (ntargets > 0 && (!targets || !score_target))) return fail(c, CHICDIFF_E_INVALID, "peaks_read: bad arguments");
    c->pk_rows = -1;  // nothing to serve until this read has succeeded
    c->pk_text_bytes = -1;
    PeaksFile f;
    if (peaks_open(path, targets, ntargets, f) != 0) return fail(c, CHICDIFF_E_INVALID, "peaks_read: %s", f.error.c_str());
    struct Closer { PeaksFile &f; ~Closer() { peaks_close(f); } } closer{f};
    const size_t body = f.file.size - f.file.body;
    peaks_info_clear(info, f.sep, f.nscore, (int64_t)f.file.body);
    for (int j = 0; j < f.nscore; j++) score_target[j] = f.score_target[j];
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    if (int rc = upload_body(c, "peaks_read", "peaks_upload", f.file)) return rc;
    const int rc = peaks_parse_impl(c, "peaks_read", (const uint8_t *)c->chin_text, (int64_t)body, f.file.base + f.file.body, f.sep, f.score_col,
                                    f.nscore, PeaksOut{}, true, (int64_t)f.file.body, info);
    if (rc) (void)hipStreamSynchronize(c->stream);
    timing_collect(c);
    if (rc) return rc;
    if (info[CHICDIFF_PEAKS_INFO_STATUS] == 0) {
        c->pk_rows = info[CHICDIFF_PEAKS_INFO_NROWS];
        c->pk_nscore = f.nscore;
        c->pk_text_bytes = (int64_t)body;
        c->pk_sep = f.sep;
    }
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_peaks_columns_dev(chicdiff_hip_ctx *c, int32_t *d_ints, double *d_dist, double *d_scores, int64_t *d_line_off,
                                              int64_t cap) {
    if (!c) return CHICDIFF_E_INVALID;
    if (c->pk_rows < 0) return fail(c, CHICDIFF_E_INVALID, "peaks_columns: nothing read (call chicdiff_hip_peaks_read_dev first)");
    const int64_t n = c->pk_rows;
    if (cap < n || (n > 0 && (!d_ints || !d_dist || !d_line_off || (c->pk_nscore > 0 && !d_scores))))
        return fail(c, CHICDIFF_E_INVALID, "peaks_columns: the columns hold %lld rows, the caller's have room for %lld", (long long)n, (long long)cap);
    if (n == 0) return CHICDIFF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const PeaksOut o = peaks_ctx_out(c, n, c->pk_nscore);
    HIPCHK(c, hipMemcpy2DAsync(d_ints, sizeof(int32_t) * (size_t)cap, o.ints, sizeof(int32_t) * (size_t)o.stride, sizeof(int32_t) * (size_t)n, 6,
                               hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_dist, o.dist, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    if (c->pk_nscore > 0)
        HIPCHK(c, hipMemcpy2DAsync(d_scores, sizeof(double) * (size_t)cap, o.scores, sizeof(double) * (size_t)o.stride, sizeof(double) * (size_t)n,
                                   (size_t)c->pk_nscore, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_line_off, o.line_off, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_peaks_filter_dev(chicdiff_hip_ctx *c, const int32_t *d_bait, const int32_t *d_oe, const double *d_dist,
                                             const double *d_scores, int64_t n, int32_t nscore, double score, const int32_t *cond_of_col,
                                             int32_t ncond, int32_t replicate_rule, int64_t maxbait, int64_t *d_kept_idx, int32_t *d_kept_bait,
                                             int32_t *d_kept_oe, int32_t *d_filtered, int64_t *nkept_host, int64_t *nfiltered_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!nkept_host || !nfiltered_host || n < 0 || n >= ((int64_t)1 << 31) || nscore < 0 || nscore > CHICDIFF_PEAKS_MAX_SCORES || ncond < 0 ||
        maxbait < -1 || maxbait > 2147483647LL || (nscore > 0 && !cond_of_col) ||
        (n > 0 && (!d_bait || !d_oe || !d_dist || (nscore > 0 && !d_scores) || !d_kept_idx || !d_kept_bait || !d_kept_oe || !d_filtered)))
        return fail(c, CHICDIFF_E_INVALID, "peaks_filter: bad arguments");
    *nkept_host = *nfiltered_host = 0;
    if (n == 0) return CHICDIFF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_aux(c, peaks_filter_workspace_bytes(n, maxbait))) return rc;
    timing_reset(c);
    const int64_t *d_totals = nullptr;
    {
        Scope t(c, "peaks_filter");
        if (launch_peaks_filter(d_bait, d_oe, d_dist, d_scores, n, n, nscore, score, cond_of_col, ncond, replicate_rule, maxbait, d_kept_idx,
                                d_kept_bait, d_kept_oe, d_filtered, c->aux, c->stream, &d_totals)) {
            (void)hipStreamSynchronize(c->stream);
            return fail(c, CHICDIFF_E_HIP, "peaks_filter: %s", hipGetErrorString(hipGetLastError()));
        }
    }
    int64_t totals = 0;
    HIPCHK(c, hipMemcpyAsync(&totals, d_totals, sizeof totals, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    timing_collect(c);
    *nkept_host = totals & 0xffffffffll;
    *nfiltered_host = totals >> 32;
    return CHICDIFF_OK;
}

// ---- .multimerge on the device (chicdiff.R:218-228, 234-236; peaks_merge_kernels.hip, peaks_textkey.h) ------------------------------------
extern "C" int chicdiff_hip_peaks_textkeys_dev(chicdiff_hip_ctx *c, int64_t *d_chr, int64_t *d_name, int64_t cap, int64_t *info) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!info || cap < 0) return fail(c, CHICDIFF_E_INVALID, "peaks_textkeys: bad arguments");
    if (c->pk_rows < 0 || c->pk_text_bytes < 0)
        return fail(c, CHICDIFF_E_INVALID, "peaks_textkeys: the text buffer holds no peak matrix (call chicdiff_hip_peaks_read_dev first, and nothing else in between)");
    const int64_t n = c->pk_rows;
    if (cap < n || (n > 0 && (!d_chr || !d_name)))
        return fail(c, CHICDIFF_E_INVALID, "peaks_textkeys: the read holds %lld rows, the caller's columns have room for %lld", (long long)n, (long long)cap);
    for (int k = 0; k < CHICDIFF_PEAKS_TEXTKEYS_WORDS; k++) info[k] = 0;
    info[CHICDIFF_PEAKS_TEXTKEYS_NROWS] = n;
    if (n == 0) return CHICDIFF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_aux(c, peaks_textkeys_workspace_bytes(cap))) return rc;
    timing_reset(c);
    const PeaksOut o = peaks_ctx_out(c, n, c->pk_nscore);
    {
        Scope t(c, "peaks_textkeys");
        if (launch_peaks_textkeys((const unsigned char *)c->chin_text, c->pk_text_bytes, c->pk_sep, o.line_off, n, cap, d_chr, d_name, c->aux, c->stream))
            return fail(c, CHICDIFF_E_HIP, "peaks_textkeys: memset failed");
    }
    int flags[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(flags, peaks_textkeys_flags(c->aux), sizeof flags, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    int status = 0;
    for (int k = 0; k < 2; k++) {
        const int cls = pk_col_class(flags[k], &status);
        info[CHICDIFF_PEAKS_TEXTKEYS_CLASS_BAIT + k] = cls;
        if (cls != CHICDIFF_PEAKS_KEY_INT)  // this column's keys are its bytes
            HIPCHK(c, hipMemcpyAsync(d_chr + (size_t)k * (size_t)cap, peaks_textkeys_bytes(c->aux) + (size_t)k * (size_t)cap, sizeof(int64_t) * (size_t)n,
                                     hipMemcpyDeviceToDevice, c->stream));
    }
    info[CHICDIFF_PEAKS_TEXTKEYS_STATUS] = status;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_peaks_merge_dev(chicdiff_hip_ctx *c, int32_t nfiles, const int32_t *const *d_ints, const double *const *d_dist,
                                            const double *const *d_scores, const int64_t *const *d_chr, const int64_t *const *d_name,
                                            const int64_t *nrows, const int32_t *nscores, int64_t cap, int32_t *d_out_ints, double *d_out_dist,
                                            double *d_out_scores, int32_t *d_src_file, int64_t *d_src_row, int64_t *info) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!info || !d_ints || !d_dist || !d_scores || !d_chr || !d_name || !nrows || !nscores || cap < 0)
        return fail(c, CHICDIFF_E_INVALID, "peaks_merge: bad arguments");
    if (nfiles < 2 || nfiles > CHICDIFF_PEAKS_MERGE_MAX_FILES)
        return fail(c, CHICDIFF_E_INVALID, "peaks_merge: 2 .. %d files", CHICDIFF_PEAKS_MERGE_MAX_FILES);
    PeaksMergeFiles F;
    memset(&F, 0, sizeof F);
    F.nfiles = nfiles;
    for (int f = 0; f < nfiles; f++) {
        if (nrows[f] < 0 || nscores[f] < 0 || (nrows[f] > 0 && (!d_ints[f] || !d_dist[f] || !d_chr[f] || !d_name[f] || (nscores[f] > 0 && !d_scores[f]))))
            return fail(c, CHICDIFF_E_INVALID, "peaks_merge: bad arguments for file %d", f);
        F.off[f + 1] = F.off[f] + nrows[f];
        F.score_off[f + 1] = F.score_off[f] + nscores[f];
        if (F.off[f + 1] >= ((int64_t)1 << 31)) return fail(c, CHICDIFF_E_INVALID, "peaks_merge: the files hold 2^31 rows or more");
        if (F.score_off[f + 1] > CHICDIFF_PEAKS_MAX_SCORES)
            return fail(c, CHICDIFF_E_INVALID, "peaks_merge: more than %d score columns", CHICDIFF_PEAKS_MAX_SCORES);
        F.ints[f] = d_ints[f]; F.dist[f] = d_dist[f]; F.scores[f] = d_scores[f]; F.chr[f] = d_chr[f]; F.name[f] = d_name[f];
    }
    const int64_t N = F.off[nfiles];
    const int T = F.score_off[nfiles];
    info[CHICDIFF_PEAKS_MERGE_NOUT] = info[CHICDIFF_PEAKS_MERGE_STATUS] = 0;
    if (N == 0) return CHICDIFF_OK;
    if (cap < N || !d_out_ints || !d_out_dist || (T > 0 && !d_out_scores) || !d_src_file || !d_src_row)
        return fail(c, CHICDIFF_E_INVALID, "peaks_merge: the files hold %lld rows, the caller's columns have room for %lld", (long long)N, (long long)cap);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_aux(c, peaks_merge_workspace_bytes(N))) return rc;
    timing_reset(c);
    PeaksMergeWork k = peaks_merge_work(c->aux, N);
    int rc = 0;
    {
        Scope t(c, "peaks_merge_sort");
        rc = launch_peaks_merge_sort(F, k, c->stream);
    }
    if (!rc) {
        Scope t(c, "peaks_merge_heads");
        rc = launch_peaks_merge_heads(F, k, c->stream);
    }
    if (!rc) {
        Scope t(c, "peaks_merge_write");
        launch_peaks_merge_write(F, k, cap, d_out_ints, d_out_dist, d_out_scores, d_src_file, d_src_row, c->stream);
    }
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        return fail(c, CHICDIFF_E_HIP, "peaks_merge: %s", hipGetErrorString(hipGetLastError()));
    }
    int status = 0;
    int32_t nout = 0;
    HIPCHK(c, hipMemcpyAsync(&status, k.status, sizeof status, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&nout, k.flags + N, sizeof nout, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    timing_collect(c);
    info[CHICDIFF_PEAKS_MERGE_NOUT] = nout;
    info[CHICDIFF_PEAKS_MERGE_STATUS] = status;
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_peaks_header(const char *path, char *names, int32_t namecap, int32_t *ncols, int32_t *sep, char *err, int32_t errcap) {
    if (!path || !names || namecap <= 0 || !ncols) return CHICDIFF_E_INVALID;
    PeaksFile f;
    std::vector<std::string> cols;
    if (peaks_open_names(path, f, cols) != 0) {
        if (err && errcap > 0) snprintf(err, (size_t)errcap, "%s", f.error.c_str());
        return CHICDIFF_E_INVALID;
    }
    peaks_close(f);
    std::string joined;
    for (size_t k = 0; k < cols.size(); k++) joined += (k ? "\n" : "") + cols[k];
    *ncols = (int32_t)cols.size();
    if (sep) *sep = f.sep;
    if (joined.size() + 1 > (size_t)namecap) {
        if (err && errcap > 0) snprintf(err, (size_t)errcap, "peaks_header: the names take %zu bytes", joined.size() + 1);
        return CHICDIFF_E_INVALID;
    }
    memcpy(names, joined.c_str(), joined.size() + 1);
    return CHICDIFF_OK;
}

// the host statement of the text-key rule (peaks.hip, peaks_textkey.h): no device, no context
extern "C" int chicdiff_hip_selftest_peaks_textkeys(const char *path, int64_t cap, int64_t *chr, int64_t *name, int64_t *info, char *err,
                                                    int32_t errcap) {
    if (!path || !info || cap < 0 || (cap > 0 && (!chr || !name))) return CHICDIFF_E_INVALID;
    auto refuse = [&](const std::string &msg) {
        if (err && errcap > 0) snprintf(err, (size_t)errcap, "%s", msg.c_str());
        return CHICDIFF_E_INVALID;
    };
    PeaksFile f;
    std::vector<std::string> cols;
    if (peaks_open_names(path, f, cols) != 0) return refuse(f.error);
    struct Closer { PeaksFile &f; ~Closer() { peaks_close(f); } } closer{f};
    for (int k = 0; k < CHICDIFF_PEAKS_TEXTKEYS_WORDS; k++) info[k] = 0;
    const char *body = f.file.base + f.file.body;
    const size_t nbytes = f.file.size - f.file.body;
    long long bad = -1;
    int quote = 0, maxbait = -1;
    const int64_t nrows = peaks_parse_host(body, nbytes, f.sep, f.score_col, 0, PeaksOut{nullptr, nullptr, nullptr, nullptr, 0, 0}, &bad, &quote, &maxbait);
    info[CHICDIFF_PEAKS_TEXTKEYS_NROWS] = nrows;
    if (quote) {
        info[CHICDIFF_PEAKS_TEXTKEYS_STATUS] = CHICDIFF_PEAKS_ST_QUOTE;
        return CHICDIFF_OK;
    }
    if (bad >= 0) return refuse(peaks_malformed(bad + (long long)f.file.body));
    if (cap == 0 || nrows == 0) return CHICDIFF_OK;
    const size_t n = (size_t)nrows;
    std::vector<int32_t> vi(6 * n);
    std::vector<double> vd(n);
    std::vector<int64_t> vo(n), vc(2 * n), vn(2 * n);
    (void)peaks_parse_host(body, nbytes, f.sep, f.score_col, 0, PeaksOut{vi.data(), vd.data(), nullptr, vo.data(), nrows, nrows}, &bad, &quote, &maxbait);
    int cls[2];
    info[CHICDIFF_PEAKS_TEXTKEYS_STATUS] = peaks_textkeys_host(body, nbytes, f.sep, vo.data(), nrows, vc.data(), vn.data(), cls);
    info[CHICDIFF_PEAKS_TEXTKEYS_CLASS_BAIT] = cls[0];
    info[CHICDIFF_PEAKS_TEXTKEYS_CLASS_OE] = cls[1];
    const size_t m = (size_t)(nrows < cap ? nrows : cap);
    for (int k = 0; k < 2; k++) {
        memcpy(chr + (size_t)k * (size_t)cap, vc.data() + (size_t)k * n, 8 * m);
        memcpy(name + (size_t)k * (size_t)cap, vn.data() + (size_t)k * n, 8 * m);
    }
    return CHICDIFF_OK;
}

// the host statement of the same rule (peaks.hip): no device, no context
extern "C" int chicdiff_hip_selftest_peaks(const char *path, const char *const *targets, int32_t ntargets, double score, const int32_t *cond_of_target,
                                           int32_t ncond, int32_t replicate_rule, int64_t cap, int32_t *ints, double *dist, double *scores,
                                           int64_t *line_off, int64_t *kept_idx, int32_t *filtered, int32_t *score_target, int64_t *info, char *err,
                                           int32_t errcap) {
    if (!path || !info || ntargets < 0 || cap < 0 || (ntargets > 0 && (!targets || !cond_of_target))) return CHICDIFF_E_INVALID;
    auto refuse = [&](const std::string &msg) {
        if (err && errcap > 0) snprintf(err, (size_t)errcap, "%s", msg.c_str());
        return CHICDIFF_E_INVALID;
    };
    PeaksFile f;
    if (peaks_open(path, targets, ntargets, f) != 0) return refuse(f.error);
    struct Closer { PeaksFile &f; ~Closer() { peaks_close(f); } } closer{f};
    peaks_info_clear(info, f.sep, f.nscore, (int64_t)f.file.body);
    const char *body = f.file.base + f.file.body;
    const size_t nbytes = f.file.size - f.file.body;
    // first the count, then the rows into columns of the statement's own
    long long bad = -1;
    int quote = 0, maxbait = -1;
    const int64_t nrows = peaks_parse_host(body, nbytes, f.sep, f.score_col, f.nscore, PeaksOut{nullptr, nullptr, nullptr, nullptr, 0, 0}, &bad, &quote, &maxbait);
    info[CHICDIFF_PEAKS_INFO_NROWS] = nrows;
    if (quote) {
        info[CHICDIFF_PEAKS_INFO_STATUS] = CHICDIFF_PEAKS_ST_QUOTE;
        return CHICDIFF_OK;
    }
    if (bad >= 0) {
        info[CHICDIFF_PEAKS_INFO_BAD] = bad;
        return refuse(peaks_malformed(bad + (long long)f.file.body));
    }
    const size_t n = (size_t)nrows;
    std::vector<int32_t> vi(6 * n + 1), cond(f.nscore + 1);
    std::vector<double> vd(n + 1), vs((size_t)f.nscore * n + 1);
    std::vector<int64_t> vo(n + 1);
    (void)peaks_parse_host(body, nbytes, f.sep, f.score_col, f.nscore, PeaksOut{vi.data(), vd.data(), vs.data(), vo.data(), nrows, nrows}, &bad, &quote, &maxbait);
    info[CHICDIFF_PEAKS_INFO_MAXBAIT] = maxbait;
    for (int j = 0; j < f.nscore; j++) {
        cond[j] = cond_of_target[f.score_target[j]];
        if (score_target) score_target[j] = f.score_target[j];
    }
    std::vector<int64_t> kept;
    std::vector<int32_t> filt;
    peaks_filter_host(vi.data() + 2 * n, vi.data() + 5 * n, vd.data(), vs.data(), nrows, nrows, f.nscore, score, cond.data(), ncond, replicate_rule, kept, filt);
    info[CHICDIFF_PEAKS_INFO_NKEPT] = (int64_t)kept.size();
    info[CHICDIFF_PEAKS_INFO_NFILTERED] = (int64_t)filt.size();
    const size_t m = (size_t)(nrows < cap ? nrows : cap);
    for (int k = 0; k < 6 && ints; k++) memcpy(ints + (size_t)k * (size_t)cap, vi.data() + (size_t)k * n, 4 * m);
    if (dist) memcpy(dist, vd.data(), 8 * m);
    for (int j = 0; j < f.nscore && scores; j++) memcpy(scores + (size_t)j * (size_t)cap, vs.data() + (size_t)j * n, 8 * m);
    if (line_off) memcpy(line_off, vo.data(), 8 * m);
    if (kept_idx) memcpy(kept_idx, kept.data(), 8 * (kept.size() < (size_t)cap ? kept.size() : (size_t)cap));
    if (filtered) memcpy(filtered, filt.data(), 4 * (filt.size() < (size_t)cap ? filt.size() : (size_t)cap));
    return CHICDIFF_OK;
}
