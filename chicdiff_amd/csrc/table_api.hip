// table_api.hip — entry points of the table writer (table_text_kernels.hip, table_text.h): the text of a table of device columns, into a
// caller's device buffer or into a file.  The rule stands above chicdiff_hip_table_text_dev in include/chicdiff_hip.h.
#include <errno.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <thread>

#include "ctx.h"
#include "table_text.h"

namespace {

// the refusals of the rule; "" = none
std::string table_refusal(const chicdiff_table_column *cols, int32_t ncol, int64_t n, int32_t sep) {
    char w[256];
    if (ncol == 1)
        return "table_text: a table has 2 .. 64 columns; a one-column table is not offered (pandas writes its NaN as \"\")";
    if (!cols || ncol < 2 || ncol > CHICDIFF_TABLE_MAX_COLUMNS) {
        snprintf(w, sizeof w, "table_text: a table has 2 .. %d columns, got %d", CHICDIFF_TABLE_MAX_COLUMNS, (int)ncol);
        return w;
    }
    if (sep != '\t' && sep != ',' && sep != ' ') return "table_text: the separator is a tab, a comma or a blank";
    if (n < 0 || n >= ((int64_t)1 << 31)) return "table_text: 0 <= rows < 2^31";
    for (int j = 0; j < ncol; j++) {
        const chicdiff_table_column &c = cols[j];
        if (c.kind < CHICDIFF_COL_INT32 || c.kind > CHICDIFF_COL_DICT) {
            snprintf(w, sizeof w, "table_text: column %d: unknown kind %d", j, (int)c.kind);
            return w;
        }
        if (c.kind != CHICDIFF_COL_DICT) {
            if (n > 0 && !c.d_data) {
                snprintf(w, sizeof w, "table_text: column %d: no data", j);
                return w;
            }
            continue;
        }
        if (c.ndict < 1 || c.ndict > CHICDIFF_TABLE_MAX_DICT || !c.dict_off) {
            snprintf(w, sizeof w, "table_text: column %d: a dictionary has 1 .. %d entries, got %d", j, CHICDIFF_TABLE_MAX_DICT, (int)c.ndict);
            return w;
        }
        if (c.dict_off[0] != 0) {
            snprintf(w, sizeof w, "table_text: column %d: the dictionary's offsets start at 0", j);
            return w;
        }
        for (int e = 0; e < c.ndict; e++) {
            const int64_t a = c.dict_off[e], b = c.dict_off[e + 1];
            if (b < a || b - a > CHICDIFF_TABLE_MAX_ENTRY_BYTES || (b > a && !c.dict_bytes)) {
                snprintf(w, sizeof w, "table_text: column %d: dictionary entry %d: offsets must ascend, an entry holds at most %d bytes", j, e,
                         CHICDIFF_TABLE_MAX_ENTRY_BYTES);
                return w;
            }
            for (int64_t k = a; k < b; k++) {
                const uint8_t ch = c.dict_bytes[k];
                if (ch == (uint8_t)sep || ch == '"' || ch == '\r' || ch == '\n') {
                    snprintf(w, sizeof w, "table_text: column %d: dictionary entry %d holds the separator, a quote or a line break: it would need quoting", j, e);
                    return w;
                }
            }
        }
    }
    return "";
}

// The dictionaries of all columns as one blob (per dictionary column: ndict + 1 offsets, then the bytes, each part 16-byte aligned), and
// where every column's parts lie in it.
struct DictBlob {
    std::vector<char> bytes;
    size_t off[CHICDIFF_TABLE_MAX_COLUMNS], txt[CHICDIFF_TABLE_MAX_COLUMNS];
};

void dict_blob(const chicdiff_table_column *cols, int ncol, DictBlob &b) {
    auto pad = [&]() { b.bytes.resize((b.bytes.size() + 15) & ~(size_t)15); };
    for (int j = 0; j < ncol; j++) {
        b.off[j] = b.txt[j] = 0;
        if (cols[j].kind != CHICDIFF_COL_DICT) continue;
        const chicdiff_table_column &c = cols[j];
        b.off[j] = b.bytes.size();
        b.bytes.insert(b.bytes.end(), (const char *)c.dict_off, (const char *)(c.dict_off + c.ndict + 1));
        pad();
        b.txt[j] = b.bytes.size();
        if (c.dict_off[c.ndict] > 0) b.bytes.insert(b.bytes.end(), (const char *)c.dict_bytes, (const char *)c.dict_bytes + c.dict_off[c.ndict]);
        pad();
    }
}

// Length pass, scan and the first host stop: *total = the size of the text.  The dictionaries go to the front of c->aux, the
// workspace behind them; `t` and *ws_out are what the write pass takes.  n >= 1.
int table_len_impl(chicdiff_hip_ctx *c, const char *what, const chicdiff_table_column *cols, int ncol, int64_t n, int sep, TtCols &t, char **ws_out,
                   int64_t *total) {
    DictBlob blob;
    dict_blob(cols, ncol, blob);
    const size_t dict_bytes = align256(blob.bytes.size());
    if (int rc = ensure_aux(c, dict_bytes + table_text_workspace_bytes(n))) return rc;
    char *ws = c->aux + dict_bytes;
    *ws_out = ws;
    memset(&t, 0, sizeof t);
    t.ncol = ncol;
    t.sep = sep;
    for (int j = 0; j < ncol; j++) {
        t.col[j].kind = cols[j].kind;
        t.col[j].data = cols[j].d_data;
        if (cols[j].kind != CHICDIFF_COL_DICT) continue;
        t.col[j].ndict = cols[j].ndict;
        t.col[j].dict_off = (const int32_t *)(c->aux + blob.off[j]);
        t.col[j].dict_bytes = (const uint8_t *)(c->aux + blob.txt[j]);
    }
    if (!blob.bytes.empty()) HIPCHK(c, hipMemcpyAsync(c->aux, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, c->stream));
    const TtResult *d_res = nullptr;
    {
        Scope s(c, "table_len");
        if (launch_table_text_len(t, n, ws, c->stream, &d_res)) return fail(c, CHICDIFF_E_HIP, "%s: memset failed", what);
    }
    {
        Scope s(c, "table_scan");
        if (launch_table_text_scan(n, ws, c->stream)) return fail(c, CHICDIFF_E_HIP, "%s: scan failed", what);
    }
    TtResult res;
    HIPCHK(c, hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the blob leaves scope behind this)
    HIPCHK(c, hipGetLastError());
    if (res.bad_code) return fail(c, CHICDIFF_E_INVALID, "%s: a dictionary code is not below its column's number of entries", what);
    if (res.nbytes >= ((int64_t)1 << 40)) return fail(c, CHICDIFF_E_INVALID, "%s: the text takes %lld bytes: fewer than 2^40 are written", what, (long long)res.nbytes);
    *total = res.nbytes;
    return CHICDIFF_OK;
}

// [p, p + len) -> fd at `at`, by up to `nthreads` threads; 0, or the errno of the first failure (EIO for a write that makes no progress)
int pwrite_all(int fd, const char *p, size_t len, off_t at, int nthreads) {
    int nt = (int)(len / ((size_t)1 << 20)) + 1;  // a thread per MiB at least
    if (nt > nthreads) nt = nthreads;
    if (nt < 1) nt = 1;
    std::atomic<int> err{0};
    auto part = [&](size_t a, size_t b) {
        while (a < b && !err.load()) {
            const ssize_t w = pwrite(fd, p + a, b - a, at + (off_t)a);
            if (w < 0 && errno == EINTR) continue;
            if (w <= 0) {
                int expect = 0;
                err.compare_exchange_strong(expect, w < 0 ? errno : EIO);
                return;
            }
            a += (size_t)w;
        }
    };
    if (nt == 1) {
        part(0, len);
    } else {
        std::vector<std::thread> th;
        const size_t per = (len / (size_t)nt + 4095) & ~(size_t)4095;
        for (int k = 0; k < nt; k++) {
            const size_t a = per * (size_t)k, b = a + per < len ? a + per : len;
            if (a < b) th.emplace_back(part, a, b);
        }
        for (auto &w : th) w.join();
    }
    return err.load();
}

}  // namespace

extern "C" int chicdiff_hip_table_text_caps(int32_t *rows_per_tile, int32_t *lds_bytes, int32_t *max_columns, int32_t *max_dict) {
    if (rows_per_tile) *rows_per_tile = CHICDIFF_TABLE_ROWS_PER_TILE;
    if (lds_bytes) *lds_bytes = CHICDIFF_TABLE_LDS_BYTES;
    if (max_columns) *max_columns = CHICDIFF_TABLE_MAX_COLUMNS;
    if (max_dict) *max_dict = CHICDIFF_TABLE_MAX_DICT;
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_table_check(const chicdiff_table_column *cols, int32_t ncol, int64_t n, int32_t sep, char *err, int32_t errcap) {
    const std::string why = table_refusal(cols, ncol, n, sep);
    if (err && errcap > 0) snprintf(err, (size_t)errcap, "%s", why.c_str());
    return why.empty() ? CHICDIFF_OK : CHICDIFF_E_INVALID;
}

extern "C" int chicdiff_hip_table_text_dev(chicdiff_hip_ctx *c, const chicdiff_table_column *cols, int32_t ncol, int64_t n, int32_t sep,
                                           uint8_t *d_out, int64_t cap, int64_t *nbytes_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!nbytes_host || cap < 0 || (cap > 0 && !d_out)) return fail(c, CHICDIFF_E_INVALID, "table_text: bad arguments");
    const std::string why = table_refusal(cols, ncol, n, sep);
    if (!why.empty()) return fail(c, CHICDIFF_E_INVALID, "%s", why.c_str());
    *nbytes_host = 0;
    if (n == 0) return CHICDIFF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    timing_reset(c);
    TtCols t;
    char *ws = nullptr;
    int rc = table_len_impl(c, "table_text", cols, ncol, n, sep, t, &ws, nbytes_host);
    if (!rc && *nbytes_host <= cap) {  // otherwise: the size alone, nothing written
        {
            Scope s(c, "table_write");
            launch_table_text_write(t, n, d_out, ws, c->stream);
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipGetLastError());
    }
    if (rc) (void)hipStreamSynchronize(c->stream);
    timing_collect(c);
    return rc;
}

extern "C" int chicdiff_hip_table_write_dev(chicdiff_hip_ctx *c, const char *path, int32_t append, const uint8_t *header, int64_t header_bytes,
                                            const chicdiff_table_column *cols, int32_t ncol, int64_t n, int32_t sep, int64_t *written_host) {
    if (!c) return CHICDIFF_E_INVALID;
    if (!path || header_bytes < 0 || (header_bytes > 0 && !header)) return fail(c, CHICDIFF_E_INVALID, "table_write: bad arguments");
    const std::string why = table_refusal(cols, ncol, n, sep);
    if (!why.empty()) return fail(c, CHICDIFF_E_INVALID, "%s", why.c_str());
    if (written_host) *written_host = 0;
    // the file: created here, or an existing one truncated (append = 0) or continued (append = 1)
    bool created = true;
    int fd = open(path, O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0666);
    if (fd < 0 && errno == EEXIST) {
        created = false;
        fd = open(path, O_WRONLY | O_CLOEXEC | (append ? 0 : O_TRUNC));
    }
    if (fd < 0) return fail(c, CHICDIFF_E_INVALID, "table_write: cannot open %s: %s", path, strerror(errno));
    // every way out below goes through done(): the file is closed, and removed again if this call created it and did not finish
    auto done = [&](int rc) {
        if (fd >= 0 && close(fd) != 0 && !rc) rc = fail(c, CHICDIFF_E_INVALID, "table_write: close(%s): %s", path, strerror(errno));
        fd = -1;
        if (rc && created) (void)unlink(path);
        return rc;
    };
    off_t base = 0;
    if (append) {
        struct stat st;
        if (fstat(fd, &st) != 0) return done(fail(c, CHICDIFF_E_INVALID, "table_write: fstat(%s): %s", path, strerror(errno)));
        base = st.st_size;
    } else if (header_bytes > 0) {
        if (const int e = pwrite_all(fd, (const char *)header, (size_t)header_bytes, 0, 1))
            return done(fail(c, CHICDIFF_E_INVALID, "table_write: pwrite(%s): %s", path, strerror(e)));
        base = (off_t)header_bytes;
    }
    int64_t total = 0;
    if (n > 0) {
        hipError_t he = hipSetDevice(c->device);
        if (he != hipSuccess) return done(fail(c, CHICDIFF_E_HIP, "table_write: %s", hipGetErrorString(he)));
        timing_reset(c);
        TtCols t;
        char *ws = nullptr;
        int rc = table_len_impl(c, "table_write", cols, ncol, n, sep, t, &ws, &total);
        if (!rc)
            rc = grow_dev(c, (void **)&c->tt_text, &c->tt_text_bytes, align256((size_t)total), 1, true, CHICDIFF_E_NOMEM,
                          "table_write: device text buffer of %lld bytes", (long long)total);
        // the pinned area of chinput_read_dev, run backwards: two halves of at most 64 MiB, whatever the size of the text
        const size_t half_max = c->host.table_write_half_kib ? (size_t)c->host.table_write_half_kib << 10 : (size_t)64 << 20;
        const size_t mib = (size_t)1 << 20;
        size_t half = (size_t)total < half_max ? (((size_t)total + mib - 1) & ~(mib - 1)) : half_max;
        if (half > half_max) half = half_max;
        if (!rc)
            rc = grow_pin(c, (void **)&c->chin_pin, &c->chin_pin_half, half, 2, true, CHICDIFF_E_NOMEM,
                          "table_write: pinned staging of %zu bytes for a text of %lld bytes", 2 * half, (long long)total);
        for (hipEvent_t &ev : c->chin_ev)
            if (!rc && !ev && (he = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess)
                rc = fail(c, CHICDIFF_E_HIP, "table_write: %s", hipGetErrorString(he));
        if (rc) {
            (void)hipStreamSynchronize(c->stream);
            timing_collect(c);
            return done(rc);
        }
        {
            Scope s(c, "table_write");
            launch_table_text_write(t, n, (uint8_t *)c->tt_text, ws, c->stream);
        }
        int werr = 0;
        he = hipSuccess;
        {
            Scope s(c, "table_download");
            const size_t bytes = (size_t)total, nchunk = (bytes + half - 1) / half;
            auto issue = [&](size_t k) {  // chunk k: device -> half k & 1; its previous content (chunk k - 2) has been written by then
                const size_t off = k * half, len = bytes - off < half ? bytes - off : half;
                char *dst = c->chin_pin + (k & 1) * half;
                hipError_t e = hipMemcpyAsync(dst, c->tt_text + off, len, hipMemcpyDeviceToHost, c->stream);
                return e != hipSuccess ? e : hipEventRecord(c->chin_ev[k & 1], c->stream);
            };
            he = issue(0);
            for (size_t k = 0; k < nchunk && he == hipSuccess && !werr; k++) {
                if (k + 1 < nchunk && (he = issue(k + 1)) != hipSuccess) break;
                if ((he = hipEventSynchronize(c->chin_ev[k & 1])) != hipSuccess) break;
                const size_t off = k * half, len = bytes - off < half ? bytes - off : half;
                werr = pwrite_all(fd, c->chin_pin + (k & 1) * half, len, base + (off_t)off, c->host.host_copy_threads);
            }
        }
        const hipError_t se = hipStreamSynchronize(c->stream);  // (a DMA may still be filling the staging area after a failure)
        if (he == hipSuccess) he = se;
        if (he == hipSuccess) he = hipGetLastError();
        timing_collect(c);
        if (he != hipSuccess) return done(fail(c, CHICDIFF_E_HIP, "table_write: %s", hipGetErrorString(he)));
        if (werr) return done(fail(c, CHICDIFF_E_INVALID, "table_write: pwrite(%s): %s", path, strerror(werr)));
    }
    if (int rc = done(CHICDIFF_OK)) return rc;
    if (written_host) *written_host = (append ? 0 : header_bytes) + total;
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_selftest_format_double_dev(chicdiff_hip_ctx *c, const double *d_x, int64_t n, uint8_t *d_text, int32_t *d_len) {
    if (!c) return CHICDIFF_E_INVALID;
    if (n < 0 || (n > 0 && (!d_x || !d_text || !d_len))) return fail(c, CHICDIFF_E_INVALID, "selftest_format_double: bad arguments");
    if (n == 0) return CHICDIFF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(d_text, 0, (size_t)n * kTtMaxCell, c->stream));
    launch_format_double_selftest(d_x, n, d_text, d_len, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return CHICDIFF_OK;
}

extern "C" int chicdiff_hip_selftest_format_double(const double *x, int64_t n, uint8_t *text, int32_t *len) {
    if (n < 0 || (n > 0 && (!x || !text || !len))) return CHICDIFF_E_INVALID;
    for (int64_t i = 0; i < n; i++) {
        uint64_t bits;
        memcpy(&bits, x + i, 8);
        memset(text + i * kTtMaxCell, 0, kTtMaxCell);
        TtBufferSink sink{text + i * kTtMaxCell};
        len[i] = tt_put_double(bits, kPow10, sink, 0);
    }
    return CHICDIFF_OK;
}
