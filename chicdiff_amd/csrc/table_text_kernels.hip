// table_text_kernels.hip — a table of device columns -> its text, what DataFrame.to_csv(index = False) writes, byte for byte.  The rule is
// stated above chicdiff_hip_table_text_dev in include/chicdiff_hip.h; table_text.h forms the cells.  gfx950 only.
//
//   table_text_len_kernel    one lane per row, 256 rows per workgroup (a tile): the lane visits every column, adds the cell lengths and
//                            the ncol separator / newline bytes, keeps the row's byte count (4 bytes per row) and the workgroup
//                            writes its tile's total
//   rocprim::exclusive_scan  of the tile totals: every tile's first byte, and behind the last tile the size of the text
//   table_text_write_kernel  the same tile: scans the lanes' row lengths inside the workgroup, every lane formats its row into LDS
//                            at its offset, and the workgroup stores the tile's bytes as one contiguous run: 16-byte stores between a
//                            byte head and a byte tail.  The LDS image is shifted by the low four bits of the run's global address, so
//                            the 16-byte LDS reads and global stores are both aligned.  A tile whose text exceeds the LDS buffer goes
//                            through it in consecutive chunks (a lane formats its row again for every chunk the row reaches into).
//
// The digits are derived twice, once per pass; the row lengths are the only record pass 1 leaves (DESIGN.md §1 says what a per-cell
// record would cost instead).  The table of powers of ten (pow10_table.h, 617 x 16 bytes) is indexed by each lane's own exponent, so it
// cannot come through the scalar cache; it is read from global memory through the vector cache (10 KB: it stays in L2 and the CU's
// cache) and not copied to LDS, which the text buffer is given to.  The column descriptors are one kernel argument, the same for all
// lanes: scalar loads.  Placement comes from the two scans alone, no value passes through an atomic (the one atomic raises the
// "code out of range" flag), and no kernel here takes a lock or polls.
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "table_text.h"

namespace cd {

namespace {

constexpr int kTtRows = CHICDIFF_TABLE_ROWS_PER_TILE;
constexpr int kTtBuf = CHICDIFF_TABLE_LDS_BYTES;
static_assert(kTtRows == 256, "the kernels below run one row per lane of a 256-lane workgroup");
static_assert(kTtBuf % 16 == 0 && 2 * (kTtBuf + 4096) <= 160 * 1024, "two workgroups stay resident on a CU's 160 KiB of LDS");
static_assert(kTtMaxCell == CHICDIFF_TABLE_MAX_CELL_BYTES, "table_text.h and the public header name one cell size");
// the most bytes of one tile: every column a dictionary entry of the largest size (fits the int offsets below)
static_assert((int64_t)kTtRows * CHICDIFF_TABLE_MAX_COLUMNS * (CHICDIFF_TABLE_MAX_ENTRY_BYTES + 1) < ((int64_t)1 << 31), "tile offsets are ints");

// the window [lo, hi) of the tile's bytes that is in LDS now; buf[shift + p - lo] holds byte p
struct TtLdsSink {
    unsigned char *buf;
    int lo, hi, shift;
    __device__ __forceinline__ void put(int p, unsigned char c) {
        if (p >= lo && p < hi) buf[p - lo + shift] = c;
    }
};

__device__ __forceinline__ int tt_dict_code(const TtCol &c, int64_t r) { return c.data ? ((const int32_t *)c.data)[r] : 0; }

__device__ __forceinline__ int tt_cell_len(const TtCol &c, int64_t r, int *bad) {
    switch (c.kind) {
    case CHICDIFF_COL_INT32: return tt_int_len(((const int32_t *)c.data)[r]);
    case CHICDIFF_COL_INT64: return tt_int_len(((const int64_t *)c.data)[r]);
    case CHICDIFF_COL_FLOAT64: return tt_double_len(((const uint64_t *)c.data)[r], kPow10);
    default: {
        const int code = tt_dict_code(c, r);
        if (code < 0) return 0;
        if (code >= c.ndict) {
            *bad = 1;
            return 0;
        }
        return c.dict_off[code + 1] - c.dict_off[code];
    }
    }
}

template <class Sink>
__device__ __forceinline__ int tt_cell_put(const TtCol &c, int64_t r, Sink &sink, int p) {
    switch (c.kind) {
    case CHICDIFF_COL_INT32: return tt_put_int(((const int32_t *)c.data)[r], sink, p);
    case CHICDIFF_COL_INT64: return tt_put_int(((const int64_t *)c.data)[r], sink, p);
    case CHICDIFF_COL_FLOAT64: return tt_put_double(((const uint64_t *)c.data)[r], kPow10, sink, p);
    default: {
        const int code = tt_dict_code(c, r);
        if (code < 0 || code >= c.ndict) return 0;
        const int a = c.dict_off[code], len = c.dict_off[code + 1] - a;
        for (int j = 0; j < len; j++) sink.put(p + j, c.dict_bytes[a + j]);
        return len;
    }
    }
}

using TtReduce = rocprim::block_reduce<unsigned int, kTtRows>;
using TtScan = rocprim::block_scan<unsigned int, kTtRows>;

__global__ __launch_bounds__(256) void table_text_len_kernel(const TtCols t, int64_t n, uint32_t *__restrict__ row_len,
                                                             int64_t *__restrict__ tile_total, TtResult *res) {
    __shared__ typename TtReduce::storage_type s_red;
    const int64_t r = (int64_t)blockIdx.x * kTtRows + threadIdx.x;
    unsigned int len = 0, total = 0;
    int bad = 0;
    if (r < n) {
        for (int j = 0; j < t.ncol; j++) len += (unsigned int)tt_cell_len(t.col[j], r, &bad);
        len += (unsigned int)t.ncol;  // ncol - 1 separators and the newline
        row_len[r] = len;
    }
    TtReduce().reduce(len, total, s_red);
    if (threadIdx.x == 0) tile_total[blockIdx.x] = (int64_t)total;
    if (bad) atomicOr(&res->bad_code, 1);
}

__global__ void table_text_total_kernel(const int64_t *__restrict__ tile_start, int64_t ntiles, TtResult *res) {
    res->nbytes = tile_start[ntiles];
}

__global__ __launch_bounds__(256) void table_text_write_kernel(const TtCols t, int64_t n, const uint32_t *__restrict__ row_len,
                                                               const int64_t *__restrict__ tile_start, unsigned char *__restrict__ out) {
    __shared__ uint4 s_buf4[kTtBuf / 16 + 1];
    __shared__ typename TtScan::storage_type s_scan;
    unsigned char *s_buf = reinterpret_cast<unsigned char *>(s_buf4);
    const int tid = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * kTtRows + tid;
    const unsigned int len = r < n ? row_len[r] : 0u;
    unsigned int off = 0, total = 0;
    TtScan().exclusive_scan(len, off, 0u, total, s_scan);
    unsigned char *dst = out + tile_start[blockIdx.x];  // the tile's run: bytes [0, total)
    for (unsigned int lo = 0; lo < total; lo += kTtBuf) {
        const int m = (int)(total - lo < (unsigned int)kTtBuf ? total - lo : (unsigned int)kTtBuf);
        unsigned char *run = dst + lo;
        const int shift = (int)((uintptr_t)run & 15);
        if (len && off < lo + (unsigned int)m && off + len > lo) {
            TtLdsSink sink{s_buf, (int)lo, (int)lo + m, shift};
            int p = (int)off;
            for (int j = 0; j < t.ncol; j++) {
                p += tt_cell_put(t.col[j], r, sink, p);
                sink.put(p++, (unsigned char)(j + 1 < t.ncol ? t.sep : '\n'));
            }
        }
        __syncthreads();
        // s_buf[shift .. shift + m) -> run[0 .. m): bytes up to the first 16-byte boundary, 16-byte words, the bytes that remain
        int head = (16 - shift) & 15;
        if (head > m) head = m;
        const int nvec = (m - head) >> 4, tail = head + (nvec << 4);
        if (tid < head) run[tid] = s_buf[shift + tid];
        const uint4 *src4 = reinterpret_cast<const uint4 *>(s_buf + shift + head);  // shift + head is 0 or 16
        uint4 *dst4 = reinterpret_cast<uint4 *>(run + head);
        for (int v = tid; v < nvec; v += kTtRows) dst4[v] = src4[v];
        if (tid < m - tail) run[tail + tid] = s_buf[shift + tail + tid];
        __syncthreads();  // the next chunk overwrites the buffer
    }
}

__global__ __launch_bounds__(256) void format_double_selftest_kernel(const uint64_t *__restrict__ x, int64_t n, unsigned char *__restrict__ text,
                                                                     int32_t *__restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    TtBufferSink sink{text + i * kTtMaxCell};
    len[i] = tt_put_double(x[i], kPow10, sink, 0);
}

size_t tt_c256(size_t x) { return (x + 255) & ~(size_t)255; }
int64_t tt_tiles(int64_t n) { return (n + kTtRows - 1) / kTtRows; }

size_t tt_prim_bytes(int64_t ntiles) {
    size_t b = 0;
    int64_t *p = nullptr;
    (void)rocprim::exclusive_scan(nullptr, b, p, p, (int64_t)0, (size_t)(ntiles + 1), rocprim::plus<int64_t>(), (hipStream_t)0);
    return b + 256;
}

struct TtWork {
    TtResult *res;
    uint32_t *row_len;
    int64_t *tile_total, *tile_start;
    void *tmp;
    size_t tmp_bytes;
};

TtWork tt_work(char *ws, int64_t n) {
    const int64_t ntiles = tt_tiles(n);
    char *q = ws;
    auto take = [&](size_t bytes) { char *r = q; q += tt_c256(bytes); return r; };
    TtWork k;
    k.res = (TtResult *)take(sizeof(TtResult));
    k.row_len = (uint32_t *)take(sizeof(uint32_t) * (size_t)n);
    k.tile_total = (int64_t *)take(sizeof(int64_t) * (size_t)(ntiles + 1));
    k.tile_start = (int64_t *)take(sizeof(int64_t) * (size_t)(ntiles + 1));
    k.tmp = q;
    k.tmp_bytes = tt_prim_bytes(ntiles);
    return k;
}

}  // namespace

size_t table_text_workspace_bytes(int64_t n) {
    const int64_t ntiles = tt_tiles(n);
    return tt_c256(sizeof(TtResult)) + tt_c256(sizeof(uint32_t) * (size_t)n) + 2 * tt_c256(sizeof(int64_t) * (size_t)(ntiles + 1)) + tt_prim_bytes(ntiles);
}

// n >= 1
int launch_table_text_len(const TtCols &t, int64_t n, char *ws, hipStream_t st, const TtResult **res_out) {
    const TtWork k = tt_work(ws, n);
    const int64_t ntiles = tt_tiles(n);
    *res_out = k.res;
    if (hipMemsetAsync(k.res, 0, sizeof(TtResult), st) != hipSuccess) return 1;
    if (hipMemsetAsync(k.tile_total + ntiles, 0, sizeof(int64_t), st) != hipSuccess) return 1;  // the entry behind the last tile: its start is the size
    table_text_len_kernel<<<(unsigned)ntiles, 256, 0, st>>>(t, n, k.row_len, k.tile_total, k.res);
    return 0;
}

int launch_table_text_scan(int64_t n, char *ws, hipStream_t st) {
    const TtWork k = tt_work(ws, n);
    const int64_t ntiles = tt_tiles(n);
    size_t tmp_bytes = k.tmp_bytes;
    if (rocprim::exclusive_scan(k.tmp, tmp_bytes, k.tile_total, k.tile_start, (int64_t)0, (size_t)(ntiles + 1), rocprim::plus<int64_t>(), st) != hipSuccess)
        return 1;
    table_text_total_kernel<<<1, 1, 0, st>>>(k.tile_start, ntiles, k.res);
    return 0;
}

void launch_table_text_write(const TtCols &t, int64_t n, uint8_t *out, char *ws, hipStream_t st) {
    const TtWork k = tt_work(ws, n);
    table_text_write_kernel<<<(unsigned)tt_tiles(n), 256, 0, st>>>(t, n, k.row_len, k.tile_start, out);
}

void launch_format_double_selftest(const double *x, int64_t n, uint8_t *text, int32_t *len, hipStream_t st) {
    format_double_selftest_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>((const uint64_t *)x, n, text, len);
}

}  // namespace cd
