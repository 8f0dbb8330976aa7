// peaks_merge_kernels.hip — .multimerge on the device (chicdiff.R:218-228, 234-236): the full outer join of F peak matrices on their
// eleven key columns, in the order of the pandas twin.  The rule is stated above chicdiff_hip_peaks_textkeys_dev and
// chicdiff_hip_peaks_merge_dev in include/chicdiff_hip.h.  gfx950 only.
//
//   text keys of one file        -> peaks_textkeys_kernel: one lane per row walks fields 0 .. 9 of its line in global memory (no LDS
//                                   staging: a line's head is read once, byte-wise); fields 0 and 5 through peaks_textkey.h, fields 4
//                                   and 9 through FNV-1a.  Both key forms are written, the column's class is known only afterwards
//   the eight words of a row     -> peaks_merge_words_kernel: six order-preserving unsigned words per concatenated row (file-major)
//   order                        -> six stable rocPRIM radix passes over a permutation, least significant word first
//   groups                       -> peaks_merge_heads_kernel compares each sorted row with its predecessor; ONE exclusive scan of the
//                                   head flags; peaks_merge_write_kernel, one lane per group
//
// No value passes through an atomic: the atomics are the ORs of flag and status words.  No kernel here takes a lock or polls.
#include <stddef.h>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "peaks.h"
#include "peaks_textkey.h"

namespace cd {

namespace {

// ---- text keys -------------------------------------------------------------------------------------------------------------------
// flags[0], flags[1]: the PK_COLF_* words of baitChr and oeChr.  d_int / d_text (2, stride): the key of every token as a plain integer
// and as bytes (whichever applies; the other form is never read).  d_name (2, stride): the hashes of baitName and oeName.
__global__ __launch_bounds__(256) void peaks_textkeys_kernel(const unsigned char *__restrict__ text, int64_t nbytes, int sep,
                                                             const int64_t *__restrict__ line_off, int64_t n, int64_t stride,
                                                             int64_t *__restrict__ d_int, int64_t *__restrict__ d_text,
                                                             int64_t *__restrict__ d_name, int *__restrict__ flags) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int f0 = 0, f1 = 0;
    if (r < n) {
        int64_t p = line_off[r];
        bool ended = p < 0 || p >= nbytes;
        for (int field = 0; field < 10; field++) {
            PkChrToken tok;
            uint64_t h = kPkFnvBasis;
            const bool chr = field == 0 || field == 5, name = field == 4 || field == 9;
            while (!ended) {
                if (p >= nbytes) { ended = true; break; }
                const unsigned char b = text[p];
                if (b == '\n') { ended = true; break; }
                p++;
                if (b == (unsigned char)sep) break;
                if (chr) tok.feed(b);
                if (name) h = pk_fnv_step(h, b);
            }
            if (chr) {
                // a line that ends inside its first ten fields never passed the parse: counted as undecided, not trusted
                const int fl = ended ? (PK_COLF_NOT_INT | PK_COLF_AMBIGUOUS) : pk_col_flags(tok);
                const int64_t at = (field == 5 ? stride : 0) + r;
                d_int[at] = tok.value;
                d_text[at] = pk_text_key(tok.packed);
                if (field == 0) f0 = fl;
                else f1 = fl;
            }
            if (name) d_name[(field == 9 ? stride : 0) + r] = (int64_t)h;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        f0 |= __shfl_xor(f0, d, 64);
        f1 |= __shfl_xor(f1, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (f0) atomicOr(&flags[0], f0);
        if (f1) atomicOr(&flags[1], f1);
    }
}

// ---- merge -----------------------------------------------------------------------------------------------------------------------
// where concatenated row g lives: the file f with off[f] <= g < off[f + 1], row g - off[f]
__device__ __forceinline__ int pm_file_of(const PeaksMergeFiles &F, int64_t g) {
    int f = 0;
    while (f + 1 < F.nfiles && g >= F.off[f + 1]) f++;
    return f;
}

__device__ __forceinline__ uint64_t pm_u32(int32_t v) { return (uint64_t)((uint32_t)v ^ 0x80000000u); }  // unsigned order = signed order

// the six sort words of every concatenated row: w[0] chr(baitChr), w[1] baitStart, w[2] (baitEnd, baitID), w[3] chr(oeChr), w[4] oeStart,
// w[5] (oeEnd, oeID); each (N) uint64, unsigned order = the order of the values
__global__ __launch_bounds__(256) void peaks_merge_words_kernel(PeaksMergeFiles F, int64_t N, uint64_t *__restrict__ w, uint32_t *__restrict__ perm) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N) return;
    const int f = pm_file_of(F, g);
    const int64_t r = g - F.off[f], n = F.off[f + 1] - F.off[f];
    const int32_t *iv = F.ints[f];
    w[g] = (uint64_t)F.chr[f][r] ^ 0x8000000000000000ull;
    w[N + g] = pm_u32(iv[r]);
    w[2 * N + g] = (pm_u32(iv[n + r]) << 32) | pm_u32(iv[2 * n + r]);
    w[3 * N + g] = (uint64_t)F.chr[f][n + r] ^ 0x8000000000000000ull;
    w[4 * N + g] = pm_u32(iv[3 * n + r]);
    w[5 * N + g] = (pm_u32(iv[4 * n + r]) << 32) | pm_u32(iv[5 * n + r]);
    perm[g] = (uint32_t)g;
}

__global__ __launch_bounds__(256) void peaks_merge_gather_kernel(const uint64_t *__restrict__ word, const uint32_t *__restrict__ perm, int64_t N,
                                                                 uint64_t *__restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) key[i] = word[perm[i]];
}

// flags[i] = 1: sorted row i opens a group (flags[N] = 0: the scan's total lands there).  status: CHICDIFF_PEAKS_ST_MERGE_* bits.
__global__ __launch_bounds__(256) void peaks_merge_heads_kernel(PeaksMergeFiles F, int64_t N, const uint64_t *__restrict__ w,
                                                                const uint32_t *__restrict__ perm, int32_t *__restrict__ flags,
                                                                int *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > N) return;
    if (i == N) {
        flags[N] = 0;
        return;
    }
    if (i == 0) {
        flags[0] = 1;
        return;
    }
    const int64_t g = perm[i], q = perm[i - 1];
    const bool bait = w[g] == w[q] && w[N + g] == w[N + q] && w[2 * N + g] == w[2 * N + q];
    const bool same = bait && w[3 * N + g] == w[3 * N + q] && w[4 * N + g] == w[4 * N + q] && w[5 * N + g] == w[5 * N + q];
    flags[i] = same ? 0 : 1;
    if (!bait) return;
    const int fg = pm_file_of(F, g), fq = pm_file_of(F, q);
    const int64_t rg = g - F.off[fg], rq = q - F.off[fq];
    const int64_t ng = F.off[fg + 1] - F.off[fg], nq = F.off[fq + 1] - F.off[fq];
    int st = 0;
    if (F.name[fg][rg] != F.name[fq][rq]) st |= CHICDIFF_PEAKS_ST_MERGE_NAME;  // baitName along a run of one bait
    if (same) {
        if (fg == fq) st |= CHICDIFF_PEAKS_ST_MERGE_DUPLICATE;
        if (F.name[fg][ng + rg] != F.name[fq][nq + rq]) st |= CHICDIFF_PEAKS_ST_MERGE_NAME;
        const double a = F.dist[fg][rg], b = F.dist[fq][rq];
        if (!(a == b || (a != a && b != b))) st |= CHICDIFF_PEAKS_ST_MERGE_DIST;  // NaN equals NaN, +0 equals -0
    }
    if (st) atomicOr(status, st);
}

// one lane per group: pos[i] = the group's output row.  A group's members lie at i, i + 1, ... in file order (the sort is stable and
// the concatenation file-major); at most one per file is looked at (more: DUPLICATE is set already).
__global__ __launch_bounds__(256) void peaks_merge_write_kernel(PeaksMergeFiles F, int64_t N, const uint32_t *__restrict__ perm,
                                                                const int32_t *__restrict__ pos, int64_t cap, int32_t *__restrict__ o_ints,
                                                                double *__restrict__ o_dist, double *__restrict__ o_scores,
                                                                int32_t *__restrict__ o_file, int64_t *__restrict__ o_row) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int64_t k = pos[i];
    if (pos[i + 1] == k || k >= cap) return;  // no head
    const int64_t g = perm[i];
    int f = pm_file_of(F, g);
    int64_t r = g - F.off[f], n = F.off[f + 1] - F.off[f];
    {
        const int32_t *iv = F.ints[f];
#pragma unroll
        for (int c = 0; c < 6; c++) o_ints[(int64_t)c * cap + k] = iv[(int64_t)c * n + r];
        o_dist[k] = F.dist[f][r];
        o_file[k] = f;
        o_row[k] = r;
    }
    int64_t j = i;  // the member looked at: row r of file f
    for (int file = 0; file < F.nfiles; file++) {
        const bool has = f == file;
        const int T = F.score_off[file + 1] - F.score_off[file];
        for (int t = 0; t < T; t++)
            o_scores[(int64_t)(F.score_off[file] + t) * cap + k] = has ? F.scores[file][(int64_t)t * n + r] : __longlong_as_double(0x7ff8000000000000ll);
        if (has) {  // on to the group's next member, if it has one
            f = -1;
            if (j + 1 < N && pos[j + 2] == pos[j + 1]) {
                j++;
                const int64_t g2 = perm[j];
                f = pm_file_of(F, g2);
                r = g2 - F.off[f];
                n = F.off[f + 1] - F.off[f];
                if (f <= file) f = -1;  // a duplicate inside one file: the call is declined, the cells stay NaN
            }
        }
    }
}

size_t pm_c256(size_t x) { return (x + 255) & ~(size_t)255; }

size_t pm_tmp_bytes(int64_t N) {
    size_t a = 0, b = 0, c = 0;
    uint64_t *k64 = nullptr;
    uint32_t *v = nullptr;
    int32_t *fl = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, a, k64, k64, v, v, (size_t)N, 0, 64, (hipStream_t)0);
    (void)rocprim::radix_sort_pairs(nullptr, b, k64, k64, v, v, (size_t)N, 0, 32, (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, c, fl, fl, (int32_t)0, (size_t)N + 1, rocprim::plus<int32_t>(), (hipStream_t)0);
    a = a > b ? a : b;
    return pm_c256(a > c ? a : c) + 256;
}

}  // namespace

// ---- text keys: workspace = [flags 256][byte keys (2, stride)] --------------------------------------------------------------------------
size_t peaks_textkeys_workspace_bytes(int64_t stride) { return 256 + pm_c256(sizeof(int64_t) * 2 * (size_t)stride); }
int *peaks_textkeys_flags(char *ws) { return (int *)ws; }
int64_t *peaks_textkeys_bytes(char *ws) { return (int64_t *)(ws + 256); }

// d_chr (2, stride) receives the plain-integer keys, the workspace the byte keys in the same shape: the caller copies a column's over
// once the flags say that it is no column of plain integers
int launch_peaks_textkeys(const unsigned char *text, int64_t nbytes, int sep, const int64_t *line_off, int64_t n, int64_t stride,
                          int64_t *d_chr, int64_t *d_name, char *ws, hipStream_t st) {
    if (hipMemsetAsync(ws, 0, 256, st) != hipSuccess) return 1;
    if (n == 0) return 0;
    peaks_textkeys_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(text, nbytes, sep, line_off, n, stride, d_chr, peaks_textkeys_bytes(ws), d_name,
                                                                       peaks_textkeys_flags(ws));
    return 0;
}

// ---- merge: workspace = [status 256][words 6 N][keys 2 N][perm 2 N][flags N + 1][sort / scan temporaries] ----------------------------------
size_t peaks_merge_workspace_bytes(int64_t N) {
    return 256 + pm_c256(sizeof(uint64_t) * 6 * (size_t)N) + 2 * pm_c256(sizeof(uint64_t) * (size_t)N) + 2 * pm_c256(sizeof(uint32_t) * (size_t)N) +
           pm_c256(sizeof(int32_t) * (size_t)(N + 1)) + pm_tmp_bytes(N);
}

PeaksMergeWork peaks_merge_work(char *ws, int64_t N) {
    PeaksMergeWork k;
    char *p = ws;
    k.status = (int *)p; p += 256;
    k.w = (uint64_t *)p; p += pm_c256(sizeof(uint64_t) * 6 * (size_t)N);
    k.ka = (uint64_t *)p; p += pm_c256(sizeof(uint64_t) * (size_t)N);
    k.kb = (uint64_t *)p; p += pm_c256(sizeof(uint64_t) * (size_t)N);
    k.pa = (uint32_t *)p; p += pm_c256(sizeof(uint32_t) * (size_t)N);
    k.pb = (uint32_t *)p; p += pm_c256(sizeof(uint32_t) * (size_t)N);
    k.flags = (int32_t *)p; p += pm_c256(sizeof(int32_t) * (size_t)(N + 1));
    k.tmp = p;
    k.tmp_bytes = pm_tmp_bytes(N);
    return k;
}

// the permutation of the N = F.off[F.nfiles] concatenated rows in the order of the eight words, left in k.pa
int launch_peaks_merge_sort(const PeaksMergeFiles &F, PeaksMergeWork &k, hipStream_t st) {
    const int64_t N = F.off[F.nfiles];
    if (hipMemsetAsync(k.status, 0, 256, st) != hipSuccess) return 1;
    const unsigned blocks = (unsigned)((N + 255) / 256);
    peaks_merge_words_kernel<<<blocks, 256, 0, st>>>(F, N, k.w, k.pa);
    static const int kOrder[6] = {5, 4, 3, 2, 1, 0};       // least significant word first
    static const int kBits[6] = {64, 32, 64, 64, 32, 64};  // by word
    for (int pass = 0; pass < 6; pass++) {
        const int word = kOrder[pass];
        peaks_merge_gather_kernel<<<blocks, 256, 0, st>>>(k.w + (size_t)word * (size_t)N, k.pa, N, k.ka);
        if (rocprim::radix_sort_pairs(k.tmp, k.tmp_bytes, k.ka, k.kb, k.pa, k.pb, (size_t)N, 0, kBits[word], st) != hipSuccess) return 1;  // stable
        uint32_t *t = k.pa; k.pa = k.pb; k.pb = t;
    }
    return 0;
}

// after _sort: the head flags, the status bits, and the scan: k.flags[i] = the output row of the group of sorted row i, k.flags[N] = n_out
int launch_peaks_merge_heads(const PeaksMergeFiles &F, const PeaksMergeWork &k, hipStream_t st) {
    const int64_t N = F.off[F.nfiles];
    peaks_merge_heads_kernel<<<(unsigned)((N + 1 + 255) / 256), 256, 0, st>>>(F, N, k.w, k.pa, k.flags, k.status);
    size_t tmp_bytes = k.tmp_bytes;
    return rocprim::exclusive_scan(k.tmp, tmp_bytes, k.flags, k.flags, (int32_t)0, (size_t)N + 1, rocprim::plus<int32_t>(), st) != hipSuccess;
}

// after _heads: the merged table into the caller's columns of `cap` rows (rows from cap on are not written)
void launch_peaks_merge_write(const PeaksMergeFiles &F, const PeaksMergeWork &k, int64_t cap, int32_t *o_ints, double *o_dist, double *o_scores,
                              int32_t *o_file, int64_t *o_row, hipStream_t st) {
    const int64_t N = F.off[F.nfiles];
    peaks_merge_write_kernel<<<(unsigned)((N + 255) / 256), 256, 0, st>>>(F, N, k.pa, k.flags, cap, o_ints, o_dist, o_scores, o_file, o_row);
}

}  // namespace cd
