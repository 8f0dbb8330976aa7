// peaks_textkey.h — the sort keys of a peak matrix's text columns, for .multimerge on the device (chicdiff.R:218-228, 234-236): the class
// and key of a chromosome token (baitChr, oeChr) and the hash of a name field (baitName, oeName).  One statement for the device kernel
// (peaks_merge_kernels.hip) and the host statement (peaks.hip); the rule stands above chicdiff_hip_peaks_textkeys_dev in
// include/chicdiff_hip.h.  A token is fed byte by byte, so that neither side needs it in one piece.
#pragma once
#include <stdint.h>

#include "common.h"

namespace cd {

// what one chromosome token is
enum { PK_TOK_INT = 0, PK_TOK_TEXT = 1, PK_TOK_LONG = 2, PK_TOK_AMBIGUOUS = 3 };

struct PkChrToken {
    uint64_t packed = 0;  // the first 8 bytes, big-endian, zero-padded
    int64_t value = 0;    // the digits read so far (of at most 10)
    int len = 0;
    bool digits = true;   // every byte a digit
    bool ascii = true;    // every byte below 0x80
    bool wordy = false;   // some byte outside 0-9 + - . e E and blank
    bool zero_first = false;
    __host__ __device__ void feed(unsigned char b) {
        if (len < 8) packed |= (uint64_t)b << (8 * (7 - len));
        const bool d = b >= '0' && b <= '9';
        if (len == 0) zero_first = b == '0';
        if (d && len < 10) value = value * 10 + (b - '0');
        digits = digits && d;
        ascii = ascii && b < 0x80;
        wordy = wordy || !(d || b == '+' || b == '-' || b == '.' || b == 'e' || b == 'E' || b == ' ');
        len++;
    }
};

__host__ __device__ inline uint64_t pk_pack8(const char *s) {
    uint64_t w = 0;
    for (int k = 0; k < 8 && s[k]; k++) w |= (uint64_t)(unsigned char)s[k] << (8 * (7 - k));
    return w;
}

// pandas' NA spellings that pass the other conditions of a text token ('' and the all-numeric-set ones never do)
__host__ __device__ inline bool pk_is_na_spelling(uint64_t packed) {
    const char *const na[] = {"#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND", "1.#QNAN", "<NA>", "N/A",
                              "NA",   "NULL",     "NaN", "None",    "n/a",      "nan",  "null"};
    for (int k = 0; k < 18; k++)
        if (packed == pk_pack8(na[k])) return true;
    return false;
}

// [+-]?(inf|infinity) in any letter case, of at most 8 bytes ("+infinity" has 9 and is long anyway)
__host__ __device__ inline bool pk_is_inf_spelling(uint64_t packed) {
    uint64_t w = packed;
    const unsigned char first = (unsigned char)(w >> 56);
    if (first == '+' || first == '-') w <<= 8;
    uint64_t low = 0;  // letters to lower case
    for (int k = 0; k < 8; k++) {
        unsigned char b = (unsigned char)(w >> (8 * (7 - k)));
        if (b >= 'A' && b <= 'Z') b += 'a' - 'A';
        low |= (uint64_t)b << (8 * (7 - k));
    }
    return low == pk_pack8("inf") || low == pk_pack8("infinity");
}

// the token's class (PK_TOK_*)
__host__ __device__ inline int pk_chr_class(const PkChrToken &t) {
    if (t.digits && t.len >= 1 && t.len <= 9 && (!t.zero_first || t.len == 1)) return PK_TOK_INT;  // 0|[1-9][0-9]{0,8}
    if (!t.ascii || !t.wordy || t.len == 0) return PK_TOK_AMBIGUOUS;
    if (t.len > 8) return PK_TOK_LONG;
    if (pk_is_na_spelling(t.packed) || pk_is_inf_spelling(t.packed)) return PK_TOK_AMBIGUOUS;
    return PK_TOK_TEXT;
}

// the key of a token's bytes (at most 8): signed int64 order = byte order
__host__ __device__ inline int64_t pk_text_key(uint64_t packed) { return (int64_t)(packed ^ 0x8000000000000000ull); }

// FNV-1a, 64 bits
constexpr uint64_t kPkFnvBasis = 0xcbf29ce484222325ull, kPkFnvPrime = 0x100000001b3ull;
__host__ __device__ inline uint64_t pk_fnv_step(uint64_t h, unsigned char b) { return (h ^ b) * kPkFnvPrime; }

// per column, what the rows add up to (flag words: integer atomics on flags only)
enum {
    PK_COLF_NOT_INT = 1,   // some row is no plain integer
    PK_COLF_TEXT = 2,      // some row is text
    PK_COLF_INT = 4,       // some row is a plain integer
    PK_COLF_INT9 = 8,      // some plain integer has 9 digits: no 8-byte key if the column is text
    PK_COLF_LONG = 16,     // some text token is over 8 bytes
    PK_COLF_AMBIGUOUS = 32 // some token is neither
};

__host__ __device__ inline int pk_col_flags(const PkChrToken &t) {
    switch (pk_chr_class(t)) {
        case PK_TOK_INT: return PK_COLF_INT | (t.len == 9 ? PK_COLF_INT9 : 0);
        case PK_TOK_TEXT: return PK_COLF_NOT_INT | PK_COLF_TEXT;
        case PK_TOK_LONG: return PK_COLF_NOT_INT | PK_COLF_LONG;
        default: return PK_COLF_NOT_INT | PK_COLF_AMBIGUOUS;
    }
}

// flag word of a column -> its class (CHICDIFF_PEAKS_KEY_*) and the status bits (CHICDIFF_PEAKS_ST_CHR_*) it raises
__host__ __device__ inline int pk_col_class(int flags, int *status) {
    int st = 0;
    if (flags & PK_COLF_LONG) st |= CHICDIFF_PEAKS_ST_CHR_LONG;
    if (flags & PK_COLF_AMBIGUOUS) st |= CHICDIFF_PEAKS_ST_CHR_AMBIGUOUS;
    const bool text = (flags & PK_COLF_NOT_INT) != 0;
    if (text && (flags & PK_COLF_INT9)) st |= CHICDIFF_PEAKS_ST_CHR_LONG;  // a 9-digit number in a column of strings
    *status |= st;
    if (!text) return CHICDIFF_PEAKS_KEY_INT;
    return (flags & PK_COLF_INT) ? CHICDIFF_PEAKS_KEY_MIXED : CHICDIFF_PEAKS_KEY_TEXT;
}

}  // namespace cd
