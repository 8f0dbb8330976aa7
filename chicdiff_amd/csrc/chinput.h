// chinput.h — the host side of reading a text table (chinput.hip), as text_api.hip and peaks.hip use it.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "common.h"

namespace cd {

struct ChinputCols {
    std::vector<int32_t> bait, oe, N;
    std::string error;
};

// The file mapped, and what its comment lines and header say: both parsers start here.  body = the bytes after the header line;
// ib, io, in = the 0-based columns of baitID, otherEndID, N (quoted names and any column order accepted).
struct ChinputFile {
    const char *base = nullptr;
    size_t size = 0, body = 0;  // body: offset of the first byte after the header line
    int ib = -1, io = -1, in = -1;
    std::string error;
};

int64_t chinput_parse(const char *path, int nthreads, ChinputCols &c);
int chinput_open(const char *path, ChinputFile &f);
void chinput_close(ChinputFile &f);
std::string chinput_malformed(long long offset);
hipError_t chinput_upload(const ChinputFile &f, char *d_text, char *pin, size_t half_bytes, int nthreads, hipStream_t st, hipEvent_t ev[2]);

}  // namespace cd
