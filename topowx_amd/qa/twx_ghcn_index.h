// twx_ghcn_index.h -- the line index that twx_ghcn.hip builds (k_gh_count / k_gh_scan / k_gh_starts), for the units that
// read text files laid end to end: how a kernel looks a line up, and the host call that uploads a buffer and builds its
// index.  Internal to libtwxqa.so.
#ifndef TWX_GHCN_INDEX_H
#define TWX_GHCN_INDEX_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// the file that holds byte q (0 <= q < file_off[nfiles]): the last f with file_off[f] <= q
__device__ __forceinline__ int gh_file_of(const int64_t *__restrict__ file_off, int nfiles, int64_t q)
{
    int lo = 0, hi = nfiles;                                     // file_off[lo] <= q < file_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (file_off[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// Line i of the index: entries 0 .. nfiles - 1 are the files' first lines, the rest the candidates.  False: no line.
__device__ __forceinline__ bool gh_line(int64_t i, int64_t nlines, int nfiles, const int64_t *__restrict__ file_off,
                                        const uint32_t *__restrict__ cand, int *f, int64_t *start, int64_t *fend)
{
    if (i >= nlines) return false;
    if (i < nfiles) {
        *f = (int)i;
        *start = file_off[i];
    } else {
        *start = (int64_t)cand[i - nfiles];
        *f = gh_file_of(file_off, nfiles, *start - 1);           // the file of the newline byte
    }
    *fend = file_off[*f + 1];
    return *start < *fend;
}

}  // namespace

// Upload buf (padded with zero bytes to a multiple of 16 and 16 more) and file_off, build the candidate list (the positions
// after the newline bytes that are not the buffer's last byte, ascending).  dev[0 .. 3]: the device buffer, the offsets, the
// candidates and the scan's scratch -- the caller's to hipFree, also after a failure (unset ones are null).  *ms: the kernels.
__attribute__((visibility("hidden"))) int gh_index_build(const uint8_t *buf, int64_t nbytes, int64_t nfiles,
                                                         const int64_t *file_off, void *dev[4], uint32_t *ncand, float *ms,
                                                         char *errbuf, int errlen);
#endif
