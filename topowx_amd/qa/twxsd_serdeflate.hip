// twxsd_serdeflate.hip -- libtwxqa.so: station-major rows as the stored bytes of their (ndays, 1) chunks: one zlib stream per row
// of the shuffled row, formed and packed on the device (include/twx_series_deflate.h, twxsd_*).  The reference stores every
// (time, station_id) variable of its station databases that way (twx/db/create_db_all_stations.py:307-311, 399-435) and lets
// libhdf5 deflate on one core.  The host arithmetic is twx_serdeflate_host.h, shared with a CPU program of the tests.
//
// The token and table code is topowx_amd/csrc/twx_deflate.h AS IT IS (df_piece, df_step_tokens, df_len_sym, DfTable,
// df_huff_sorted, df_finish_table, df_huff_bytes, df_seg_stored, dfl::block_scan, the piece layout).  What differs from the
// int16 coder: a row has es = 1, 2 or 4 byte planes with different statistics, so every plane is Huffman coded with a code of
// its own (the int16 coder stores its low plane raw), and the rows are contiguous, so a segment is loaded with aligned 16-byte
// units instead of a gather.
//
// A work item is (row, segment): 16 384 elements.  Its work-group loads them ONCE per pass into registers -- 4 es aligned
// 16-byte units per thread, the elements before the first and after the last unit one by one, nothing outside the segment --
// and forms the es planes from the registers one after the other in the same 17 KB of LDS (piece p at p * TWX_DF_PSTRIDE).
//   k_sd_hist    token counts of the sampled items (row % 4 == 0, segment % 16 == 0) per plane: LDS, then integer atomics
//   k_deflate_table  (the int16 coder's, as it is) a work-group per plane: the plane's code and block header
//   k_sd_count   bits of every thread's piece, bytes of every block (Huffman or stored), Adler partial sums
//   k_sd_scan    a wavefront per row: block offsets, stream size, Adler-32, stored blocks
//   k_sd_emit    (the row offsets are scanned on the host from the sizes, 8 bytes a row) every block assembled in LDS as in
//                k_deflate_emit and copied to its FINAL place in the packed buffer with k_mo_compact's copy (bytes up to the
//                destination's alignment, funnel-shifted aligned words, bytes): there are no slots and no compaction pass
// The packed buffer comes out in one transfer.  Integers only: two calls give the same bytes.
// Roofline: HBM.  Bytes per input byte: 2 read (+ 1/8 at most for the counts) + the stream written once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cstdio>
#include <vector>

#include "twx_series_deflate.h"
#include "twx_qa_common.h"
#include "twx_serdeflate_host.h"

namespace {                                 // (the coder's kernels get internal linkage in this library)
#include "../csrc/twx_deflate.h"

static_assert(TWXSD_SEG == TWX_DF_SEG && TWXSD_THREADS == TWX_DF_THREADS && TWXSD_NSYM == TWX_DF_NSYM,
              "twx_serdeflate_host.h restates the coder's constants");
static_assert(TWXSD_NTIMES == TWXSD_NKERNELS + 2 && TWXSD_C_N == 8, "timing groups and counts");

struct SdArgs {
    const uint8_t *rows;        // [nrows][n] elements of es bytes
    uint8_t *packed;            // the streams, row r at row_off[r]
    uint32_t *seg_bytes;        // [nrows][es][nseg] bytes of every block; bit 31: stored
    uint32_t *seg_off;          // [nrows][es][nseg] its offset behind the stream's two header bytes
    uint32_t *adl;              // [nrows][es][nseg][2]: sum d, sum (len - j) d  (mod 65521)
    uint16_t *piece_bits;       // [nrows][es][nseg][256] token bits of every thread's piece (k_sd_count -> k_sd_emit)
    int64_t *row_bytes;         // [nrows] bytes of every stream
    const int64_t *row_off;     // [nrows + 1] (from the host, before k_sd_emit)
    uint32_t *row_adler;        // [nrows]
    uint32_t *hist;             // [es][TWX_DF_NSYM] (zeroed before k_sd_hist)
    DfTable *table;             // [es]
    uint32_t *counters;         // [0] stored blocks (zeroed)
    int64_t n, nrows;
    int32_t nseg;
};

// the elements of a (row, segment) item in registers
template <int ES> struct SdStage {
    uint32_t v[4 * ES][4];      // unit k = j * 256 + thread: 16 aligned bytes
    uint32_t hd, tl, pe;        // thread t < h: head element t; t < tail: tail element t; thread 0: the element before the segment
    int len, h, nv, tail;
};

template <int ES> __device__ __forceinline__ uint32_t sd_elem(const uint8_t *p)
{
    if (ES == 4) return *reinterpret_cast<const uint32_t *>(p);
    if (ES == 2) return *reinterpret_cast<const uint16_t *>(p);
    return *p;
}

template <int ES>
__device__ __forceinline__ void sd_load(const SdArgs &a, int64_t row, int seg, SdStage<ES> &s)
{
    constexpr int V = 16 / ES;
    const int t = threadIdx.x;
    s.len = (int)sd_seg_len(a.n, seg);
    const uint8_t *base = a.rows + (row * a.n + (int64_t)seg * TWXSD_SEG) * ES;
    s.h = sd_head((uint64_t)reinterpret_cast<uintptr_t>(base), ES, s.len);
    s.nv = (s.len - s.h) / V;
    s.tail = s.len - s.h - s.nv * V;
    const uint4 *vb = reinterpret_cast<const uint4 *>(base + s.h * ES);        // (16-byte aligned, or nv = 0)
#pragma unroll
    for (int j = 0; j < 4 * ES; ++j) {
        const int k = j * TWXSD_THREADS + t;
        uint4 x = make_uint4(0u, 0u, 0u, 0u);
        if (k < s.nv) x = vb[k];
        s.v[j][0] = x.x; s.v[j][1] = x.y; s.v[j][2] = x.z; s.v[j][3] = x.w;
    }
    s.hd = t < s.h ? sd_elem<ES>(base + t * ES) : 0u;
    s.tl = t < s.tail ? sd_elem<ES>(base + (s.h + s.nv * V + t) * ES) : 0u;
    s.pe = (t == 0 && seg > 0) ? sd_elem<ES>(base - ES) : 0u;
}

__device__ __forceinline__ int sd_at(int q) { return (q >> 6) * TWX_DF_PSTRIDE + (q & 63); }      // (TWX_DF_PIECE = 64)
static_assert(TWX_DF_PIECE == 64, "sd_at");

// plane p of the staged item into s_pl; returns the byte before the plane's segment (256: none)
template <int ES>
__device__ __forceinline__ int sd_plane(const SdStage<ES> &s, int seg, int p, uint8_t *s_pl)
{
    constexpr int V = 16 / ES;
    const int t = threadIdx.x;
    const unsigned sp = 8u * (unsigned)p;
    const bool words = (s.h & 3) == 0;                       // (work-group uniform) a unit's plane bytes start 4-byte aligned
#pragma unroll
    for (int j = 0; j < 4 * ES; ++j) {
        const int k = j * TWXSD_THREADS + t;
        if (k < s.nv) {
            const int q0 = s.h + k * V;
#pragma unroll
            for (int i = 0; i < V / 4; ++i) {
                uint32_t w = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int m = 4 * i + b;                 // byte p of element m of the unit
                    w |= ((s.v[j][(m * ES) / 4] >> (8u * (unsigned)((m * ES) & 3) + sp)) & 255u) << (8 * b);
                }
                const int q = q0 + 4 * i;
                if (words) *reinterpret_cast<uint32_t *>(s_pl + sd_at(q)) = w;
                else {
#pragma unroll
                    for (int b = 0; b < 4; ++b) s_pl[sd_at(q + b)] = (uint8_t)(w >> (8 * b));
                }
            }
        }
    }
    if (t < s.h) s_pl[sd_at(t)] = (uint8_t)(s.hd >> sp);
    if (t < s.tail) s_pl[sd_at(s.h + s.nv * V + t)] = (uint8_t)(s.tl >> sp);
    return seg > 0 ? (int)((s.pe >> sp) & 255u) : 256;
}

__device__ __forceinline__ int sd_prev(int t, int first, const uint8_t *s_pl)
{
    return t == 0 ? first : (int)s_pl[(t - 1) * TWX_DF_PSTRIDE + TWX_DF_PIECE - 1];
}

}  // namespace

// (the kernels have names of their own and external linkage, so that the build's resource table lists them)
// token counts of the sampled items, per plane
template <int ES>
__global__ __launch_bounds__(TWXSD_THREADS) void k_sd_hist(SdArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_pl[TWXSD_THREADS * TWX_DF_PSTRIDE];
    __shared__ uint32_t s_h[ES * TWX_DF_NSYM];
    const int t = threadIdx.x;
    const int nss = (a.nseg + TWXSD_SAMPLE_SEG - 1) / TWXSD_SAMPLE_SEG;
    const int64_t row = (int64_t)(blockIdx.x / nss) * TWXSD_SAMPLE_ROW;
    const int seg = (int)(blockIdx.x % nss) * TWXSD_SAMPLE_SEG;
    for (int i = t; i < ES * TWX_DF_NSYM; i += TWXSD_THREADS) s_h[i] = 0u;
    SdStage<ES> s;
    sd_load<ES>(a, row, seg, s);
    for (int p = 0; p < ES; ++p) {
        __syncthreads();                                     // (the pieces of the plane before are read)
        const int first = sd_plane<ES>(s, seg, p, s_pl);
        __syncthreads();
        const int plen = max(0, min(TWX_DF_PIECE, s.len - t * TWX_DF_PIECE));
        uint32_t *h = s_h + p * TWX_DF_NSYM;
        df_piece<true>(&s_pl[t * TWX_DF_PSTRIDE], plen, sd_prev(t, first, s_pl), [&](int run, int pv, int c) {
            df_step_tokens(run, pv, c, [&](int sym, unsigned, unsigned) { atomicAdd(&h[sym], 1u); });
        });
    }
    __syncthreads();
    for (int i = t; i < ES * TWX_DF_NSYM; i += TWXSD_THREADS)
        if (s_h[i]) atomicAdd(&a.hist[i], s_h[i]);
}

// How often the table builder halves the counts of `hist` before the code fits 15 bits: the loop of df_build_table, which
// k_deflate_table takes step by step on the device, run on the host over the histogram that came down.
static int sd_halvings(const uint32_t *hist)
{
    uint32_t cnt[TWX_DF_NSYM], wt[2 * TWX_DF_NSYM];
    uint16_t order[TWX_DF_NSYM], parent[2 * TWX_DF_NSYM], depth[2 * TWX_DF_NSYM];
    uint8_t len[TWX_DF_NSYM + 3];
    for (int i = 0; i < TWX_DF_NSYM; ++i) cnt[i] = hist[i] + 1u;
    for (int h = 0;; ++h) {
        df_sort_order(cnt, TWX_DF_NSYM, order);
        if (df_huff_sorted(cnt, order, TWX_DF_NSYM, 15, wt, parent, depth, len)) return h;
        for (int i = 0; i < TWX_DF_NSYM; ++i) cnt[i] = (cnt[i] + 1u) >> 1;
    }
}

template <int ES>
__global__ __launch_bounds__(TWXSD_THREADS) void k_sd_count(SdArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_pl[TWXSD_THREADS * TWX_DF_PSTRIDE];
    __shared__ uint32_t s_w[4];
    __shared__ unsigned long long s_sum[2];
    __shared__ uint8_t s_len[TWX_DF_NSYM + 3];
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x / a.nseg;
    const int seg = (int)(blockIdx.x % a.nseg);
    SdStage<ES> s;
    sd_load<ES>(a, row, seg, s);
    for (int p = 0; p < ES; ++p) {
        __syncthreads();                                     // (the plane before is done with s_pl, s_len, s_sum)
        for (int i = t; i < TWX_DF_NSYM; i += TWXSD_THREADS) s_len[i] = a.table[p].len[i];
        if (t < 2) s_sum[t] = 0ull;
        const int first = sd_plane<ES>(s, seg, p, s_pl);
        __syncthreads();
        const int plen = max(0, min(TWX_DF_PIECE, s.len - t * TWX_DF_PIECE));
        const uint8_t *mine = &s_pl[t * TWX_DF_PSTRIDE];
        uint32_t bits = 0;
        df_piece<true>(mine, plen, sd_prev(t, first, s_pl), [&](int run, int pv, int c) {
            if (run >= 3) { unsigned ex, ne; const int sym = df_len_sym(run, ex, ne); bits += (uint32_t)s_len[sym] + ne + 1u; }     // (+ the one-bit distance code)
            else bits += (uint32_t)run * s_len[pv < 256 ? pv : 0];
            if (c >= 0) bits += s_len[c];
        });
        // Adler partial sums of the piece: sum d, sum (len - j) d  (< 64 * 16 384 * 255: 32 bits)
        uint32_t sd = 0, wd = 0;
        for (int i = 0; i < plen; i += 4) {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(mine + i);
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (i + b < plen) { const uint32_t d = (w >> (8 * b)) & 255u; sd += d; wd += (uint32_t)(s.len - t * TWX_DF_PIECE - i - b) * d; }
        }
        const int64_t blk = (row * ES + p) * a.nseg + seg;
        a.piece_bits[blk * TWXSD_THREADS + t] = (uint16_t)bits;
        uint32_t tot;
        dfl::block_scan(bits, s_w, &tot);
        const uint64_t vs = dfl::wave_sum((uint64_t)sd), vw = dfl::wave_sum((uint64_t)wd);
        if ((t & 63) == 0) { atomicAdd(&s_sum[0], (unsigned long long)vs); atomicAdd(&s_sum[1], (unsigned long long)vw); }
        __syncthreads();
        if (t == 0) {
            const uint32_t hb = df_huff_bytes(tot, a.table[p].hdr_bits, s_len[256]);
            a.seg_bytes[blk] = df_seg_stored(hb, s.len) ? ((uint32_t)s.len + 5u) | 0x80000000u : hb;
            a.adl[blk * 2] = (uint32_t)(s_sum[0] % TWX_ADLER_P);
            a.adl[blk * 2 + 1] = (uint32_t)(s_sum[1] % TWX_ADLER_P);
        }
    }
}

// a wavefront per row: the offsets of its es * nseg blocks, its size, its Adler-32 (k_deflate_scan's recurrence over the
// (plane, segment) pieces in stream order), its stored blocks
__global__ __launch_bounds__(TWXSD_THREADS) void k_sd_scan(SdArgs a, int es)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (TWXSD_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= a.nrows) return;                              // (wave-uniform; no work-group barrier below)
    const int64_t nblk = (int64_t)es * a.nseg;
    uint64_t run = 0, B = 0;
    uint32_t A = 1u, nst = 0;
    for (int64_t base = 0; base < nblk; base += 64) {
        const int64_t k = base + lane;
        const bool valid = k < nblk;
        const uint32_t raw = valid ? a.seg_bytes[row * nblk + k] : 0u;
        const uint32_t v = raw & 0x7fffffffu;
        nst += raw >> 31;
        uint32_t x = v, xs = valid ? a.adl[(row * nblk + k) * 2] : 0u;
        const uint32_t S = xs, W = valid ? a.adl[(row * nblk + k) * 2 + 1] : 0u;
        const uint64_t L = valid ? (uint64_t)sd_seg_len(a.n, k % a.nseg) : 0ull;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64), ys = __shfl_up(xs, o, 64);
            if (lane >= o) { x += y; xs += ys; }              // (64 values below 16 390 and below 65 521: 32 bits)
        }
        if (valid) a.seg_off[row * nblk + k] = (uint32_t)(run + x - v);
        run += __shfl(x, 63, 64);
        const uint64_t P = ((uint64_t)A + xs - S) % TWX_ADLER_P;
        B += dfl::wave_sum((L * P + W) % TWX_ADLER_P);
        A = (uint32_t)(((uint64_t)A + __shfl(xs, 63, 64)) % TWX_ADLER_P);
    }
    nst = (uint32_t)dfl::wave_sum((uint64_t)nst);
    if (lane == 0) {
        a.row_bytes[row] = 2 + (int64_t)run + 9;
        a.row_adler[row] = ((uint32_t)(B % TWX_ADLER_P) << 16) | A;
        if (nst) atomicAdd(&a.counters[0], nst);
    }
}

template <int ES>
__global__ __launch_bounds__(TWXSD_THREADS) void k_sd_emit(SdArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_pl[TWXSD_THREADS * TWX_DF_PSTRIDE];
    __shared__ uint32_t s_out[(TWX_DF_SEG + 5 + 3) / 4 + 2];          // (a block longer than its bytes stored is not assembled)
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_cl[TWX_DF_NSYM + 3];                        // code | length << 16 | (a match: the distance bit) << 24
    const int t = threadIdx.x;
    const int64_t row = blockIdx.x / a.nseg;
    const int seg = (int)(blockIdx.x % a.nseg);
    uint8_t *stream = a.packed + a.row_off[row];
    uint8_t *sb = reinterpret_cast<uint8_t *>(s_out);
    SdStage<ES> s;
    sd_load<ES>(a, row, seg, s);
    const int len = s.len;
    for (int p = 0; p < ES; ++p) {
        __syncthreads();                                     // (the block before is copied out)
        const DfTable *tb = a.table + p;
        for (int i = t; i < TWX_DF_NSYM; i += TWXSD_THREADS)
            s_cl[i] = (uint32_t)tb->code[i] | ((uint32_t)tb->len[i] << 16) | (i > 256 ? 1u << 24 : 0u);
        const uint32_t hdr_bits = tb->hdr_bits;
        for (int i = t; i < (int)(sizeof(s_out) / 4); i += TWXSD_THREADS) s_out[i] = 0u;
        const int first = sd_plane<ES>(s, seg, p, s_pl);
        __syncthreads();
        const int64_t blk = (row * ES + p) * a.nseg + seg;
        const uint32_t bits = a.piece_bits[blk * TWXSD_THREADS + t];  // (counted by k_sd_count)
        const int plen = max(0, min(TWX_DF_PIECE, len - t * TWX_DF_PIECE));
        const uint8_t *mine = &s_pl[t * TWX_DF_PSTRIDE];
        uint32_t tot;
        const uint32_t inc = dfl::block_scan(bits, s_w, &tot);
        const uint32_t eob = s_cl[256];
        uint32_t nbytes = df_huff_bytes(tot, hdr_bits, (eob >> 16) & 255u);
        if (df_seg_stored(nbytes, len)) {                    // (work-group uniform) 00 LEN ~LEN and the bytes
            const unsigned bl = (unsigned)len;
            if (t == 0) { sb[0] = 0; sb[1] = (uint8_t)bl; sb[2] = (uint8_t)(bl >> 8); sb[3] = (uint8_t)~bl; sb[4] = (uint8_t)(~bl >> 8); }
            for (int i = t; i < len; i += TWXSD_THREADS) sb[5 + i] = s_pl[sd_at(i)];
            nbytes = bl + 5u;
        } else {
            // k_deflate_emit's assembly: the block header, then every thread's tokens at bit hdr_bits + (bits of the threads
            // before it), gathered in a 64-bit register, whole words stored as they fill; only the first and the last word of a
            // piece are shared with a neighbour (atomic or)
            for (uint32_t i = t; i < (hdr_bits + 31u) / 32u; i += TWXSD_THREADS) atomicOr(&s_out[i], tb->hdr[i]);
            const uint32_t pos = hdr_bits + inc - bits;
            uint64_t acc = 0;
            uint32_t nacc = pos & 31u, w = pos >> 5;
            bool firstw = true;
            auto flush = [&]() __attribute__((always_inline)) {
                if (nacc >= 32u) {
                    if (firstw) atomicOr(&s_out[w], (uint32_t)acc); else s_out[w] = (uint32_t)acc;
                    firstw = false;
                    ++w;
                    acc >>= 32;
                    nacc -= 32u;
                }
            };
            df_piece<true>(mine, plen, sd_prev(t, first, s_pl), [&](int run, int pv, int c) {
                uint64_t sv = 0;
                uint32_t sn = 0;
                if (run >= 3) {
                    unsigned ex, ne;
                    const uint32_t cl = s_cl[df_len_sym(run, ex, ne)], l = (cl >> 16) & 255u;
                    sv = (cl & 0xFFFFu) | (ex << l);             // code, extra bits, the distance code (one 0 bit)
                    sn = l + ne + 1u;
                } else if (run >= 1) {
                    const uint32_t cl = s_cl[pv], l = (cl >> 16) & 255u;
                    sv = cl & 0xFFFFu;
                    sn = l;
                    if (run == 2) { sv |= (uint64_t)(cl & 0xFFFFu) << l; sn += l; }
                }
                if (c >= 0) {
                    const uint32_t cl = s_cl[c];
                    sv |= (uint64_t)(cl & 0xFFFFu) << sn;
                    sn += (cl >> 16) & 255u;
                }
                acc |= (sv & 0xFFFFFFFFull) << nacc;             // (nacc < 32)
                nacc += sn < 32u ? sn : 32u;
                flush();
                if (sn > 32u) { acc |= (sv >> 32) << nacc; nacc += sn - 32u; flush(); }
            });
            if (nacc) atomicOr(&s_out[w], (uint32_t)acc);
            if (t == 0) {                                        // end of block, at bit hdr_bits + tot
                const uint32_t e = hdr_bits + tot, sh = e & 31u, c = eob & 0xFFFFu;
                atomicOr(&s_out[e >> 5], c << sh);
                if (sh + ((eob >> 16) & 255u) > 32u) atomicOr(&s_out[(e >> 5) + 1], c >> (32u - sh));
            }
            __syncthreads();
            if (t == 0) { sb[nbytes - 2] = 0xFF; sb[nbytes - 1] = 0xFF; }     // the empty stored block is zeros but for FF FF
        }
        __syncthreads();
        // k_mo_compact's copy, from LDS: bytes up to the destination's alignment, aligned words, bytes
        uint8_t *d = stream + 2 + a.seg_off[blk];
        int head = (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(d) & 3u)) & 3u);
        if (head > (int)nbytes) head = (int)nbytes;
        if (t < head) d[t] = sb[t];
        const int nw = ((int)nbytes - head) / 4;
        uint32_t *dw = reinterpret_cast<uint32_t *>(d + head);
        const unsigned sh = 8u * (unsigned)head;                 // destination word j = source bytes head + 4 j ..
        for (int j = t; j < nw; j += TWXSD_THREADS) {
            const uint32_t lo = s_out[j];
            dw[j] = sh ? (lo >> sh) | (s_out[j + 1] << (32u - sh)) : lo;      // (s_out has a word behind the longest block)
        }
        const int t0 = head + nw * 4;
        if (t < (int)nbytes - t0) d[t0 + t] = sb[t0 + t];
    }
    if (seg == 0 && t == 0) {                                // the stream's header and its end: the final block, the Adler-32
        stream[0] = 0x78; stream[1] = 0x01;
        uint8_t *tail = a.packed + a.row_off[row + 1] - 9;
        const uint32_t ad = a.row_adler[row];
        tail[0] = 1; tail[1] = 0; tail[2] = 0; tail[3] = 0xFF; tail[4] = 0xFF;
        tail[5] = (uint8_t)(ad >> 24); tail[6] = (uint8_t)(ad >> 16); tail[7] = (uint8_t)(ad >> 8); tail[8] = (uint8_t)ad;
    }
}

namespace {

template <class T> T *sd_carve(char *&cur, int64_t count)
{
    T *r = reinterpret_cast<T *>(cur);
    cur += sd_round256(count * (int64_t)sizeof(T));
    return r;
}

template <int ES>
int sd_run(const SdDims &d, SdArgs &a, char *work, const void *rows, uint8_t *out, int64_t out_cap, int64_t *offsets,
           int64_t *counts, float *ms, QaPool &pool, QaTimer &tm, char *errbuf, int errlen)
{
    const dim3 th(TWXSD_THREADS), grid((unsigned)d.items);
    const int64_t nsr = (d.nrows + TWXSD_SAMPLE_ROW - 1) / TWXSD_SAMPLE_ROW, nss = (d.nseg + TWXSD_SAMPLE_SEG - 1) / TWXSD_SAMPLE_SEG;
    auto t0 = std::chrono::steady_clock::now();
    QACHK(hipMemcpy(const_cast<uint8_t *>(a.rows), rows, (size_t)d.in_bytes, hipMemcpyHostToDevice));
    QACHK(hipMemset(a.hist, 0, (size_t)ES * TWX_DF_NSYM * 4));
    QACHK(hipMemset(a.counters, 0, 256));
    ms[TWXSD_NKERNELS] = qa_since(t0);
    QACHK(tm.start());
    hipLaunchKernelGGL(k_sd_hist<ES>, dim3((unsigned)(nsr * nss)), th, 0, nullptr, a);
    QACHK(hipGetLastError());
    for (int p = 0; p < ES; p += 2) {                         // k_deflate_table builds two codes side by side
        const int q = p + 1 < ES ? p + 1 : p;
        hipLaunchKernelGGL(k_deflate_table, dim3(ES > 1 ? 2 : 1), th, 0, nullptr, (const uint32_t *)(a.hist + p * TWX_DF_NSYM), a.table + p,
                           (const uint32_t *)(a.hist + q * TWX_DF_NSYM), a.table + q);
        QACHK(hipGetLastError());
    }
    QACHK(tm.stop_set(&ms[0]));
    QACHK(tm.start());
    hipLaunchKernelGGL(k_sd_count<ES>, grid, th, 0, nullptr, a);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[1]));
    QACHK(tm.start());
    hipLaunchKernelGGL(k_sd_scan, dim3((unsigned)((d.nrows + 3) / 4)), th, 0, nullptr, a, ES);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[2]));
    // the sizes (8 bytes a row) come down; their scan is the rows' offsets in the packed buffer
    std::vector<int64_t> sizes((size_t)d.nrows);
    uint32_t stored = 0, hist[ES * TWX_DF_NSYM];
    QADOWN(sizes.data(), a.row_bytes, int64_t, d.nrows);
    QADOWN(&stored, a.counters, uint32_t, 1);
    QADOWN(hist, a.hist, uint32_t, ES * TWX_DF_NSYM);
    const char *bad = sd_offsets(sizes.data(), d.nrows, d.bound, offsets);
    if (bad) {
        char msg[160];
        snprintf(msg, sizeof msg, "twxsd_deflate: %s (device fault?)", bad);
        return qa_fail(errbuf, errlen, msg);
    }
    const int64_t total = offsets[d.nrows];
    counts[TWXSD_C_BLOCKS] = d.nrows * d.nblk;
    counts[TWXSD_C_STORED] = stored;
    for (int p = 0; p < ES; ++p) counts[TWXSD_C_HALVINGS + p] = sd_halvings(hist + p * TWX_DF_NSYM);
    counts[TWXSD_C_BYTES_IN] = d.in_bytes;
    counts[TWXSD_C_BYTES_OUT] = total;
    if (total > out_cap) {
        char msg[200];
        snprintf(msg, sizeof msg, "twxsd_deflate: the packed streams need %lld bytes, out_cap is %lld", (long long)total,
                 (long long)out_cap);
        (void)qa_fail(errbuf, errlen, msg);
        return TWXSD_E_CAP;
    }
    int64_t *d_off = sd_carve<int64_t>(work, d.nrows + 1);
    a.row_off = d_off;
    QAUP(d_off, offsets, int64_t, d.nrows + 1);
    QAALLOC(pool, a.packed, uint8_t, total);
    QACHK(tm.start());
    hipLaunchKernelGGL(k_sd_emit<ES>, grid, th, 0, nullptr, a);
    QACHK(hipGetLastError());
    QACHK(tm.stop_set(&ms[3]));
    t0 = std::chrono::steady_clock::now();
    QACHK(hipMemcpy(out, a.packed, (size_t)total, hipMemcpyDeviceToHost));      // the one transfer out
    ms[TWXSD_NKERNELS + 1] = qa_since(t0);
    return TWXSD_OK;
}

}  // namespace

extern "C" int64_t twxsd_bound(int64_t n, int32_t es) { return sd_bound(n, es); }

extern "C" int twxsd_deflate(int device, const void *rows, int64_t nrows, int64_t n, int32_t es, uint8_t *out, int64_t out_cap,
                             int64_t *offsets, int64_t *counts, float *kernel_ms, char *errbuf, int errlen)
{
    SdDims d;
    const char *bad = sd_dims(nrows, n, es, (int64_t)sizeof(DfTable), &d);
    if (!bad && (!offsets || !counts)) bad = "offsets and counts must not be NULL";
    if (!bad && out_cap < 0) bad = "out_cap must not be negative";
    if (!bad && nrows > 0 && (!rows || !out)) bad = "rows and out must not be NULL";
    if (!bad && device < 0) bad = "device must not be negative";
    if (bad) {
        char msg[160];
        snprintf(msg, sizeof msg, "twxsd_deflate: %s", bad);
        return qa_fail(errbuf, errlen, msg);
    }
    float ms[TWXSD_NTIMES] = {0.f};
    for (int k = 0; k < TWXSD_C_N; ++k) counts[k] = 0;
    offsets[0] = 0;
    if (nrows == 0) {
        if (kernel_ms) for (int k = 0; k < TWXSD_NTIMES; ++k) kernel_ms[k] = 0.f;
        return TWXSD_OK;
    }
    QACHK(hipSetDevice(device));
    QaPool pool;
    QaTimer tm;
    QACHK(tm.init());
    uint8_t *d_rows = nullptr;
    char *work = nullptr;
    QAALLOC(pool, d_rows, uint8_t, d.in_bytes);
    QAALLOC(pool, work, char, d.work_bytes);
    SdArgs a{};
    a.rows = d_rows; a.n = n; a.nrows = nrows; a.nseg = (int32_t)d.nseg;
    const int64_t per = nrows * d.nblk;
    char *cur = work;
    a.seg_bytes = sd_carve<uint32_t>(cur, per);
    a.seg_off = sd_carve<uint32_t>(cur, per);
    a.adl = sd_carve<uint32_t>(cur, per * 2);
    a.piece_bits = sd_carve<uint16_t>(cur, per * TWXSD_THREADS);
    a.row_bytes = sd_carve<int64_t>(cur, nrows);
    a.row_adler = sd_carve<uint32_t>(cur, nrows);
    a.hist = sd_carve<uint32_t>(cur, (int64_t)es * TWX_DF_NSYM);
    a.table = reinterpret_cast<DfTable *>(cur);
    cur += sd_round256((int64_t)es * (int64_t)sizeof(DfTable));
    a.counters = sd_carve<uint32_t>(cur, 64);
    // (what is left is the rows' offsets, carved by sd_run)
    if (cur - work + sd_round256((nrows + 1) * 8) != d.work_bytes) return qa_fail(errbuf, errlen, "twxsd_deflate: workspace arithmetic");
    int rc;
    if (es == 4) rc = sd_run<4>(d, a, cur, rows, out, out_cap, offsets, counts, ms, pool, tm, errbuf, errlen);
    else if (es == 2) rc = sd_run<2>(d, a, cur, rows, out, out_cap, offsets, counts, ms, pool, tm, errbuf, errlen);
    else rc = sd_run<1>(d, a, cur, rows, out, out_cap, offsets, counts, ms, pool, tm, errbuf, errlen);
    if (kernel_ms) for (int k = 0; k < TWXSD_NTIMES; ++k) kernel_ms[k] = ms[k];
    return rc;
}
