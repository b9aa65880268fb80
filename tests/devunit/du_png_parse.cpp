// du_png_parse.cpp -- device units over the two halves of the PNG row's DEFLATE parse on arbitrary bytes: lz_chunk (caesium-clt_amd/csrc/png_lz.h, the greedy
// tokenizer on one wave) and deep_chunk (png_parse.h, the min-cost-path parse on a workgroup of CSP_DEEP_THREADS with its tables in a CSH_SHARED DeepLds and its
// 512 KiB scratch area in device memory), each called the way its kernels call it, with a sink that records instead of coding.  The stream need not be a filtered
// PNG: tests/_deflate_parse_model.py says what must come back.  See du_common.h.
#include "../../caesium-clt_amd/csrc/png_parse.h"
#include "du_common.h"
using namespace csp;

// per position of the chunk: the length (0: a literal), the distance, the byte, and whether the parse visits it
struct RecSink {
    uint32_t *len, *dist;
    uint8_t *lit, *taken;
    uint64_t start;
    __device__ __forceinline__ void tile(uint64_t t0, uint32_t count, uint64_t tk, const LV<uint32_t> &mlen, const LV<uint32_t> &mdist, const LV<uint32_t> &l) {
        LFOR(j) if (uint32_t(j) < count) {
            const uint64_t at = t0 - start + uint32_t(j);
            len[at] = mlen[j]; dist[at] = mdist[j]; lit[at] = uint8_t(l[j]); taken[at] = uint8_t((tk >> j) & 1u);
        }
    }
};

__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_du_lz_chunk(const uint8_t *__restrict__ data, uint64_t total, uint64_t start, uint64_t end, RecSink sink) {
    CSH_SHARED LzLds L;
    lz_chunk(data, total, start, end, L, sink);
}

// as k_png_deep_emit calls it: every wave enters, the first one walks the path and feeds the sink, the others wait at the barrier behind the call
__global__ void __launch_bounds__(CSP_DEEP_THREADS) k_du_deep_chunk(const uint8_t *__restrict__ data, uint64_t total, uint64_t start, uint64_t end, uint8_t *scratch, int iters, RecSink sink,
                                                                    uint32_t *__restrict__ out_hist) {
    CSH_SHARED DeepLds S;
    deep_chunk(data, total, start, end, S, scratch, iters, true, sink);
    if (CSP_WAVE0) {
        CSP_WAVE_SYNC();
        LFOR(l) for (uint32_t i = uint32_t(l); i < CSP_NSYM; i += 64) out_hist[i] = S.hist[i];
    }
    CSP_WG_SYNC();
}

// what both entries take: the stream at buf + front (front >= 64: the eight bytes in front of a position are read wherever it lies), `total` bytes, 64 bytes of
// slack behind it (png_plan.cpp: stream_stride = align_up(raw_len + 64, 256)); one chunk [start, end) of it, as the product cuts them
static bool du_chunk_ok(size_t front, size_t total, size_t start, size_t end) {
    return front >= 64 && front <= (1u << 20) && total <= (1u << 24) && start % CSP_CHUNK == 0 && start <= total && end > start && end <= total && end - start <= CSP_CHUNK;
}

extern "C" {
// buf: front + total + 64 bytes.  out_len / out_dist: uint32[end - start]; out_lit / out_taken: uint8[end - start]
int csdu_lz_chunk(const uint8_t *buf, size_t front, size_t total, size_t start, size_t end, uint32_t *out_len, uint32_t *out_dist, uint8_t *out_lit, uint8_t *out_taken) {
    if (!du_chunk_ok(front, total, start, end)) return -1;
    const size_t n = end - start;
    DuBufs B;
    uint8_t *d_buf;
    RecSink sink;
    DU_TRY(B.upload(&d_buf, buf, front + total + 64));
    DU_TRY(B.zeroed(&sink.len, n * 4, 0x55));
    DU_TRY(B.zeroed(&sink.dist, n * 4, 0x55));
    DU_TRY(B.zeroed(&sink.lit, n, 0x55));
    DU_TRY(B.zeroed(&sink.taken, n, 0x55));
    sink.start = start;
    CSH_LAUNCH(k_du_lz_chunk, dim3(1), dim3(CSP_WAVE_THREADS), 0, d_buf + front, uint64_t(total), uint64_t(start), uint64_t(end), sink);
    DU_TRY(du_finish());
    DU_TRY(du_download(out_len, sink.len, n * 4));
    DU_TRY(du_download(out_dist, sink.dist, n * 4));
    DU_TRY(du_download(out_lit, sink.lit, n));
    return du_download(out_taken, sink.taken, n);
}
// scratch_fill: the byte the scratch area holds before the launch.  out_scratch: CSP_DEEP_SCRATCH bytes (png_parse.h lays them out); out_hist: uint32[CSP_NSYM]
int csdu_deep_chunk(const uint8_t *buf, size_t front, size_t total, size_t start, size_t end, int iters, int scratch_fill, uint32_t *out_len, uint32_t *out_dist, uint8_t *out_lit,
                    uint8_t *out_taken, uint8_t *out_scratch, uint32_t *out_hist) {
    if (!du_chunk_ok(front, total, start, end) || iters < 1 || iters > 64 || scratch_fill < 0 || scratch_fill > 255) return -1;
    const size_t n = end - start;
    DuBufs B;
    uint8_t *d_buf, *d_scratch;
    uint32_t *d_hist;
    RecSink sink;
    DU_TRY(B.upload(&d_buf, buf, front + total + 64));
    DU_TRY(B.zeroed(&d_scratch, CSP_DEEP_SCRATCH, scratch_fill));
    DU_TRY(B.zeroed(&d_hist, CSP_NSYM * 4, 0x55));
    DU_TRY(B.zeroed(&sink.len, n * 4, 0x55));
    DU_TRY(B.zeroed(&sink.dist, n * 4, 0x55));
    DU_TRY(B.zeroed(&sink.lit, n, 0x55));
    DU_TRY(B.zeroed(&sink.taken, n, 0x55));
    sink.start = start;
    CSH_LAUNCH(k_du_deep_chunk, dim3(1), dim3(CSP_DEEP_THREADS), 0, d_buf + front, uint64_t(total), uint64_t(start), uint64_t(end), d_scratch, iters, sink, d_hist);
    DU_TRY(du_finish());
    DU_TRY(du_download(out_len, sink.len, n * 4));
    DU_TRY(du_download(out_dist, sink.dist, n * 4));
    DU_TRY(du_download(out_lit, sink.lit, n));
    DU_TRY(du_download(out_taken, sink.taken, n));
    DU_TRY(du_download(out_scratch, d_scratch, CSP_DEEP_SCRATCH));
    return du_download(out_hist, d_hist, CSP_NSYM * 4);
}
}
