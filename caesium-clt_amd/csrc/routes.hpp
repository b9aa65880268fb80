// routes.hpp -- what capi.cpp's entry points route their files through: one function per kind of input and target (route_jpeg.cpp, route_png.cpp,
// route_webp.cpp, route_gif.cpp, route_tiff.cpp) and the pieces they share.  Every route takes the files of ONE kind as a batch of their own and answers per file: outputs zeroed and results
// success-initialised by the caller (for_subset), results never null, the number of failed files returned.
#pragma once
#include <vector>

#include "../../include/caesium_hip.h"
#include "result.h"
#include "size_walk.h"

uint64_t csg_declared_pixels(const uint8_t *d, size_t n);   // gif_container.cpp: canvas x frames of a GIF file, with cs_batch_extent

namespace route {

// a JPEG span's files per device batch (CSH_GROUP overrides): see jpeg_compress
enum { CS_SPAN = 256 };

int jpeg_compress(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results);
int jpeg_compress_to_size(const CByteArray *inputs, size_t count, CCSParameters *p, size_t max_output_size, bool return_smallest, int device, CByteArray *outputs, CCSResult *results);
int jpeg_to_webp(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results);   // lossy
int jpeg_to_pixels(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results, bool lossless_webp);   // -> PNG / lossless WebP
int png_compress(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results, bool to_webp);   // PNG -> PNG / lossy WebP
int png_convert(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results, bool lossless_webp);   // PNG -> JPEG / lossless WebP
int rerun_to_size(const CByteArray *inputs, size_t count, const CCSParameters *p, size_t max_output_size, bool return_smallest, int device, CByteArray *outputs, CCSResult *results, bool webp);
int webp_inputs(const CByteArray *inputs, size_t count, const CCSParameters *p, uint32_t target, int device, CByteArray *outputs, CCSResult *results);
int gif_compress(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results, bool lossy);   // GIF -> GIF, the files CSH_GIF=device / lossy sends here
int tiff_compress(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results, int compression);   // TIFF -> TIFF, the files CSH_TIFF sends here; compression: CST_OUT_*

uint64_t webp_declared_pixels(const uint8_t *d, size_t n);   // capi.cpp, with cs_batch_extent
// the alpha planes (grey pictures in device memory) of the lossy files outs[whose[j]]: the VP8L coder over them, each attached as an ALPH chunk (vp8l_encode.cpp).
// A file whose plane fails loses its output and gets the failure as its result; returns how many did.
int attach_alpha_planes(const std::vector<csp_pixels> &planes, const std::vector<size_t> &whose, CByteArray *outs, CCSResult *results, int device);

inline uint64_t png_declared_pixels(const uint8_t *d) {   // IHDR's width x height; the caller has seen that the file is long enough
    const uint64_t w = (uint64_t(d[16]) << 24) | (d[17] << 16) | (d[18] << 8) | d[19], h = (uint64_t(d[20]) << 24) | (d[21] << 16) | (d[22] << 8) | d[23];
    return w * h;
}

// how many of the files in front go into one device batch: files are taken until there are max_files of them, or the next one would take the files' bytes
// past byte_cap or the sum of estimate(file) past pool_cap; the first file always goes in
const uint64_t NO_CAP = ~uint64_t(0);
template <class Estimate>
size_t group_extent(const CByteArray *inputs, size_t count, size_t max_files, uint64_t byte_cap, uint64_t pool_cap, Estimate estimate) {
    uint64_t bytes = 0, pools = 0;
    size_t n = 0;
    while (n < count && n < max_files) {
        const uint64_t len = inputs[n].length, est = estimate(inputs[n]);
        if (n && (bytes + len > byte_cap || pools + est > pool_cap)) break;
        bytes += len; pools += est; n++;
    }
    return n;
}

// the files idx[] of a call through one route, as a batch of their own, and what comes back into their places
template <class Fn>
int for_subset(const CByteArray *inputs, const std::vector<size_t> &idx, CByteArray *outputs, CCSResult *results, Fn fn) {
    if (idx.empty()) return 0;
    std::vector<CByteArray> in(idx.size()), out(idx.size(), CByteArray{nullptr, 0});
    std::vector<CCSResult> res(idx.size(), make_result(0, nullptr));
    for (size_t k = 0; k < idx.size(); k++) in[k] = inputs[idx[k]];
    const int failed = fn(in.data(), in.size(), out.data(), res.data());
    for (size_t k = 0; k < idx.size(); k++) { outputs[idx[k]] = out[k]; results[idx[k]] = res[k]; }
    return failed;
}

// One file's try of a size walk has come back as cur / res.  Returns the quality of its next try (cur and res released), or 0 when the file leaves the walk:
// its file -- or none -- in output, its result in result (which held success), failed counted up for a failure.  one_try: quality does not apply (lossless).
inline int walk_advance(SizeWalk &w, bool one_try, CByteArray &cur, CCSResult &res, size_t max_output_size, bool return_smallest, CByteArray &output, CCSResult &result, int &failed) {
    if (!res.success) { w.done = true; result = res; failed++; return 0; }
    const WalkStep s = one_try ? WalkStep{WalkStep::KEEP, w.quality, nullptr} : step(w, cur.length, max_output_size, return_smallest);
    if (s.what == WalkStep::TRY) { cs_free_bytes(&cur); cs_free_result(&res); return s.quality; }
    w.done = true;
    if (s.what == WalkStep::KEEP) { output = cur; result = res; }
    else { cs_free_bytes(&cur); cs_free_result(&res); result = make_result(CS_ERR_TOO_BIG, s.msg); failed++; }
    return 0;
}

}  // namespace route
