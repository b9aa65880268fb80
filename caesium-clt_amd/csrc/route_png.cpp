// route_png.cpp -- PNG inputs: the PNG row's groups (PNG -> PNG, PNG -> lossy WebP), the conversions that decode and code in one call of the row (PNG -> JPEG /
// lossless WebP), and the size walk that runs a route again per try (PNG and WebP files)
#include <chrono>
#include <cstdio>
#include <map>

#include "routes.hpp"

namespace route {

// PNG -> PNG (png.optimize: lossless, else the quantising form of the same pipeline) and PNG -> lossy WebP: groups sized by what they occupy in HBM -- per file
// the inflated stream, the pixels, one filtered stream per trial slot (up to 10) and the output region, ~13 x the raw size.
// png.force_zopfli (--zopfli): libcaesium hands the streams to zopfli; here the same coder runs CSP_DEEP_ITERS_ZOPFLI passes of its cost model
// over the chunks that take the min-cost-path parse (png_run.cpp, png_parse.h)
int png_compress(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results, bool to_webp) {
    int failed_total = 0;
    for (size_t g0 = 0, n = 0; g0 < count; g0 += n) {
        n = group_extent(inputs + g0, count - g0, 4096, NO_CAP, uint64_t(96) << 30, [](const CByteArray &f) {
            return uint64_t(1 << 20) + (f.length >= 33 ? png_declared_pixels(f.data) * 8 * 14 : 0);   // at most 8 bytes per pixel
        });
        csp_batch *b = nullptr;
        const bool trace = getenv("CSH_TRACE") != nullptr;
        auto t0 = std::chrono::steady_clock::now();
        int rc = to_webp ? csp_batch_create_webp(inputs + g0, n, p, device, &b) : csp_batch_create(inputs + g0, n, p, device, &b);
        auto t1 = std::chrono::steady_clock::now();
        if (rc == 0) rc = csp_batch_run(b, nullptr);
        auto t2 = std::chrono::steady_clock::now();
        if (rc != 0) {
            for (size_t i = 0; i < n; i++) { outputs[g0 + i].data = nullptr; outputs[g0 + i].length = 0; results[g0 + i] = make_result(rc, csh_last_error()); }
            failed_total += int(n);
        } else {
            int failed = csp_batch_fetch(b, outputs + g0, results + g0);
            failed_total += failed < 0 ? int(n) : failed;
        }
        csp_batch_destroy(b);
        if (trace) {
            auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            fprintf(stderr, "[csh] %zu PNG files on device %d: create %.1f ms, run %.1f ms, fetch+destroy %.1f ms\n", n, device, ms(t0, t1), ms(t1, t2), ms(t2, std::chrono::steady_clock::now()));
        }
    }
    return failed_total;
}

// PNG -> JPEG (alpha dropped) and PNG -> lossless WebP (the same decode, the VP8L coder behind it): groups of at most 256 files and 96 GB of decode buffers
// (8 bytes per pixel at most, three regions)
int png_convert(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results, bool lossless_webp) {
    int failed_total = 0;
    for (size_t g0 = 0, n = 0; g0 < count; g0 += n) {
        n = group_extent(inputs + g0, count - g0, 256, NO_CAP, uint64_t(96) << 30, [](const CByteArray &f) {
            return uint64_t(1 << 20) + (f.length >= 33 ? png_declared_pixels(f.data) * 24 : 0);
        });
        failed_total += lossless_webp ? csp_png_to_lossless_webp(inputs + g0, n, p, device, outputs + g0, results + g0) : csp_png_to_jpeg(inputs + g0, n, p, device, outputs + g0, results + g0);
    }
    return failed_total;
}

// PNG and WebP files under --max-size: the size walk (size_walk.h) over png.quality (the quantiser's palette size follows it) or webp.quality.  Every try is a
// full run of the route for the files still searching (libcaesium's png::compress / webp::compress per try), grouped by the quality they are at: the first
// round is one batch, later rounds a few; under png.optimize the quality does not apply and one try is all there is
int rerun_to_size(const CByteArray *inputs, size_t count, const CCSParameters *p, size_t max_output_size, bool return_smallest, int device, CByteArray *outputs, CCSResult *results, bool webp) {
    int failed_total = 0;
    std::vector<SizeWalk> walk(count);
    for (;;) {   // rounds: at most ten per file (SizeWalk::tries)
        std::map<int, std::vector<size_t>> by_quality;
        for (size_t i = 0; i < count; i++) if (!walk[i].done) by_quality[walk[i].quality].push_back(i);
        if (by_quality.empty()) break;
        for (auto &g : by_quality) {
            const std::vector<size_t> &idx = g.second;
            std::vector<CByteArray> cur(count);
            std::vector<CCSResult> res(count);
            CCSParameters q = *p;
            q.png_quality = q.webp_quality = uint32_t(g.first);
            for_subset(inputs, idx, cur.data(), res.data(), [&](const CByteArray *in, size_t n, CByteArray *out, CCSResult *r) {
                return webp ? webp_inputs(in, n, &q, CS_TYPE_WEBP, device, out, r) : png_compress(in, n, &q, device, out, r, false);
            });
            for (size_t i : idx) walk_advance(walk[i], !webp && p->png_optimize, cur[i], res[i], max_output_size, return_smallest, outputs[i], results[i], failed_total);
        }
    }
    return failed_total;
}

}  // namespace route
