// route_jpeg.cpp -- JPEG inputs: the compress call in spans on worker threads, the size walk over the retained DCT, and the conversions (lossy WebP from the
// same batch object; PNG and lossless WebP from the decoded pixels in device memory)
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <thread>

#include "routes.hpp"

namespace route {

// One device batch of a span; a group that fails as a whole for want of memory is tried again in halves
static int jpeg_span_compress(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results, size_t span) {
    int failed_total = 0;
    size_t limit = span;   // halved when a whole group fails for want of memory: one oversized neighbour must not fail the others;
    for (size_t g0 = 0; g0 < count;) {   // back to the full group once a group has gone through (the shortage belonged to those files)
        size_t n = cs_batch_extent(inputs + g0, count - g0);
        if (n > limit) n = limit;
        csh_batch *b = nullptr;
        const bool trace = getenv("CSH_TRACE") != nullptr;   // host-side phase times of the boundary call, on stderr
        auto t0 = std::chrono::steady_clock::now();
        int rc = csh_batch_create(inputs + g0, n, p, device, &b);
        auto t1 = std::chrono::steady_clock::now();
        if (rc == 0) rc = csh_batch_run(b, nullptr);
        auto t2 = std::chrono::steady_clock::now();
        if (rc != 0) {
            csh_batch_destroy(b);
            if (n > 1 && (rc == CS_ERR_NO_DEVICE || rc == CS_ERR_POOL_OVERFLOW) && csh_device_count() > device) { limit = (n + 1) / 2; continue; }   // same files again, in smaller groups
            for (size_t i = 0; i < n; i++) results[g0 + i] = make_result(rc, csh_last_error());
            failed_total += int(n);
            g0 += n;
            continue;
        }
        int failed = csh_batch_fetch(b, outputs + g0, results + g0);
        auto t3 = std::chrono::steady_clock::now();
        csh_batch_destroy(b);
        if (trace) {
            auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            fprintf(stderr, "[csh] %zu files on device %d: create %.1f ms, run %.1f ms, fetch %.1f ms, destroy %.1f ms\n", n, device, ms(t0, t1), ms(t1, t2), ms(t2, t3),
                    ms(t3, std::chrono::steady_clock::now()));
        }
        failed_total += failed < 0 ? int(n) : failed;
        g0 += n;
        limit = span;
    }
    return failed_total;
}

// Device batches of one boundary call: at most CS_SPAN files each (CSH_GROUP overrides), up to three in flight on as many host threads -- one is parsed
// and uploaded while another is in its kernels, and the second batch onwards reuses the first ones' device pools (devmem.hpp).  One batch
// of 2048 files allocated ~100 GB at once: 0.7 s when everything was cached, 4-10 s when it was not (measured); batches of
// 256 take 13 GB each and the call's time no longer depends on what the cache happens to hold (2048 files: 0.50-0.55 s warm, 0.9 s cold).
int jpeg_compress(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results) {
    for (size_t i = 0; i < count; i++) { outputs[i].data = nullptr; outputs[i].length = 0; }
    const size_t span = getenv("CSH_GROUP") ? std::max<size_t>(1, size_t(atol(getenv("CSH_GROUP")))) : size_t(CS_SPAN);
    if (count <= span) return jpeg_span_compress(inputs, count, p, device, outputs, results, span);
    const size_t nspans = (count + span - 1) / span;
    std::atomic<size_t> next{0};
    std::atomic<int> failed{0};
    auto worker = [&]() {
        for (size_t k; (k = next++) < nspans;)
            failed += jpeg_span_compress(inputs + k * span, std::min(span, count - k * span), p, device, outputs + k * span, results + k * span, span);
    };
    const size_t nworkers = std::min<size_t>(nspans, getenv("CSH_WORKERS") ? std::max<size_t>(1, size_t(atol(getenv("CSH_WORKERS")))) : 3);   // three batches in flight: one in its kernels, one being parsed and uploaded, one being fetched (2048 x 1080p: 181 ms with 2, 156 with 3, no gain beyond)
    std::vector<std::thread> others;
    for (size_t t = 1; t < nworkers; t++) others.emplace_back(worker);
    worker();
    for (auto &t : others) t.join();
    return failed.load();
}

// The size walk (size_walk.h) in its device form: the whole group is decoded and transformed ONCE (unquantised DCT retained in HBM); every round re-quantises
// and re-codes with each file's current quality, and files leave the search as they finish.
int jpeg_compress_to_size(const CByteArray *inputs, size_t count, CCSParameters *p, size_t max_output_size, bool return_smallest, int device, CByteArray *outputs, CCSResult *results) {
    for (size_t i = 0; i < count; i++) { outputs[i].data = nullptr; outputs[i].length = 0; results[i] = make_result(0, nullptr); }
    int failed_total = 0;
    for (size_t g0 = 0, n = 0; g0 < count; g0 += n) {
        n = cs_batch_extent(inputs + g0, count - g0);
        p->jpeg_quality = p->png_quality = p->webp_quality = 80;
        csh_batch *b = nullptr;
        int rc = csh_batch_create(inputs + g0, n, p, device, &b);
        if (rc == 0 && !p->jpeg_optimize) rc = csh_batch_retain_dct(b, 1) ? CS_ERR_NO_DEVICE : 0;
        std::vector<SizeWalk> walk(n);
        std::vector<uint32_t> q(n, 0);
        std::vector<CByteArray> cur(n);
        std::vector<CCSResult> res(n);
        for (int round = 0; rc == 0; round++) {
            rc = round == 0 ? csh_batch_run(b, nullptr) : csh_batch_rerun_encode(b, nullptr);
            if (rc) break;
            if (csh_batch_fetch(b, cur.data(), res.data()) < 0) { rc = CS_ERR_NO_DEVICE; break; }
            bool any = false;
            for (size_t i = 0; i < n; i++) {
                if (walk[i].done) { q[i] = 0; cs_free_bytes(&cur[i]); cs_free_result(&res[i]); continue; }
                // jpeg.optimize is lossless: quality does not apply, one try
                q[i] = uint32_t(walk_advance(walk[i], p->jpeg_optimize, cur[i], res[i], max_output_size, return_smallest, outputs[g0 + i], results[g0 + i], failed_total));
                any |= q[i] != 0;
            }
            if (!any) break;
            if (csh_batch_set_quality(b, q.data())) { rc = CS_ERR_NO_DEVICE; break; }
        }
        if (rc)
            for (size_t i = 0; i < n; i++)
                if (!walk[i].done) { cs_free_result(&results[g0 + i]); results[g0 + i] = make_result(rc, csh_last_error()); failed_total++; }
        // the reference leaves the quality of the last try in its &mut CSParameters; with many files that is per file, so a
        // batch reports the first file's
        if (g0 == 0 && n) p->jpeg_quality = p->png_quality = p->webp_quality = uint32_t(walk[0].quality);
        csh_batch_destroy(b);
    }
    return failed_total;
}

// JPEG -> lossy WebP: the JPEG path's decode and resize, then the VP8 encoder, in one batch object
int jpeg_to_webp(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results) {
    int failed_total = 0;
    for (size_t g0 = 0, n = 0; g0 < count; g0 += n) {
        n = cs_batch_extent(inputs + g0, std::min<size_t>(count - g0, 1024));
        csh_batch *b = nullptr;
        int rc = csh_batch_create_webp(inputs + g0, n, p, device, &b);
        if (rc == 0) rc = csh_batch_run(b, nullptr);
        const int failed = rc ? -1 : csh_batch_fetch(b, outputs + g0, results + g0);   // (a fetch that fails has written nothing)
        for (size_t k = 0; k < n && failed < 0; k++) results[g0 + k] = make_result(rc ? rc : CS_ERR_NO_DEVICE, csh_last_error());
        csh_batch_destroy(b);
        failed_total += failed < 0 ? int(n) : failed;
    }
    return failed_total;
}

// JPEG -> PNG / lossless WebP: the JPEG path's decode and resize leave the pixels in device memory, the PNG coder (lossless under png.optimize, quantising
// otherwise -- what png::compress does to the intermediate file libcaesium makes) or the VP8L coder takes them from there
int jpeg_to_pixels(const CByteArray *inputs, size_t count, const CCSParameters *p, int device, CByteArray *outputs, CCSResult *results, bool lossless_webp) {
    int failed_total = 0;
    for (size_t g0 = 0, n = 0; g0 < count; g0 += n) {
        // the PNG coder keeps about 14 bytes per sample in flight: groups of at most 512 files and 400 MB of JPEG (some 5 GB of pixels)
        n = group_extent(inputs + g0, count - g0, 512, uint64_t(400) << 20, NO_CAP, [](const CByteArray &) { return uint64_t(0); });
        csh_batch *jb = nullptr;
        csp_batch *pb = nullptr;
        int rc = csh_batch_create_pixels(inputs + g0, n, p, device, &jb);
        if (rc == 0) rc = csh_batch_run(jb, nullptr);
        std::vector<csp_pixels> px;
        std::vector<size_t> at;
        for (size_t k = 0; k < n && rc == 0; k++) {
            csp_pixels s; const char *msg = "";
            const int code = csh_batch_pixels(jb, k, &s.device_pixels, &s.width, &s.height, &s.channels, &msg);
            if (code) { results[g0 + k] = make_result(code, msg); failed_total++; } else { px.push_back(s); at.push_back(g0 + k); }
        }
        if (rc) { for (size_t k = 0; k < n; k++) results[g0 + k] = make_result(rc, csh_last_error()); failed_total += int(n); }
        else if (!px.empty()) {
            std::vector<CByteArray> out(px.size());
            std::vector<CCSResult> res(px.size());
            int failed = -1;
            if (lossless_webp) failed = csl_encode_pixels(px.data(), px.size(), device, out.data(), res.data());
            else {
                rc = csp_batch_create_pixels(px.data(), px.size(), p, device, &pb);
                if (rc == 0) rc = csp_batch_run(pb, nullptr);
                if (rc == 0 && (failed = csp_batch_fetch(pb, out.data(), res.data())) < 0) rc = CS_ERR_NO_DEVICE;
            }
            for (size_t k = 0; k < px.size(); k++) {
                if (rc) results[at[k]] = make_result(rc, csh_last_error());
                else { outputs[at[k]] = out[k]; results[at[k]] = res[k]; }
            }
            failed_total += rc ? int(px.size()) : failed;
        }
        csp_batch_destroy(pb);
        csh_batch_destroy(jb);
    }
    return failed_total;
}

}  // namespace route
