// routes_asan.cpp -- the C entry points over the files named on the command line, as one mixed batch: for a sanitizer build of the emulation sources on the
// CPU (the routes pass malloc'd outputs and messages through several hands).  Stand-alone, with its own main; build and run from caesium-clt_amd/csrc:
// (shift checks off, as in asan_emul.sh: the emulation's __mul24 shim shifts negative ints; UBSan reports and goes on, so look at what it prints):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize=shift -ffp-contract=off -DCSH_EMUL -Wno-unknown-pragmas -Wno-attributes \
//       $(for f in k_*.hip *.cpp; do echo -x c++ $f; done) -x c++ ../../tools/routes_asan.cpp -o /tmp/routes_asan -lpthread
//   ASAN_OPTIONS=detect_leaks=1 /tmp/routes_asan FILE...
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/caesium_hip.h"

static std::vector<std::string> blobs;
static std::vector<CByteArray> inputs;
static long calls = 0, items = 0, failures = 0;

// one call's outputs and results looked at and released; null_results: the call had no results array
static void done(const char *what, int failed, std::vector<CByteArray> &out, std::vector<CCSResult> &res, bool null_results) {
    int counted = 0;
    for (size_t i = 0; i < out.size(); i++) {
        if (!null_results && !res[i].success) counted++;
        if (!null_results && res[i].success && !out[i].data) { printf("%s: item %zu succeeded without an output\n", what, i); failures++; }
        if (out[i].data && out[i].length) { volatile uint8_t touch = out[i].data[0] ^ out[i].data[out[i].length - 1]; (void)touch; }   // the whole region is the caller's
        if (!null_results && res[i].error_message) { volatile size_t n = strlen(res[i].error_message); (void)n; }
        cs_free_bytes(&out[i]);
        if (!null_results) cs_free_result(&res[i]);
    }
    if (!null_results && counted != failed) { printf("%s: returned %d failures, results say %d\n", what, failed, counted); failures++; }
    calls++; items += long(out.size());
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; i++) {
        FILE *f = fopen(argv[i], "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
        std::string s; char buf[65536]; size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
        fclose(f);
        blobs.push_back(s);
    }
    for (std::string &s : blobs) inputs.push_back(CByteArray{reinterpret_cast<uint8_t *>(&s[0]), s.size()});
    const size_t n = inputs.size();
    auto fresh = [&](std::vector<CByteArray> &out, std::vector<CCSResult> &res) { out.assign(n, CByteArray{nullptr, 0}); res.assign(n, CCSResult{false, 0, nullptr}); };
    std::vector<CByteArray> out;
    std::vector<CCSResult> res;
    for (int null_results = 0; null_results < 2; null_results++) {
        CCSResult *r = nullptr;
        for (int k = 0; k < 6; k++) {   // cs_batch_compress: lossy, optimize, a width, keep_metadata, webp_lossless, lossless with a width and metadata
            CCSParameters p; cs_default_parameters(&p);
            if (k == 0) { p.jpeg_quality = 70; p.png_quality = 60; p.webp_quality = 65; }
            if (k == 1) { p.jpeg_optimize = p.png_optimize = true; p.png_optimization_level = 2; }
            if (k == 2) p.width = 24;
            if (k == 3) p.keep_metadata = true;
            if (k == 4) p.webp_lossless = true;
            if (k == 5) { p.webp_lossless = true; p.width = 20; p.keep_metadata = true; }
            fresh(out, res); r = null_results ? nullptr : res.data();
            done("compress", cs_batch_compress(inputs.data(), n, &p, 0, out.data(), r), out, res, null_results != 0);
        }
        for (size_t target : {size_t(1) << 20, size_t(1500), size_t(40)})   // fits at once, needs the walk, nothing reaches it
            for (int smallest = 0; smallest < 2; smallest++) {
                CCSParameters p; cs_default_parameters(&p);
                fresh(out, res); r = null_results ? nullptr : res.data();
                done("compress_to_size", cs_batch_compress_to_size(inputs.data(), n, &p, target, smallest != 0, 0, out.data(), r), out, res, null_results != 0);
            }
        for (uint32_t fmt : {uint32_t(CS_TYPE_JPEG), uint32_t(CS_TYPE_PNG), uint32_t(CS_TYPE_WEBP)})
            for (int k = 0; k < 4; k++) {   // plain, a width, lossless, lossless with a width
                CCSParameters p; cs_default_parameters(&p);
                if (k & 1) p.width = 24;
                if (k & 2) { p.webp_lossless = true; p.png_optimize = true; p.png_optimization_level = 1; }
                fresh(out, res); r = null_results ? nullptr : res.data();
                done("convert", cs_batch_convert(inputs.data(), n, &p, fmt, 0, out.data(), r), out, res, null_results != 0);
            }
    }
    for (size_t i = 0; i < n; i++) {   // the three *_in_memory forms, file by file
        CCSParameters p; cs_default_parameters(&p);
        CByteArray o{nullptr, 0};
        CCSResult a = cs_compress_in_memory(inputs[i].data, inputs[i].length, &p, &o); cs_free_bytes(&o); cs_free_result(&a);
        a = cs_compress_to_size_in_memory(inputs[i].data, inputs[i].length, &p, 1500, true, &o); cs_free_bytes(&o); cs_free_result(&a);
        cs_default_parameters(&p);
        a = cs_convert_in_memory(inputs[i].data, inputs[i].length, &p, CS_TYPE_PNG, &o); cs_free_bytes(&o); cs_free_result(&a);
        calls += 3; items += 3;
    }
    csh_release_cached_memory();
    printf("%ld calls, %ld items, %ld inconsistencies\n", calls, items, failures);
    return failures ? 1 : 0;
}
