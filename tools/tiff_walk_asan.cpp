// tiff_walk_asan.cpp -- the TIFF route's container walk (caesium-clt_amd/csrc/tiff_container.cpp) over the files named on the command line: for a sanitizer build of
// the host code on the CPU.  The walk reads offsets and counts a file states about itself, and the head writer copies what they point to: both are given every file
// with and without keep_metadata, the writer with one segment and with many, with and without the predictor tag.  Stand-alone, with its own main; it launches no
// kernel.  Build and run from caesium-clt_amd/csrc (the files: tests/test_tiff_emul.py's malformed_cases(), fallback_cases(), decoder_cases() and rich_file()):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DCSH_EMUL -Wall -Wno-unknown-pragmas -Wno-attributes -x c++ tiff_container.cpp -x c++ ../../tools/tiff_walk_asan.cpp -o /tmp/tiff_walk_asan
//   ASAN_OPTIONS=detect_leaks=1 /tmp/tiff_walk_asan FILE...
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../caesium-clt_amd/csrc/tiff_batch.hpp"

int main(int argc, char **argv) {
    long bad = 0, passed = 0, coded = 0, heads_written = 0;
    for (int i = 1; i < argc; i++) {
        FILE *fp = fopen(argv[i], "rb");
        if (!fp) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
        std::vector<uint8_t> raw;
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, fp)) > 0) raw.insert(raw.end(), buf, buf + n);
        fclose(fp);
        // an exact-size heap copy: a read one byte past the file is a report
        uint8_t *d = static_cast<uint8_t *>(malloc(raw.size() ? raw.size() : 1));
        memcpy(d, raw.data(), raw.size());
        for (int keep = 0; keep < 2; keep++) {
            cst_file f;
            std::string msg;
            const int rc = cst_parse(d, raw.size(), keep != 0, f, msg);
            if (!keep) printf("%s: %s%s\n", argv[i], rc ? "bad: " : f.pass ? "passed through" : "coded", rc ? msg.c_str() : "");
            if (rc) { if (rc != CS_ERR_BAD_TIFF || msg.empty()) { printf("  unexpected code %d\n", rc); return 1; } bad += !keep; continue; }
            if (f.pass) { passed += !keep; continue; }
            coded += !keep;
            for (const cst_page_src &s : f.pages) {
                if (s.seg_off.size() != s.nseg || s.seg_len.size() != s.nseg) { printf("  a coded page without its segments\n"); return 1; }
                for (uint32_t k = 0; k < s.nseg; k++) if (s.seg_off[k] + s.seg_len[k] > raw.size()) { printf("  a segment outside the file\n"); return 1; }
                for (uint32_t nout : {1u, 2u, 1000u})
                    for (int pred = 0; pred < 2; pred++) {
                        std::vector<uint8_t> heads;
                        std::vector<uint32_t> relocs;
                        cst::TiffHead H;
                        cst_write_head(d, f, s, keep != 0, 5, pred != 0, nout, 8, heads, relocs, H);
                        if (H.off + H.len != heads.size() || H.ifd_pos + 6 > H.len || H.off_pos + 4 * uint64_t(nout) > H.len || H.cnt_pos + 4 * uint64_t(nout) > H.len) { printf("  a head that does not hold its fields\n"); return 1; }
                        for (uint32_t r : relocs) if (r + 4 > H.len) { printf("  an offset field outside the head\n"); return 1; }
                        heads_written++;
                    }
            }
        }
        if (cst_declared_bytes(d, raw.size()) > (uint64_t(1) << 31)) { printf("  more decoded bytes than a coded file may have\n"); return 1; }
        free(d);
    }
    printf("%ld bad, %ld passed through, %ld coded, %ld heads written\n", bad, passed, coded, heads_written);
    return 0;
}
