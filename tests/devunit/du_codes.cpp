// du_codes.cpp -- device unit over caesium-clt_amd/csrc/png_codes.h: csp::code_lengths and csp::canonical, one lane per code with the arrays in scratch, as
// k_png_codes and the lossless WebP coders run them: the 64 lanes of a wave work on 64 different histograms at once.  See du_common.h.
#include "../../caesium-clt_amd/csrc/png_codes.h"
#include "du_common.h"
using namespace csp;

// case c: freq[c * n ..] -> len[c * n ..], code[c * n ..]; lane l of wave w takes case 64 w + l
__global__ void __launch_bounds__(256) k_du_code_lengths(int ncases, int n, int limit, const uint32_t *__restrict__ freq, uint8_t *__restrict__ len, uint16_t *__restrict__ code) {
    const uint32_t wave = DU_WAVE_INDEX();
    LFOR(l) {
        const uint32_t c = wave * 64u + uint32_t(l);
        if (c < uint32_t(ncases)) {
            const size_t at = size_t(c) * size_t(n);
            code_lengths(freq + at, n, limit, len + at);
            canonical(len + at, n, code + at);
        }
    }
}

extern "C" {
// refused: an alphabet code_lengths' arrays do not hold (288), a limit outside what canonical() can code, a limit the alphabet does not fit under
int csdu_code_lengths(int ncases, int n, int limit, const uint32_t *freq, uint8_t *len, uint16_t *code) {
    if (ncases <= 0 || n < 2 || n > 288 || limit < 7 || limit > 15 || (1 << limit) < n) return -1;
    DuBufs B;
    uint32_t *d_f;
    uint8_t *d_l;
    uint16_t *d_c;
    const size_t cnt = size_t(ncases) * size_t(n);
    DU_TRY(B.upload(&d_f, freq, cnt * 4));
    DU_TRY(B.zeroed(&d_l, cnt, 0x55));
    DU_TRY(B.zeroed(&d_c, cnt * 2, 0x55));
    DU_WAVE_LAUNCH(k_du_code_lengths, (ncases + 63) / 64, 1, ncases, n, limit, d_f, d_l, d_c);
    DU_TRY(du_finish());
    DU_TRY(du_download(len, d_l, cnt));
    return du_download(code, d_c, cnt * 2);
}
}
