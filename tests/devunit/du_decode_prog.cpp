// du_decode_prog.cpp -- device unit over caesium-clt_amd/csrc/k_decode_prog.hip: WaveReader, the MSB-first wave-uniform bit reader whose window of 64
// words lives one word a lane.  One reader per wave.  See du_common.h.
#include "../../caesium-clt_amd/csrc/k_decode_prog.hip"
#include "du_common.h"
using namespace csh;

// As k_du_lereader (du_wave.cpp): a wave reads pool + off[wave] (4-byte aligned), len[wave] bytes, from its start; step i is (0 get(n) / 1 peek16() / 2 skip(n), n).
// val / over: [nwaves][nsteps] -- what the step returned (0 for a skip) and insufficient() behind it
__global__ void __launch_bounds__(256) k_du_wavereader(const uint8_t *__restrict__ pool, const uint32_t *__restrict__ off, const uint32_t *__restrict__ len,
                                                       const int32_t *__restrict__ script, int nsteps, uint32_t *__restrict__ val, uint32_t *__restrict__ over) {
    const uint32_t wave = DU_WAVE_INDEX();
    WaveReader rd;
    rd.begin(pool + uniform32(off[wave]), uniform32(len[wave]));
    for (int i = 0; i < nsteps; i++) {
        const int what = int(uniform32(uint32_t(script[2 * i]))), n = int(uniform32(uint32_t(script[2 * i + 1])));
        uint32_t v = 0;
        if (what == 0) v = rd.get(n); else if (what == 1) v = rd.peek16(); else rd.skip(n);
        const uint32_t o = rd.insufficient() ? 1u : 0u;
        VFOR(l) if (l == (i & 63)) { val[size_t(wave) * nsteps + i] = v; over[size_t(wave) * nsteps + i] = o; }
    }
}

extern "C" {
int csdu_wavereader(int nwaves, int wpb, const uint8_t *pool, size_t pool_bytes, const uint32_t *off, const uint32_t *len, const int32_t *script, int nsteps, uint32_t *val, uint32_t *over) {
    if ((wpb != 1 && wpb != 4) || nwaves <= 0 || nwaves % wpb || nsteps <= 0) return -1;
    for (int w = 0; w < nwaves; w++) if ((off[w] & 3u) || size_t(off[w]) + len[w] > pool_bytes) return -1;
    for (int i = 0; i < nsteps; i++) if (script[2 * i] < 0 || script[2 * i] > 2 || script[2 * i + 1] < 1 || script[2 * i + 1] > 32) return -1;
    DuBufs B;
    uint8_t *d_pool;
    uint32_t *d_off, *d_len, *d_val, *d_over;
    int32_t *d_script;
    const size_t nb = size_t(nwaves) * nsteps * 4;
    DU_TRY(B.upload(&d_pool, pool, pool_bytes));
    DU_TRY(B.upload(&d_off, off, size_t(nwaves) * 4));
    DU_TRY(B.upload(&d_len, len, size_t(nwaves) * 4));
    DU_TRY(B.upload(&d_script, script, size_t(nsteps) * 8));
    DU_TRY(B.zeroed(&d_val, nb, 0x55));
    DU_TRY(B.zeroed(&d_over, nb, 0x55));
    DU_WAVE_LAUNCH(k_du_wavereader, nwaves, wpb, d_pool, d_off, d_len, d_script, nsteps, d_val, d_over);
    DU_TRY(du_finish());
    DU_TRY(du_download(val, d_val, nb));
    return du_download(over, d_over, nb);
}
}
