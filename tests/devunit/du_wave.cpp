// du_wave.cpp -- device units over the wave helpers of caesium-clt_amd/csrc/png_wave.h and wave.h (scans, sums, minima, lane moves, the ballot, the
// LSB-first bit reader) and the unaligned loads / byte alignment of png_lz.h.  One case per wave; workgroups of one and of four waves.  See du_common.h.
#include "../../caesium-clt_amd/csrc/wave.h"
#include "../../caesium-clt_amd/csrc/png_lz.h"
#include "du_common.h"
using namespace csh;

// op: 0 lscan (out = the scan, out2 = its total)  1 lsum32  2 lprev (arg[0]: carry)  3 llast  4 lget (arg[0]: lane)  5 lset (arg[0]: lane, arg[1]: value)
//     6 lballot of "in != 0" (out = low word, out2 = high word)  7 uni (arg[0])
// in / out / out2: [nwaves][64]; arg: [nwaves][2], wave-uniform.  Every lane writes what it holds, so a wave-uniform result is checked in every lane.
__global__ void __launch_bounds__(256) k_du_wave32(int op, const uint32_t *__restrict__ in, const uint32_t *__restrict__ arg, uint32_t *__restrict__ out, uint32_t *__restrict__ out2) {
    const uint32_t wave = DU_WAVE_INDEX();
    const uint32_t a0 = arg[2 * wave], a1 = arg[2 * wave + 1];
    LV<uint32_t> x, r;
    LFOR(l) { x[l] = in[wave * 64u + uint32_t(l)]; r[l] = 0; }
    uint32_t u2 = 0;
    if (op == 0) r = lscan(x, u2);
    else if (op == 1) { const uint32_t s = lsum32(x); LFOR(l) r[l] = s; }
    else if (op == 2) r = lprev(x, a0);
    else if (op == 3) { const uint32_t s = llast(x); LFOR(l) r[l] = s; }
    else if (op == 4) { const uint32_t s = lget(x, uni(a0)); LFOR(l) r[l] = s; }
    else if (op == 5) { r = x; lset(r, uni(a0), uni(a1)); }
    else if (op == 6) { const uint64_t m = lballot([&](int l) { return x[l] != 0u; }); LFOR(l) r[l] = uint32_t(m); u2 = uint32_t(m >> 32); }
    else { const uint32_t s = uni(a0); LFOR(l) r[l] = s; }
    LFOR(l) { out[wave * 64u + uint32_t(l)] = r[l]; out2[wave * 64u + uint32_t(l)] = u2; }
}
// op: 0 lsum  1 lmin64
__global__ void __launch_bounds__(256) k_du_wave64(int op, const uint64_t *__restrict__ in, uint64_t *__restrict__ out) {
    const uint32_t wave = DU_WAVE_INDEX();
    LV<uint64_t> x;
    LFOR(l) x[l] = in[wave * 64u + uint32_t(l)];
    const uint64_t s = op == 0 ? lsum(x) : lmin64(x);
    LFOR(l) out[wave * 64u + uint32_t(l)] = s;
}

// A wave reads its own buffer -- pool + off[wave] (4-byte aligned), len[wave] bytes, from byte at[wave] -- through a script shared by all: step i is
// (script[2 i], script[2 i + 1]) = (0 get / 1 peek / 2 skip, n).  val / pos / over: [nwaves][nsteps] -- what the step returned (0 for a skip), byte_pos() and
// overrun() behind it.
__global__ void __launch_bounds__(256) k_du_lereader(const uint8_t *__restrict__ pool, const uint32_t *__restrict__ off, const uint32_t *__restrict__ len, const uint32_t *__restrict__ at,
                                                     const int32_t *__restrict__ script, int nsteps, uint32_t *__restrict__ val, uint32_t *__restrict__ pos, uint32_t *__restrict__ over) {
    const uint32_t wave = DU_WAVE_INDEX();
    csp::LeReader rd;
    rd.begin(pool + uni(off[wave]), uni(len[wave]), uni(at[wave]));
    for (int i = 0; i < nsteps; i++) {
        const int what = int(uni(uint32_t(script[2 * i]))), n = int(uni(uint32_t(script[2 * i + 1])));
        uint32_t v = 0;
        if (what == 0) v = rd.get(n); else if (what == 1) v = rd.peek(n); else rd.skip(n);
        const uint32_t p = rd.byte_pos(), o = rd.overrun() ? 1u : 0u;
        LFOR(l) if (l == (i & 63)) { val[size_t(wave) * nsteps + i] = v; pos[size_t(wave) * nsteps + i] = p; over[size_t(wave) * nsteps + i] = o; }   // (any lane holds the wave-uniform results: a different one each step)
    }
}

// thread i: load32u / load64u at pool + i (every misalignment), and align_bytes(hi[i], lo[i], shift[i])
__global__ void __launch_bounds__(256) k_du_lz(int n, const uint8_t *__restrict__ pool, const uint32_t *__restrict__ hi, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ shift,
                                               uint32_t *__restrict__ o32, uint64_t *__restrict__ o64, uint32_t *__restrict__ oal) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    o32[i] = csp::load32u(pool + i);
    o64[i] = csp::load64u(pool + i);
    oal[i] = csp::align_bytes(hi[i], lo[i], shift[i]);
}

extern "C" {
int csdu_wave32(int op, int nwaves, int wpb, const uint32_t *in, const uint32_t *arg, uint32_t *out, uint32_t *out2) {
    if (op < 0 || op > 7 || (wpb != 1 && wpb != 4) || nwaves <= 0 || nwaves % wpb) return -1;
    DuBufs B;
    uint32_t *d_in, *d_arg, *d_o, *d_o2;
    const size_t nb = size_t(nwaves) * 64 * 4;
    DU_TRY(B.upload(&d_in, in, nb));
    DU_TRY(B.upload(&d_arg, arg, size_t(nwaves) * 8));
    DU_TRY(B.zeroed(&d_o, nb, 0x55));
    DU_TRY(B.zeroed(&d_o2, nb, 0x55));
    DU_WAVE_LAUNCH(k_du_wave32, nwaves, wpb, op, d_in, d_arg, d_o, d_o2);
    DU_TRY(du_finish());
    DU_TRY(du_download(out, d_o, nb));
    return du_download(out2, d_o2, nb);
}
int csdu_wave64(int op, int nwaves, int wpb, const uint64_t *in, uint64_t *out) {
    if (op < 0 || op > 1 || (wpb != 1 && wpb != 4) || nwaves <= 0 || nwaves % wpb) return -1;
    DuBufs B;
    uint64_t *d_in, *d_o;
    const size_t nb = size_t(nwaves) * 64 * 8;
    DU_TRY(B.upload(&d_in, in, nb));
    DU_TRY(B.zeroed(&d_o, nb, 0x55));
    DU_WAVE_LAUNCH(k_du_wave64, nwaves, wpb, op, d_in, d_o);
    DU_TRY(du_finish());
    return du_download(out, d_o, nb);
}
int csdu_lereader(int nwaves, int wpb, const uint8_t *pool, size_t pool_bytes, const uint32_t *off, const uint32_t *len, const uint32_t *at, const int32_t *script, int nsteps,
                  uint32_t *val, uint32_t *pos, uint32_t *over) {
    if ((wpb != 1 && wpb != 4) || nwaves <= 0 || nwaves % wpb || nsteps <= 0) return -1;
    for (int w = 0; w < nwaves; w++) if ((off[w] & 3u) || size_t(off[w]) + len[w] > pool_bytes || at[w] > len[w]) return -1;
    for (int i = 0; i < nsteps; i++) if (script[2 * i] < 0 || script[2 * i] > 2 || script[2 * i + 1] < 1 || script[2 * i + 1] > 32) return -1;
    DuBufs B;
    uint8_t *d_pool;
    uint32_t *d_off, *d_len, *d_at, *d_val, *d_pos, *d_over;
    int32_t *d_script;
    const size_t nb = size_t(nwaves) * nsteps * 4;
    DU_TRY(B.upload(&d_pool, pool, pool_bytes));
    DU_TRY(B.upload(&d_off, off, size_t(nwaves) * 4));
    DU_TRY(B.upload(&d_len, len, size_t(nwaves) * 4));
    DU_TRY(B.upload(&d_at, at, size_t(nwaves) * 4));
    DU_TRY(B.upload(&d_script, script, size_t(nsteps) * 8));
    DU_TRY(B.zeroed(&d_val, nb, 0x55));
    DU_TRY(B.zeroed(&d_pos, nb, 0x55));
    DU_TRY(B.zeroed(&d_over, nb, 0x55));
    DU_WAVE_LAUNCH(k_du_lereader, nwaves, wpb, d_pool, d_off, d_len, d_at, d_script, nsteps, d_val, d_pos, d_over);
    DU_TRY(du_finish());
    DU_TRY(du_download(val, d_val, nb));
    DU_TRY(du_download(pos, d_pos, nb));
    return du_download(over, d_over, nb);
}
// pool: n + 7 bytes
int csdu_lz(int n, const uint8_t *pool, const uint32_t *hi, const uint32_t *lo, const uint32_t *shift, uint32_t *o32, uint64_t *o64, uint32_t *oal) {
    if (n <= 0) return -1;
    for (int i = 0; i < n; i++) if (shift[i] > 3u) return -1;   // align_bytes' contract (see tests/_devunit_cases.py)
    DuBufs B;
    uint8_t *d_pool;
    uint32_t *d_hi, *d_lo, *d_sh, *d_o32, *d_oal;
    uint64_t *d_o64;
    DU_TRY(B.upload(&d_pool, pool, size_t(n) + 7));
    DU_TRY(B.upload(&d_hi, hi, size_t(n) * 4));
    DU_TRY(B.upload(&d_lo, lo, size_t(n) * 4));
    DU_TRY(B.upload(&d_sh, shift, size_t(n) * 4));
    DU_TRY(B.zeroed(&d_o32, size_t(n) * 4, 0x55));
    DU_TRY(B.zeroed(&d_o64, size_t(n) * 8, 0x55));
    DU_TRY(B.zeroed(&d_oal, size_t(n) * 4, 0x55));
    CSH_LAUNCH(k_du_lz, dim3(unsigned((n + 255) / 256)), dim3(256), 0, n, d_pool, d_hi, d_lo, d_sh, d_o32, d_o64, d_oal);
    DU_TRY(du_finish());
    DU_TRY(du_download(o32, d_o32, size_t(n) * 4));
    DU_TRY(du_download(o64, d_o64, size_t(n) * 8));
    return du_download(oal, d_oal, size_t(n) * 4);
}
}
