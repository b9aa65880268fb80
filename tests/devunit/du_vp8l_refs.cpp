// du_vp8l_refs.cpp -- device unit over caesium-clt_amd/csrc/k_vp8l_refs.hip: its two lane moves, lget (readlane of a wave-uniform lane) and lshfl (a gather by
// per-lane source, a negative source meaning the lane itself), one case per wave; and code_lengths_wide (vp8l_refs.h), a wave per case with lane 0 working in
// LDS, as k_vp8l_refs_codes and k_vp8l_group_codes run it.  See du_common.h.
#include "../../caesium-clt_amd/csrc/k_vp8l_refs.hip"
#include "du_common.h"
using namespace csw;
using csp::LV;

// the host symbols of another file that this one's launcher names (k_vp8l_enc.hip has them); nothing here launches the coder
namespace csw {
void launch_vp8l_front(hipStream_t, const Vp8lImg *, int, uint32_t, uint64_t, uint32_t *, uint8_t *, uint32_t *) {}
void launch_vp8l_pack_plain(hipStream_t, const Vp8lImg *, int, const uint32_t *, const uint8_t *, const uint32_t *, const uint32_t *, uint8_t *, uint32_t *, uint32_t *) {}
}  // namespace csw

// op: 0 lget(x, arg[wave]) in every lane   1 lshfl(x, src)
__global__ void __launch_bounds__(256) k_du_refs_lanes(int op, const uint32_t *__restrict__ in, const int32_t *__restrict__ src, const int32_t *__restrict__ arg, uint32_t *__restrict__ out) {
    const uint32_t wave = DU_WAVE_INDEX();
    LV<uint32_t> x, r;
    LV<int> s;
    LFOR(l) { x[l] = in[wave * 64u + uint32_t(l)]; s[l] = src[wave * 64u + uint32_t(l)]; }
    if (op == 0) { const uint32_t v = csw::lget(x, int(csp::uni(uint32_t(arg[wave])))); LFOR(l) r[l] = v; }
    else r = lshfl(x, s);
    LFOR(l) out[wave * 64u + uint32_t(l)] = r[l];
}
// case c: freq[c * n ..] -> len[c * n ..]
__global__ void __launch_bounds__(CSP_WAVE_THREADS) k_du_code_lengths_wide(int n, int limit, const uint32_t *__restrict__ freq, uint8_t *__restrict__ len) {
    CSH_SHARED CodeWs ws;
    const size_t at = size_t(blockIdx.x) * size_t(n);
    LFOR(l) if (l == 0) code_lengths_wide(freq + at, n, limit, len + at, ws);
}

extern "C" {
// refused: an alphabet CodeWs does not hold, a limit outside what canonical() can code, a limit the alphabet does not fit under
int csdu_code_lengths_wide(int ncases, int n, int limit, const uint32_t *freq, uint8_t *len) {
    if (ncases <= 0 || n < 2 || n > int(VP8L_GREEN_MAX) || limit < 7 || limit > 15 || (1 << limit) < n) return -1;
    DuBufs B;
    uint32_t *d_f;
    uint8_t *d_l;
    const size_t cnt = size_t(ncases) * size_t(n);
    DU_TRY(B.upload(&d_f, freq, cnt * 4));
    DU_TRY(B.zeroed(&d_l, cnt, 0x55));
    CSH_LAUNCH(k_du_code_lengths_wide, dim3(unsigned(ncases)), dim3(CSP_WAVE_THREADS), 0, n, limit, d_f, d_l);
    DU_TRY(du_finish());
    return du_download(len, d_l, cnt);
}
int csdu_refs_lanes(int op, int nwaves, int wpb, const uint32_t *in, const int32_t *src, const int32_t *arg, uint32_t *out) {
    if (op < 0 || op > 1 || (wpb != 1 && wpb != 4) || nwaves <= 0 || nwaves % wpb) return -1;
    for (int i = 0; i < nwaves * 64; i++) if (src[i] > 63) return -1;
    for (int i = 0; i < nwaves; i++) if (arg[i] < 0 || arg[i] > 63) return -1;
    DuBufs B;
    uint32_t *d_in, *d_o;
    int32_t *d_src, *d_arg;
    const size_t nb = size_t(nwaves) * 64 * 4;
    DU_TRY(B.upload(&d_in, in, nb));
    DU_TRY(B.upload(&d_src, src, nb));
    DU_TRY(B.upload(&d_arg, arg, size_t(nwaves) * 4));
    DU_TRY(B.zeroed(&d_o, nb, 0x55));
    DU_WAVE_LAUNCH(k_du_refs_lanes, nwaves, wpb, op, d_in, d_src, d_arg, d_o);
    DU_TRY(du_finish());
    return du_download(out, d_o, nb);
}
}
