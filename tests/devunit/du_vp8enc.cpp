// du_vp8enc.cpp -- device units over caesium-clt_amd/csrc/k_vp8enc.hip: the sums and minima over rows of sixteen and halves of eight lanes (DPP on the
// device) and the row broadcasts its mode decision makes with __shfl.  One case per wave.  See du_common.h.
#include "../../caesium-clt_amd/csrc/k_vp8enc.hip"
#include "du_common.h"
using namespace csw;
using csp::LV;

// the one host symbol of another file that k_vp8enc.hip's launcher names (k_webp.hip has it); nothing here launches the encoder
namespace csw {
int launch_webp_backend(hipStream_t, const WebpImg *, const WebpImg *, int, const int16_t *, const Vp8FrameDev *, const std::vector<uint64_t> &, const uint64_t *, csh::DevBuf<uint32_t> &, const uint16_t *,
                        uint8_t *, uint32_t *, uint8_t *, uint32_t *, uint32_t *) {
    csh_set_error("launch_webp_backend is not part of the device-unit library");
    return -1;
}
}  // namespace csw

// op: 0 rowsum  1 halfsum  2 the broadcast of lane l & 48  3 the broadcast of lane (l & 48) + 8, both as k_vp8_loop takes the U and V sums from halfsum's lanes
__global__ void __launch_bounds__(256) k_du_row32(int op, const int32_t *__restrict__ in, int32_t *__restrict__ out) {
    const uint32_t wave = DU_WAVE_INDEX();
    LV<int> x, r;
    LFOR(l) x[l] = in[wave * 64u + uint32_t(l)];
    if (op == 0) r = rowsum(x);
    else if (op == 1) r = halfsum(x);
    else {
        LFOR(l) {
#ifdef CSH_EMUL
            r[l] = op == 2 ? x.v[l & 48] : x.v[(l & 48) + 8];
#else
            r[l] = op == 2 ? __shfl(x.v, l & 48, 64) : __shfl(x.v, (l & 48) + 8, 64);
#endif
        }
    }
    LFOR(l) out[wave * 64u + uint32_t(l)] = r[l];
}
// op: 0 rowmin64  1 halfmin64
__global__ void __launch_bounds__(256) k_du_row64(int op, const uint64_t *__restrict__ in, uint64_t *__restrict__ out) {
    const uint32_t wave = DU_WAVE_INDEX();
    LV<uint64_t> x, r;
    LFOR(l) x[l] = in[wave * 64u + uint32_t(l)];
    if (op == 0) r = rowmin64(x); else r = halfmin64(x);
    LFOR(l) out[wave * 64u + uint32_t(l)] = r[l];
}

extern "C" {
int csdu_row32(int op, int nwaves, int wpb, const int32_t *in, int32_t *out) {
    if (op < 0 || op > 3 || (wpb != 1 && wpb != 4) || nwaves <= 0 || nwaves % wpb) return -1;
    DuBufs B;
    int32_t *d_in, *d_o;
    const size_t nb = size_t(nwaves) * 64 * 4;
    DU_TRY(B.upload(&d_in, in, nb));
    DU_TRY(B.zeroed(&d_o, nb, 0x55));
    DU_WAVE_LAUNCH(k_du_row32, nwaves, wpb, op, d_in, d_o);
    DU_TRY(du_finish());
    return du_download(out, d_o, nb);
}
int csdu_row64(int op, int nwaves, int wpb, const uint64_t *in, uint64_t *out) {
    if (op < 0 || op > 1 || (wpb != 1 && wpb != 4) || nwaves <= 0 || nwaves % wpb) return -1;
    DuBufs B;
    uint64_t *d_in, *d_o;
    const size_t nb = size_t(nwaves) * 64 * 8;
    DU_TRY(B.upload(&d_in, in, nb));
    DU_TRY(B.zeroed(&d_o, nb, 0x55));
    DU_WAVE_LAUNCH(k_du_row64, nwaves, wpb, op, d_in, d_o);
    DU_TRY(du_finish());
    return du_download(out, d_o, nb);
}
}
