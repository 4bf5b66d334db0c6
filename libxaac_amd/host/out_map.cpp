/*
 * out_map.cpp -- the output maps of include/xaac_amd.h (xaac_out_map) on the host: the CPU twin of the mapped GPU calls, from the
 * arithmetic header they share (libxaac_amd/csrc/out_map.h).  The command line decoder mixes the limiter's flushed delay line
 * with it; the tests hold the GPU calls against it.
 */
#include <stdint.h>
#include <string.h>

#include "../../include/xaac_parse.h"
#include "../csrc/out_map.h"

namespace {
template <int NCH>
void downmix(const int32_t coef[2][8], const int16_t *in, int64_t n, int16_t *out) {
  int32_t cl[NCH], cr[NCH];
  for (int s = 0; s < NCH; s++) cl[s] = coef[0][s], cr[s] = coef[1][s];
  for (int64_t i = 0; i < n; i++) {
    int16_t x[NCH], l, r;
    for (int s = 0; s < NCH; s++) x[s] = in[i * NCH + s];
    xo_downmix<NCH>(cl, cr, x, l, r);
    out[2 * i] = l, out[2 * i + 1] = r;
  }
}
}  // namespace

extern "C" {

int32_t xaac_out_map_apply_host(const xaac_out_map *map, int32_t num_channels, const int16_t *in, int64_t n_samples, int16_t *out) {
  if (!map || !in || !out || n_samples < 0 || num_channels < 1 || num_channels > 8) return -1;
  const int oc = xo_out_channels(map->kind, num_channels);
  if (!oc) return -1;
  switch (map->kind) {
    case XAAC_OUT_MAP_NONE:
      if (in != out) memmove(out, in, (size_t)n_samples * num_channels * sizeof(int16_t));
      break;
    case XAAC_OUT_MAP_DOWNMIX_STEREO: {
      int32_t coef[2][8];
      if (xo_resolve(map, num_channels, coef)) return -1;
      switch (num_channels) {
        case 3: downmix<3>(coef, in, n_samples, out); break;
        case 4: downmix<4>(coef, in, n_samples, out); break;
        case 5: downmix<5>(coef, in, n_samples, out); break;
        default: downmix<6>(coef, in, n_samples, out); break;
      }
      break;
    }
    case XAAC_OUT_MAP_MONO_MIX:
      for (int64_t i = 0; i < n_samples; i++) out[i] = xo_mono_mix(in[2 * i], in[2 * i + 1]);
      break;
    case XAAC_OUT_MAP_MONO_MIX_DUP:
      for (int64_t i = 0; i < n_samples; i++) out[2 * i] = out[2 * i + 1] = xo_mono_mix(in[2 * i], in[2 * i + 1]);
      break;
    case XAAC_OUT_MAP_DUP_STEREO:
      for (int64_t i = n_samples - 1; i >= 0; i--) { /* from the back: in place */
        const int16_t v = in[i];
        out[2 * i] = out[2 * i + 1] = v;
      }
      break;
  }
  return oc;
}

int32_t xaac_out_map_row_bound(int32_t matrix, int64_t *row_sum) {
  if (matrix < 0 || matrix > 1 || !xo_term_fits()) return -1;
  return xo_row_bound(matrix, row_sum);
}

}  // extern "C"
