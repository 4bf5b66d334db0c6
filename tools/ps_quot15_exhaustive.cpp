/* tools/ps_quot15_exhaustive.cpp -- xp_quot15 (libxaac_amd/csrc/sbr_ps_frame.h) against the integer division of
   xp_divide16_pos on every pair of normalised heads: v in [2^14, 2^16), u in [0, v] (a positive divisor normalises into the
   lower half; the upper half is what a divisor with the sign bit would give), then every u < 2^16 for every 64th v.
   A developer tool, about twenty seconds on one core:

     g++ -O2 -std=c++17 -ffp-contract=off tools/ps_quot15_exhaustive.cpp -o ps_quot15 && ./ps_quot15

   tests/test_ps_prep_cpu.py runs a strided sample of the same domain. */
#include <stdint.h>
#include <stdio.h>

#include "../include/xaac_amd.h"
#include "../libxaac_amd/csrc/sbr_core.h"
#include "../libxaac_amd/csrc/sbr_ps.h"
#include "../libxaac_amd/csrc/sbr_ps_frame.h"

#include <string.h>

int main() {
  uint64_t all_bad = 0;
  for (int ulps = -1; ulps <= 1; ulps++) { /* the reciprocal: the host's 1 / v and the floats next to it */
    uint64_t n = 0, bad = 0;
    for (uint32_t v = 1u << 14; v < (1u << 16); v++) {
      float r = 1.0f / (float)v;
      uint32_t bits;
      memcpy(&bits, &r, 4);
      bits += ulps;
      memcpy(&r, &bits, 4);
      const uint32_t top = v % 64 == 0 ? 65535u : v;
      for (uint32_t u = 0; u <= top; u++, n++) bad += xp_quot15_rcp(u, v, r) != (u << 15) / v;
    }
    printf("xp_quot15 vs (u << 15) / v, reciprocal %+d ulp: %llu pairs, %llu differ\n", ulps, (unsigned long long)n,
           (unsigned long long)bad);
    all_bad += bad;
  }
  return all_bad != 0;
}
